"""``mhhip.bodies``: the faces, tables and argument checks the maps over bodies share, on CPU tensors."""
import numpy as np
import pytest
import torch

import proximity_ref as pr
from mhhip import bodies

FACES = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2], [3, 4, 9]], np.int64)      # the last names a vertex out of range
V = 5


class _WithFaces(object):
    def __init__(self):
        self.faces = FACES


class _WithF(object):
    def __init__(self):
        self.f = FACES.astype(np.uint32)


@pytest.mark.parametrize('make', [_WithFaces, _WithF, lambda: FACES], ids=['faces', 'f', 'array'])
def test_faces_and_their_cache(make):
    model = make()
    assert np.array_equal(bodies.faces_of(model), FACES)
    fc = bodies.faces(model, 'cpu')
    assert fc.dtype == torch.int32 and np.array_equal(fc.numpy(), FACES)
    cache = getattr(model, '_body_tables', None)
    if isinstance(model, np.ndarray):
        assert cache is None                                  # an array has nothing to keep them on
    else:
        assert list(cache) == ['cpu'] and bodies.faces(model, 'cpu') is fc and list(cache['cpu']) == ['faces']


@pytest.mark.parametrize('make', [_WithFaces, lambda: FACES], ids=['faces', 'array'])
def test_adjacency(make):
    model = make()
    fc, start, face = bodies.adjacency(model, V, 'cpu')
    want = pr.vertex_faces_ref(FACES, V)
    assert np.array_equal(fc.numpy(), FACES)
    for got, ref in zip((start, face), want):
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), ref)
    if not isinstance(model, np.ndarray):                     # built once, next to the faces
        assert bodies.adjacency(model, V, 'cpu')[1] is start and bodies.faces(model, 'cpu') is fc
        assert set(model._body_tables['cpu']) == {'faces', V}


@pytest.mark.parametrize('shape', [(4, 2), (0, 3)])
def test_faces_refused(shape):
    with pytest.raises(ValueError, match=r'faces must be \(F,3\), got \(%d, %d\)' % shape):
        bodies.faces(np.zeros(shape, np.int32), 'cpu')


def test_shapes():
    assert bodies.shape(torch.zeros(2, 32, 7, 3)) == (2, 32, 7)
    with pytest.raises(ValueError, match='at most 32 people per frame, got 33'):
        bodies.shape(torch.zeros(1, 33, 7, 3))
    with pytest.raises(ValueError, match=r'verts must be \(T,N,V,3\)'):
        bodies.shape(torch.zeros(2, 7, 3))
    assert bodies.batch_shape(torch.zeros(2, 7, 3), torch.zeros(2, 4, 3)) == (2, 7, 4)
    with pytest.raises(ValueError, match=r'verts must be \(V,3\) or \(B,V,3\)'):
        bodies.batch_shape(torch.zeros(7, 3), torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match=r'points must be \(Q,3\) for verts \(V,3\) or \(B,Q,3\) for verts \(B,V,3\)'):
        bodies.batch_shape(torch.zeros(2, 7, 3), torch.zeros(3, 4, 3))


def test_live():
    assert bodies.live_mask(None, 2, 3) is None
    lv = bodies.live_mask(np.array([[1, 0, 2], [0, 0, -1]]), 2, 3)
    assert lv.dtype == torch.uint8 and lv.tolist() == [[1, 0, 1], [0, 0, 1]]
    assert bodies.live_mask([True, False], 2).tolist() == [1, 0]
    with pytest.raises(ValueError, match=r'live must be \(T,N\) = \(2,3\), got \(3, 2\)'):
        bodies.live_mask(np.ones((3, 2)), 2, 3)
    with pytest.raises(ValueError, match=r'live must be \(B\) = \(4\), got \(2, 2\)'):
        bodies.live_mask(np.ones((2, 2)), 4)


def test_parts_and_radii():
    w = np.zeros((V, 24), np.float32)
    w[np.arange(V), [3, 0, 23, 3, 7]] = 1.0
    part, P = bodies.part_table(w, V, 'cpu')
    assert P == 24 == len(bodies.PART_NAMES) and part.dtype == torch.uint8 and part.tolist() == [3, 0, 23, 3, 7]
    with pytest.raises(ValueError, match='the model has 5 vertices, verts 6'):
        bodies.part_table(w, 6, 'cpu')
    with pytest.raises(ValueError, match='the model has more than 24 parts'):
        bodies.part_table(np.eye(25, dtype=np.float32), 25, 'cpu')
    assert bodies.cell_radius(0.1) == float(np.float32(0.1)) and bodies.any_radius(np.inf) == np.inf
    for bad in (0.0, -1.0, np.nan, np.inf, 0.65):
        with pytest.raises(ValueError, match='radius must be positive and at most 0.64 m'):
            bodies.cell_radius(bad)
    for bad in (0.0, -np.inf, np.nan):
        with pytest.raises(ValueError, match=r'radius must be positive \(inf is allowed\)'):
            bodies.any_radius(bad)
    assert bodies.contact_within(0.02, 0.1) == float(np.float32(0.02))
    with pytest.raises(ValueError, match=r'contact must lie in \[0, radius = 0.1\]'):
        bodies.contact_within(0.2, 0.1)
