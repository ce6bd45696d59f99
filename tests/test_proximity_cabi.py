"""CPU-side checks of the person-to-person contact map's boundary: the four entry points are declared and exported, bad
arguments answer with the error status and a message before any device call, the workspace size behaves, and the Python
signatures are the documented ones."""
import ctypes
import inspect

import numpy as np
import pytest

from mhhip import _lib

SYMBOLS = ['mh_vertex_normals', 'mh_person_nearest_bytes', 'mh_person_nearest', 'mh_person_pairs']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _addr(buf, v):
    return ctypes.addressof(buf) if v else None


def _nearest(L, T=2, N=3, V=10, verts=1, live=1, radius=0.1, ws=1, ws_bytes=None, d2=1, idx=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    if ws_bytes is None:
        ws_bytes = L.mh_person_nearest_bytes(max(T, 1), max(N, 1), max(V, 1))
    return L.mh_person_nearest(T, N, V, _addr(buf, verts), _addr(buf, live), radius, _addr(buf, ws), ws_bytes, _addr(buf, d2),
                               _addr(buf, idx), None)


def test_nearest_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('T', 'N', 'V'):
        for bad in (0, -1):
            assert _nearest(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _nearest(L, N=33) == -1 and b'at most 32' in L.mh_last_error()
    assert _nearest(L, T=1, N=32, V=2 ** 26) == -1 and b'2^31' in L.mh_last_error()            # N V = 2^31
    assert _nearest(L, T=2 ** 20, N=2, V=1024) == -1 and b'one launch' in L.mh_last_error()    # N V small, T N V = 2^31
    assert _nearest(L, T=2 ** 16, N=32, V=1024, ws_bytes=2 ** 62) == -1 and b'one launch' in L.mh_last_error()
    assert _nearest(L, verts=None) == -1 and b'null' in L.mh_last_error()
    assert _nearest(L, ws=None) == -1 and b'null' in L.mh_last_error()
    need = L.mh_person_nearest_bytes(2, 3, 10)
    assert _nearest(L, ws_bytes=need - 1) == -1 and b'workspace too small' in L.mh_last_error()
    assert _nearest(L, ws_bytes=0) == -1 and b'workspace too small' in L.mh_last_error()
    assert _nearest(L, d2=None, idx=None) == -1 and b'no output' in L.mh_last_error()
    for bad in (0.0, -0.1, float('inf'), float('-inf'), float('nan')):
        assert _nearest(L, radius=bad) == -1 and b'finite and positive' in L.mh_last_error(), bad
    assert _nearest(L, radius=0.65) == -1 and b'radius too large' in L.mh_last_error()
    assert _nearest(L, radius=1e6) == -1 and b'radius too large' in L.mh_last_error()


def test_workspace_bytes_are_positive_and_monotone():
    L = _lib.lib()
    base = L.mh_person_nearest_bytes(4, 4, 6890)
    assert base > 4 * 4 * 6890 * 16
    assert L.mh_person_nearest_bytes(1, 1, 1) > 0
    assert L.mh_person_nearest_bytes(0, 0, 0) > 0 and L.mh_person_nearest_bytes(-3, -3, -3) > 0
    for T, N, V in ((5, 4, 6890), (4, 5, 6890), (4, 4, 6891), (4, 4, 8000), (8, 32, 6890)):
        assert L.mh_person_nearest_bytes(T, N, V) >= base, (T, N, V)
    assert L.mh_person_nearest_bytes(8, 4, 6890) > base and L.mh_person_nearest_bytes(4, 8, 6890) > base
    assert L.mh_person_nearest_bytes(4, 4, 2 * 6890) > base
    # a chunk of 8 frames of 32 people stays in the tens of MB
    assert L.mh_person_nearest_bytes(8, 32, 6890) < 64 << 20


def _normals(L, B=2, V=10, F=5, verts=1, faces=1, adj_start=1, adj_face=1, A=15, normals=1):
    buf = (ctypes.c_float * 64)()
    return L.mh_vertex_normals(B, V, F, _addr(buf, verts), _addr(buf, faces), _addr(buf, adj_start), _addr(buf, adj_face), A,
                               _addr(buf, normals), None)


def test_normals_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V', 'F'):
        for bad in (0, -1):
            assert _normals(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _normals(L, A=-1) == -1 and b'A ' in L.mh_last_error()
    assert _normals(L, B=2 ** 16, V=2 ** 15) == -1 and b'one launch' in L.mh_last_error()
    for name in ('verts', 'faces', 'adj_start', 'adj_face', 'normals'):
        assert _normals(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name


def _pairs(L, T=2, N=3, V=10, verts=1, normals=1, d2=1, idx=1, part=1, P=24, thr=0.02, outs=(1, 1, 1, 1, 1, 1)):
    buf = (ctypes.c_float * 64)()
    return L.mh_person_pairs(T, N, V, _addr(buf, verts), _addr(buf, normals), _addr(buf, d2), _addr(buf, idx), _addr(buf, part), P, thr,
                             *[_addr(buf, o) for o in outs], None)


def test_pairs_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('T', 'N', 'V'):
        for bad in (0, -1):
            assert _pairs(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _pairs(L, N=33) == -1 and b'at most 32' in L.mh_last_error()
    for bad in (0, -1, 33):
        assert _pairs(L, P=bad) == -1 and b'1..32' in L.mh_last_error(), bad
    assert _pairs(L, T=1, N=32, V=2 ** 26) == -1 and b'2^31' in L.mh_last_error()
    assert _pairs(L, T=2 ** 20, N=2, V=1024) == -1 and b'one launch' in L.mh_last_error()
    for name in ('verts', 'd2', 'idx', 'part'):
        assert _pairs(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    assert _pairs(L, outs=(0,) * 6) == -1 and b'no output' in L.mh_last_error()
    for bad in (-0.01, float('inf'), float('nan')):
        assert _pairs(L, thr=bad) == -1 and b'thr' in L.mh_last_error(), bad


def test_optimiser_method_and_module_signatures():
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import contact, proximity
    p = inspect.signature(SMPLDepthSequenceOptimizer.proximity_map).parameters
    assert list(p) == ['self', 'frames', 'radius', 'contact', 'nearest', 'chunk']
    assert (p['frames'].default, p['radius'].default, p['contact'].default, p['nearest'].default, p['chunk'].default) == (None, 0.1, 0.02, False, 8)
    p = inspect.signature(proximity.proximity_map).parameters
    assert list(p) == ['model', 'verts', 'live', 'radius', 'contact', 'nearest', 'chunk']
    assert (p['live'].default, p['radius'].default, p['contact'].default, p['nearest'].default, p['chunk'].default) == (None, 0.1, 0.02, False, 8)
    assert list(inspect.signature(proximity.person_nearest).parameters) == ['verts', 'radius', 'live']
    assert list(inspect.signature(proximity.vertex_normals).parameters) == ['model', 'verts']
    assert list(inspect.signature(proximity.vertex_faces).parameters) == ['faces', 'V']
    # the parts are the contact map's, not a copy
    assert proximity.PART_NAMES is contact.PART_NAMES and proximity.body_parts is contact.body_parts
    assert proximity.MAX_RADIUS == contact.MAX_RADIUS == 0.64


# SMPLDepthSequenceOptimizer.__init__ as it stood before the method was added: its named parameters, and the options it takes
# out of **kargs
INIT_PARAMETERS = ['self', 'image_size', 'num_frames', 'fov', 'focal_length', 'znear', 'zfar', 'cam_K', 'cam_dist_coef',
                   'proj2d_loss_coef', 'depth_loss_coef', 'silhouette_loss_coef', 'reg_velocity_coef', 'reg_verts_filter_coef',
                   'reg_poses_coef', 'reg_scales_coef', 'reg_contact_coef', 'reg_foot_sliding_coef', 'joint_confidence_thr', 'eps',
                   'kargs']
INIT_OPTIONS = ['use_rasteriser', 'scene_update', 'use_graphs', 'process_group', 'shard_frames', 'reg_scene_pen_coef',
                'scene_pen_margin', 'scene_pen_band', 'scene_pen_edge', 'reg_order_coef', 'order_margin', 'order_delta']


def test_the_constructor_has_gained_no_keyword():
    import re
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    assert list(inspect.signature(SMPLDepthSequenceOptimizer.__init__).parameters) == INIT_PARAMETERS
    popped = re.findall(r"kargs\.pop\('(\w+)'", inspect.getsource(SMPLDepthSequenceOptimizer.__init__))
    assert popped == INIT_OPTIONS, popped


def test_python_value_errors():
    """shapes, the radius cap, 0 <= contact <= radius and the model's V against verts are refused before any device call"""
    import torch
    from mhhip import proximity
    V = 12
    model = np.zeros((V, 24), np.float32)                 # skinning weights: every vertex belongs to part 0
    verts = torch.zeros(2, 2, V, 3)
    for bad in (verts[0], torch.zeros(2, 2, V, 2), torch.zeros(2, 0, V, 3)):
        with pytest.raises(ValueError, match='verts'):
            proximity.proximity_map(model, bad)
    with pytest.raises(ValueError, match='at most 32'):
        proximity.proximity_map(model, torch.zeros(1, 33, V, 3))
    for bad in (0.0, -1.0, 0.65, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='radius'):
            proximity.proximity_map(model, verts, radius=bad)
    for bad in (-0.01, 0.11, float('nan')):
        with pytest.raises(ValueError, match='contact'):
            proximity.proximity_map(model, verts, radius=0.1, contact=bad)
    with pytest.raises(ValueError, match='vertices'):
        proximity.proximity_map(model, torch.zeros(2, 2, V + 1, 3))
    with pytest.raises(ValueError, match='live'):
        proximity.proximity_map(model, verts, live=np.ones((2, 3)))
    with pytest.raises(ValueError, match='verts'):
        proximity.person_nearest(verts[0], 0.1)
    with pytest.raises(ValueError, match='radius'):
        proximity.person_nearest(verts, 1.0)
    with pytest.raises(ValueError, match='live'):
        proximity.person_nearest(verts, 0.1, live=[1, 1])
    with pytest.raises(ValueError, match='verts'):
        proximity.vertex_normals(np.zeros((4, 3), np.int64), torch.zeros(5))
    with pytest.raises(ValueError, match='faces'):
        proximity.vertex_faces(np.zeros((4, 2), np.int64), 5)
