"""The scene-penetration kernels (``mh_scene_zmap``, ``mh_scene_pen_term``, ``mh_scene_pen_term_sel``) against the float64
restatement of tests/scene_pen_ref.py.

The tolerance is not chosen in advance: the header's formulas are evaluated in numpy float32 and float64 on the cases of
scene_pen_ref.py and the kernel may be off by 4x the largest float32 error over all of them (``sp.budgets``; the factor is
the project's margin for such sums, tests/test_fit_report_gpu.py) -- the per-body value relative to the value of the whole
case (every vertex counts: |kernel - float64| of each body), the gradients of the decided vertices relative to the case's
largest gradient entry; nothing is said about the gradients of undecided vertices (scene_pen_ref.py).  Everything else is exact: a second launch gives the same
bits, the gradient is ADDED (the sum with a non-zero start is the float32 sum of the start and of what a zero start gives),
decided inactive vertices keep their start bit for bit.
"""
import numpy as np
import pytest

import scene_pen_ref as sp

pytestmark = pytest.mark.gpu

GRID = [(B, V, H, W) for (B, V) in sp.SHAPES for (H, W) in sp.IMAGES]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda:0')


def _launch(c, zmap=None, start=None, want_grad=True, want_body=True, pool=False, words=None, zmaps=None):
    """one launch -> (body_loss (B) or None, gverts (B,V,3) or None); start: what gverts holds before (default zeros);
    pool: the accumulators from the stream's memory pool (acc = NULL); words / zmaps: the gated form"""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    L = _lib.lib()
    B, V, H, W = c['B'], c['V'], c['H'], c['W']
    K = np.ascontiguousarray(c['K'], np.float32).reshape(9)
    Kp = K.ctypes.data_as(_lib.c_float_p)
    verts = _dev(c['verts'])
    g = _dev(np.zeros((B, V, 3), np.float32) if start is None else start) if want_grad else None
    body = torch.full((B,), 77.0, dtype=torch.float32, device='cuda:0') if want_body else None
    acc = None if pool else torch.full((B,), 77, dtype=torch.int64, device='cuda:0')       # cleared by the call
    st = _lib.stream_ptr(verts.device)
    tail = (sp.COEF, sp.MARGIN, sp.BAND, sp.EDGE, ptr(g), ptr(body), ptr(acc), st)
    if words is not None:
        z0, z1, w = _dev(zmaps[0]), _dev(zmaps[1]), _dev(np.asarray(words, np.int32))
        check(L.mh_scene_pen_term_sel(B, V, H, W, Kp, ptr(verts), ptr(z0), ptr(z1), ptr(w), *tail))
    else:
        zm = _dev(c['zmap'] if zmap is None else zmap)
        check(L.mh_scene_pen_term(B, V, H, W, Kp, ptr(verts), ptr(zm), *tail))
    torch.cuda.synchronize()
    return (None if body is None else body.cpu().numpy()), (None if g is None else g.cpu().numpy())


@pytest.fixture(scope='module')
def cases(smpl_struct):
    cs = sp.all_cases()
    cs['body'] = sp.body_case(smpl_struct.v_template)
    return cs, sp.budgets(cs.values())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check_case(c, budget, tag):
    bv, bg = budget
    r64 = sp.evaluate(c['verts'], c['K'], c['zmap'])
    body, grad = _launch(c)
    ev, eg = sp.errors(body, grad, r64)
    print('%s: %d active, %d undecided of %d; kernel off by %.3e (value) %.3e (gradient), numpy float32 over all cases %.3e %.3e'
          % (tag, r64['active'].sum(), r64['undecided'].sum(), c['B'] * c['V'], ev, eg, bv, bg))
    assert np.isfinite(body).all() and np.isfinite(grad).all()
    assert ev <= 4 * bv, 'per-body value'
    assert eg <= 4 * bg, 'gradients of the decided vertices'
    idle = ~r64['undecided'] & ~r64['active']
    assert (grad[idle] == 0).all()
    if not r64['active'].any():
        assert (body == 0).all()
    # a second launch, and the accumulators from the stream's pool: the same bits
    body2, grad2 = _launch(c, pool=True)
    assert np.array_equal(_bits(body), _bits(body2)) and np.array_equal(_bits(grad), _bits(grad2))
    # added to, not overwritten
    rng = np.random.RandomState(3)
    start = rng.uniform(-0.01, 0.01, grad.shape).astype(np.float32)
    body3, grad3 = _launch(c, start=start)
    assert np.array_equal(_bits(body), _bits(body3))
    assert np.array_equal(grad3, (start + grad).astype(np.float32))
    assert np.array_equal(_bits(grad3[idle]), _bits(start[idle]))
    # either output alone
    body4, _ = _launch(c, want_grad=False)
    assert np.array_equal(_bits(body), _bits(body4))
    _, grad5 = _launch(c, want_body=False)
    assert np.array_equal(_bits(grad), _bits(grad5))
    return body, grad


@pytest.mark.parametrize('shape', GRID)
def test_term_against_float64(cases, shape):
    cs, budget = cases
    for kind in sp.KINDS:
        _check_case(cs[shape + (kind,)], budget, '%s %s' % (shape, kind))


def test_term_on_two_bodies_of_the_model(cases):
    cs, budget = cases
    body, _ = _check_case(cs['body'], budget, 'two bodies of 6890 vertices')
    assert (body > 0).all()


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (3, 65, 9, 16), (2, 257, 135, 240)])
def test_gated_form(cases, shape):
    cs, _ = cases
    c = cs[shape + ('floor',)]
    other = cs[shape + ('holes',)]['zmap']
    zmaps = (c['zmap'], other)
    rng = np.random.RandomState(4)
    start = rng.uniform(-0.01, 0.01, (c['B'], c['V'], 3)).astype(np.float32)
    # no scene yet: the gradient buffer is not touched, the loss is written as 0 -- whatever the second word says
    for which in (0, 1):
        body, grad = _launch(c, start=start, words=[0, which], zmaps=zmaps)
        assert (body == 0).all() and np.array_equal(_bits(grad), _bits(start))
    # live: the plain form on the chosen map
    for which in (0, 1):
        want_b, want_g = _launch(c, zmap=zmaps[which], start=start)
        body, grad = _launch(c, start=start, words=[1, which], zmaps=zmaps)
        assert np.array_equal(_bits(body), _bits(want_b)) and np.array_equal(_bits(grad), _bits(want_g)), which
    a, b = _launch(c, zmap=zmaps[0])[0], _launch(c, zmap=zmaps[1])[0]
    if shape[0] * shape[1] > 1:
        assert not np.array_equal(a, b)          # (the two maps do give different values: the selector is really read)


@pytest.mark.parametrize('size', [(1, 1), (2, 2), (9, 16), (135, 240), (54, 97)])
def test_zmap_is_exactly_the_masked_depth(size):
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    H, W = size
    rng = np.random.RandomState(H * 1000 + W)
    depth = rng.uniform(-1.0, 9.0, (H, W)).astype(np.float32)
    mask = rng.choice(np.float32([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.25, 7.0]), (H, W))
    out = torch.full((H, W), 77.0, dtype=torch.float32, device='cuda:0')
    d, m = _dev(depth), _dev(mask)
    check(_lib.lib().mh_scene_zmap(H, W, ptr(d), ptr(m), ptr(out), _lib.stream_ptr(out.device)))
    torch.cuda.synchronize()
    want = np.where(mask > np.float32(0.5), depth, np.float32(0))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
