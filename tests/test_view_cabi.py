"""CPU-side checks of the free-viewpoint renderer's boundary: its five entry points are declared and exported, the Python
entry points have the documented signatures, the argument errors answer with a status and a message before any device call,
and the camera helpers return proper rotations that look at their target."""
import ctypes
import inspect

import numpy as np
import pytest

from mhhip import _lib

SYMBOLS = ['mh_view_project', 'mh_view_clear', 'mh_view_raster', 'mh_view_splat', 'mh_view_resolve']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def test_signatures():
    from mhhip import view
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    p = inspect.signature(view.render_view).parameters
    assert list(p)[:16] == ['model', 'verts', 'view', 'K', 'image_size', 'cloud', 'cloud_rgb', 'cloud_size_m', 'palette', 'light',
                            'ambient', 'background', 'near', 'max_half', 'outputs', 'chunk']
    assert all(p[k].default is None for k in ('cloud', 'cloud_rgb', 'cloud_size_m', 'palette', 'outputs'))
    assert p['light'].default == (0, 0, 1) and p['ambient'].default == 0.3 and p['background'].default == (255, 255, 255)
    assert p['near'].default == 0.1 and p['max_half'].default == 3 and p['chunk'].default == 32
    q = inspect.signature(SMPLDepthSequenceOptimizer.render_view).parameters
    assert list(q) == ['self', 'view', 'frames', 'image_size', 'K', 'scene', 'splat', 'kw']
    assert q['frames'].default is None and q['image_size'].default is None and q['K'].default is None
    assert q['scene'].default is True and q['splat'].default == 1.0
    assert inspect.signature(view.look_at).parameters['up'].default == (0, -1, 0)
    assert list(inspect.signature(view.orbit).parameters) == ['center', 'radius', 'elevation_deg', 'azimuth_deg']
    assert list(inspect.signature(view.top_down).parameters) == ['center', 'height']


# the pointers are never followed: every case below is refused by the argument check
BUF = (ctypes.c_float * 64)()
A = ctypes.addressof(BUF)
FP = ctypes.cast(BUF, _lib.c_float_p)
U8 = ctypes.cast(BUF, ctypes.POINTER(ctypes.c_uint8))


def _refused(rc, L, word):
    msg = L.mh_last_error()
    assert rc != 0 and msg.startswith(b'invalid argument') and word in msg, (rc, msg)


def test_project_argument_errors():
    L = _lib.lib()
    ok = dict(count=4, per_view=1, Tv=1, xyz=A, R=FP, t=FP, K=FP, near=0.1, out=A)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mh_view_project(a['count'], a['per_view'], a['Tv'], a['xyz'], a['R'], a['t'], a['K'], a['near'], a['out'], None)
    for k in ('xyz', 'R', 't', 'K', 'out'):
        _refused(call(**{k: None}), L, b'null')
    _refused(call(near=0.0), L, b'near')
    _refused(call(near=-1.0), L, b'near')
    _refused(call(near=float('nan')), L, b'near')
    _refused(call(count=0), L, b'empty')
    _refused(call(Tv=0), L, b'empty')
    _refused(call(Tv=65), L, b'64 views')
    _refused(call(per_view=2), L, b'per_view')


def test_clear_and_raster_argument_errors():
    L = _lib.lib()
    _refused(L.mh_view_clear(1, 8, 8, None, None), L, b'null')
    _refused(L.mh_view_clear(1, 8, 4097, A, None), L, b'4096')
    _refused(L.mh_view_clear(0, 8, 8, A, None), L, b'empty')
    ok = dict(T=1, N=1, V=4, F=2, H=8, W=8, vq=A, faces=A, keys=A)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mh_view_raster(a['T'], a['N'], a['V'], a['F'], a['H'], a['W'], a['vq'], a['faces'], a['keys'], None)
    for k in ('vq', 'faces', 'keys'):
        _refused(call(**{k: None}), L, b'null')
    _refused(call(W=4097), L, b'4096')
    _refused(call(H=4097), L, b'4096')
    _refused(call(N=33), L, b'32 people')
    _refused(call(F=0), L, b'empty')
    _refused(call(N=32, F=2 ** 26), L, b'2^31')


def test_splat_argument_errors():
    L = _lib.lib()
    ok = dict(T=1, P=4, H=8, W=8, pq=A, size_q=A, fq=6400, max_half=3, keys=A)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mh_view_splat(a['T'], a['P'], a['H'], a['W'], a['pq'], a['size_q'], a['fq'], a['max_half'], a['keys'], None)
    for k in ('pq', 'keys'):
        _refused(call(**{k: None}), L, b'null')
    _refused(call(max_half=9), L, b'max_half')
    _refused(call(max_half=-1), L, b'max_half')
    _refused(call(W=4097), L, b'4096')
    _refused(call(fq=0), L, b'fq')
    _refused(call(P=0), L, b'empty')


def test_resolve_argument_errors():
    L = _lib.lib()
    ok = dict(keys=A, verts=A, faces=A, rgb=A, palette=A, light=FP, bg=U8, image=A, depth=A, label=A, face=A, coverage=A, N=1, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mh_view_resolve(1, a['N'], 4, 2, 8, a['W'], a['keys'], a['verts'], a['faces'], a['rgb'], a['palette'], a['light'], 0.3,
                                 a['bg'], a['image'], a['depth'], a['label'], a['face'], a['coverage'], None)
    _refused(call(image=None, depth=None, label=None, face=None, coverage=None), L, b'no output')
    _refused(call(keys=None), L, b'null')
    for k in ('verts', 'faces', 'palette', 'light', 'bg'):      # what the image reads
        _refused(call(**{k: None}), L, b'null')
    _refused(call(N=33), L, b'32 people')
    _refused(call(W=4097), L, b'4096')


def test_python_layer_refuses_before_the_device():
    import torch
    from mhhip import view
    v = torch.zeros(2, 1, 4, 3)
    eye = (np.eye(3), np.zeros(3))
    K = np.eye(3)
    with pytest.raises(ValueError, match='outputs'):
        view.render_view(None, v, eye, K, (8, 8), outputs=('colour',))
    with pytest.raises(ValueError, match='4096'):
        view.render_view(None, v, eye, K, (4097, 8))
    with pytest.raises(ValueError, match='max_half'):
        view.render_view(None, v, eye, K, (8, 8), max_half=9)
    with pytest.raises(ValueError, match='view'):
        view.render_view(None, v, (np.zeros((3, 3, 3)), np.zeros((3, 3))), K, (8, 8))
    with pytest.raises(ValueError, match='T,N,V,3'):
        view.render_view(None, v[0], eye, K, (8, 8))


def _is_rotation(R):
    return np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_cameras_are_rotations_looking_at_the_target():
    from mhhip import view
    rng = np.random.RandomState(3)
    for _ in range(20):
        eye, target = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        R, t = view.look_at(eye, target)
        assert _is_rotation(R)
        c = R @ target + t
        assert np.abs(c[:2]).max() < 1e-12 and abs(c[2] - np.linalg.norm(target - eye)) < 1e-12
        assert np.abs(R @ eye + t).max() < 1e-12
    # the fit camera itself: identity
    R, t = view.look_at((0, 0, 0), (0, 0, 3))
    assert np.array_equal(R, np.eye(3)) and not t.any()
    # straight up and straight down (forward parallel to `up`)
    for target in ((0, -2, 0), (0, 2, 0)):
        R, t = view.look_at((0, 0, 0), target)
        assert _is_rotation(R) and np.allclose(R @ np.asarray(target, float) + t, (0, 0, 2))
    center = np.asarray([0.3, 0.8, 3.0])
    el, az = np.asarray([0.0, 20.0, 90.0, -30.0, 45.0]), np.asarray([0.0, 90.0, 10.0, 180.0, 275.0])
    Rs, ts = view.orbit(center, 2.5, el, az)
    assert Rs.shape == (5, 3, 3) and ts.shape == (5, 3)
    for R, t in zip(Rs, ts):
        assert _is_rotation(R) and np.allclose(R @ center + t, (0, 0, 2.5), atol=1e-12)
    assert np.allclose(Rs[0], np.eye(3)) and np.allclose(ts[0], (-0.3, -0.8, -0.5))          # azimuth 0, elevation 0: the fit's side
    assert (-Rs[1].T @ ts[1])[1] < center[1]                   # a positive elevation raises the camera (y points down)
    R1, t1 = view.orbit(center, 2.5, 20.0, 90.0)
    assert R1.shape == (3, 3) and np.allclose(R1, Rs[1]) and np.allclose(t1, ts[1])
    R, t = view.top_down(center, 4.0)
    assert _is_rotation(R) and np.allclose(R @ center + t, (0, 0, 4.0))
    assert np.allclose(-R.T @ t, center - (0, 4.0, 0)) and np.allclose(R[1], (0, 0, -1))    # the fit's forward is the top of the image
