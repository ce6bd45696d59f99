"""CPU-side checks of the point-to-surface boundary: the entry points are declared and exported, bad arguments answer with the
error status and a message before any device call, the workspace size behaves, the switch returns the previous setting, and
the Python signatures and refusals are the documented ones."""
import ctypes
import inspect

import numpy as np
import pytest

from mhhip import _lib

SYMBOLS = ['mh_surface_grid_bytes', 'mh_surface_grid', 'mh_surface_set_all_faces', 'mh_mesh_closest', 'mh_person_surface',
           'mh_surface_pairs']
INF, NAN = float('inf'), float('nan')


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _addr(buf, v):
    return ctypes.addressof(buf) if v else None


def _grid(L, B=6, V=10, F=12, verts=1, faces=1, live=1, ws=1, ws_bytes=None, status=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    if ws_bytes is None:
        ws_bytes = L.mh_surface_grid_bytes(max(B, 1), max(F, 1))
    return L.mh_surface_grid(B, V, F, _addr(buf, verts), _addr(buf, faces), _addr(buf, live), _addr(buf, ws), ws_bytes, _addr(buf, status), None)


def test_grid_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V', 'F'):
        for bad in (0, -1):
            assert _grid(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _grid(L, B=2 ** 16, V=2 ** 15, ws_bytes=2 ** 62) == -1 and b'one launch' in L.mh_last_error()        # B V = 2^31
    assert _grid(L, B=2 ** 13, F=2 ** 14, ws_bytes=2 ** 62) == -1 and b'one launch' in L.mh_last_error()        # 16 B F = 2^31
    assert b'2^31' in L.mh_last_error()
    for name in ('verts', 'faces', 'ws'):
        assert _grid(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    need = L.mh_surface_grid_bytes(6, 12)
    assert _grid(L, ws_bytes=need - 1) == -1 and b'workspace too small' in L.mh_last_error()
    assert _grid(L, ws_bytes=0) == -1 and b'workspace too small' in L.mh_last_error()


def test_workspace_bytes_are_positive_and_monotone():
    L = _lib.lib()
    base = L.mh_surface_grid_bytes(32, 13776)
    assert base > 32 * 13776 * (48 + 16 * 4)                # the face records and the lists of 16 F entries
    assert L.mh_surface_grid_bytes(1, 1) > 0
    assert L.mh_surface_grid_bytes(0, 0) > 0 and L.mh_surface_grid_bytes(-3, -3) > 0
    for B, F in ((33, 13776), (32, 13777), (64, 13776), (32, 20000)):
        assert L.mh_surface_grid_bytes(B, F) >= base, (B, F)
    assert L.mh_surface_grid_bytes(64, 13776) > base and L.mh_surface_grid_bytes(32, 2 * 13776) > base
    # the default chunk of 8 frames of 4 people stays in the tens of MB, 8 frames of 32 people below half a GB
    assert base < 64 << 20 and L.mh_surface_grid_bytes(256, 13776) < 512 << 20


def _closest(L, B=2, V=10, F=12, faces=1, ws=1, Q=5, points=1, radius=0.1, outs=(1, 1, 1, 1)):
    buf = (ctypes.c_float * 64)()
    return L.mh_mesh_closest(B, V, F, _addr(buf, faces), _addr(buf, ws), Q, _addr(buf, points), radius, *[_addr(buf, o) for o in outs], None)


def test_closest_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V', 'F', 'Q'):
        for bad in (0, -1):
            assert _closest(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _closest(L, B=2 ** 16, Q=2 ** 15) == -1 and b'one launch' in L.mh_last_error()
    assert _closest(L, B=2 ** 13, F=2 ** 14) == -1 and b'one launch' in L.mh_last_error()
    for name in ('faces', 'ws', 'points'):
        assert _closest(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    assert _closest(L, outs=(0, 0, 0, 0)) == -1 and b'no output' in L.mh_last_error()
    for bad in (NAN, 0.0, -0.1, -INF):
        assert _closest(L, radius=bad) == -1 and b'radius must be positive' in L.mh_last_error(), bad


def _person(L, T=2, N=3, V=10, F=12, faces=1, ws=1, verts=1, mask=1, radius=0.1, outs=(1,) * 7):
    buf = (ctypes.c_float * 64)()
    return L.mh_person_surface(T, N, V, F, _addr(buf, faces), _addr(buf, ws), _addr(buf, verts), _addr(buf, mask), radius,
                               *[_addr(buf, o) for o in outs], None)


def test_person_surface_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('T', 'N', 'V', 'F'):
        for bad in (0, -1):
            assert _person(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _person(L, N=33) == -1 and b'at most 32' in L.mh_last_error()
    assert _person(L, T=1, N=32, F=2 ** 26) == -1 and b'm * F + f' in L.mh_last_error()           # N F = 2^31
    assert _person(L, T=2 ** 20, N=2, V=1024) == -1 and b'one launch' in L.mh_last_error()       # T N V = 2^31
    assert _person(L, T=2 ** 12, N=2, F=2 ** 14) == -1 and b'one launch' in L.mh_last_error()    # 16 T N F = 2^31
    for name in ('faces', 'ws', 'verts'):
        assert _person(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    assert _person(L, outs=(0,) * 7) == -1 and b'no output' in L.mh_last_error()
    for bad in (NAN, 0.0, -0.1, -INF):
        assert _person(L, radius=bad) == -1 and b'radius must be positive' in L.mh_last_error(), bad


def _pairs(L, T=2, N=3, V=10, F=12, ins=(1,) * 5, P=24, contact=0.02, outs=(1,) * 6):
    buf = (ctypes.c_float * 64)()
    return L.mh_surface_pairs(T, N, V, F, *[_addr(buf, i) for i in ins], P, contact, *[_addr(buf, o) for o in outs], None)


def test_pairs_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('T', 'N', 'V', 'F'):
        for bad in (0, -1):
            assert _pairs(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _pairs(L, N=33) == -1 and b'at most 32' in L.mh_last_error()
    for bad in (0, -1, 33):
        assert _pairs(L, P=bad) == -1 and b'1..32' in L.mh_last_error(), bad
    assert _pairs(L, T=1, N=32, F=2 ** 26) == -1 and b'm * F + f' in L.mh_last_error()
    assert _pairs(L, T=2 ** 20, N=2, V=1024) == -1 and b'one launch' in L.mh_last_error()
    for k in range(5):
        ins = [1] * 5
        ins[k] = 0
        assert _pairs(L, ins=ins) == -1 and b'null' in L.mh_last_error(), k
    assert _pairs(L, outs=(0,) * 6) == -1 and b'no output' in L.mh_last_error()
    for bad in (NAN, INF, -INF, -0.01):
        assert _pairs(L, contact=bad) == -1 and b'contact must be finite' in L.mh_last_error(), bad


def test_the_switch_returns_the_previous_setting():
    L = _lib.lib()
    was = L.mh_surface_set_all_faces(1)
    try:
        assert was == 0 and L.mh_surface_set_all_faces(5) == 1 and L.mh_surface_set_all_faces(0) == 1
        assert L.mh_surface_set_all_faces(0) == 0
        assert L.mh_mesh_set_all_faces(0) == 0              # the inside test's switch is another one
    finally:
        L.mh_surface_set_all_faces(was)


def test_optimiser_method_and_module_signatures():
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import contact, surface
    p = inspect.signature(SMPLDepthSequenceOptimizer.clearance_map).parameters
    assert list(p) == ['self', 'frames', 'radius', 'contact', 'nearest', 'chunk']
    assert [p[k].default for k in list(p)[1:]] == [None, 0.1, 0.02, False, 8]
    p = inspect.signature(surface.clearance_map).parameters
    assert list(p) == ['model', 'verts', 'live', 'radius', 'contact', 'nearest', 'chunk']
    assert [p[k].default for k in list(p)[2:]] == [None, 0.1, 0.02, False, 8]
    for fn in (surface.closest_point_on_mesh, surface.signed_distance):
        p = inspect.signature(fn).parameters
        assert list(p) == ['verts', 'faces', 'points', 'radius'] and p['radius'].default == INF
    # the parts are the contact map's, not a copy
    assert surface.PART_NAMES is contact.PART_NAMES and surface.body_parts is contact.body_parts
    assert (surface.NOT_LIVE, surface.NOT_TESTABLE, surface.ALL_FACES) == (1, 2, 4)


def test_python_value_errors():
    """shapes, more than 32 people, the model's V against verts, live's shape, the radius and the contact threshold are
    refused before any device call"""
    import torch
    from mhhip import surface
    V = 12
    model = np.zeros((V, 24), np.float32)                 # skinning weights: every vertex belongs to part 0
    verts = torch.zeros(2, 2, V, 3)
    for bad in (verts[0], torch.zeros(2, 2, V, 2), torch.zeros(2, 0, V, 3)):
        with pytest.raises(ValueError, match='verts'):
            surface.clearance_map(model, bad)
    with pytest.raises(ValueError, match='at most 32'):
        surface.clearance_map(model, torch.zeros(1, 33, V, 3))
    with pytest.raises(ValueError, match='vertices'):
        surface.clearance_map(model, torch.zeros(2, 2, V + 1, 3))
    with pytest.raises(ValueError, match='live'):
        surface.clearance_map(model, verts, live=np.ones((2, 3)))
    for bad in (0.0, -1.0, NAN, INF, 0.65):               # the other maps' cap of 0.64 m
        with pytest.raises(ValueError, match='radius'):
            surface.clearance_map(model, verts, radius=bad)
    for bad in (-0.01, 0.11, NAN):
        with pytest.raises(ValueError, match='contact'):
            surface.clearance_map(model, verts, radius=0.1, contact=bad)
    faces = np.zeros((4, 3), np.int64)
    for fn in (surface.closest_point_on_mesh, surface.signed_distance):
        for bad in (torch.zeros(5), torch.zeros(2, V, 2), torch.zeros(0, 3)):
            with pytest.raises(ValueError, match='verts'):
                fn(bad, faces, torch.zeros(3, 3))
        for bad in (torch.zeros(3), torch.zeros(3, 2), torch.zeros(3, 5, 3)):
            with pytest.raises(ValueError, match='points'):
                fn(torch.zeros(2, V, 3), faces, bad)
        for bad in (0.0, -1.0, NAN, -INF):
            with pytest.raises(ValueError, match='radius'):
                fn(torch.zeros(2, V, 3), faces, torch.zeros(2, 5, 3), radius=bad)
    with pytest.raises(ValueError, match='live'):
        surface.mesh_closest(torch.zeros(2, V, 3), faces, torch.zeros(2, 5, 3), live=[1, 1, 1])
