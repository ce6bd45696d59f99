"""CPU-side checks of the points-inside-mesh boundary: the entry points are declared and exported, bad arguments answer with
the error status and a message before any device call, the workspace size behaves, and the Python signatures are the
documented ones."""
import ctypes
import inspect

import numpy as np
import pytest

from mhhip import _lib

SYMBOLS = ['mh_mesh_bins_bytes', 'mh_mesh_bins', 'mh_mesh_set_all_faces', 'mh_mesh_winding', 'mh_person_inside']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _addr(buf, v):
    return ctypes.addressof(buf) if v else None


def _bins(L, B=6, V=10, F=12, verts=1, faces=1, live=1, ws=1, ws_bytes=None, status=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    if ws_bytes is None:
        ws_bytes = L.mh_mesh_bins_bytes(max(B, 1), max(F, 1))
    return L.mh_mesh_bins(B, V, F, _addr(buf, verts), _addr(buf, faces), _addr(buf, live), _addr(buf, ws), ws_bytes, _addr(buf, status), None)


def test_bins_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V', 'F'):
        for bad in (0, -1):
            assert _bins(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _bins(L, B=2 ** 16, V=2 ** 15, ws_bytes=2 ** 62) == -1 and b'one launch' in L.mh_last_error()        # B V = 2^31
    assert _bins(L, B=2 ** 14, F=2 ** 14, ws_bytes=2 ** 62) == -1 and b'one launch' in L.mh_last_error()        # 8 B F = 2^31
    assert _bins(L, B=2 ** 14, F=2 ** 14, ws_bytes=2 ** 62) == -1 and b'2^31' in L.mh_last_error()
    for name in ('verts', 'faces', 'ws'):
        assert _bins(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    need = L.mh_mesh_bins_bytes(6, 12)
    assert _bins(L, ws_bytes=need - 1) == -1 and b'workspace too small' in L.mh_last_error()
    assert _bins(L, ws_bytes=0) == -1 and b'workspace too small' in L.mh_last_error()


def test_workspace_bytes_are_positive_and_monotone():
    L = _lib.lib()
    base = L.mh_mesh_bins_bytes(32, 13776)
    assert base > 32 * 13776 * (48 + 8 * 4)                 # the face records and the lists of 8 F entries
    assert L.mh_mesh_bins_bytes(1, 1) > 0
    assert L.mh_mesh_bins_bytes(0, 0) > 0 and L.mh_mesh_bins_bytes(-3, -3) > 0
    for B, F in ((33, 13776), (32, 13777), (64, 13776), (32, 20000)):
        assert L.mh_mesh_bins_bytes(B, F) >= base, (B, F)
    assert L.mh_mesh_bins_bytes(64, 13776) > base and L.mh_mesh_bins_bytes(32, 2 * 13776) > base
    # the default chunk of 8 frames of 4 people stays in the tens of MB, 8 frames of 32 people below half a GB
    assert base < 64 << 20 and L.mh_mesh_bins_bytes(256, 13776) < 512 << 20


def _winding(L, B=2, V=10, F=12, faces=1, ws=1, Q=5, points=1, outs=(1, 1, 1)):
    buf = (ctypes.c_float * 64)()
    return L.mh_mesh_winding(B, V, F, _addr(buf, faces), _addr(buf, ws), Q, _addr(buf, points), *[_addr(buf, o) for o in outs], None)


def test_winding_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V', 'F', 'Q'):
        for bad in (0, -1):
            assert _winding(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _winding(L, B=2 ** 16, Q=2 ** 15) == -1 and b'one launch' in L.mh_last_error()
    assert _winding(L, B=2 ** 14, F=2 ** 14) == -1 and b'one launch' in L.mh_last_error()
    for name in ('faces', 'ws', 'points'):
        assert _winding(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    assert _winding(L, outs=(0, 0, 0)) == -1 and b'no output' in L.mh_last_error()


def _inside(L, T=2, N=3, V=10, F=12, faces=1, ws=1, verts=1, part=1, P=24, outs=(1,) * 7):
    buf = (ctypes.c_float * 64)()
    return L.mh_person_inside(T, N, V, F, _addr(buf, faces), _addr(buf, ws), _addr(buf, verts), _addr(buf, part), P,
                              *[_addr(buf, o) for o in outs], None)


def test_person_inside_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('T', 'N', 'V', 'F'):
        for bad in (0, -1):
            assert _inside(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _inside(L, N=33) == -1 and b'at most 32' in L.mh_last_error()
    for bad in (0, -1, 33):
        assert _inside(L, P=bad) == -1 and b'1..32' in L.mh_last_error(), bad
    assert _inside(L, T=2 ** 20, N=2, V=1024) == -1 and b'one launch' in L.mh_last_error()       # T N V = 2^31
    assert _inside(L, T=2 ** 13, N=2, F=2 ** 14) == -1 and b'one launch' in L.mh_last_error()    # 8 T N F = 2^31
    for name in ('faces', 'ws', 'verts', 'part'):
        assert _inside(L, **{name: None}) == -1 and b'null' in L.mh_last_error(), name
    assert _inside(L, outs=(0,) * 7) == -1 and b'no output' in L.mh_last_error()


def test_the_switch_returns_the_previous_setting():
    L = _lib.lib()
    was = L.mh_mesh_set_all_faces(1)
    try:
        assert was == 0 and L.mh_mesh_set_all_faces(5) == 1 and L.mh_mesh_set_all_faces(0) == 1
        assert L.mh_mesh_set_all_faces(0) == 0
    finally:
        L.mh_mesh_set_all_faces(was)


def test_optimiser_method_and_module_signatures():
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import contact, inside
    p = inspect.signature(SMPLDepthSequenceOptimizer.penetration_map).parameters
    assert list(p) == ['self', 'frames', 'chunk'] and (p['frames'].default, p['chunk'].default) == (None, 8)
    p = inspect.signature(inside.penetration_map).parameters
    assert list(p) == ['model', 'verts', 'live', 'chunk'] and (p['live'].default, p['chunk'].default) == (None, 8)
    assert list(inspect.signature(inside.points_inside_mesh).parameters) == ['verts', 'faces', 'points']
    assert list(inspect.signature(inside.mesh_winding).parameters) == ['verts', 'faces', 'points', 'live']
    # the parts are the contact map's, not a copy
    assert inside.PART_NAMES is contact.PART_NAMES and inside.body_parts is contact.body_parts
    assert inside.LATTICE_M == 2.0 ** -16 and (inside.NOT_LIVE, inside.NOT_TESTABLE, inside.ALL_FACES) == (1, 2, 4)


def test_python_value_errors():
    """shapes, more than 32 people, the model's V against verts and live's shape are refused before any device call"""
    import torch
    from mhhip import inside
    V = 12
    model = np.zeros((V, 24), np.float32)                 # skinning weights: every vertex belongs to part 0
    verts = torch.zeros(2, 2, V, 3)
    for bad in (verts[0], torch.zeros(2, 2, V, 2), torch.zeros(2, 0, V, 3)):
        with pytest.raises(ValueError, match='verts'):
            inside.penetration_map(model, bad)
    with pytest.raises(ValueError, match='at most 32'):
        inside.penetration_map(model, torch.zeros(1, 33, V, 3))
    with pytest.raises(ValueError, match='vertices'):
        inside.penetration_map(model, torch.zeros(2, 2, V + 1, 3))
    with pytest.raises(ValueError, match='live'):
        inside.penetration_map(model, verts, live=np.ones((2, 3)))
    faces = np.zeros((4, 3), np.int64)
    for bad in (torch.zeros(5), torch.zeros(2, V, 2), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match='verts'):
            inside.points_inside_mesh(bad, faces, torch.zeros(3, 3))
    for bad in (torch.zeros(3), torch.zeros(3, 2), torch.zeros(3, 5, 3)):
        with pytest.raises(ValueError, match='points'):
            inside.points_inside_mesh(torch.zeros(2, V, 3), faces, bad)
    with pytest.raises(ValueError, match='live'):
        inside.mesh_winding(torch.zeros(2, V, 3), faces, torch.zeros(2, 5, 3), live=[1, 1, 1])
