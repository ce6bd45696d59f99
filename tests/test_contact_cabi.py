"""CPU-side checks of the contact map's boundary: the two entry points are declared and exported, and bad arguments answer
with the error status and a message before any device call."""
import ctypes

import pytest

from mhhip import _lib

SYMBOLS = ['mh_scene_nearest', 'mh_contact_parts']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _nearest(L, grid=1, M=100, queries=1, Q=10, radius=0.1, d2=1, near=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    a = lambda v: ctypes.addressof(buf) if v else None
    return L.mh_scene_nearest(a(grid), M, a(queries), Q, radius, a(d2), a(near), None)


def test_nearest_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('Q', 'M'):
        for bad in (0, -1):
            assert _nearest(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _nearest(L, grid=None) == -1 and b'null' in L.mh_last_error()
    assert _nearest(L, queries=None) == -1 and b'null' in L.mh_last_error()
    assert _nearest(L, d2=None, near=None) == -1 and b'no output' in L.mh_last_error()
    for bad in (0.0, -0.1, float('inf'), float('-inf'), float('nan')):
        assert _nearest(L, radius=bad) == -1 and b'finite and positive' in L.mh_last_error(), bad
    # the stated bound: MH_SCENE_NEAREST_MAX_CELLS = 32 cells of the smallest cell, 0.02 m
    assert _nearest(L, radius=0.65) == -1 and b'radius too large' in L.mh_last_error()
    assert _nearest(L, radius=1e6) == -1 and b'radius too large' in L.mh_last_error()
    assert _nearest(L, Q=0x7fffffff) == -1 and b'too many' in L.mh_last_error()


def _parts(L, B=2, V=10, d2=1, part=1, P=24, thr=0.03, counts=1, mins=1):
    buf = (ctypes.c_float * 64)()
    a = lambda v: ctypes.addressof(buf) if v else None
    return L.mh_contact_parts(B, V, a(d2), a(part), P, thr, a(counts), a(mins), None)


def test_parts_argument_errors_answer_with_a_message():
    L = _lib.lib()
    for dim in ('B', 'V'):
        for bad in (0, -1):
            assert _parts(L, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    for bad in (0, -1, 33):
        assert _parts(L, P=bad) == -1 and b'1..32' in L.mh_last_error(), bad
    assert _parts(L, d2=None) == -1 and b'null' in L.mh_last_error()
    assert _parts(L, part=None) == -1 and b'null' in L.mh_last_error()
    assert _parts(L, counts=None, mins=None) == -1 and b'no output' in L.mh_last_error()
    for bad in (-0.01, float('inf'), float('nan')):
        assert _parts(L, thr=bad) == -1 and b'thr' in L.mh_last_error(), bad


def test_optimiser_method_and_module():
    import inspect
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import contact
    p = inspect.signature(SMPLDepthSequenceOptimizer.contact_map).parameters
    assert list(p) == ['self', 'frames', 'radius', 'contact', 'nearest', 'chunk']
    assert (p['radius'].default, p['contact'].default, p['nearest'].default, p['chunk'].default) == (0.1, 0.03, False, 32)
    p = inspect.signature(contact.contact_map).parameters
    assert list(p) == ['model', 'verts', 'scene_points', 'radius', 'contact', 'nearest', 'chunk']
    assert contact.MAX_RADIUS == 0.64
