"""CPU-side checks of the scene-penetration term's boundary: the three entry points are declared and exported, and bad
arguments answer with the error status and a message before any device call."""
import ctypes

import pytest

from mhhip import _lib

SYMBOLS = ['mh_scene_zmap', 'mh_scene_pen_term', 'mh_scene_pen_term_sel']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _term(L, B=1, V=4, H=8, W=8, K=1, verts=1, zmap=1, margin=0.05, band=0.5, edge=0.25, sel=False, zmap1=1, words=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    Kh = (ctypes.c_float * 9)(100, 0, 4, 0, 100, 4, 0, 0, 1)
    a = lambda v: ctypes.addressof(buf) if v else None
    if sel:
        return L.mh_scene_pen_term_sel(B, V, H, W, Kh if K else None, a(verts), a(zmap), a(zmap1), a(words), 1.0, margin, band, edge,
                                       a(1), a(1), a(1), None)
    return L.mh_scene_pen_term(B, V, H, W, Kh if K else None, a(verts), a(zmap), 1.0, margin, band, edge, a(1), a(1), a(1), None)


@pytest.mark.parametrize('sel', [False, True])
def test_term_argument_errors_answer_with_a_message(sel):
    L = _lib.lib()
    for dim in ('B', 'V', 'H', 'W'):
        for bad in (0, -1):
            assert _term(L, sel=sel, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _term(L, sel=sel, band=0.0) == -1 and b'band' in L.mh_last_error()
    assert _term(L, sel=sel, band=-0.5) == -1 and b'band' in L.mh_last_error()
    assert _term(L, sel=sel, edge=0.0) == -1 and b'edge' in L.mh_last_error()
    assert _term(L, sel=sel, margin=-0.05) == -1 and b'margin' in L.mh_last_error()
    assert _term(L, sel=sel, zmap=None) == -1 and b'zmap' in L.mh_last_error()
    assert _term(L, sel=sel, verts=None) == -1 and b'null' in L.mh_last_error()
    assert _term(L, sel=sel, K=None) == -1 and b'null' in L.mh_last_error()
    assert _term(L, sel=sel, band=100.0, V=6890) == -1 and b'fixed-point' in L.mh_last_error()
    if sel:
        assert _term(L, sel=True, zmap1=None) == -1 and b'zmap' in L.mh_last_error()
        assert _term(L, sel=True, words=None) == -1 and b'words' in L.mh_last_error()


def test_zmap_argument_errors_answer_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    assert L.mh_scene_zmap(0, 4, a, a, a, None) == -1 and b'empty input' in L.mh_last_error()
    assert L.mh_scene_zmap(4, -1, a, a, a, None) == -1 and b'empty input' in L.mh_last_error()
    for k in range(3):
        args = [a, a, a]
        args[k] = None
        assert L.mh_scene_zmap(4, 4, *args, None) == -1 and b'null' in L.mh_last_error()


def test_optimiser_keywords_and_sharding():
    """the four keywords are popped from **kargs (the reference's positional signature stays) and a frame-sharded optimiser
    with the term switched on is refused"""
    import inspect
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import sequence
    p = inspect.signature(SMPLDepthSequenceOptimizer.__init__).parameters
    assert 'reg_scene_pen_coef' not in p and list(p)[-1] == 'kargs'
    assert sequence.PEN_DEFAULTS == dict(reg_scene_pen=0.0, scene_pen_margin=0.05, scene_pen_band=0.5, scene_pen_edge=0.25)
    assert 'reg_scene_pen' not in sequence.LOG_KEYS and len(sequence.LOG_KEYS) == 9
    with pytest.raises(ValueError, match='shard'):       # refused before anything touches a device
        SMPLDepthSequenceOptimizer(image_size=(48, 32), num_frames=4, shard_frames=True, reg_scene_pen_coef=1.0)
