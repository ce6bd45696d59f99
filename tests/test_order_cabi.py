"""CPU-side checks of the depth-ordering term's boundary: the two entry points are declared and exported, bad arguments
answer with the error status and a message before any device call, and the optimiser's keywords stay out of the reference's
signature."""
import ctypes

import pytest

from mhhip import _lib

SYMBOLS = ['mh_order_term_keys', 'mh_order_term']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def _term(L, ws_form, T=1, N=2, V=4, F=4, H=8, W=8, win=1, koff=1, keys=1, ws=1, bits=1, ebits=1, gate=1, margin=0.05, delta=0.5,
          outputs=(1, 1, 1, 1), acc=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    a = lambda v: ctypes.addressof(buf) if v else None
    tail = (a(bits), a(ebits), a(gate), 1.0, margin, delta) + tuple(a(o) for o in outputs) + (a(acc), None)
    if ws_form:
        return L.mh_order_term(T, N, V, F, H, W, a(ws), *tail)
    return L.mh_order_term_keys(T, N, F, H, W, a(win), a(koff), a(keys), *tail)


@pytest.mark.parametrize('ws_form', [False, True])
def test_argument_errors_answer_with_a_message(ws_form):
    L = _lib.lib()
    for dim in ('T', 'N', 'F', 'H', 'W') + (('V',) if ws_form else ()):
        for bad in (0, -1):
            assert _term(L, ws_form, **{dim: bad}) == -1 and b'empty input' in L.mh_last_error(), dim
    assert _term(L, ws_form, N=33) == -1 and b'32 people' in L.mh_last_error()
    assert _term(L, ws_form, margin=-0.05) == -1 and b'margin' in L.mh_last_error()
    assert _term(L, ws_form, margin=float('nan')) == -1 and b'margin' in L.mh_last_error()
    assert _term(L, ws_form, delta=0.0) == -1 and b'delta' in L.mh_last_error()
    assert _term(L, ws_form, delta=2000.0) == -1 and b'delta' in L.mh_last_error()
    assert _term(L, ws_form, N=32, H=4096, W=4096) == -1 and b'fixed-point' in L.mh_last_error()
    assert b'2^61' in L.mh_last_error()
    assert _term(L, ws_form, T=65536) == -1 and b'frames' in L.mh_last_error()      # the composite's limits
    assert _term(L, ws_form, N=1, H=4096, W=8) == -1 and b'image larger' in L.mh_last_error()
    assert _term(L, ws_form, N=1, H=8, W=65536) == -1 and b'image larger' in L.mh_last_error()
    for table in (('ws',) if ws_form else ('win', 'koff', 'keys')) + ('bits', 'ebits'):
        assert _term(L, ws_form, **{table: None}) == -1 and b'null' in L.mh_last_error(), table
    assert _term(L, ws_form, outputs=(0, 0, 0, 0)) == -1 and b'no output' in L.mh_last_error()


def test_optimiser_keywords_defaults_and_sharding():
    """the three keywords are popped from **kargs (the reference's positional signature stays), the defaults have a dict and
    a log slot of their own, and a frame-sharded optimiser with the term switched on is refused"""
    import inspect
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import sequence
    p = inspect.signature(SMPLDepthSequenceOptimizer.__init__).parameters
    for k in ('reg_order_coef', 'order_margin', 'order_delta'):
        assert k not in p
    assert list(p)[-1] == 'kargs'
    assert sequence.ORDER_DEFAULTS == dict(reg_order=0.0, order_margin=0.05, order_delta=0.5)
    assert sequence.ORDER_LOG == 13 and sequence.PEN_LOG == 12
    assert sequence.PEN_DEFAULTS == dict(reg_scene_pen=0.0, scene_pen_margin=0.05, scene_pen_band=0.5, scene_pen_edge=0.25)
    assert 'reg_order' not in sequence.LOG_KEYS and len(sequence.LOG_KEYS) == 9
    with pytest.raises(ValueError, match='shard'):       # refused before anything touches a device
        SMPLDepthSequenceOptimizer(image_size=(48, 32), num_frames=4, shard_frames=True, reg_order_coef=1.0)
