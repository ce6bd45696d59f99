"""CPU-side checks of the fit report's boundary: both kernels' entry points are declared and exported, the two Python entry
points have the documented signatures, and the argument errors answer with a status and a message before any device call."""
import ctypes
import inspect

import pytest

from mhhip import _lib

SYMBOLS = ['mh_fit_report_pixels', 'mh_fit_report_verts']


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def test_fit_report_signatures():
    from mhhip import report
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    p = inspect.signature(report.fit_report).parameters
    assert list(p) == ['model', 'verts', 'cam_K', 'image_size', 'bits', 'disp', 'min_z', 'max_z', 'scene_depth', 'scene_mask',
                       'scene_points', 'joints', 'pose2d', 'cam_dist_coef', 'joint_confidence_thr', 'verts_prev', 'has_prev', 'margin',
                       'depth_offset', 'chunk']
    assert all(p[k].default is None for k in list(p)[4:14] + ['verts_prev', 'has_prev'])
    assert p['joint_confidence_thr'].default == 0.5 and p['margin'].default == 0.05 and p['depth_offset'].default == 0.2
    assert p['chunk'].default == 32
    q = inspect.signature(SMPLDepthSequenceOptimizer.fit_report).parameters
    assert list(q) == ['self', 'frames', 'margin', 'chunk']
    assert q['frames'].default is None and q['margin'].default == 0.05 and q['chunk'].default == 32
    assert len(report.COLUMNS) == 14 and len(set(report.COLUMNS)) == 14


def _pixels(L, N=1, person=1, depth=1, bits=1, disp=None, min_z=None, max_z=None, scene_depth=None, scene_mask=None, counts=1, dsum=1):
    """the pointers are never followed: every case here is refused by the argument check"""
    buf = (ctypes.c_float * 64)()
    a = lambda v: ctypes.addressof(buf) if v else None
    return L.mh_fit_report_pixels(1, N, 2, 2, a(person), a(depth), a(bits), a(disp), a(min_z), a(max_z), a(scene_depth), a(scene_mask),
                                  0.2, 0.05, a(counts), a(dsum), None)


def test_pixel_argument_errors_answer_with_a_message():
    L = _lib.lib()
    assert _pixels(L, N=33) != 0 and b'32 people' in L.mh_last_error()
    assert _pixels(L, counts=None, dsum=None) != 0 and b'output' in L.mh_last_error()
    assert _pixels(L, disp=1, min_z=1) != 0 and b'min_z or max_z' in L.mh_last_error()
    assert _pixels(L, disp=1, max_z=1) != 0 and b'min_z or max_z' in L.mh_last_error()
    assert _pixels(L, scene_depth=1) != 0 and b'only one of' in L.mh_last_error()
    assert _pixels(L, scene_mask=1) != 0 and b'only one of' in L.mh_last_error()


def test_vertex_argument_errors_answer_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    K = (ctypes.c_float * 9)(100, 0, 4, 0, 100, 4, 0, 0, 1)
    a = ctypes.addressof(buf)
    assert L.mh_fit_report_verts(1, 4, 8, 8, K, a, a, a, 0.05, None, None, None) != 0 and b'output' in L.mh_last_error()
    assert L.mh_fit_report_verts(1, 4, 8, 8, K, a, None, a, 0.05, a, a, None) != 0 and b'null' in L.mh_last_error()
    assert L.mh_fit_report_verts(1, 4, 8, 8, K, a, a, a, -0.05, a, a, None) != 0 and b'margin' in L.mh_last_error()
