"""CPU-side checks of the scene renderer's boundary: ``mh_scene_composite`` is declared and exported, the two Python entry
points have the documented signatures, and the argument check that needs no device answers with a status and a message."""
import ctypes
import inspect

from mhhip import _lib


def test_header_declares_and_library_exports_scene_composite():
    from mhhip import build
    build.build()
    assert 'mh_scene_composite' in _lib.declared_symbols()
    assert hasattr(_lib.lib(), 'mh_scene_composite')


def test_render_scene_signatures():
    from mhhip import raster
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    p = inspect.signature(raster.render_scene).parameters
    assert list(p) == ['model', 'verts', 'cam_K', 'image_size', 'images', 'palette', 'light', 'ambient', 'alpha', 'outputs', 'chunk']
    assert p['images'].default is None and p['palette'].default is None and p['outputs'].default is None
    assert tuple(p['light'].default) == (0, 0, -1) and p['ambient'].default == 0.3 and p['alpha'].default == 0.6
    assert p['chunk'].default == 32
    q = inspect.signature(SMPLDepthSequenceOptimizer.render_scene).parameters
    assert list(q) == ['self', 'frames', 'images', 'kw']
    assert q['frames'].default is None and q['images'].default is True and q['kw'].kind is inspect.Parameter.VAR_KEYWORD


def test_default_palette_does_not_depend_on_the_number_of_people():
    import numpy as np
    from mhhip import raster
    a, b = raster.default_palette(2), raster.default_palette(7)
    assert a.shape == (2, 3) and b.shape == (7, 3) and a.dtype == np.float32
    assert np.array_equal(a, b[:2]) and b.min() >= 0.0 and b.max() <= 1.0
    assert len({tuple(c) for c in b}) == 7


def test_scene_composite_without_outputs_is_an_error_with_a_message():
    """every output NULL: rejected before any HIP call"""
    L = _lib.lib()
    light = (ctypes.c_float * 3)(0.0, 0.0, -1.0)
    rc = L.mh_scene_composite(1, 1, 10, 10, 8, 8, None, None, None, None, None, light, 0.3, 0.6, *([None] * 8))
    assert rc != 0 and b'output' in L.mh_last_error()
