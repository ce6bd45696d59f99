"""CPU-side checks of the boundary of csrc/mh_image.hip: its 14 entry points are declared and exported, and bad arguments
answer with status -1 and a message before any device call -- null pointers, 0 and 33 people, every non-positive
dimension, an even or non-positive kernel size, aliased erosion buffers, 0 and 9 sums in one launch.  The pointers are
never followed: every call here is refused by the argument check."""
import ctypes

import pytest

from mhhip import _lib

PTR, OPT = 'ptr', 'optional ptr'
# name -> [(argument, PTR | OPT | a good value)]; the stream is always NULL
SPEC = {
    'mh_pack_masks': [('seg', PTR), ('T', 1), ('N', 2), ('H', 4), ('W', 4), ('bits', PTR), ('area', PTR)],
    'mh_erode_bits': [('in', PTR), ('out', PTR), ('T', 1), ('H', 4), ('W', 4)],
    'mh_stage_gates': [('pose2d', PTR), ('area', PTR), ('B', 2), ('thr', 0.5), ('min_area', 3.0), ('pose2d_valid', PTR),
                       ('mask_valid', PTR)],
    'mh_sil_mask_stats': [('bits', PTR), ('T', 1), ('N', 2), ('H', 4), ('W', 4), ('pT', PTR), ('pose2d_valid', PTR),
                          ('mask_valid', PTR), ('front', PTR), ('apply', PTR), ('D', PTR), ('S', PTR)],
    'mh_sil_mask_stats_cached': [('bits', PTR), ('T', 1), ('N', 2), ('H', 4), ('W', 4), ('pT', PTR), ('pose2d_valid', PTR),
                                 ('mask_valid', PTR), ('front', PTR), ('apply', PTR), ('D', PTR), ('S', PTR), ('tag', PTR)],
    'mh_prior_terms': [('T', 1), ('N', 2), ('nbatches', 1), ('poses', PTR), ('poses_ref', PTR), ('valid', PTR), ('betas', PTR),
                       ('betas_ref', PTR), ('xscale', OPT), ('coef_poses', 0.002), ('coef_scales', 1e-4), ('gposes', PTR),
                       ('gbetas', OPT), ('gxscale', OPT), ('body_loss', PTR), ('loss3', PTR)],
    'mh_reduce_sum': [('x', PTR), ('n', 4), ('scale', 1.0), ('out', PTR)],
    'mh_reduce_sum2': [('x0', PTR), ('x1', PTR), ('n', 4), ('scale', 1.0), ('out0', PTR), ('out1', PTR)],
    'mh_avg_depth_loss': [('pred', PTR), ('tru', PTR), ('mask', PTR), ('rows', 2), ('group', 1), ('P', 4), ('eps', 1e-3),
                          ('row_sums', PTR), ('row_loss', PTR)],
    'mh_avg_depth_loss_backward': [('pred', PTR), ('tru', PTR), ('mask', PTR), ('rows', 2), ('group', 1), ('P', 4), ('eps', 1e-3),
                                   ('row_sums', PTR), ('grad_out', 1.0), ('gpred', OPT), ('gtrue_rows', OPT)],
    'mh_masked_mse': [('a', PTR), ('b', PTR), ('mask', PTR), ('n', 4), ('sums2', PTR)],
    'mh_masked_mse_backward': [('a', PTR), ('b', PTR), ('mask', PTR), ('n', 4), ('sums2', PTR), ('grad_out', 1.0), ('ga', PTR)],
    'mh_morph_f32': [('in', PTR), ('out', PTR), ('n_images', 1), ('H', 4), ('W', 4), ('kernel_size', 3), ('dilate', 0)],
}
SYMBOLS = sorted(list(SPEC) + ['mh_reduce_sum_multi'])
# every dimension that must be positive, and the words its refusal carries
POSITIVE = {
    'mh_pack_masks': (('T', 'N', 'H', 'W'), b'32 people'),
    'mh_erode_bits': (('T', 'H', 'W'), b'empty input'),
    'mh_stage_gates': (('B',), b'B must be positive'),
    'mh_sil_mask_stats': (('T', 'N', 'H', 'W'), None),
    'mh_sil_mask_stats_cached': (('T', 'N', 'H', 'W'), None),
    'mh_prior_terms': (('T', 'N', 'nbatches'), b'empty input'),
    'mh_avg_depth_loss': (('rows', 'group', 'P'), b'empty input'),
    'mh_avg_depth_loss_backward': (('rows', 'group', 'P'), b'empty input'),
    'mh_masked_mse': (('n',), b'empty input'),
    'mh_masked_mse_backward': (('n',), b'empty input'),
    'mh_morph_f32': (('n_images', 'H', 'W'), b'bad shape'),
}
UNSIGNED = {'P', 'n'}                                        # size_t: no negative value to hand in

_buf = (ctypes.c_float * 1024)()


def _call(L, name, **over):
    """one call with good arguments but for `over` (a pointer argument: True keeps it, None / False nulls it, an int is
    the index of the 64-byte slot it points to)"""
    args = []
    for i, (arg, kind) in enumerate(SPEC[name]):
        v = over.get(arg, kind)
        if kind in (PTR, OPT):
            if v in (PTR, OPT, True):
                v = ctypes.addressof(_buf) + 64 * i
            elif v is None or v is False:
                v = None
            else:
                v = ctypes.addressof(_buf) + 64 * int(v)
        args.append(v)
    return getattr(L, name)(*(args + [None]))


def _refused(L, rc, words=None):
    assert rc == -1, rc
    msg = L.mh_last_error()
    assert msg.startswith(b'invalid argument'), msg
    if words is not None:
        assert words in msg, msg


@pytest.mark.parametrize('name', SYMBOLS)
def test_header_declares_and_library_exports(name):
    from mhhip import build
    build.build()
    assert name in _lib.declared_symbols()
    assert hasattr(_lib.lib(), name)


def test_the_file_has_no_other_entry_point():
    import os
    import re
    src = open(os.path.join(os.path.dirname(_lib.HERE), 'csrc', 'mh_image.hip')).read()
    assert sorted(re.findall(r'extern "C" int (mh_[a-z0-9_]+)\(', src)) == SYMBOLS and len(SYMBOLS) == 14
    assert len(re.findall(r'__global__', src)) == 13


@pytest.mark.parametrize('name', sorted(SPEC))
def test_null_pointers_are_refused(name):
    L = _lib.lib()
    for arg, kind in SPEC[name]:
        if kind == PTR:
            _refused(L, _call(L, name, **{arg: None}), b'null')
        elif kind == OPT and name == 'mh_prior_terms':
            # optional outputs do not excuse a bad dimension: still refused, for the dimension
            _refused(L, _call(L, name, **{arg: None, 'T': 0}), b'empty input')


@pytest.mark.parametrize('name', sorted(POSITIVE))
def test_non_positive_dimensions_are_refused(name):
    L = _lib.lib()
    dims, words = POSITIVE[name]
    for d in dims:
        for bad in (0,) if d in UNSIGNED else (0, -1, -2 ** 31):
            _refused(L, _call(L, name, **{d: bad}), words)


@pytest.mark.parametrize('name', ['mh_pack_masks', 'mh_sil_mask_stats', 'mh_sil_mask_stats_cached'])
def test_people_per_frame(name):
    L = _lib.lib()
    for bad in (0, 33, -1):
        _refused(L, _call(L, name, N=bad), b'32 people')


@pytest.mark.parametrize('name', ['mh_sil_mask_stats', 'mh_sil_mask_stats_cached'])
def test_an_empty_image_is_refused_by_the_statistics(name):
    L = _lib.lib()
    for d in ('H', 'W'):
        for bad in (0, -3):
            _refused(L, _call(L, name, **{d: bad}), b'empty image')


def test_kernel_sizes():
    L = _lib.lib()
    for bad in (0, -1, -3, 2, 4, 6):
        _refused(L, _call(L, 'mh_morph_f32', kernel_size=bad), b'even kernel')


@pytest.mark.parametrize('name', ['mh_erode_bits', 'mh_morph_f32'])
def test_aliased_buffers_are_refused(name):
    L = _lib.lib()
    _refused(L, _call(L, name, **{'in': 5, 'out': 5}), b'aliased')


def _multi(L, n, xs=True, lens=True, outs=True, null_entry=None):
    m = max(n, 1)
    vp = ctypes.c_void_p
    px = (vp * m)(*[ctypes.addressof(_buf) + 64 * k for k in range(m)])
    po = (vp * m)(*[ctypes.addressof(_buf) + 64 * (16 + k) for k in range(m)])
    pl = (ctypes.c_size_t * m)(*([4] * m))
    if null_entry is not None:
        (px if null_entry[0] == 'x' else po)[null_entry[1]] = None
    return L.mh_reduce_sum_multi(n, px if xs else None, pl if lens else None, po if outs else None, None)


def test_sums_per_launch():
    L = _lib.lib()
    for bad in (0, 9, -1):
        _refused(L, _multi(L, bad), b'1..8 sums')
    for k in ('xs', 'lens', 'outs'):
        _refused(L, _multi(L, 2, **{k: False}), b'null')
    for n in (1, 8):
        _refused(L, _multi(L, n, null_entry=('x', n - 1)), b'null')
        _refused(L, _multi(L, n, null_entry=('o', 0)), b'null')


def test_an_empty_masked_mse_backward_is_refused():
    """it used to reach the launch with an empty grid"""
    L = _lib.lib()
    _refused(L, _call(L, 'mh_masked_mse_backward', n=0), b'empty input')
