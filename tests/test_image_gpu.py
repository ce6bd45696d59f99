"""The image-space kernels of csrc/mh_image.hip through the C ABI (and the stand-alone losses / morphology also through
mhmocap.losses / mhmocap.morphology) on the cases of tests/image_cases.py, against references that share none of the
kernels' tricks.  Output buffers start as NaN or 0xA5 bytes: an element nobody writes shows.  Integer results are
compared exactly, and no pixel, body or case is left out.

  pack        N = 1, 5, 31, 32 (bit 31); values 0, the float below 0.5, 0.5, 0.7; 1x1, 1x37, 37x1; 130x127 beyond the 64
              workgroups; two slab calls equal one; the area is overwritten
  erode       the same images and 2x2, all ones, 182x181 beyond the 128 workgroups; one and two passes against the
              per-plane reference and against mh_morph_f32
  morph       k = 1, 3, 5, 7, erosion and dilation, images smaller than the window, leading dimensions (2,3,H,W); against
              the reference-generated fixture and the numpy reference
  gates       B = 1, 255, 256, 257; exactly one and exactly two joints at the threshold; thr = 0.5 and float32(0.3);
              area at and one pixel below min_area
  statistics  both forms at N = 1 .. 32 on both sides of every instantiation, T = 1 .. 2048 with 8 | 4 | 1 parts on 15
              pixels, ties, -0.0 / +0.0, +inf, gates with zeros; the cached form over a sequence of translations with a
              sentinel in D and S, changing gates and a zeroed tag
  priors      (T,N) = (1,1) .. (2,32), 1 and 3 batches, xscale zero / NULL / 1e-3 / large, NULL leaves, coef_scales = 0;
              gposes and gbetas bit for bit the float32 products, the rest against float64
  sums        n = 0 .. 65537 with cancellation against math.fsum within (ceil(n/256) + 9) * 2^-24 * sum|x|; the two- and
              eight-array forms bit for bit mh_reduce_sum; two runs bit-identical
  losses      the fixture's cases with the gradients of both arguments, P = 1, 255, 257 with group 1 and N, n = 1, 1023,
              1025: values within 2e-5, gradients within 2e-4 of the float64 reference, relative to the sum of the
              magnitudes of the terms where they cancel

Allowance of body_loss, the scale terms and gxscale: 4 times the error of the float32 numpy evaluation of the same
formula on the same cases (tests/test_image_cases.py prints it).  Each test prints its own worst figure (-s).

Measured on an MI355X (worst over the cases): every integer output equal; priors 0.24 of the allowance for body_loss
(relative error 1.3e-7 of 4 x 1.35e-7), 0.40 for the scale terms and 0.25 for gxscale, gposes and gbetas bit for bit; sums
2.0e-4 of a bound of 2.3 at n = 65537 and 2.1e-5 of 4.5e-4 at n = 257; depth loss 5.3e-8 (bound 2e-5) with gradients
1.4e-7 (2e-4); masked MSE 1.7e-7 with gradients 1.9e-7, the second argument's included.  The slowest test takes 0.3 s.

Seven deliberate changes of the kernels, each run once against this file: the tie rule without the index tie-break fails
16 tests (every statistics test with more than one person), apply indexed by the person instead of the rank the same 16,
<4> launched for N <= 8 fails 2 (N = 5 and 8), out-of-image neighbours counted as background in k_erode_bits fails 4
(every erosion test), c >= 1 in k_gates fails 6 (every B that has a body with exactly one joint at the threshold),
nbatches dropped from gxscale fails 4 (every priors shape), > for >= in the clamp of k_depth_loss_grads fails 5 (the
module test and the four row cases with room for a pixel at eps).  On the parent's losses.py the masked-MSE module test
fails in the second argument's gradient (None).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
import image_cases as ic

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = np.uint32(0xA5A5A5A5)


@pytest.fixture(scope='module')
def golden_image():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_image_cpu.npz'), allow_pickle=False)


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.tensor(a, device=DEV)


def _nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def _a5(*shape):
    """int32 words of 0xA5 bytes"""
    n = int(np.prod(shape))
    return torch.full((n * 4,), 0xA5, dtype=torch.uint8, device=DEV).view(torch.int32).view(*shape)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _close(got, want, scale, rtol, what):
    """|got - want| <= rtol * scale everywhere (scale = the magnitude the error is relative to; where it is 0 the value
    has to be exact) -> worst error / scale"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what + ': an element was not written'
    err = np.abs(got - want)
    worst = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    assert (err[scale == 0] == 0).all(), what + ': not exact where the reference is exact'
    assert worst <= rtol, '%s: worst error / scale %.3e above %.1e' % (what, worst, rtol)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------
def _pack(seg, bits=None, area=None):
    L, check, ptr, st = _api()
    T, N, H, W = seg.shape
    bits = _a5(T, H, W) if bits is None else bits
    area = _nan(T, N) if area is None else area
    tseg = _dev(seg)                                  # (every input stays referenced until the kernel has run)
    check(L.mh_pack_masks(ptr(tseg), T, N, H, W, ptr(bits), ptr(area), st))
    torch.cuda.synchronize()
    return bits, area


@pytest.mark.parametrize('N', ic.PACK_PEOPLE)
def test_pack_small_images(N):
    for H, W in ic.PACK_IMAGES:
        seg = ic.pack_input(2, N, H, W)
        bits, area = _pack(seg)
        want_bits, want_area = ic.pack_reference(seg)
        np.testing.assert_array_equal(_u32(bits), want_bits, err_msg='N=%d %dx%d' % (N, H, W))
        np.testing.assert_array_equal(area.cpu().numpy(), want_area, err_msg='N=%d %dx%d' % (N, H, W))


def test_pack_beyond_the_grid_cap():
    T, N, H, W = ic.PACK_LARGE
    seg = ic.pack_input(T, N, H, W)
    bits, area = _pack(seg)
    want_bits, want_area = ic.pack_reference(seg)
    np.testing.assert_array_equal(_u32(bits), want_bits)
    np.testing.assert_array_equal(area.cpu().numpy(), want_area)
    assert (want_bits >> np.uint32(31)).any()


def test_pack_in_slabs_and_twice():
    """two slab calls on slices of bits and area (sequence.py:253-257) equal one call; a second call overwrites the area"""
    T, N, H, W = 5, 5, 21, 30
    seg = ic.pack_input(T, N, H, W, binary=True)
    want_bits, want_area = ic.pack_reference(seg)
    np.testing.assert_array_equal(want_area, seg.sum((2, 3)))
    bits, area = _a5(T, H, W), _nan(T, N)
    for lo, hi in ((0, 2), (2, 5)):
        _pack(seg[lo:hi], bits[lo:hi], area[lo:hi])
    np.testing.assert_array_equal(_u32(bits), want_bits)
    np.testing.assert_array_equal(area.cpu().numpy(), want_area)
    _pack(seg, bits, area)
    _pack(seg, bits, area)
    np.testing.assert_array_equal(_u32(bits), want_bits)
    np.testing.assert_array_equal(area.cpu().numpy(), want_area)


# ---------------------------------------------------------------------------------------------------------------
# erode, morph
# ---------------------------------------------------------------------------------------------------------------
def _erode(bits, passes):
    L, check, ptr, st = _api()
    T, H, W = bits.shape
    src = _dev(bits)
    for _ in range(passes):
        out = _a5(T, H, W)
        check(L.mh_erode_bits(ptr(src), ptr(out), T, H, W, st))
        src = out
    torch.cuda.synchronize()
    return _u32(src)


def _morph(x, k, dilate):
    L, check, ptr, st = _api()
    x = np.ascontiguousarray(x, np.float32)
    H, W = x.shape[-2:]
    out, tx = _nan(*x.shape), _dev(x)
    check(L.mh_morph_f32(ptr(tx), ptr(out), x.size // (H * W), H, W, k, int(dilate), st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _erode_everything(seg, tag):
    N = seg.shape[1]
    bits = ic.pack_reference(seg)[0]
    one = _erode(bits, 1)
    two = _erode(bits, 2)
    np.testing.assert_array_equal(one, ic.erode_bits_reference(bits, N, 1), err_msg=tag)
    np.testing.assert_array_equal(two, ic.erode_bits_reference(bits, N, 2), err_msg=tag)
    # the float form on the same planes
    f1 = _morph((seg >= 0.5).astype(np.float32), 3, False)
    np.testing.assert_array_equal(ic.planes(one, N), f1, err_msg=tag)
    np.testing.assert_array_equal(ic.planes(two, N), _morph(f1, 3, False), err_msg=tag)
    return two


@pytest.mark.parametrize('N', (1, 5, 32))
def test_erode_small_images(N):
    for H, W in ic.ERODE_IMAGES:
        _erode_everything(ic.pack_input(2, N, H, W), 'N=%d %dx%d' % (N, H, W))
        _erode_everything(ic.erode_input(2, N, H, W), 'dense N=%d %dx%d' % (N, H, W))
        full = np.full((2, H, W), np.uint32(2 ** N - 1), np.uint32)
        np.testing.assert_array_equal(_erode(full, 1), full)            # pixels outside the image are not background
        np.testing.assert_array_equal(_erode(full, 2), full)


def test_erode_beyond_the_grid_cap():
    T, N, H, W = ic.ERODE_LARGE
    two = _erode_everything(ic.erode_input(T, N, H, W), '%dx%d' % (H, W))
    share = ic.planes(two, N).mean()
    assert 0.1 < share < 0.5, share


@pytest.mark.parametrize('k', ic.MORPH_KSIZES)
def test_morph_against_the_numpy_reference(k):
    for H, W in ic.MORPH_IMAGES + ((1, 37), (37, 1), (21, 30)):
        x = ic.morph_input(H, W)
        assert x.shape == (2, 3, H, W)
        for dilate in (False, True):
            np.testing.assert_array_equal(_morph(x, k, dilate), ic.morph_reference(x, k, dilate), err_msg='k=%d %dx%d dilate=%d' % (k, H, W, dilate))


def test_morphology_modules_against_the_fixture(golden_image):
    from mhmocap.morphology import Dilate2D, Erode2D
    for (H, W), x in gi.image_morph_inputs().items():
        tx = _dev(x)
        for k in ic.MORPH_KSIZES:
            np.testing.assert_array_equal(Erode2D(kernel_size=k)(tx).cpu().numpy(), golden_image['erode_%dx%d_k%d' % (H, W, k)])
            np.testing.assert_array_equal(Dilate2D(kernel_size=k)(tx).cpu().numpy(), golden_image['dilate_%dx%d_k%d' % (H, W, k)])
        np.testing.assert_array_equal(Erode2D()(tx).cpu().numpy(), golden_image['erode_%dx%d_k5' % (H, W)])        # the default is 5
        np.testing.assert_array_equal(Dilate2D()(tx).cpu().numpy(), golden_image['dilate_%dx%d_k5' % (H, W)])
    x = ic.morph_input(6, 9)                                       # leading dimensions (2,3,H,W) through the module
    np.testing.assert_array_equal(Erode2D(5)(_dev(x)).cpu().numpy(), ic.morph_reference(x, 5, False))


# ---------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', ic.GATE_THRESHOLDS)
@pytest.mark.parametrize('B', ic.GATE_BODIES)
def test_gates(B, thr):
    L, check, ptr, st = _api()
    pose2d, area, t, min_area = ic.gates_case(B, thr)
    p2d, mv = _nan(B), _nan(B)
    tpose, tarea = _dev(pose2d), _dev(area)
    check(L.mh_stage_gates(ptr(tpose), ptr(tarea), B, t, min_area, ptr(p2d), ptr(mv), st))
    torch.cuda.synchronize()
    want_p2d, want_mv = ic.gates_reference(pose2d, area, t, min_area)
    np.testing.assert_array_equal(p2d.cpu().numpy(), want_p2d)
    np.testing.assert_array_equal(mv.cpu().numpy(), want_mv)


# ---------------------------------------------------------------------------------------------------------------
# silhouette statistics
# ---------------------------------------------------------------------------------------------------------------
def _pT(z):
    pT = np.random.RandomState(0).randn(z.shape[0], z.shape[1], 3).astype(np.float32)
    pT[..., 2] = z
    return pT


def _sil_plain(bits, z, p2d, mv, H, W):
    L, check, ptr, st = _api()
    T, N = z.shape
    front, apply, D, S = _a5(T, N), _nan(T, N), _nan(T, N), _nan(T, N)
    tbits, tpT, tp2d, tmv = _dev(bits), _dev(_pT(z)), _dev(p2d), _dev(mv)
    check(L.mh_sil_mask_stats(ptr(tbits), T, N, H, W, ptr(tpT), ptr(tp2d), ptr(tmv), ptr(front), ptr(apply), ptr(D), ptr(S), st))
    torch.cuda.synchronize()
    return ic.SilRef(_u32(front), apply.cpu().numpy(), D.cpu().numpy(), S.cpu().numpy())


class _Cached(object):
    """the arrays that persist between calls of the cached form"""

    def __init__(self, bits, T, N, H, W):
        self.bits, self.shape = _dev(bits), (T, N, H, W)
        self.front, self.apply, self.D, self.S = _a5(T, N), _nan(T, N), _nan(T, N), _nan(T, N)
        self.tag = torch.zeros(T, dtype=torch.int32, device=DEV)

    def __call__(self, z, p2d, mv):
        L, check, ptr, st = _api()
        T, N, H, W = self.shape
        tpT, tp2d, tmv = _dev(_pT(z)), _dev(p2d), _dev(mv)
        check(L.mh_sil_mask_stats_cached(ptr(self.bits), T, N, H, W, ptr(tpT), ptr(tp2d), ptr(tmv), ptr(self.front),
                                         ptr(self.apply), ptr(self.D), ptr(self.S), ptr(self.tag), st))
        torch.cuda.synchronize()
        return ic.SilRef(_u32(self.front), self.apply.cpu().numpy(), self.D.cpu().numpy(), self.S.cpu().numpy())


def _same(got, want, tag):
    for name, g, w in zip(ic.SilRef._fields, got, want):
        np.testing.assert_array_equal(g, w, err_msg='%s: %s' % (tag, name))


@pytest.mark.parametrize('N', ic.SIL_PEOPLE)
def test_statistics_at_every_instantiation(N):
    T, H, W = ic.SIL_PEOPLE_SHAPE
    for kind in ic.SIL_ORDERINGS:
        c = ic.sil_case(T, N, H, W, kind)
        want = ic.sil_case_reference(T, N, H, W, kind)
        _same(_sil_plain(c.bits, c.z, c.p2d_valid, c.mask_valid, H, W), want, 'plain N=%d %s' % (N, kind))
        _same(_Cached(c.bits, T, N, H, W)(c.z, c.p2d_valid, c.mask_valid), want, 'cached N=%d %s' % (N, kind))


@pytest.mark.parametrize('T', ic.SIL_FRAMES)
def test_statistics_at_every_split(T):
    N, H, W = ic.SIL_FRAMES_SHAPE
    for kind in ('random', 'all_equal', 'zeros', 'inf'):
        c = ic.sil_case(T, N, H, W, kind)
        want = ic.sil_case_reference(T, N, H, W, kind)
        _same(_sil_plain(c.bits, c.z, c.p2d_valid, c.mask_valid, H, W), want, 'plain T=%d %s' % (T, kind))
        _same(_Cached(c.bits, T, N, H, W)(c.z, c.p2d_valid, c.mask_valid), want, 'cached T=%d %s' % (T, kind))


@pytest.mark.parametrize('N', (4, 9, 17))
def test_cached_statistics_over_a_sequence_of_translations(N):
    """against the reference at every step.  After the first call D and S are overwritten with a sentinel: it survives in
    the frames whose ordering has not changed since (the pixel pass was skipped), while apply follows gates that change at
    every step; a frame whose tag is zeroed is counted again."""
    T, H, W = 7, 17, 19
    rng = np.random.RandomState(50 + N)
    c = ic.sil_case(T, N, H, W, 'random')
    z = c.z.copy()
    cached = _Cached(c.bits, T, N, H, W)
    want = ic.sil_reference(c.seg, z, c.p2d_valid, c.mask_valid)
    _same(cached(z, c.p2d_valid, c.mask_valid), want, 'first call')
    assert int(cached.tag.sum()) == T
    cached.D.fill_(-7.0)
    cached.S.fill_(-7.0)
    expect_D, expect_S = np.full((T, N), -7.0, np.float32), np.full((T, N), -7.0, np.float32)
    prev_front = want.front
    kept = recounted = 0
    for step in range(1, 10):
        if step % 3 == 1:                                         # the even frames move, the odd ones stay
            z[::2] += (rng.randn(*z[::2].shape) * 0.6).astype(np.float32)
        if step == 5:
            z[0, 1] = z[0, 0]                                     # a tie: the lower index is in front
        if step == 8:
            cached.tag[3] = 0                                     # an odd frame: its ordering never changed
        p2d = (rng.rand(T, N) > 0.3).astype(np.float32)
        mv = (rng.rand(T, N) > 0.3).astype(np.float32)
        want = ic.sil_reference(c.seg, z, p2d, mv)
        changed = (want.front != prev_front).any(axis=1)
        if step == 8:
            changed[3] = True
        expect_D[changed], expect_S[changed] = want.D[changed], want.S[changed]
        got = cached(z, p2d, mv)
        np.testing.assert_array_equal(got.front, want.front, err_msg='step %d' % step)
        np.testing.assert_array_equal(got.apply, want.apply, err_msg='step %d' % step)
        np.testing.assert_array_equal(got.D, expect_D, err_msg='step %d' % step)
        np.testing.assert_array_equal(got.S, expect_S, err_msg='step %d' % step)
        recounted += int(changed.sum())
        kept += int((~changed).sum())
        prev_front = want.front
    assert (expect_D[1] == -7).all() and (expect_D[5] == -7).all() and (expect_D[3] == want.D[3]).all()     # odd frames: only the re-tagged one
    assert recounted >= 4 and kept > recounted
    assert int(cached.tag.sum()) == T


# ---------------------------------------------------------------------------------------------------------------
# priors
# ---------------------------------------------------------------------------------------------------------------
def _priors(c, with_gbetas=True, with_gxscale=True):
    L, check, ptr, st = _api()
    gposes, gbetas, gxscale = _dev(c.gposes0), _dev(c.gbetas0), _dev(c.gxscale0)
    body, loss3 = _nan(c.T, c.N), _nan(3)
    xs = None if c.xscale is None else _dev(c.xscale)
    poses, ref, valid, betas, betas_ref = (_dev(a) for a in (c.poses, c.ref, c.valid, c.betas, c.betas_ref))
    check(L.mh_prior_terms(c.T, c.N, c.nbatches, ptr(poses), ptr(ref), ptr(valid), ptr(betas),
                           ptr(betas_ref), ptr(xs), c.cp, c.cs, ptr(gposes), ptr(gbetas) if with_gbetas else None,
                           ptr(gxscale) if with_gxscale else None, ptr(body), ptr(loss3), st))
    torch.cuda.synchronize()
    return ic.PriorRef(body.cpu().numpy(), loss3.cpu().numpy(), gposes.cpu().numpy(), gbetas.cpu().numpy(), gxscale.cpu().numpy())


@pytest.mark.parametrize('T,N', ic.PRIOR_SHAPES)
def test_priors(T, N):
    y = ic.prior_yardstick()
    worst = {}
    for nb in ic.PRIOR_BATCHES:
        for xk in ic.PRIOR_XSCALE:
            c = ic.prior_case(T, N, nb, xk)
            tag = 'T=%d N=%d nbatches=%d xscale %s' % (T, N, nb, xk)
            got = _priors(c)
            want, f32 = ic.prior_reference(c), ic.prior_float32(c)
            assert np.isfinite(got.body_loss).all() and np.isfinite(got.loss3).all(), tag
            np.testing.assert_array_equal(got.gposes.view(np.uint32), f32.gposes.view(np.uint32), err_msg=tag + ' gposes')
            np.testing.assert_array_equal(got.gbetas.view(np.uint32), f32.gbetas.view(np.uint32), err_msg=tag + ' gbetas')
            assert abs(float(got.loss3[0]) - want.loss3[0]) <= ic.LOSS_RTOL * abs(want.loss3[0]), tag + ' shape term'
            for group, e in ic.prior_errors(c, got, want).items():
                allow = 4 * y[(group, xk) if group != 'body_loss' else (group, None)]
                print('%s %-12s error %.3e, allowance %.3e' % (tag, group, e, allow))
                assert e <= allow, '%s %s: error %.3e above 4 x the float32 numpy evaluation (%.3e)' % (tag, group, e, allow)
                worst[group] = max(worst.get(group, 0.0), e / allow if allow else 0.0)
    print('T=%d N=%d: worst error / allowance %s' % (T, N, worst))


def test_priors_with_null_leaves_and_the_scale_switch():
    c = ic.prior_case(5, 9, 3, 'large')
    f32 = ic.prior_float32(c)
    full = _priors(c)
    got = _priors(c, with_gbetas=False, with_gxscale=False)
    np.testing.assert_array_equal(got.gbetas, c.gbetas0)                      # not handed in: untouched
    np.testing.assert_array_equal(got.gxscale, c.gxscale0)
    np.testing.assert_array_equal(got.gposes.view(np.uint32), f32.gposes.view(np.uint32))
    np.testing.assert_array_equal(got.body_loss.view(np.uint32), full.body_loss.view(np.uint32))
    np.testing.assert_array_equal(got.loss3.view(np.uint32), full.loss3.view(np.uint32))
    # coef_scales = 0: the (coef > 0) switch is off, nothing is added to gxscale; the logged terms do not depend on it
    c0 = ic.prior_case(5, 9, 3, 'large', cs=0.0)
    got0 = _priors(c0)
    np.testing.assert_array_equal(got0.gxscale, c0.gxscale0)
    np.testing.assert_array_equal(got0.loss3.view(np.uint32), full.loss3.view(np.uint32))
    np.testing.assert_array_equal(got0.gposes.view(np.uint32), f32.gposes.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------
def _sum1(x, scale=1.0):
    L, check, ptr, st = _api()
    tx = _dev(x) if len(x) else torch.zeros(1, device=DEV)                    # n = 0 still needs a pointer
    out = _nan(1)
    check(L.mh_reduce_sum(ptr(tx), len(x), scale, ptr(out), st))
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


@pytest.mark.parametrize('n', ic.SUM_LENGTHS)
def test_sum_within_its_bound(n):
    x = ic.sum_input(n)
    got = _sum1(x)
    want, bound = ic.sum_reference(x), ic.sum_bound(x)
    print('n = %d: error %.3e, bound %.3e' % (n, abs(float(got) - want), bound))
    assert np.isfinite(got) and abs(float(got) - want) <= bound
    assert _sum1(x).view(np.uint32) == got.view(np.uint32)                    # two runs: the same bits
    half = _sum1(x, 0.5)
    assert half == np.float32(0.5) * got                                      # the scale is applied to the finished sum


def test_sum_forms_agree_bit_for_bit():
    from mhhip import _lib
    L, check, ptr, st = _api()
    lens = (65537, 0, 1, 255, 256, 257, 1000, 3)
    xs = [ic.sum_input(n, seed=k) for k, n in enumerate(lens)]
    single = [_sum1(x) for x in xs]
    for count in (1, 8):
        tx = [_dev(x) if len(x) else torch.zeros(1, device=DEV) for x in xs[:count]]
        outs = [_nan(1) for _ in range(count)]
        vp = ctypes.c_void_p
        check(L.mh_reduce_sum_multi(count, (vp * count)(*[t.data_ptr() for t in tx]), (ctypes.c_size_t * count)(*lens[:count]),
                                    (vp * count)(*[o.data_ptr() for o in outs]), st))
        torch.cuda.synchronize()
        for k in range(count):
            assert outs[k].cpu().numpy()[0].view(np.uint32) == single[k].view(np.uint32), (count, k)
    for n in (0, 1, 257, 65537):
        a, b = ic.sum_input(n, seed=1), ic.sum_input(n, seed=2)
        ta, tb = (_dev(v) if n else torch.zeros(1, device=DEV) for v in (a, b))
        o0, o1 = _nan(1), _nan(1)
        check(L.mh_reduce_sum2(ptr(ta), ptr(tb), n, 1.0, ptr(o0), ptr(o1), st))
        torch.cuda.synchronize()
        assert o0.cpu().numpy()[0].view(np.uint32) == _sum1(a).view(np.uint32), n
        assert o1.cpu().numpy()[0].view(np.uint32) == _sum1(b).view(np.uint32), n
    # the helper the engine logs through
    items = [(_dev(xs[3]), _nan(1)), (_dev(xs[5]), _nan(1))]
    _lib.reduce_sum_multi(items, st)
    torch.cuda.synchronize()
    assert items[0][1].cpu().numpy()[0].view(np.uint32) == single[3].view(np.uint32)
    assert items[1][1].cpu().numpy()[0].view(np.uint32) == single[5].view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------
def test_depth_loss_module_on_the_fixture_cases(golden_image):
    from mhmocap.losses import build_avg_depth_loss_fn
    for name, (pred, true, mask) in gi.image_depth_loss_cases().items():
        r = ic.depth_reference(pred, true, mask)
        tp, tt = _dev(pred).requires_grad_(True), _dev(true).requires_grad_(True)
        l = build_avg_depth_loss_fn()(tp, tt, _dev(mask))
        l.backward()
        w = [_close(float(l.detach()), r.loss, r.loss_scale, ic.LOSS_RTOL, name),
             _close(tp.grad.cpu().numpy(), r.gpred, r.gpred_scale, ic.GRAD_RTOL, name + ' gpred'),
             _close(tt.grad.cpu().numpy(), r.gtrue, r.gtrue_scale, ic.GRAD_RTOL, name + ' gtrue')]
        # and the reference's own float32 numbers, each side within its tolerance of float64
        _close(float(l.detach()), float(golden_image['depth_' + name]), r.loss_scale, 2 * ic.LOSS_RTOL, name + ' fixture')
        _close(tp.grad.cpu().numpy(), golden_image['depth_%s_gpred' % name], r.gpred_scale, 2 * ic.GRAD_RTOL, name + ' gpred fixture')
        _close(tt.grad.cpu().numpy(), golden_image['depth_%s_gtrue' % name], r.gtrue_scale, 2 * ic.GRAD_RTOL, name + ' gtrue fixture')
        print('depth %-9s loss %.2e of 2e-5, gpred %.2e, gtrue %.2e of 2e-4' % (name, w[0], w[1], w[2]))
    # only the first argument's gradient asked for, and an upstream gradient that is not 1
    pred, true, mask = gi.image_depth_loss_cases()['t1_m3']
    r = ic.depth_reference(pred, true, mask)
    tp, tt = _dev(pred).requires_grad_(True), _dev(true)
    (0.5 * build_avg_depth_loss_fn()(tp, tt, _dev(mask))).backward()
    _close(tp.grad.cpu().numpy(), 0.5 * r.gpred, 0.5 * r.gpred_scale, ic.GRAD_RTOL, 'half gpred')
    assert tt.grad is None
    with pytest.raises(ValueError, match='mask'):
        build_avg_depth_loss_fn()(tp, tt, _dev(mask).requires_grad_(True))


def test_masked_mse_module_on_the_fixture_cases(golden_image):
    from mhmocap.losses import build_masked_mse_loss_fn
    for name, (y1, y2, mask) in gi.image_mse_cases().items():
        r = ic.mse_reference(y1, y2, mask)
        t1, t2 = _dev(y1).requires_grad_(True), _dev(y2).requires_grad_(True)
        l = build_masked_mse_loss_fn()(t1, t2, _dev(mask))
        l.backward()
        assert t2.grad is not None, 'the second argument has no gradient'
        assert tuple(t2.grad.shape) == y2.shape and tuple(t1.grad.shape) == y1.shape
        w = [_close(float(l.detach()), r.loss, abs(r.loss), ic.LOSS_RTOL, name),
             _close(t1.grad.cpu().numpy(), r.g1, np.abs(r.g1), ic.GRAD_RTOL, name + ' g1'),
             _close(t2.grad.cpu().numpy(), r.g2, r.g2_scale, ic.GRAD_RTOL, name + ' g2')]
        _close(float(l.detach()), float(golden_image['mse_' + name]), abs(r.loss), 2 * ic.LOSS_RTOL, name + ' fixture')
        _close(t2.grad.cpu().numpy(), golden_image['mse_%s_g2' % name], r.g2_scale, 2 * ic.GRAD_RTOL, name + ' g2 fixture')
        print('mse %-9s loss %.2e of 2e-5, g1 %.2e, g2 %.2e of 2e-4' % (name, w[0], w[1], w[2]))
    y1, y2, mask = gi.image_mse_cases()['broadcast']
    r = ic.mse_reference(y1, y2, mask)
    t1, t2 = _dev(y1), _dev(y2).requires_grad_(True)                      # the second argument alone
    (2.0 * build_masked_mse_loss_fn()(t1, t2, _dev(mask))).backward()
    _close(t2.grad.cpu().numpy(), 2 * r.g2, 2 * r.g2_scale, ic.GRAD_RTOL, 'second argument alone')
    assert t1.grad is None
    with pytest.raises(ValueError, match='mask'):
        build_masked_mse_loss_fn()(t1, t2, _dev(mask).requires_grad_(True))


@pytest.mark.parametrize('group', (1, 3))
@pytest.mark.parametrize('H,W', ic.DEPTH_PIXELS)
def test_depth_loss_rows_through_the_c_abi(H, W, group):
    L, check, ptr, st = _api()
    pred, true, mask = ic.depth_rows_case(H, W, group)
    b, N = pred.shape[:2]
    rows, P = b * N, H * W
    r = ic.depth_reference(pred, true, mask)
    tp, tt, tm = _dev(pred), _dev(true), _dev(mask)
    sums = _nan(rows, 3)
    row_loss = _a5(rows)
    check(L.mh_avg_depth_loss(ptr(tp), ptr(tt), ptr(tm), rows, group, P, 1e-3, ptr(sums), ptr(row_loss), st))
    torch.cuda.synchronize()
    assert (_u32(row_loss) == SENTINEL).all()                             # include/mhmocap_hip.h: never written
    s = sums.cpu().numpy().astype(np.float64)
    assert np.isfinite(s).all()
    loss = float((((s[:, 0] - s[:, 1]) / (s[:, 2] + 1)) ** 2).sum())
    w0 = _close(loss, r.loss, r.loss_scale, ic.LOSS_RTOL, 'loss')
    np.testing.assert_allclose(s[:, 2], mask.reshape(rows, P).astype(np.float64).sum(1), rtol=1e-6)
    gout = 0.75
    gp, gt = _nan(rows, P), _nan(rows, P)
    check(L.mh_avg_depth_loss_backward(ptr(tp), ptr(tt), ptr(tm), rows, group, P, 1e-3, ptr(sums), gout, ptr(gp), ptr(gt), st))
    torch.cuda.synchronize()
    gtn = gt.cpu().numpy().astype(np.float64).reshape(b, N, H, W)
    gtn = gtn.sum(axis=1, keepdims=True) if group > 1 else gtn
    w1 = _close(gp.cpu().numpy().reshape(pred.shape), gout * r.gpred, gout * r.gpred_scale, ic.GRAD_RTOL, 'gpred')
    w2 = _close(gtn, gout * r.gtrue, gout * r.gtrue_scale, ic.GRAD_RTOL, 'gtrue')
    # either gradient alone: the same bits, the other buffer untouched
    gp2, gt2 = _nan(rows, P), _nan(rows, P)
    check(L.mh_avg_depth_loss_backward(ptr(tp), ptr(tt), ptr(tm), rows, group, P, 1e-3, ptr(sums), gout, ptr(gp2), None, st))
    check(L.mh_avg_depth_loss_backward(ptr(tp), ptr(tt), ptr(tm), rows, group, P, 1e-3, ptr(sums), gout, None, ptr(gt2), st))
    torch.cuda.synchronize()
    assert torch.equal(gp2, gp) and torch.equal(gt2, gt)
    print('P=%d group=%d: loss %.2e of 2e-5, gpred %.2e, gtrue %.2e of 2e-4' % (P, group, w0, w1, w2))


@pytest.mark.parametrize('n', ic.MSE_COUNTS)
def test_masked_mse_through_the_c_abi(n):
    L, check, ptr, st = _api()
    a, b, m = ic.mse_flat_case(n)
    r = ic.mse_reference(a, b, m)
    ta, tb, tm = _dev(a), _dev(b), _dev(m)
    sums, ga = _nan(2), _nan(n)
    check(L.mh_masked_mse(ptr(ta), ptr(tb), ptr(tm), n, ptr(sums), st))
    check(L.mh_masked_mse_backward(ptr(ta), ptr(tb), ptr(tm), n, ptr(sums), 1.5, ptr(ga), st))
    torch.cuda.synchronize()
    s = sums.cpu().numpy().astype(np.float64)
    w0 = _close(s[0] / (s[1] + 1), r.loss, abs(r.loss), ic.LOSS_RTOL, 'loss')
    w1 = _close(ga.cpu().numpy(), 1.5 * r.g1, 1.5 * np.abs(r.g1), ic.GRAD_RTOL, 'gradient')
    print('n=%d: loss %.2e of 2e-5, gradient %.2e of 2e-4' % (n, w0, w1))
