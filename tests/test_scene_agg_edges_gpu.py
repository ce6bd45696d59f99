"""The device scene update (csrc/mh_sceneagg.hip, k_unproject of csrc/mh_scene.hip) through the C ABI on the cases of
tests/scene_agg_cases.py -- every instantiation its dispatch can pick, at the sizes where one hands over to the next:

  median over time   k_scene_median_t<4 | 8 | 32> (T = 1 .. 2048) and k_scene_median<true | false> (LDS columns up to
                     T = 600, recomputed values beyond) on 1, 21 and 65 pixels; depth mode against
                     oracle.scene_oracle.aggregate_scene_median (mask exact, rtol 3e-6), raw mode against np.ma.median
                     (integer planes exact, floats rtol 1e-6); both forms bit for bit equal at every T <= 2048; pixels
                     built by hand (one valid frame alone in a register slot, ties, adjacent floats, 60 binades, 0.0)
  fill               k_scene_fill at window sizes 2 .. 11 (3, 5, 7 sorted by the network; 9, 11 by insertion) against the
                     looped oracle.scene_oracle.fillin_values: windows larger than the image, 39 sweeps, more listed
                     pixels than threads, nothing listed, nothing reachable, truncation, NaN under the mask
  un-projection      k_scene_points and k_unproject with a skewed K against oracle.fit_oracle.unproject_points in float64
                     (rtol 2e-6, atol 1e-6: the float32 evaluation of the formula stays below 0.07 of that)
  post-processing    whole images at 1e-4 * max(1, |want|) with no pixel left out, on inputs whose edge decision is at
                     least 1 % away from the threshold (tests/test_scene_agg_cases.py)

Measured on an MI355X (worst over the cases): median, relative error 2.4e-7 in depth mode (bound 3e-6), 5.9e-8 on raw
floats (1e-6), 0 on integer planes; fill 0 at every window size; un-projection 0.05 of its tolerance; post-processing
1.5e-7 with the bilateral filter and 0 without (1e-4).  Each test prints its own figure (-s).

Five deliberate changes of the kernels, each run once against this file: counting a clamped frame in the T <= 512 load
path fails 32 tests (the random medians and the constructed pixels at every T <= 511 that is no multiple of 256),
launching <4> up to T = 512 fails 16 (T = 257 .. 512), the upper instead of the mean of the two middles in the sorting
network fails 38 (fills at windows 2 .. 7 and every post-processing case), a transposed 2 x 2 inverse fails 16 (every
points case with a pixel in it).  `less >= n / 2` for `less == n / 2` in the lower-middle pass fails none and cannot: the
value found is the (n / 2)-th smallest, so at most n / 2 values are smaller; `less <= n / 2` fails 53 (every tie)."""
import numpy as np
import pytest
import torch

import scene_agg_cases as sc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _workspace(L, T, H, W):
    # 0xA5 everywhere: no kernel may rely on what a workspace held before
    return torch.full((L.mh_scene_workspace_bytes(T, H, W),), 0xA5, dtype=torch.uint8, device=DEV)


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def _rejected(L, rc, why):
    assert rc != 0
    assert why in L.mh_last_error(), L.mh_last_error()


# ---------------------------------------------------------------------------------------------------------------
# median over time
# ---------------------------------------------------------------------------------------------------------------
def _medians(T, H, W, vals, back, zmin, zmax):
    """vals / back (T, H * W) -> {'frame_major': (values, mask), 'pixel_major': ...}; the register form only up to its
    2048 frames.  The outputs start as NaN: a pixel nobody writes shows."""
    L, check, ptr, st = _api()
    P = H * W
    ws = _workspace(L, T, H, W)
    tv, tb, tzmin, tzmax = _dev(vals.reshape(T, P)), _dev(back.reshape(T, P)), _dev(zmin), _dev(zmax)
    out = {}
    md, mm = torch.full((H, W), float('nan'), device=DEV), torch.full((H, W), float('nan'), device=DEV)
    check(L.mh_scene_median(T, H, W, ptr(tv), ptr(tb), ptr(tzmin), ptr(tzmax), ptr(md), ptr(mm), ptr(ws), st))
    torch.cuda.synchronize()
    out['frame_major'] = (md.cpu().numpy(), mm.cpu().numpy())
    if T <= sc.T_REGISTER_FORM_MAX:
        tvt, tbt = tv.t().contiguous(), tb.t().contiguous()
        md2, mm2 = torch.full((H, W), float('nan'), device=DEV), torch.full((H, W), float('nan'), device=DEV)
        check(L.mh_scene_median_t(T, H, W, ptr(tvt), ptr(tbt), ptr(tzmin), ptr(tzmax), ptr(md2), ptr(mm2), ptr(ws), st))
        torch.cuda.synchronize()
        out['pixel_major'] = (md2.cpu().numpy(), mm2.cpu().numpy())
    return out


@pytest.mark.parametrize('mode', sc.MEDIAN_MODES)
@pytest.mark.parametrize('T', sc.T_ALL)
def test_median_over_time_at_every_instantiation(T, mode):
    worst = 0.0
    for H, W in sc.MEDIAN_SHAPES:
        c = sc.median_inputs(T, H, W, mode)
        want, want_mask = sc.median_reference(T, H, W, mode)
        out = _medians(T, H, W, c.vals, c.back, c.zmin, c.zmax)
        for form, (got, mask) in out.items():
            tag = '%s T=%d %dx%d %s' % (mode, T, H, W, form)
            np.testing.assert_array_equal(mask, want_mask.astype(np.float32), err_msg=tag)
            assert (got[~want_mask] == 0).all(), tag
            if mode == 'raw_int':
                np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=tag)
            else:
                np.testing.assert_allclose(got[want_mask], want[want_mask], rtol=3e-6 if mode == 'depth' else 1e-6, err_msg=tag)
                if want_mask.any():
                    worst = max(worst, float(np.abs(got[want_mask] / want[want_mask] - 1).max()))
        if 'pixel_major' in out:
            # the in-kernel range evaluation of the register form gives the bits of k_scene_ranges
            np.testing.assert_array_equal(out['pixel_major'][0].view(np.uint32), out['frame_major'][0].view(np.uint32))
            np.testing.assert_array_equal(out['pixel_major'][1], out['frame_major'][1])
    print('%s T=%d: worst relative error %.2e, forms run: %s' % (mode, T, worst, ' '.join(out)))


@pytest.mark.parametrize('T', sc.T_ALL)
def test_median_of_constructed_pixels(T):
    """raw mode: the expected values are written down in scene_agg_cases.constructed_pixels"""
    names, vals, back, want = sc.constructed_pixels(T)
    n = len(names)
    for form, (got, mask) in _medians(T, 1, n, vals, back, None, None).items():
        bad = [names[i] for i in range(n) if got[0, i].view(np.uint32) != want[i].view(np.uint32)]
        assert not bad, '%s T=%d: %s: got %s, expected %s' % (form, T, bad, got[0], want)
        np.testing.assert_array_equal(mask, np.ones((1, n), np.float32))


def test_median_rejections():
    L, check, ptr, st = _api()
    H, W, T = 3, 7, 2049
    tv = torch.ones(H * W, T, device=DEV)
    tb = torch.ones(H * W, T, dtype=torch.uint8, device=DEV)
    z = torch.ones(T, device=DEV)
    md, mm = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
    ws = _workspace(L, T, H, W)
    _rejected(L, L.mh_scene_median_t(2049, H, W, ptr(tv), ptr(tb), None, None, ptr(md), ptr(mm), ptr(ws), st), b'too long')
    for fn in (L.mh_scene_median_t, L.mh_scene_median):
        _rejected(L, fn(8, H, W, ptr(tv), ptr(tb), ptr(z), None, ptr(md), ptr(mm), ptr(ws), st), b'come in pairs')
        _rejected(L, fn(8, H, W, ptr(tv), ptr(tb), None, ptr(z), ptr(md), ptr(mm), ptr(ws), st), b'come in pairs')
        _rejected(L, fn(0, H, W, ptr(tv), ptr(tb), None, None, ptr(md), ptr(mm), ptr(ws), st), b'empty input')
    torch.cuda.synchronize()
    assert float(md.abs().sum()) == 0 and float(mm.abs().sum()) == 0          # nothing was launched
    check(L.mh_scene_median_t(2048, H, W, ptr(tv), ptr(tb), None, None, ptr(md), ptr(mm), ptr(ws), st))   # the limit itself is fine
    torch.cuda.synchronize()
    assert float(md.min()) == 1.0 and float(mm.min()) == 1.0


# ---------------------------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------------------------
def _fill(x, mask, ksize, truncate):
    L, check, ptr, st = _api()
    H, W = x.shape
    ws = _workspace(L, 1, H, W)
    tv, tm = _dev(x), _dev(mask)
    check(L.mh_scene_fill(H, W, ksize, truncate, ptr(tv), ptr(tm), ptr(ws), st))
    torch.cuda.synchronize()
    return tv.cpu().numpy(), tm.cpu().numpy()


@pytest.mark.parametrize('name', sc.FILL_NAMES)
def test_fill_at_every_window_size(name):
    c, r = sc.fill_case(name), sc.fill_case_reference(name)
    got, got_mask = _fill(c.x, c.mask, c.ksize, c.truncate)
    np.testing.assert_array_equal(got_mask, r.mask)
    assert np.isfinite(got).all() and (got >= 0).all()                       # nothing from under the mask (-100 or NaN)
    old = c.mask > 0
    np.testing.assert_array_equal(got[old].view(np.uint32), c.x[old].view(np.uint32))
    if c.truncate:
        np.testing.assert_array_equal(got, r.x)
    else:
        np.testing.assert_allclose(got, r.x, rtol=1e-6)
    print('%s: %d listed, %d sweeps, worst error %.2e' % (name, int((~old).sum()), r.sweeps, float(np.abs(got - r.x).max())))


@pytest.mark.parametrize('ksize', [7, 11])
def test_fill_stops_when_nothing_is_reachable(ksize):
    """an all-zero mask: the first sweep fills nothing, k_scene_fill's `filled > 0 ? rest : 0` empties the list and the
    loop ends; values and mask come back as they went in"""
    rng = np.random.RandomState(ksize)
    x = rng.uniform(1, 9, (16, 30)).astype(np.float32)
    mask = np.zeros((16, 30), np.float32)
    got, got_mask = _fill(x, mask, ksize, 0)
    np.testing.assert_array_equal(got.view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(got_mask.view(np.uint32), mask.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# un-projection
# ---------------------------------------------------------------------------------------------------------------
def _K_arg(K):
    from mhhip import _lib
    Kc = np.ascontiguousarray(K.reshape(9), dtype=np.float32)
    return Kc, Kc.ctypes.data_as(_lib.c_float_p)


def _close(tag, got, want):
    err = np.abs(got.astype(np.float64) - want)
    tol = sc.UNPROJECT_ATOL + sc.UNPROJECT_RTOL * np.abs(want)
    print('%s: worst error / tolerance %.3f over %d rows' % (tag, float((err / tol).max()) if err.size else 0.0, got.shape[0]))
    assert (err <= tol).all(), '%s: %d entries off, worst error / tolerance %.1f' % (tag, int((err > tol).sum()), float((err / tol).max()))


@pytest.mark.parametrize('kind', sc.POINTS_MASKS)
@pytest.mark.parametrize('H,W', sc.POINTS_SHAPES)
def test_points_with_a_skewed_K(H, W, kind):
    L, check, ptr, st = _api()
    depth, K, want = sc.unproject_case(H, W)
    mask = sc.points_mask(H, W, kind)
    P = H * W
    pts = torch.full((P, 3), -7.0, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    Kc, Kp = _K_arg(K)
    tdepth, tmask = _dev(depth), _dev(mask)
    check(L.mh_scene_points(H, W, Kp, ptr(tdepth), ptr(tmask), ptr(pts), ptr(cnt), st))
    torch.cuda.synchronize()
    n = int(cnt.item())
    got = pts.cpu().numpy()
    assert n == int(mask.sum())
    assert (got[n:] == -7.0).all()                                           # rows behind the count are not touched
    _close('points %dx%d %s' % (H, W, kind), got[:n], want[mask.ravel() > 0.5])          # row-major order


@pytest.mark.parametrize('H,W', sc.UNPROJECT_SHAPES)
def test_unproject_with_a_skewed_K(H, W):
    L, check, ptr, st = _api()
    depth, K, want = sc.unproject_case(H, W)
    pts = torch.full((H * W, 3), float('nan'), device=DEV)
    Kc, Kp = _K_arg(K)
    tdepth = _dev(depth)
    check(L.mh_scene_unproject(ptr(tdepth), H, W, Kp, ptr(pts), st))
    torch.cuda.synchronize()
    _close('unproject %dx%d' % (H, W), pts.cpu().numpy(), want)


def test_unprojection_rejections():
    L, check, ptr, st = _api()
    H, W = 7, 9
    depth, K, _ = sc.unproject_case(H, W)
    singular = np.array([[2.0, 4.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 1.0]], np.float32)      # 2 * 2 - 1 * 4 == 0
    tdepth, tmask = _dev(depth), _dev(np.ones((H, W), np.float32))
    pts = torch.full((H * W, 3), -7.0, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    Ks, Ksp = _K_arg(singular)
    Kc, Kp = _K_arg(K)
    _rejected(L, L.mh_scene_points(H, W, Ksp, ptr(tdepth), ptr(tmask), ptr(pts), ptr(cnt), st), b'singular')
    _rejected(L, L.mh_scene_unproject(ptr(tdepth), H, W, Ksp, ptr(pts), st), b'singular')
    _rejected(L, L.mh_scene_points(0, W, Kp, ptr(tdepth), ptr(tmask), ptr(pts), ptr(cnt), st), b'empty image')
    _rejected(L, L.mh_scene_unproject(ptr(tdepth), 0, W, Kp, ptr(pts), st), b'empty image')
    torch.cuda.synchronize()
    assert int(cnt.item()) == -1 and float(pts.max()) == -7.0                # nothing was launched


# ---------------------------------------------------------------------------------------------------------------
# post-processing: the whole image, no pixel left out
# ---------------------------------------------------------------------------------------------------------------
def _postprocess(depth, mask, bilateral, ksize):
    L, check, ptr, st = _api()
    H, W = depth.shape
    ws = _workspace(L, 1, H, W)
    out = torch.full((H, W), float('nan'), device=DEV)
    tdepth, tmask = _dev(depth), _dev(mask)
    check(L.mh_scene_postprocess(H, W, ptr(tdepth), ptr(tmask), bilateral, ksize, ptr(out), ptr(ws), st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_image(tag, got, want):
    assert np.isfinite(got).all(), tag
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print('%s: worst |got - want| / max(1, |want|) %.2e (bound 1e-4)' % (tag, float(err.max())))
    bad = err > 1e-4
    assert not bad.any(), '%s: %d pixels differ, first at %s' % (tag, int(bad.sum()), np.argwhere(bad)[0])


@pytest.mark.parametrize('H,W,bilateral,seed', sc.POSTPROCESS_CASES)
def test_postprocess_whole_image(H, W, bilateral, seed):
    depth, mask = sc.postprocess_input(H, W, seed)
    want = sc.postprocess_reference(H, W, bilateral, seed)
    _same_image('%dx%d bilateral %d' % (H, W, bilateral), _postprocess(depth, mask, bilateral, 7), want)


@pytest.mark.parametrize('bilateral', [0, 1])
@pytest.mark.parametrize('H,W', sc.POSTPROCESS_VARIANT_SIZES)
def test_postprocess_without_a_mask(H, W, bilateral):
    depth, _ = sc.postprocess_input(H, W, 1)
    want = sc.postprocess_reference(H, W, bilateral, 1, with_mask=False)
    _same_image('%dx%d bilateral %d, ma_mask = NULL' % (H, W, bilateral), _postprocess(depth, None, bilateral, 7), want)


@pytest.mark.parametrize('ksize', [3, 11])
@pytest.mark.parametrize('bilateral', [0, 1])
@pytest.mark.parametrize('H,W', sc.POSTPROCESS_VARIANT_SIZES)
def test_postprocess_with_another_fill_window(H, W, bilateral, ksize):
    depth, mask = sc.postprocess_input(H, W, 1)
    want = sc.postprocess_reference(H, W, bilateral, 1, ksize=ksize)
    _same_image('%dx%d bilateral %d, window %d' % (H, W, bilateral, ksize), _postprocess(depth, mask, bilateral, ksize), want)


def test_postprocess_rejections():
    L, check, ptr, st = _api()
    ws = _workspace(L, 1, 16, 16)
    d, m = torch.full((16, 16), 3.0, device=DEV), torch.ones(16, 16, device=DEV)
    out = torch.full((16, 16), -7.0, device=DEV)
    _rejected(L, L.mh_scene_postprocess(4, 16, ptr(d), ptr(m), 1, 7, ptr(out), ptr(ws), st), b'smaller than')
    _rejected(L, L.mh_scene_postprocess(16, 4, ptr(d), ptr(m), 1, 7, ptr(out), ptr(ws), st), b'smaller than')
    _rejected(L, L.mh_scene_postprocess(16, 16, ptr(d), ptr(m), 1, 1, ptr(out), ptr(ws), st), b'2..11')
    _rejected(L, L.mh_scene_postprocess(16, 16, ptr(d), ptr(m), 1, 12, ptr(out), ptr(ws), st), b'2..11')
    _rejected(L, L.mh_scene_postprocess(16, 16, ptr(d), ptr(m), 1, 7, ptr(d), ptr(ws), st), b'alias')
    _rejected(L, L.mh_scene_fill(16, 16, 1, 0, ptr(d), ptr(m), ptr(ws), st), b'2..11')
    _rejected(L, L.mh_scene_fill(16, 16, 12, 0, ptr(d), ptr(m), ptr(ws), st), b'2..11')
    torch.cuda.synchronize()
    assert float(out.max()) == -7.0 and float(d.min()) == 3.0 and float(d.max()) == 3.0       # nothing was launched
