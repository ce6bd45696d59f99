"""The scene-aggregation edge cases of tests/scene_agg_cases.py against numpy alone (no GPU): every case has to have the
property that tests/test_scene_agg_edges_gpu.py relies on -- the constructed medians are np.ma.median's, the fills take
the sweeps and list more pixels than the workgroup has threads where they are meant to, the skewed intrinsics make a
transposed inverse visible, and no post-processing input has a pixel near the edge threshold."""
import numpy as np
import pytest

import scene_agg_cases as sc


# ---- median over time --------------------------------------------------------------------------------------------------------
def test_sequence_lengths_cover_the_dispatch():
    """mh_scene_median_t: <4> up to 256 frames, <8> up to 512, <32> up to 2048; mh_scene_median: LDS columns up to 600"""
    t = set(sc.T_PIXEL_MAJOR)
    assert {1, 256, 257, 512, 513, 2048} <= t and max(t) == sc.T_REGISTER_FORM_MAX      # both ends of every instantiation
    assert {65, 257, 513} <= t                            # one frame alone in a new 64-frame register slot
    f = set(sc.T_FRAME_MAJOR)
    assert {sc.T_LDS_MAX - 1, sc.T_LDS_MAX, sc.T_LDS_MAX + 1} <= f and sc.T_LDS_MAX * 64 * 4 == 150 * 1024
    assert [h * w for h, w in sc.MEDIAN_SHAPES] == [1, 21, 65]


@pytest.mark.parametrize('T', sc.T_ALL)
def test_constructed_medians(T):
    names, vals, back, want = sc.constructed_pixels(T)
    assert len(set(names)) == len(names) and vals.shape == back.shape == (T, len(names)) and vals.dtype == np.float32
    assert {'first_only', 'last_only', 'all_equal'} <= set(names)
    if T >= 5:
        assert len(names) == 10
    md = np.ma.median(np.ma.array(vals, mask=back == 0), axis=0)
    np.testing.assert_array_equal(np.ma.getdata(md).astype(np.float32), want)
    md64 = np.ma.median(np.ma.array(vals.astype(np.float64), mask=back == 0), axis=0)
    np.testing.assert_array_equal(np.ma.getdata(md64).astype(np.float32), want)
    assert (vals[back == 0] == sc.GARBAGE).all() and (back.sum(0) >= 1).all()
    col = lambda n: (vals[:, names.index(n)], back[:, names.index(n)] > 0)
    v, b = col('last_only')
    assert b.sum() == 1 and b[T - 1]
    v, b = col('all_equal')
    assert b.all() and (v.view(np.uint32) == v.view(np.uint32)[0]).all()            # no bit varies
    if 'last_three' in names:
        v, b = col('last_three')
        assert b.sum() == 3 and b[T - 3:].all() and v[T - 1] != want[names.index('last_three')]
    if 'two_distinct' in names:
        v, b = col('two_distinct')
        assert b.sum() == 2 and b[0] and b[T - 1] and v[0] != v[T - 1]
    if 'adjacent_floats' in names:
        v, b = col('adjacent_floats')
        bits = np.sort(v[b].view(np.uint32))
        assert b[0] and b[T - 1] and (np.diff(bits) == 1).all() and np.bitwise_xor.reduce(bits[[0, -1]]) == 2
    for n in ('aabb', 'abbb', 'zero_lower_middle'):
        if n in names:
            v, b = col(n)
            s = np.sort(v[b])
            assert b.sum() == 4 and b[0] and b[T - 1]
            assert (s[1] != s[2]) == (n != 'abbb')                                  # lower middle != upper, or a tie
            if n == 'zero_lower_middle':
                assert s[1] == 0.0 and s[2] > 0
    if 'wide_exponents' in names:
        v, b = col('wide_exponents')
        e = v[b].view(np.uint32) >> 23
        assert (e.max() - e.min()) > 190                                            # the high exponent bits vary


@pytest.mark.parametrize('mode', sc.MEDIAN_MODES)
def test_random_median_inputs(mode):
    for T in (1, 65, 257, 601):
        for H, W in sc.MEDIAN_SHAPES:
            c = sc.median_inputs(T, H, W, mode)
            want, mask = sc.median_reference(T, H, W, mode)
            assert c.vals.shape == c.back.shape == (T, H, W) and want.shape == mask.shape == (H, W)
            assert (c.zmin is None) == (mode != 'depth') and (c.vals >= 0).all()
            np.testing.assert_array_equal(mask, c.back.max(0) > 0)
            assert (want[~mask] == 0).all() and (want[mask] >= 0).all()
            if H * W >= 3:
                assert not mask[0, 0] and c.back[:, 0, 1].sum() == 1 and c.back[:, 0, 2].sum() == min(T, 2)
            if mode == 'raw_int':
                assert (c.vals == np.round(c.vals)).all() and c.vals.max() <= 255
                assert (want * 2 == np.round(want * 2)).all()
            if T >= 65 and H * W >= 21:
                n = c.back.sum(0)
                assert ((n > 0) & (n % 2 == 0)).any() and (n % 2 == 1).any()        # both parities
                if mode != 'depth':                                                 # ties among the valid values of a quantised row
                    v = c.vals[:, 0, W - 1][c.back[:, 0, W - 1] > 0]
                    assert np.unique(v).size < v.size


# ---- fill ---------------------------------------------------------------------------------------------------------------
def test_fill_cases_cover_every_window_size():
    ks = sorted({sc.fill_case(n).ksize for n in sc.FILL_NAMES})
    assert ks == list(range(2, 12))
    assert {k | 1 for k in ks} == set(sc.FILL_THREADS)


@pytest.mark.parametrize('name', sc.FILL_NAMES)
def test_fill_case(name):
    c, r = sc.fill_case(name), sc.fill_case_reference(name)
    H, W = c.x.shape
    listed = int((c.mask == 0).sum())
    assert r.mask.min() == 1 and np.isfinite(r.x).all() and (r.x >= 0).all()        # everything reachable, no garbage read
    np.testing.assert_array_equal(r.x[c.mask > 0], c.x[c.mask > 0])
    if listed:
        bad = c.x[c.mask == 0]
        assert (np.isnan(bad) if name.startswith('nan_') else bad == -100.0).all()
    if name.startswith('random_k') or name.startswith('columns_k'):
        assert r.sweeps == {2: 5, 3: 5, 4: 3, 5: 3}.get(c.ksize, 2 if c.ksize < 10 else 1) and c.x.shape == (16, 30)
    if name == 'columns_k7':
        import test_scene_oracle as tso
        np.testing.assert_allclose(r.x[:, 10:19], tso.column_hole_case()[2][None, :].repeat(H, 0), rtol=1e-6)
    if name in ('row_1x9_k11', 'column_9x1_k11', 'tiny_2x3_k11'):
        assert max(H, W) < c.ksize and r.sweeps == (1 if name == 'tiny_2x3_k11' else 2)
    if name == 'corner_40x40_k3':
        assert listed == 1599 and r.sweeps == 39 and (r.x == 5.0).all()            # the lists swap every sweep
    if name.startswith('dense_33x33'):
        assert 0.55 < listed / (H * W) < 0.65 and listed > 256
    if name.startswith('sparse_33x33') or name == 'corner_40x40_k3':
        assert listed > 1024 >= sc.FILL_THREADS[c.ksize | 1]                       # more listed pixels than any workgroup has threads
    if name == 'dense_33x33_k11' or name == 'sparse_33x33_k9':
        assert listed > sc.FILL_THREADS[c.ksize | 1] == 256
    if name == 'full_mask_k7':
        assert listed == 0 and r.sweeps == 0
    if name.startswith('truncate_k'):
        assert c.truncate == 1 and (c.x[c.mask > 0] == np.round(c.x[c.mask > 0])).all()
        new = c.mask == 0
        halves = (r.first_sweep[new] % 1) == 0.5
        assert halves.sum() >= 20                                                   # even valid counts: medians that end in .5
        assert (r.x == np.floor(r.x)).all()
        plain = sc.fill_reference(c.x, c.mask, c.ksize, False)
        assert (plain.x != r.x).sum() >= 20                                         # flooring is visible in the result
    else:
        assert c.truncate == 0


@pytest.mark.parametrize('k', [2, 4, 6, 8, 10])
def test_an_even_window_is_the_next_odd_one(k):
    """utils.py:117: k = filter_size // 2 on both sides, so sizes 2k and 2k + 1 read exactly the same pixels"""
    c = sc.fill_case('random_k%d' % k)
    a, b = sc.fill_reference(c.x, c.mask, k), sc.fill_reference(c.x, c.mask, k + 1)
    np.testing.assert_array_equal(a.x, b.x)
    assert a.sweeps == b.sweeps


def test_fill_reference_stops_when_nothing_is_reachable():
    x = np.full((6, 7), 3.0, np.float32)
    r = sc.fill_reference(x, np.zeros((6, 7), np.float32), 7)
    assert r.sweeps == 0 and r.mask.max() == 0 and (r.x == x).all()


# ---- un-projection ------------------------------------------------------------------------------------------------------
def test_unprojection_cases():
    assert [h * w for h, w in sc.POINTS_SHAPES] == [1, 63, 64, 65, 1023, 1024, 1025, 2049]
    assert [h * w for h, w in sc.UNPROJECT_SHAPES] == [255, 256, 257]
    worst = 0.0
    for H, W in sc.POINTS_SHAPES + sc.UNPROJECT_SHAPES:
        depth, K, want = sc.unproject_case(H, W)
        assert K[0, 1] == np.float32(3.7) and K[1, 0] == np.float32(-1.9) and 190 < K[0, 0] < 210 and 190 < K[1, 1] < 210
        assert abs(K[0, 2] - W / 2) > 0.1 * W and abs(K[1, 2] - H / 2) > 0.1 * H
        # the reference projects back onto the pixel centres: K [x/z, y/z, 1]
        uv = (K.astype(np.float64) @ (want / want[:, 2:3]).T).T
        ys, xs = np.mgrid[0:H, 0:W]
        np.testing.assert_allclose(uv[:, 0], xs.ravel() + 0.5, atol=1e-9)
        np.testing.assert_allclose(uv[:, 1], ys.ravel() + 0.5, atol=1e-9)
        tol = sc.UNPROJECT_ATOL + sc.UNPROJECT_RTOL * np.abs(want)
        # float32 evaluation of the formula: well inside the tolerance (0.08 of it at worst, 3 x 683) ...
        err = np.abs(sc.unproject_float32(depth, K).astype(np.float64) - want)
        worst = max(worst, float((err / tol).max()))
        # ... and a transposed 2 x 2 inverse far outside it wherever the image has more than one pixel
        Kt = K.copy()
        Kt[0, 1], Kt[1, 0] = K[1, 0], K[0, 1]
        swapped = np.abs(sc.unproject_float32(depth, Kt).astype(np.float64) - want)
        if H * W > 1:
            assert ((swapped > 4 * tol).any(axis=1)).mean() > 0.9
    print('float32 evaluation / tolerance, worst over the cases: %.3f' % worst)
    assert worst < 0.25


def test_points_masks():
    for H, W in sc.POINTS_SHAPES:
        m = sc.points_mask(H, W, 'random')
        assert sc.points_mask(H, W, 'ones').all() and not sc.points_mask(H, W, 'zeros').any()
        if H * W >= 63:
            assert 0 < m.sum() < H * W and set(np.unique(m)) == {0.0, 1.0}


# ---- post-processing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,bilateral,seed', sc.POSTPROCESS_CASES)
def test_no_pixel_is_near_the_edge_threshold(H, W, bilateral, seed):
    depth, mask = sc.postprocess_input(H, W, seed)
    assert mask[0, 0] == 0 and depth[0, 0] == 0 and (depth[mask > 0] > 1).all() and ((mask == 0) & (depth == 0)).sum() >= 5
    assert (mask[H - 1, :2] == 0).all() and (depth[H - 1, :2] > 1).all()
    e32, e64, margin = sc.edge_decision(depth, bilateral)
    print('%d x %d bilateral %d: margin %.4f, %d edge pixels' % (H, W, bilateral, margin, int(e32.sum())))
    np.testing.assert_array_equal(e32, e64)
    assert margin >= sc.EDGE_MARGIN_MIN
    assert e32.any() or (H, W) == (5, 5)
    want = sc.postprocess_reference(H, W, bilateral, seed)
    assert np.isfinite(want).all() and (want > 0).all()


def test_postprocess_sizes():
    p = sorted({h * w for h, w, _, _ in sc.POSTPROCESS_CASES})
    assert 25 in p and 255 in p and 256 in p and any(256 < q <= 272 for q in p)     # one | two Sobel partial sums
    for H, W in sc.POSTPROCESS_VARIANT_SIZES:
        assert (H, W, 0, 1) in sc.POSTPROCESS_CASES and (H, W, 1, 1) in sc.POSTPROCESS_CASES
        for bil in (0, 1):
            a = sc.postprocess_reference(H, W, bil, 1)
            assert np.abs(sc.postprocess_reference(H, W, bil, 1, with_mask=False) - a).max() > 1e-3     # the mask matters
            assert np.abs(sc.postprocess_reference(H, W, bil, 1, ksize=3) - a).max() > 1e-3             # so does the window
            assert np.abs(sc.postprocess_reference(H, W, bil, 1, ksize=11) - a).max() > 1e-3
