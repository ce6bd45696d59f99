"""The references of tests/image_cases.py against the reference-generated fixtures and against numpy alone (no GPU): they
reproduce tests/golden/reference_image_cpu.npz (make_golden_image.py) and the erosion and loss entries of
reference_cpu.npz, the silhouette statistics agree with the loop of oracle.fit_oracle.SequenceOracle, every case has the
property that tests/test_image_gpu.py relies on, and each float case prints the error that a float32 numpy evaluation of
its formula makes against float64 (-s): the yardstick of the tolerances there."""
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
import image_cases as ic


@pytest.fixture(scope='module')
def golden_image():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_image_cpu.npz'), allow_pickle=False)


# ---- morphology ---------------------------------------------------------------------------------------------------------
def test_morph_reference_reproduces_the_fixture(golden_image):
    assert gi.IMAGE_MORPH_KSIZES == ic.MORPH_KSIZES and gi.IMAGE_MORPH_SIZES == ic.MORPH_IMAGES
    for (H, W), x in gi.image_morph_inputs().items():
        assert set(np.unique(x)) <= {np.float32(0), ic.BELOW_HALF, ic.HALF, np.float32(0.7), np.float32(1)}
        for k in ic.MORPH_KSIZES:
            for name, dilate in (('erode', False), ('dilate', True)):
                np.testing.assert_array_equal(ic.morph_reference(x, k, dilate), golden_image['%s_%dx%d_k%d' % (name, H, W, k)],
                                              err_msg='%s %dx%d k=%d' % (name, H, W, k))
    x = gi.image_morph_inputs()[(6, 9)]
    assert (ic.morph_reference(x, 1, False) == (x >= 0.5)).all() and (ic.morph_reference(x, 1, True) == (x >= 0.5)).all()
    assert (ic.morph_reference(x, 3, False) != ic.morph_reference(x, 5, False)).any()       # the window size matters


def test_morph_reference_reproduces_the_double_erosion(golden):
    x = gi.erode_inputs()
    np.testing.assert_array_equal(ic.morph_reference(ic.morph_reference(x, 3, False), 3, False), golden['erode2'])
    from oracle import fit_oracle
    np.testing.assert_array_equal(ic.morph_reference(x, 3, False), fit_oracle.erode3x3(torch.tensor(x)).numpy())


def test_erosion_counts_only_pixels_of_the_image():
    """an all-ones image stays all ones (the outside is not background); one zero removes its whole window"""
    for H, W in ic.ERODE_IMAGES + ic.MORPH_IMAGES:
        assert ic.morph_reference(np.ones((H, W), np.float32), 3, False).all()
    x = np.ones((6, 9), np.float32)
    x[0, 0] = 0
    assert ic.morph_reference(x, 3, False).sum() == 54 - 4 and ic.morph_reference(x, 5, False).sum() == 54 - 9


def test_bit_planes_round_trip():
    T, N, H, W = ic.PACK_LARGE
    assert H * W > 64 * 256
    assert ic.ERODE_LARGE[2] * ic.ERODE_LARGE[3] > 128 * 256
    for n in ic.PACK_PEOPLE:
        seg = ic.pack_input(2, n, 1, 37)
        bits, area = ic.pack_reference(seg)
        assert bits.dtype == np.uint32 and (bits >> np.uint32(n) == 0).all() if n < 32 else bits.max() >= 2 ** 31
        np.testing.assert_array_equal(ic.planes(bits, n), (seg >= 0.5).astype(np.float32))
        np.testing.assert_array_equal(ic.words(ic.planes(bits, n)), bits)
        np.testing.assert_array_equal(area, (seg >= 0.5).sum((2, 3)))
        # the four values meet in every plane: 0.5 is set, the float below it is not
        assert all(set(ic.PACK_VALUES) <= set(seg[t, m].ravel()) for t in range(2) for m in range(n))
    assert ic.BELOW_HALF < ic.HALF and np.float32(ic.BELOW_HALF + np.float32(2.0 ** -25)) == ic.HALF
    # on {0, 1} masks the count is the reference's sum(seg_mask, dim=(2, 3)) (optimizer.py:408)
    seg = ic.pack_input(2, 5, 21, 30, binary=True)
    np.testing.assert_array_equal(ic.pack_reference(seg)[1], seg.sum((2, 3)))


# ---- gates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', ic.GATE_THRESHOLDS)
def test_gate_cases_sit_on_the_comparisons(thr):
    H, W = ic.GATE_IMAGE
    assert (H * W) % 200 == 0
    for B in ic.GATE_BODIES:
        pose2d, area, t, min_area = ic.gates_case(B, thr)
        assert np.float32(min_area) == 3.0 and min_area == 0.005 * H * W
        p2d, mv = ic.gates_reference(pose2d, area, t, min_area)
        # the reference's expressions (optimizer.py:404-409) on float32 tensors
        conf = torch.ge(torch.tensor(pose2d)[None, ..., 2:3], t).float()
        np.testing.assert_array_equal(torch.ge(conf.sum(dim=(2, 3)), 2).float().numpy()[0], p2d)
        np.testing.assert_array_equal(torch.ge(torch.tensor(area), min_area).float().numpy(), mv)
        assert p2d[0] == 1 and mv[0] == 1 and (pose2d[0, :, 2] == np.float32(thr)).sum() == 2
        assert (pose2d[0, :, 2] >= np.float32(thr)).sum() == 2
        if B > 3:
            assert p2d[1] == 0 and mv[1] == 0 and area[1] == 2 and (pose2d[1, :, 2] == np.float32(thr)).sum() == 1
            assert p2d[2] == 0 and (pose2d[2, :, 2] > 0).sum() == 2
            assert p2d[3] == 1 and 0 < p2d.mean() < 1 and 0 < mv.mean() < 1
    assert float(np.float32(0.3)) > 0.3 > float(np.nextafter(np.float32(0.3), np.float32(0)))    # float32(0.3) is not the double


# ---- silhouette statistics -------------------------------------------------------------------------------------------------
def test_sil_cases_cover_the_dispatch():
    assert {4, 5, 8, 9, 16, 17, 32} <= set(ic.SIL_PEOPLE) and {511, 512, 2047, 2048} <= set(ic.SIL_FRAMES)
    N, H, W = ic.SIL_FRAMES_SHAPE
    assert H * W == 15                                       # 8 parts: one of one pixel, seven of two
    assert sorted({15 * (p + 1) // 8 - 15 * p // 8 for p in range(8)}) == [1, 2]


@pytest.mark.parametrize('kind', ic.SIL_ORDERINGS)
def test_sil_orderings(kind):
    T, H, W = ic.SIL_PEOPLE_SHAPE
    differs = 0
    for N in ic.SIL_PEOPLE:
        c = ic.sil_case(T, N, H, W, kind)
        r = ic.sil_case_reference(T, N, H, W, kind)
        for t in range(T):
            order = np.argsort(c.z[t], kind='stable')
            assert sorted(order) == list(range(N))
            # front sets: nested along the order, person of rank r has r people in front
            assert [bin(int(r.front[t, n])).count('1') for n in order] == list(range(N))
            assert r.D[t, order[0]] == H * W and (np.diff(r.D[t, order]) <= 0).all()
            assert (r.S[t] <= r.D[t]).all() and (r.S[t] <= c.seg[t].sum((1, 2))).all()
            if kind == 'all_equal':
                assert list(order) == list(range(N))
            if kind == 'pairs' and N > 1:
                assert len(np.unique(c.z[t])) == (N + 1) // 2
            if kind == 'zeros' and N > 3:
                zs = c.z[t][c.z[t] == 0]
                assert np.signbit(zs).any() and not np.signbit(zs).all()
                i = np.flatnonzero(c.z[t] == 0)
                assert [int(n) for n in order if c.z[t, n] == 0] == list(i)          # ties among the zeros: by index
            if kind == 'inf' and N > 2:
                i = np.flatnonzero(np.isinf(c.z[t]))
                assert len(i) == 2 and list(order[-2:]) == list(i)
        differs += int((r.apply != ic.apply_by_person(c)).sum())
    assert differs > 0 or kind == 'all_equal'                # rank-indexed and person-indexed gates differ somewhere
    if kind == 'all_equal':
        assert differs == 0                                  # rank == person


def test_sil_reference_agrees_with_the_sequence_oracle(oracle_model):
    """oracle.fit_oracle.SequenceOracle.batch_loss itself, with a rasteriser that renders nothing: its silhouette term is
    then the sum over the gated ranks of masked_mse(0, seg, 1 - acc) = S / (D + 1).  The gates come out of batch_loss's own
    expressions (confidences, mask areas), the ordering out of its argsort of poses_T."""
    from mhhip import synthetic
    from oracle import fit_oracle as fo
    T, N, H, W = 3, 5, 17, 19
    rng = np.random.RandomState(9)
    c = ic.sil_case(T, N, H, W, 'random')                    # (ties: torch.argsort promises no order for them)
    seg = c.seg.copy()
    seg[0, 1] = 0
    seg[0, 1, 3, 4] = 1                                      # one pixel < 0.005 * H * W: no valid mask
    seg[2, 3] = 0
    pose2d = rng.uniform(0, 1, (T, N, 17, 3)).astype(np.float32)
    pose2d[..., 2] = (rng.rand(T, N, 1) > 0.3)               # all joints confident, or none
    pT = rng.randn(T, N, 1, 3).astype(np.float32)
    pT[..., 0, 2] = np.abs(c.z) + 2
    stub = lambda v: (-torch.ones(v.shape[0], H, W), torch.zeros(v.shape[0], H, W))
    o = fo.SequenceOracle(oracle_model, (W, H), T, synthetic.default_cam_K((W, H), 60.0), rasteriser=stub)
    o.xscale = torch.zeros(1, N, 1, 1)
    poses = rng.normal(0, 0.2, (T, N, 72)).astype(np.float32)
    o.init_optimized_variables(pose2d, poses, np.zeros((T, N, 10), np.float32), np.ones((T, N, 1), np.float32), poses_T=pT)
    with torch.no_grad():
        _, terms, _ = o.batch_loss(dict(idxs=torch.arange(T), pose2d=torch.tensor(pose2d), seg_mask=torch.tensor(seg),
                                        depths=torch.rand(T, H, W), poses_smpl=torch.tensor(poses)))
    p2d, mv = ic.gates_reference(pose2d.reshape(T * N, 17, 3), seg.sum((2, 3)).reshape(-1), 0.5, 0.005 * H * W)
    assert mv.reshape(T, N)[0, 1] == 0 and mv.reshape(T, N)[2, 3] == 0 and mv.sum() == T * N - 2 and 0 < p2d.mean() < 1
    r = ic.sil_reference(seg, pT[..., 0, 2], p2d.reshape(T, N), mv.reshape(T, N))
    assert (r.apply != (p2d * mv).reshape(T, N)).any()       # the rank-indexed gate is not the person-indexed one
    want = float(terms['loss_silhouette'])
    got = float((r.apply.astype(np.float64) * r.S / (r.D + 1.0)).sum())
    assert want > 0 and abs(got - want) <= 1e-5 * want, (got, want)


def test_sil_reference_agrees_with_the_sequence_oracle_loop():
    """oracle.fit_oracle.SequenceOracle.batch_loss :325-335, copied as a loop over the same argsort, with a rendered
    silhouette of zeros: the term of a counted person is masked_mse(0, seg, 1 - acc) = S / (D + 1)"""
    from oracle import fit_oracle
    T, N, H, W = 3, 5, 17, 19
    c = ic.sil_case(T, N, H, W, 'random')
    r = ic.sil_case_reference(T, N, H, W, 'random')
    order = torch.argsort(torch.tensor(c.z), dim=1)
    want = 0.0
    for j in range(T):
        acc = torch.zeros(H, W)
        for rank in range(N):
            n = int(order[j, rank])
            seg = torch.tensor(c.seg[j, n])
            if float(c.mask_valid[j, rank] * c.p2d_valid[j, rank]) > 0:
                want += float(fit_oracle.masked_mse_loss(torch.zeros(H, W), seg, 1 - acc))
            acc = ((acc + seg) > 0).float()
    got = float((r.apply * r.S / (r.D + 1)).sum())
    assert abs(got - want) <= 1e-5 * want and want > 0


# ---- priors ---------------------------------------------------------------------------------------------------------------
def test_prior_cases_and_float32_yardstick():
    for T, N, nb, xk in ic.prior_cases():
        c = ic.prior_case(T, N, nb, xk)
        w = ic.prior_reference(c)
        same = c.poses == c.ref
        assert same.any() and (np.abs(c.poses - c.ref)[~same] >= 0.99e-3).all()
        assert (c.valid == 0).any() or T * N == 1
        gadd = w.gposes - c.gposes0
        assert (gadd[same] == 0).all() and (gadd[(c.valid == 0)] == 0).all()
        live = ~same & (c.valid[..., None] > 0)
        np.testing.assert_allclose(np.abs(gadd[live]), c.cp, rtol=1e-12)
        np.testing.assert_allclose(np.abs((w.gbetas - c.gbetas0)[c.betas != c.betas_ref]), c.cp * T, rtol=1e-12)
        if xk in ('zero', 'null'):
            assert w.loss3[1] == 0 and w.loss3[2] == 0 and (w.gxscale == c.gxscale0).all()
        f = ic.prior_float32(c)
        np.testing.assert_allclose(f.gposes, w.gposes, atol=1e-6)
        np.testing.assert_allclose(f.gbetas, w.gbetas, atol=1e-6)
        np.testing.assert_allclose(f.loss3[0], w.loss3[0], rtol=1e-5)
    # nbatches multiplies the scale gradient and nothing else
    a = ic.prior_case(3, 2, 1, 'large')
    b = a._replace(nbatches=3)
    ra, rb = ic.prior_reference(a), ic.prior_reference(b)
    np.testing.assert_allclose(rb.gxscale - b.gxscale0, 3 * (ra.gxscale - a.gxscale0), rtol=1e-12)
    assert np.abs(ra.gxscale - a.gxscale0).min() > 1e-3
    np.testing.assert_array_equal(ra.gposes, rb.gposes)
    np.testing.assert_array_equal(ra.gbetas, rb.gbetas)
    np.testing.assert_array_equal(ra.loss3, rb.loss3)
    y = ic.prior_yardstick()
    for k in sorted(y, key=str):
        print('float32 numpy against float64, worst over the cases: %-13s xscale %-5s %.3e' % (k[0], k[1], y[k]))
    assert y[('body_loss', None)] < 1e-6
    for g in ('scale_avg', 'scale_person', 'gxscale'):
        assert y[(g, 'zero')] == 0 and y[(g, 'null')] == 0
        assert y[(g, 'large')] < 1e-5
    assert y[('gxscale', 'small')] < 1e-6


def test_the_switch_of_the_scale_term():
    """coef_scales = 0 switches the (coef > 0) * (sum(s-1))^2 term off: no scale gradient at all"""
    c = ic.prior_case(3, 2, 3, 'large', cs=0.0)
    w = ic.prior_reference(c)
    assert (w.gxscale == c.gxscale0).all() and w.loss3[1] > 0
    assert (ic.prior_float32(c).gxscale == c.gxscale0).all()


# ---- sums ------------------------------------------------------------------------------------------------------------------
def test_sum_cases_cancel():
    for n in ic.SUM_LENGTHS:
        x = ic.sum_input(n)
        want = ic.sum_reference(x)
        mag = ic.sum_reference(np.abs(x))
        got = float(np.sum(x, dtype=np.float32))
        print('n = %5d: float32 numpy sum error %.3e, bound %.3e, |sum| / sum|x| = %.3f'
              % (n, abs(got - want), ic.sum_bound(x), abs(want) / mag if mag else 0))
        assert abs(got - want) <= ic.sum_bound(x)
        if n >= 255:
            assert abs(want) < 0.2 * mag and (x > 0).any() and (x < 0).any()
    assert ic.sum_reference(ic.sum_input(0)) == 0.0 and ic.sum_bound(ic.sum_input(0)) == 0.0


# ---- losses ---------------------------------------------------------------------------------------------------------------
def _close(got, want, scale, rtol, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= rtol * scale + 1e-300).all(), '%s: worst error / scale %.3e' % (what, float((err / np.maximum(scale, 1e-300)).max()))
    return float((err / np.maximum(scale, 1e-300)).max()) if np.size(err) else 0.0


def test_depth_reference_reproduces_the_fixture(golden_image, golden):
    cases = dict(gi.image_depth_loss_cases())
    assert set(cases) == {'t1_m1', 't1_m3', 't3_m1', 't3_m3', 'soft_mask'}
    e = np.float32(1e-3)
    for name, (pred, true, mask) in cases.items():
        for a in (pred, true):
            flat = a.reshape(-1)
            assert (flat == e).any() and (flat == np.nextafter(e, np.float32(0), dtype=np.float32)).any() and (flat == 0).any() and (flat < 0).any()
        assert (set(np.unique(mask)) <= {0.0, 1.0}) == (name != 'soft_mask')
        r = ic.depth_reference(pred, true, mask)
        # the fixture is float32 torch: it is held to the tolerances the kernels are held to
        w = _close(golden_image['depth_' + name], r.loss, r.loss_scale, ic.LOSS_RTOL, name)
        _close(golden_image['depth_%s_gpred' % name], r.gpred, r.gpred_scale, ic.GRAD_RTOL, name + ' gpred')
        _close(golden_image['depth_%s_gtrue' % name], r.gtrue, r.gtrue_scale, ic.GRAD_RTOL, name + ' gtrue')
        # below eps no gradient, at eps the gradient of the unclamped branch (>=)
        gp = golden_image['depth_%s_gpred' % name]
        m = np.broadcast_to(mask, pred.shape)
        assert (gp[pred < e] == 0).all() and (gp[(pred == e) & (m > 0)] != 0).all()
        assert (r.gpred[pred < e] == 0).all() and (r.gpred[(pred == e) & (m > 0)] != 0).all()
        f32 = abs(float(ic.depth_float32(pred, true, mask)) - r.loss) / r.loss_scale
        print('depth %-9s float32 numpy error / scale %.3e, reference torch float32 %.3e, cancellation |loss| / scale %.3f'
              % (name, f32, w, r.loss / r.loss_scale))
        assert f32 < ic.LOSS_RTOL
    pred, true, mask = gi.image_loss_inputs()
    r = ic.depth_reference(pred, true, mask)
    _close(golden['depth_loss'], r.loss, r.loss_scale, ic.LOSS_RTOL, 'depth_loss')
    _close(golden['depth_loss_gpred'], r.gpred, r.gpred_scale, ic.GRAD_RTOL, 'depth_loss_gpred')
    _close(golden['depth_loss_gtrue'], r.gtrue, r.gtrue_scale, ic.GRAD_RTOL, 'depth_loss_gtrue')


def test_mse_reference_reproduces_the_fixture(golden_image, golden):
    cases = dict(gi.image_mse_cases())
    for name, (y1, y2, mask) in cases.items():
        r = ic.mse_reference(y1, y2, mask)
        assert r.g2.shape == y2.shape
        np.testing.assert_allclose(r.g2, -torch.tensor(r.g1).sum_to_size(y2.shape).numpy(), rtol=1e-12, atol=1e-18)
        _close(golden_image['mse_' + name], r.loss, abs(r.loss), ic.LOSS_RTOL, name)
        _close(golden_image['mse_%s_g1' % name], r.g1, np.abs(r.g1), ic.GRAD_RTOL, name + ' g1')
        _close(golden_image['mse_%s_g2' % name], r.g2, r.g2_scale, ic.GRAD_RTOL, name + ' g2')
        assert np.abs(r.g2).max() > 0
        print('mse %-9s float32 numpy relative error %.3e' % (name, abs(float(ic.mse_float32(y1, y2, mask)) - r.loss) / r.loss))
    y1, y2, mask = cases['broadcast']
    assert y2.shape[1] == 1 and mask.shape[0] == 1 and mask.shape[3] == 1 and y1.shape == (2, 3, 5, 7)
    pred, true, mask = gi.image_loss_inputs()
    r = ic.mse_reference(pred[:, 0], true[:, 0], mask[:, 0])
    _close(golden['mse_loss'], r.loss, abs(r.loss), ic.LOSS_RTOL, 'mse_loss')
    _close(golden['mse_loss_grad'], r.g1, np.abs(r.g1), ic.GRAD_RTOL, 'mse_loss_grad')


def test_row_and_flat_cases():
    assert [h * w for h, w in ic.DEPTH_PIXELS] == [1, 255, 257]
    e = np.float32(1e-3)
    for H, W in ic.DEPTH_PIXELS:
        for group in (1, 3):
            pred, true, mask = ic.depth_rows_case(H, W, group)
            assert true.shape[1] == (1 if group > 1 else 3) and len(np.unique(mask[1])) > 2
            assert (pred == e).any() and (true < e).any()
            r = ic.depth_reference(pred, true, mask)
            assert np.isfinite(r.loss) and r.loss_scale >= r.loss > 0
    for n in ic.MSE_COUNTS:
        a, b, m = ic.mse_flat_case(n)
        assert a.shape == (n,) and ic.mse_reference(a, b, m).loss >= 0
