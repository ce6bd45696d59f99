"""Pins tests/cycle_ref.py (the float64 references of the per-cycle kernels) to the oracle and to the reference's
fixtures.  No GPU."""
import numpy as np
import torch

import cycle_ref as cr
import golden_inputs as gi
from oracle import fit_oracle as fo
from oracle import lbs_oracle as lo


def test_updates_agree_with_the_oracle():
    rng = np.random.RandomState(9)
    n = 1000
    p0 = rng.normal(0, 1, n)
    for name in ('rmsprop', 'adam'):
        p, a, b = p0.copy(), np.zeros(n), np.zeros(n)
        tp, ta, tb = torch.tensor(p0), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        lr = 0.01 if name == 'rmsprop' else 0.5
        for it in range(5):
            g = rng.normal(0, 1, n) * (it != 3)
            if name == 'rmsprop':
                cr.rmsprop64(p, g, a, b, lr)
                fo.rmsprop_step(tp, torch.tensor(g), ta, tb, lr)
            else:
                cr.adam64(p, g, a, b, it + 1, lr)
                fo.adam_step(tp, torch.tensor(g), ta, tb, it + 1, lr)
            lr *= 0.99
        # the same recurrence in the same precision: rounding of differently grouped float64 operations only
        np.testing.assert_allclose(p, tp.numpy(), rtol=0, atol=1e-14)
        np.testing.assert_allclose(a, ta.numpy(), rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(b, tb.numpy(), rtol=0, atol=1e-13)


def test_one_euro_agrees_with_the_oracle_and_the_fixtures(golden):
    x = gi.one_euro_inputs()
    for (c, b), key in [((0.01, 0.02), 'one_euro_a'), ((0.001, 0.5), 'one_euro_b')]:
        y, _ = cr.one_euro64(x, c, b)
        np.testing.assert_allclose(y, golden[key], rtol=0, atol=1e-6)              # the fixture's own gate (test_oracle_golden)
        np.testing.assert_allclose(y, fo.one_euro_sequence(x, c, b), rtol=0, atol=5e-8)
        # in float32 it IS the oracle (so its outgoing dx is the oracle's, which one_euro_sequence does not return)
        y32, _ = cr.one_euro64(x, c, b, dtype=np.float32)
        assert y32.dtype == np.float32 and np.array_equal(y32, fo.one_euro_sequence(x, c, b))
    rng = np.random.RandomState(4)
    worst = 0.0
    for T in (2, 9, 17, 40):
        for c, b in [(0.01, 0.02), (0.001, 0.5)]:
            w = np.cumsum(rng.normal(0, 0.02, (T, 64)), axis=0)
            w = (0.5 * w / max(0.5, np.abs(w).max())).astype(np.float32)          # |x| <= 0.5
            y, _ = cr.one_euro64(w, c, b)
            worst = max(worst, float(np.abs(y - fo.one_euro_sequence(w, c, b)).max()))
    print('float32 oracle against one_euro64, random walks: %.2e' % worst)
    assert worst <= 5e-8


def test_one_euro_is_continuous_under_sharding():
    rng = np.random.RandomState(6)
    x = np.cumsum(rng.normal(0, 0.02, (17, 3, 5)), axis=0)
    whole, dx_whole = cr.one_euro64(x, 0.01, 0.02)
    for cut in (1, 7, 8, 9, 16):
        a, dxa = cr.one_euro64(x[:cut], 0.01, 0.02)
        b, dxb = cr.one_euro64(x[cut:], 0.01, 0.02, state=(a[-1], dxa, cut))
        assert np.array_equal(np.concatenate([a, b]), whole), cut
        assert np.array_equal(dxb, dx_whole), cut
    a, dxa = cr.one_euro64(x[:5], 0.01, 0.02)
    b, dxb = cr.one_euro64(x[5:11], 0.01, 0.02, state=(a[-1], dxa, 5))
    c, dxc = cr.one_euro64(x[11:], 0.01, 0.02, state=(b[-1], dxb, 11))
    assert np.array_equal(np.concatenate([a, b, c]), whole) and np.array_equal(dxc, dx_whole)
    assert float(cr.one_euro_time_before(1)) == 0.0


def test_temporal_terms_agree_with_autograd_and_split_with_halos():
    rng = np.random.RandomState(17)
    T, E = 9, 30
    v, vf = rng.normal(0, 1, (T, E)), rng.normal(0, 1, (T, E))
    tv = torch.tensor(v, requires_grad=True)
    lv = ((tv[1:] - tv[:-1]) ** 2).sum()                                          # fit_oracle.temporal_loss
    (0.05 * lv).backward()
    l, g = cr.velocity64(v, 0.05)
    np.testing.assert_allclose(l, float(lv.detach()), rtol=1e-14)
    np.testing.assert_allclose(g, tv.grad.numpy(), rtol=0, atol=1e-14)
    tv = torch.tensor(v, requires_grad=True)
    tf = torch.tensor(vf)
    lf = (((tv[1:] - tv[:-1]) - (tf[1:] - tf[:-1])) ** 2).sum()
    (0.002 * lf).backward()
    l, g = cr.filtered64(v, vf, 0.002)
    np.testing.assert_allclose(l, float(lf.detach()), rtol=1e-14)
    np.testing.assert_allclose(g, tv.grad.numpy(), rtol=0, atol=1e-15)
    for cuts in ([4], [1], [8], [3, 4]):                                          # a one-frame shard has both halos
        b = [0] + cuts + [T]
        ls, gs, lfs, gfs = 0.0, [], 0.0, []
        for s, e in zip(b[:-1], b[1:]):
            l1, g1 = cr.velocity64(v[s:e], 0.05, prev=v[s - 1] if s else None, nxt=v[e] if e < T else None)
            l2, g2 = cr.filtered64(v[s:e], vf[s:e], 0.002, prev=(v[s - 1], vf[s - 1]) if s else None,
                                   nxt=(v[e], vf[e]) if e < T else None)
            ls, lfs = ls + l1, lfs + l2
            gs.append(g1)
            gfs.append(g2)
        np.testing.assert_allclose(ls, float(lv.detach()), rtol=1e-14)
        np.testing.assert_allclose(lfs, float(lf.detach()), rtol=1e-14)
        np.testing.assert_allclose(np.concatenate(gs), cr.velocity64(v, 0.05)[1], rtol=0, atol=1e-14)
        np.testing.assert_allclose(np.concatenate(gfs), g, rtol=0, atol=1e-15)
    l, g = cr.filtered64(v[:1], vf[:1], 0.002)
    assert l == 0 and not g.any()


def test_project_loss_agrees_with_the_oracle_construction(golden):
    """fo.project_points + autograd, as tests/test_lbs_gpu.py::test_project_joints_loss builds it"""
    pts, K, Kd = gi.projection_inputs()
    rng = np.random.RandomState(5)
    p2d = np.concatenate([rng.uniform(0, 200, (5, 17, 2)), rng.uniform(0, 1, (5, 17, 1))], -1).astype(np.float32)
    for kd, key in [(None, 'proj_plain'), (Kd, 'proj_dist')]:
        for mode, thr in [(0, 0.5), (1, 0.15)]:
            uv, loss, gj = cr.project_loss64(pts, K[0], kd, p2d, thr, mode, 240, 135, coef=0.7)
            np.testing.assert_allclose(uv, golden[key], rtol=0, atol=1e-4)          # test_camera's gate on the fixture
            tp = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
            puv = fo.project_points(tp, torch.tensor(K, dtype=torch.float64), None if kd is None else [float(c) for c in kd])
            gt = torch.tensor(p2d[..., :2], dtype=torch.float64)
            if mode == 0:
                c = torch.tensor((p2d[..., 2:] >= np.float32(thr)).astype(np.float64))
                nrm = torch.tensor([240.0, 135.0], dtype=torch.float64)
                l = ((c * puv / nrm - c * gt / nrm) ** 2).sum()
            else:
                c = torch.tensor((p2d[..., 2:] > np.float32(thr)).astype(np.float64))
                l = torch.mean((c * puv - c * gt) ** 2)
            (0.7 * l).backward()
            np.testing.assert_allclose(loss.sum(), float(l.detach()), rtol=1e-13)
            np.testing.assert_allclose(gj, tp.grad.numpy(), rtol=0, atol=1e-13 * np.abs(gj).max())
    # the warm-up form is the mode-1 residual of scaled, translated local joints
    xs, tr = np.array([0.5, -1.0]), rng.normal(0, 1, (5, 3)) + [0, 0, 4]
    loss, gt = cr.warmup64(pts, xs, tr, 2, K[0], Kd, p2d, 0.15, coef=0.7)
    sc = (1.1 ** xs[np.arange(5) % 2])[:, None, None]
    _, want, gj = cr.project_loss64(sc * pts + tr[:, None], K[0], Kd, p2d, 0.15, 1, 1, 1, coef=0.7)
    np.testing.assert_allclose(loss, want, rtol=1e-13)
    np.testing.assert_allclose(gt, gj.sum(1), rtol=0, atol=1e-13 * np.abs(gt).max())


def test_keypoint64_agrees_with_the_fixture(golden, smpl_struct, smpl_regs):
    m64 = lo.BodyModel(smpl_struct, smpl_regs, dtype=torch.float64)
    betas, poses = gi.lbs_inputs()
    B = poses.shape[0]
    K = np.array([[117.0, 0.3, 120.0], [0.1, 118.5, 67.5], [0, 0, 1]], np.float32)
    p2d = np.ones((B, 17, 3), np.float32)
    tr = np.tile(np.array([[0.1, -0.2, 5.0]]), (B, 1))
    out = cr.keypoint64(m64, betas, poses, np.zeros(B), np.zeros((B, 3)), K, None, p2d, 0.5, 240, 135)
    np.testing.assert_allclose(out['kp'], golden['smpl_joints_alphapose'], rtol=0, atol=2e-6)   # test_oracle_golden's gate
    out = cr.keypoint64(m64, betas, poses, np.full(B, 2.0), tr, K, None, p2d, 0.5, 240, 135)
    np.testing.assert_allclose(out['kp'], 1.21 * golden['smpl_joints_alphapose'] + tr[:, None], rtol=0, atol=3e-6)
    uv, loss, gj = cr.project_loss64(out['kp'], K, None, p2d, 0.5, 0, 240, 135)
    np.testing.assert_allclose(out['uv'], uv, rtol=0, atol=1e-10)
    np.testing.assert_allclose(out['loss'], loss, rtol=1e-12)
    np.testing.assert_allclose(out['transl'], gj.sum(1), rtol=0, atol=1e-12 * np.abs(gj).max())
    assert all(np.abs(out[k]).max() > 0 for k in ('poses', 'betas', 'xscale'))
