"""mh_keypoint_terms (k_kp_p, k_kp_mid, k_kp_gf of csrc/mh_keypoints.hip) and the backward that consumes its chunk
(mh_lbs_backward_kp with gverts = NULL) against tests/cycle_ref.keypoint64: the float64 oracle's key-points, scaled,
translated, projected and compared with the detections, with autograd gradients down to the leaves.

Call sequence of tests/test_keypoints_gpu.py: lbs_forward, mh_keypoint_terms, mh_lbs_backward_kp -- here on plain device
tensors, without an optimiser, at B = 1, 31, 32, 33 (the 32-body group edge: one full group, one body into the second) and 65
(three groups), in the exact-fp32 and in the split 16-bit LBS mode (mh_lbs_backward_extra_slot lays the extra chunk out per
mode).  Every output, the key-point workspace (mh_keypoint_workspace_bytes) and the backward's workspace sit between canaries.

Gates.  kp, uv, loss: twice the deviation from keypoint64 of the VERTEX path on the same inputs (joints_regress on the
forward's vertices, then mh_project_joints_loss_w; pinned to the reference by tests/test_lbs_gpu.py), measured in the test.
Leaf gradients: the gates of tests/test_lbs_fuzz_gpu.py for lbs_backward against float64 -- 5e-5 of the leaf's largest entry,
2e-3 for xscale.  One detection per body has its confidence exactly at the threshold (it counts: mode 0 is >=), one lies below.

The loss is a summed loss, so its gate also has the 4-ulp floor every summed loss has: at B = 1 the vertex path's ONE loss value
sits 4e-8 to 6e-8 from float64, a third of an ulp of its value 1.7 (a gate of 1.1e-7), which no float32 result can be held to
-- the kernel's is 1.8e-7 away, one and a half ulp.  At B >= 31 the kernel is also inside the unfloored gate (0.62 to 0.76 of it).

Measured on the MI355X, largest error as a fraction of its gate, the same in both LBS modes unless two figures are given (every case
prints its own with pytest -s): kp 0.24 to 0.35; uv 0.50 to 0.86; loss 0.22 to 0.47 (of the floored gate); leaf gradients: poses
0.01, transl 0.01, betas 0.01, xscale 0.00 -- i.e. 5e-7 of the leaf's largest entry.
"""
import numpy as np
import pytest
import torch

import cycle_ref as cr
import golden_inputs as gi
import test_cycle_kernels_gpu as ck
from oracle import lbs_oracle as lo

pytestmark = pytest.mark.gpu

W_IMG, H_IMG, THR, COEF = 240.0, 135.0, 0.5, 0.7
NB_OF = {1: 1, 31: 31, 32: 4, 33: 3, 65: 5}
VARIANTS = [(False, False), (False, True), (True, True)]          # (distortion, non-uniform joint weights)
_REF = {}


@pytest.fixture(scope='module')
def models(smpl_struct, smpl_regs):
    from mhhip import engine
    return engine.BodyModel(smpl_struct, smpl_regs), lo.BodyModel(smpl_struct, smpl_regs, dtype=torch.float64)


def _inputs(B):
    NB = NB_OF[B]
    rng = np.random.RandomState(300 + B)
    betas = rng.normal(0, 0.7, (NB, 10)).astype(np.float32)                 # as test_backward_matches_autograd
    poses = rng.normal(0, 0.3, (B, 72)).astype(np.float32)
    poses[:, 66:] = 0                                                        # hand rotations are zero
    xs = rng.normal(0, 1.0, (NB,)).astype(np.float32)
    tr = np.concatenate([rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(3, 8, (B, 1))], -1).astype(np.float32)
    p2d = np.concatenate([rng.uniform(0, W_IMG, (B, 17, 1)), rng.uniform(0, H_IMG, (B, 17, 1)), rng.uniform(0, 1, (B, 17, 1))],
                         -1).astype(np.float32)
    p2d[np.arange(B), rng.randint(0, 8, B), 2] = np.float32(THR)            # exactly at the threshold: counts
    p2d[np.arange(B), rng.randint(8, 17, B), 2] = 0.25                      # below it
    _, K, Kd = gi.projection_inputs()
    return NB, betas, poses, xs, tr, p2d, K[0], Kd


def _ref(m64, B, dist, weighted):
    """float64 reference, computed once per (B, variant) and shared by both LBS modes"""
    key = (B, dist, weighted)
    if key not in _REF:
        NB, betas, poses, xs, tr, p2d, K, Kd = _inputs(B)
        _REF[key] = cr.keypoint64(m64, betas, poses, xs, tr, K, Kd if dist else None, p2d, THR, W_IMG, H_IMG, COEF,
                                  ck.JW if weighted else None)
        at = p2d[..., 2] == np.float32(THR)
        assert at.sum() == B
    return _REF[key]


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('B', [1, 31, 32, 33, 65])
def test_keypoint_terms_against_float64(models, B, mode):
    from mhhip import engine
    hip, m64 = models
    L, check, st = ck.lib()
    ptr, dev = ck.ptr, ck.dev
    NB, betas, poses, xs, tr, p2d, K, Kd = _inputs(B)
    Kh = np.ascontiguousarray(K.reshape(9), np.float32)
    mode0 = L.mh_lbs_get_mode()
    try:
        check(L.mh_lbs_set_mode(mode))
        db, dp, dx, dt, d2 = dev(betas), dev(poses), dev(xs), dev(tr), dev(p2d)
        verts, vposed, _, ws = hip.lbs_forward(db, dp, dx, dt)
        kp_v = hip.joints_regress(engine.REG_ALPHAPOSE, verts, corr=dt)
        for dist, weighted in VARIANTS:
            ref = _ref(m64, B, dist, weighted)
            kdh = np.asarray(Kd, np.float32) if dist else None
            jw = ck.JW if weighted else None
            # the vertex path on the same inputs: what the gates of kp, uv and loss are measured with
            uv_v, gj_v, l_v = torch.empty(B, 17, 2, device=ck.DEV), torch.empty(B, 17, 3, device=ck.DEV), torch.empty(B, device=ck.DEV)
            check(L.mh_project_joints_loss_w(B, ptr(kp_v), ck._fp(Kh), ck._fp(kdh), ck._fp(jw), ptr(d2), THR, 0, W_IMG, H_IMG, COEF,
                                             ptr(uv_v), ptr(gj_v), ptr(l_v), st))
            gate = {k: 2.0 * float(np.abs(v.cpu().numpy().astype(np.float64) - ref[k]).max())
                    for k, v in (('kp', kp_v), ('uv', uv_v), ('loss', l_v))}
            # the loss is a summed loss: its gate has the 4-ulp floor of every summed loss (module docstring)
            floor = 4 * ck.EPS32 * float(np.abs(ref['loss']).max())
            if floor > gate['loss']:
                print('B %d mode %d: loss gate %.2e from the vertex path raised to the 4-ulp floor %.2e' % (B, mode, gate['loss'], floor))
                gate['loss'] = floor
            G = ck.Guard()
            kp, uv, gkp, loss = G((B, 17, 3), init=9.0), G((B, 17, 2), init=9.0), G((B, 17, 3), init=9.0), G(B, init=9.0)
            kp_ws = G(max(1, L.mh_keypoint_workspace_bytes(hip.handle, B)), dtype=torch.uint8, init=0)
            ws2 = G(L.mh_lbs_backward_workspace_bytes(B), dtype=torch.uint8, init=0)
            check(L.mh_keypoint_terms(hip.handle, B, ptr(dt), ck._fp(Kh), ck._fp(kdh), ck._fp(jw), ptr(d2), THR, W_IMG, H_IMG, COEF,
                                      ptr(kp), ptr(uv), ptr(gkp), ptr(loss), ptr(ws), ptr(ws2), ptr(kp_ws), st))
            G.check()
            tag = 'kp B%d mode%d ' % (B, mode)
            for k, got in (('kp', kp), ('uv', uv), ('loss', loss)):
                ck.within(tag + k, got, ref[k], gate[k])
            # values only: the same key-points and loss, bit for bit, and nothing of the backward's workspace touched
            kp2, loss2, before = G((B, 17, 3), init=9.0), G(B, init=9.0), ws2.clone()
            check(L.mh_keypoint_terms(hip.handle, B, ptr(dt), ck._fp(Kh), ck._fp(kdh), ck._fp(jw), ptr(d2), THR, W_IMG, H_IMG, COEF,
                                      ptr(kp2), None, None, ptr(loss2), ptr(ws), None, ptr(kp_ws), st))
            G.check()
            assert torch.equal(kp2, kp) and torch.equal(loss2, loss) and torch.equal(ws2, before)
            gp, gt, gb, gx = G((B, 72)), G((B, 3)), G((NB, 10)), G(NB)
            check(L.mh_lbs_backward_kp(hip.handle, B, NB, ptr(db), ptr(dp), ptr(vposed), None, ptr(gp), ptr(gt), ptr(gb), ptr(gx),
                                       ptr(ws), ptr(ws2), st))
            G.check()
            for name, got in (('poses', gp), ('transl', gt), ('betas', gb), ('xscale', gx)):
                scale = float(np.abs(ref[name]).max())
                assert scale > 0, name
                ck.within(tag + name, got, ref[name], (2e-3 if name == 'xscale' else 5e-5) * scale)
            assert not bool(gp[:, 66:].any())
        ck.report('kp B%d mode%d' % (B, mode))
    finally:
        check(L.mh_lbs_set_mode(mode0))
