"""Plain high-precision references of the per-cycle kernels (csrc/mh_optim.hip) and of the key-point term
(csrc/mh_keypoints.hip): NumPy / torch-CPU, float64 unless ``dtype`` says otherwise, no GPU.

Every function restates the recurrence or the loss of ``oracle/fit_oracle.py`` (itself pinned to the reference's
fixtures by tests/test_oracle_golden.py); tests/test_cycle_ref.py pins them to it.  With ``dtype=float32`` the same
compositions are the project's float32 oracle the GPU tests measure their gates with.
"""
import math

import numpy as np
import torch

from oracle import fit_oracle as fo
from oracle import lbs_oracle as lo

NKP = 17


# ---- optimiser updates (fit_oracle.py:144-159) -------------------------------------------------------------------------------

def rmsprop64(p, g, sq, buf, lr, alpha=0.5, momentum=0.9, eps=1e-8):
    """one step on float64 arrays, in place (square_avg, momentum buffer, parameters)"""
    sq *= alpha
    sq += (1 - alpha) * g * g
    buf *= momentum
    buf += g / (np.sqrt(sq) + eps)
    p -= lr * buf


def adam64(p, g, m, v, step, lr, b1=0.5, b2=0.5, eps=1e-6):
    """one step on float64 arrays, in place; ``step`` counts from 1"""
    m *= b1
    m += (1 - b1) * g
    v *= b2
    v += (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    p -= (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)


# ---- one-euro filter (fit_oracle.one_euro_sequence) ---------------------------------------------------------------------------

def one_euro_time_before(first_frame, frame_rate=25):
    """the float32 running time stamp after global frame ``first_frame - 1``"""
    t = np.float32(0)
    for i in range(1, int(first_frame)):
        t = np.float32(t + np.float32(i / frame_rate))
    return t


def one_euro64(x, min_cutoff, beta, frame_rate=25, state=None, dtype=np.float64):
    """x (T, ...) -> (y (T, ...) float64, dx_hat of the last frame).

    The arithmetic is float64; the time stamp stays the reference's float32 running sum of ``i / frame_rate`` and the
    elapsed time the float32 difference of two such sums (the quirk is part of the semantics).
    ``state = (x_prev, dx_prev, first_frame)``: x holds the global frames first_frame, first_frame + 1, ... of a longer
    sequence and every one of them is filtered; without it frame 0 passes through.
    ``dtype=np.float32``: fit_oracle.one_euro_sequence operation for operation (the same bits), with the state."""
    x = np.asarray(x, dtype)
    y = x.copy()
    two_pi = 2 * math.pi
    if state is None:
        x_prev, dx_prev, i0, k0 = x[0].copy(), np.zeros_like(x[0]), 0, 1
    else:
        x_prev, dx_prev, i0, k0 = np.asarray(state[0], dtype).reshape(x[0].shape), \
            np.asarray(state[1], dtype).reshape(x[0].shape), int(state[2]), 0
        assert i0 >= 1
    t_prev = time_i = one_euro_time_before(i0 + k0, frame_rate)
    for k in range(k0, len(x)):
        time_i = np.float32(time_i + np.float32((i0 + k) / frame_rate))
        t_e = np.dtype(dtype).type(np.float32(time_i - t_prev))      # python scalars below are weak (NEP 50)
        r = two_pi * t_e
        a_d = r / (r + 1)
        dx = (x[k] - x_prev) / t_e
        dx_hat = a_d * dx + (1 - a_d) * dx_prev
        cutoff = float(min_cutoff) + float(beta) * np.abs(dx_hat)
        r = two_pi * cutoff * t_e
        a = r / (r + 1)
        x_hat = a * x[k] + (1 - a) * x_prev
        x_prev, dx_prev, t_prev = x_hat, dx_hat, time_i
        y[k] = x_hat
    return y, dx_prev


# ---- temporal terms (fit_oracle.SequenceOracle.temporal_loss) -----------------------------------------------------------------

def _pairs(d, T, has_prev, coef):
    """d: differences of consecutive frames of [prev?] + own + [next?] -> (sum over the owned pairs, coef * gradient)"""
    n_own = T if has_prev else T - 1               # the pair (t-1, t) belongs to the owner of t: the first n_own of d
    loss = (d[:n_own] ** 2).sum(dtype=d.dtype)
    g = np.zeros((T,) + d.shape[1:], d.dtype)
    o = 1 if has_prev else 0                       # d[o + t - 1] is the pair (t-1, t), d[o + t] the pair (t, t+1)
    for t in range(T):
        if o + t - 1 >= 0:
            g[t] += 2 * d[o + t - 1]
        if o + t < len(d):
            g[t] -= 2 * d[o + t]
    return loss, (d.dtype.type(coef) * g)


def velocity64(pT, coef, prev=None, nxt=None, dtype=np.float64):
    """sum_t |pT[t] - pT[t-1]|^2 over the owned pairs and coef * d/d pT; prev / nxt: the neighbouring ranks' frames"""
    x = np.asarray(pT, dtype)
    T = x.shape[0]
    seq = ([np.asarray(prev, dtype).reshape((1,) + x.shape[1:])] if prev is not None else []) + [x] + \
          ([np.asarray(nxt, dtype).reshape((1,) + x.shape[1:])] if nxt is not None else [])
    seq = np.concatenate(seq, 0)
    return _pairs(seq[1:] - seq[:-1], T, prev is not None, coef)


def filtered64(v, vf, coef, prev=None, nxt=None, dtype=np.float64):
    """sum_t |(v[t] - v[t-1]) - (vf[t] - vf[t-1])|^2 over the owned pairs and coef * d/d v; prev / nxt: (v, vf) pairs"""
    x, xf = np.asarray(v, dtype), np.asarray(vf, dtype)
    T = x.shape[0]
    row = lambda a: np.asarray(a, dtype).reshape((1,) + x.shape[1:])
    sv = ([row(prev[0])] if prev is not None else []) + [x] + ([row(nxt[0])] if nxt is not None else [])
    sf = ([row(prev[1])] if prev is not None else []) + [xf] + ([row(nxt[1])] if nxt is not None else [])
    sv, sf = np.concatenate(sv, 0), np.concatenate(sf, 0)
    return _pairs((sv[1:] - sv[:-1]) - (sf[1:] - sf[:-1]), T, prev is not None, coef)


# ---- projection + 2D residual (fit_oracle.project_points, batch_loss, init_global_poses) --------------------------------------

def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _residual(joints, K, Kd, pose2d, thr, mode, img_w, img_h, jw, dtype):
    """joints (B,17,3) torch -> uv (B,17,2), per-body loss (B,)"""
    B = joints.shape[0]
    Kt = _t(K, dtype).reshape(1, 3, 3).expand(B, 3, 3)
    kd = None if Kd is None else [float(np.float32(c)) for c in Kd]
    uv = fo.project_points(joints, Kt, kd)                   # keeps the (sic) second tangential term
    conf, thr = np.asarray(pose2d, np.float32)[..., 2:3], np.float32(thr)
    w = np.ones(NKP, np.float32) if jw is None else np.asarray(jw, np.float32)
    gt = _t(np.asarray(pose2d, np.float32)[..., :2], dtype)
    if mode == 0:                                            # batch_loss: mask = weights * (conf >= thr), normalised pixels
        c = _t(w.reshape(1, NKP, 1) * (conf >= thr), dtype)
        nrm = torch.tensor([float(img_w), float(img_h)], dtype=dtype)
        loss = ((c * uv / nrm - c * gt / nrm) ** 2).sum(dim=(1, 2))
    else:                                                    # init_global_poses: weights * (conf > thr), mean over B*17*2
        c = _t(w.reshape(1, NKP, 1) * (conf > thr), dtype)
        loss = ((c * uv - c * gt) ** 2).sum(dim=(1, 2)) / (B * NKP * 2)
    return uv, loss


def project_loss64(joints, K, Kd, pose2d, thr, mode, img_w, img_h, coef=1.0, jw=None, dtype=torch.float64):
    """-> uv (B,17,2), loss (B,) (without ``coef``), coef * d sum(loss) / d joints (B,17,3), by autograd"""
    j = _t(joints, dtype).requires_grad_(True)
    uv, loss = _residual(j, K, Kd, pose2d, thr, mode, img_w, img_h, jw, dtype)
    (coef * loss.sum()).backward()
    return uv.detach().numpy(), loss.detach().numpy(), j.grad.numpy()


def warmup64(local, xscale, transl, NB, K, Kd, pose2d, thr, coef=1.0, jw=None, dtype=torch.float64):
    """joints = 1.1 ** xscale[b % NB] * local + transl through the mode-1 residual -> loss (B,), coef * d/d transl (B,3)"""
    B = np.asarray(local).shape[0]
    tt = _t(transl, dtype).requires_grad_(True)
    if xscale is None:
        sc = torch.ones(B, 1, 1, dtype=dtype)
    else:
        sc = torch.pow(torch.tensor(1.1, dtype=dtype), _t(xscale, dtype)[torch.arange(B) % NB]).view(B, 1, 1)
    j = sc * _t(local, dtype) + tt.view(B, 1, 3)
    _, loss = _residual(j, K, Kd, pose2d, thr, 1, 1.0, 1.0, jw, dtype)
    (coef * loss.sum()).backward()
    return loss.detach().numpy(), tt.grad.numpy()


# ---- key-point term --------------------------------------------------------------------------------------------------------------

def keypoint64(model, betas, poses, xscale, transl, K, Kd, pose2d, thr, img_w, img_h, coef=1.0, jw=None):
    """``model``: lbs_oracle.BodyModel(..., dtype=float64).  betas (NB,10), poses (B,72), xscale (NB,), transl (B,3);
    body b has shape and scale b % NB.  -> dict kp (B,17,3), uv, loss (B,), and the gradients of coef * sum(loss) with
    respect to poses, transl, betas, xscale."""
    dtype = model.dtype
    B, NB = np.asarray(poses).shape[0], np.asarray(betas).shape[0]
    bidx = torch.arange(B) % NB
    tb, tp = _t(betas, dtype).requires_grad_(True), _t(poses, dtype).requires_grad_(True)
    tx, tt = _t(xscale, dtype).requires_grad_(True), _t(transl, dtype).requires_grad_(True)
    out = lo.smpl_forward(model, tb[bidx], tp)
    s = torch.pow(torch.tensor(1.1, dtype=dtype), tx[bidx])[:, None, None]
    kp = s * out['joints_alphapose'] + tt[:, None]
    uv, loss = _residual(kp, K, Kd, pose2d, thr, 0, img_w, img_h, jw, dtype)
    (coef * loss.sum()).backward()
    return dict(kp=kp.detach().numpy(), uv=uv.detach().numpy(), loss=loss.detach().numpy(), poses=tp.grad.numpy(),
                transl=tt.grad.numpy(), betas=tb.grad.numpy(), xscale=tx.grad.numpy())
