"""The contact map's definition in numpy (include/mhmocap_hip.h, mh_scene_nearest / mh_contact_parts): a brute force over
all cloud points in float32, every operation rounded on its own and in the stated order, the tie rule, and the per-part
counts and minima.  The device kernels are compared with it bit for bit (tests/test_contact_gpu.py)."""
import numpy as np

F = np.float32


def nearest_ref(pts, q, radius, block=512):
    """pts (M,3), q (Q,3) float32 -> d2 (Q) float32, near (Q,3) float32: the smallest d2 = (dx dx + dy dy) + dz dz over the
    points with d2 <= radius radius, and the point that attains it -- on equal d2 the smallest x, then y, then z; +inf and
    (0,0,0) without a candidate or for a query that is not finite"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    M, Q = pts.shape[0], q.shape[0]
    d2o = np.full(Q, np.inf, F)
    near = np.zeros((Q, 3), F)
    if M == 0:
        return d2o, near
    r2 = F(radius) * F(radius)
    # lexicographic rank of every point by (x, y, z): equal points get ranks next to each other and are interchangeable
    order = np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0]))
    rank = np.empty(M, np.int64)
    rank[order] = np.arange(M)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(0, Q, block):
            qq = q[s:s + block]
            dx = pts[None, :, 0] - qq[:, None, 0]
            dy = pts[None, :, 1] - qq[:, None, 1]
            dz = pts[None, :, 2] - qq[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            cand = (d2 <= r2) & np.isfinite(qq).all(1)[:, None]
            dm = np.where(cand, d2, F(np.inf)).min(1)
            tie = cand & (d2 == dm[:, None])
            pick = np.where(tie, rank[None, :], M).min(1)
            has = pick < M
            d2o[s:s + block] = np.where(has, dm, F(np.inf))
            near[s:s + block][has] = pts[order[pick[has]]]
    return d2o, near


def nearest_ref64(pts, q, radius):
    """the same search in float64 without the tie rule: (d2 (Q), index of the nearest point or -1, second smallest d2)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    d2 = ((pts[None] - q[:, None]) ** 2).sum(-1)
    idx = d2.argmin(1)
    best = d2[np.arange(len(q)), idx]
    second = np.partition(d2, 1, axis=1)[:, 1] if pts.shape[0] > 1 else np.full(len(q), np.inf)
    inside = best <= float(radius) ** 2
    return np.where(inside, best, np.inf), np.where(inside, idx, -1), second


def parts_ref(d2, part, P, thr):
    """d2 (B,V) float32, part (V) uint8 -> counts (B,P) int32: vertices of the part with d2 <= thr thr (float32 product),
    min_d2 (B,P) float32: the smallest d2 of the part (NaN and negative values never), +inf without one"""
    d2 = np.asarray(d2, F)
    part = np.asarray(part)
    B = d2.shape[0]
    t2 = F(thr) * F(thr)
    counts = np.zeros((B, P), np.int32)
    mins = np.full((B, P), np.inf, F)
    with np.errstate(invalid='ignore'):
        for k in range(P):
            sel = d2[:, part == k]
            counts[:, k] = (sel <= t2).sum(1)
            if sel.shape[1]:
                mins[:, k] = np.where(sel >= 0, sel, F(np.inf)).min(1)
    return counts, mins


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)
