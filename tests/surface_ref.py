"""The point-to-surface distance's definition in numpy (include/mhmocap_hip.h: mh_surface_grid, mh_mesh_closest,
mh_person_surface, mh_surface_pairs): every face against every query, no grid, in float32 -- the bits the device must give --
or in float64, the yardstick for what float32 loses.  A restatement of the definitions, not of the kernels; ``grid_ref`` alone
mirrors the kernel's choice of a grid, for the status word."""
import numpy as np

from inside_ref import cube, icosphere, u_prism  # noqa: F401  (the shapes the tests use)

NOT_LIVE, ALL_FACES = 1, 4
MAX_DIM, MAX_CELLS, MIN_CELLS, CAP_PER_FACE, SHAPE_STEPS = 64, 8192, 256, 16, 128


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def tri_ref(q, a, b, c, dtype=np.float32):
    """q (Q,3) against the faces a, b, c (F,3) -> (D2 (Q,F), x (Q,F,3) closest point minus query, v, w (Q,F)) by the header's
    formula, every operation in ``dtype`` and in the header's order"""
    q = np.asarray(q, dtype)[:, None, :]
    a, b, c = (np.asarray(p, dtype)[None] for p in (a, b, c))
    one, zero = dtype(1), dtype(0)
    with np.errstate(all='ignore'):
        A, B, C, ab, ac = a - q, b - q, c - q, b - a, c - a
        d1, d2, d3, d4, d5, d6 = -_dot(ab, A), -_dot(ac, A), -_dot(ab, B), -_dot(ac, B), -_dot(ab, C), -_dot(ac, C)
        vc, vb, va, e1, e2 = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
        t = e1 / (e1 + e2)
        den = (va + vb) + vc
        regions = [((d1 <= 0) & (d2 <= 0), zero, zero),
                   ((d3 >= 0) & (d4 <= d3), one, zero),
                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                   ((d6 >= 0) & (d5 <= d6), zero, one),
                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                   ((va <= 0) & (e1 >= 0) & (e2 >= 0), one - t, t)]
        v, w = vb / den, vc / den
        for cond, rv, rw in reversed(regions):              # the FIRST region that holds wins: apply them last to first
            v = np.where(cond, rv, v).astype(dtype)
            w = np.where(cond, rw, w).astype(dtype)
        x = (A + ab * v[..., None]) + ac * w[..., None]
        D2 = _dot(x, x)
    assert D2.dtype == dtype and x.dtype == dtype
    return D2, x, v, w


def valid_faces(verts, faces):
    """faces that name three vertices in [0, V) with nine finite coordinates -> (valid (F) bool, corners (F,3,3))"""
    verts = np.asarray(verts)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    named = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    fc = np.where(named[:, None], faces, 0)
    P = verts[fc]
    return named & np.isfinite(P).all((1, 2)), P


def closest_ref(verts, faces, points, radius=np.inf, live=True, dtype=np.float32, block=64):
    """verts (V,3), faces (F,3), points (Q,3) -> (d2 (Q) dtype, face (Q) int32, point (Q,3), weights (Q,3) dtype): the smallest
    candidate D2, on a tie the smallest face; inf / -1 / zeros without a candidate"""
    verts, points = np.asarray(verts, np.float32), np.asarray(points, np.float32)
    nq = points.shape[0]
    d2, face = np.full(nq, np.inf, dtype), np.full(nq, -1, np.int32)
    point, weights = np.zeros((nq, 3), dtype), np.zeros((nq, 3), dtype)
    valid, P = valid_faces(verts, faces)
    if not live or not valid.any():
        return d2, face, point, weights
    ids = np.nonzero(valid)[0]
    P = P[valid]
    with np.errstate(all='ignore'):
        r2 = dtype(np.float32(radius)) * dtype(np.float32(radius))
    for q0 in range(0, nq, block):
        q = points[q0:q0 + block]
        D2, x, v, w = tri_ref(q, P[:, 0], P[:, 1], P[:, 2], dtype)
        cand = ~np.isnan(D2) & (D2 <= r2) & np.isfinite(q).all(1)[:, None]
        key = np.where(cand, D2, dtype(np.inf))
        best = key.min(1)
        k = np.argmax(cand & (D2 == best[:, None]), 1)      # the first face that attains it: the smallest index
        has = cand.any(1)
        r = np.arange(q.shape[0])
        sl = slice(q0, q0 + block)
        d2[sl] = np.where(has, best, dtype(np.inf))
        face[sl] = np.where(has, ids[k], -1)
        one = dtype(1)
        with np.errstate(all='ignore'):
            point[sl] = np.where(has[:, None], q.astype(dtype) + x[r, k], 0)
            weights[sl] = np.where(has[:, None], np.stack([(one - v[r, k]) - w[r, k], v[r, k], w[r, k]], 1), 0)
    return d2, face, point, weights


def grid_ref(verts, faces, live=True, force=False):
    """the status word mh_surface_grid gives the body, and the grid it chose: (status, dims (3), cell edge, list entries)"""
    f32 = np.float32
    verts = np.asarray(verts, f32)
    F = np.asarray(faces).reshape(-1, 3).shape[0]
    if not live:
        return NOT_LIVE, np.ones(3, np.int64), f32(1), 0
    fin = np.isfinite(verts).all(1)
    d, h, overflow = np.ones(3, np.int64), f32(1), False
    mn = np.zeros(3, f32)
    if fin.any():
        mn, mx = verts[fin].min(0), verts[fin].max(0)
        with np.errstate(all='ignore'):
            ext = mx - mn
        maxext = ext.max()
        if not np.isfinite(maxext):
            overflow = True
        elif maxext >= f32(1e-30):
            most = min(max(F // 2, MIN_CELLS), MAX_CELLS)
            e = maxext / f32(MAX_DIM)
            for _ in range(SHAPE_STEPS):
                d = np.minimum(np.floor(ext / e), f32(MAX_DIM - 1)).astype(np.int64) + 1
                if d.prod() <= most:
                    h = e
                    break
                e = e * f32(1.0625)
            else:
                d = np.ones(3, np.int64)
    total = 0
    valid, P = valid_faces(verts, faces)
    if valid.any() and not overflow:
        inv = f32(1) / h
        lo, hi = P[valid].min(1), P[valid].max(1)

        def cell(x):
            return np.fmin(np.fmax(np.floor((x - mn) * inv), f32(0)), (d - 1).astype(f32)).astype(np.int64)
        c0 = cell(lo)
        c1 = np.maximum(cell(hi), c0)
        total = int((c1 - c0 + 1).prod(1).sum())
    walks_all = force or overflow or total > CAP_PER_FACE * F
    return (ALL_FACES if walks_all else 0), d, h, total


def person_surface_ref(verts, faces, mask, radius, live=None, sub=None, dtype=np.float32):
    """verts (T,N,V,3), faces (F,3), mask (T,N,V) uint32 as mh_person_inside writes it (or None), live (T,N) or None; sub:
    the vertices asked about (default all) -> dict of out_d2, in_d2 (T,N,S) dtype, out_idx, in_idx (T,N,S) int32, out_pt,
    in_pt (T,N,S,3) dtype"""
    verts = np.asarray(verts, np.float32)
    T, N, V = verts.shape[:3]
    F = np.asarray(faces).reshape(-1, 3).shape[0]
    sub = np.arange(V) if sub is None else np.asarray(sub)
    S = len(sub)
    live = np.ones((T, N), bool) if live is None else np.asarray(live) != 0
    mask = np.zeros((T, N, V), np.uint32) if mask is None else np.asarray(mask).view(np.uint32)
    out_d2, in_d2 = np.full((T, N, S), np.inf, dtype), np.full((T, N, S), np.inf, dtype)
    out_idx, in_idx = np.full((T, N, S), -1, np.int32), np.full((T, N, S), -1, np.int32)
    out_pt, in_pt = np.zeros((T, N, S, 3), dtype), np.zeros((T, N, S, 3), dtype)
    for t in range(T):
        for n in range(N):
            if not live[t, n]:
                continue
            q = verts[t, n, sub]
            deepest = np.full(S, -1, dtype)
            for m in range(N):                              # ascending m: the smallest m on a tie
                if m == n or not live[t, m]:
                    continue
                ins = ((mask[t, n, sub] >> np.uint32(m)) & np.uint32(1)) != 0
                d_in, f_in, p_in, _ = closest_ref(verts[t, m], faces, q, np.inf, dtype=dtype)
                # within the radius: the smallest candidate D2 of all is a candidate there or nothing is (same D2, same tie)
                r2 = dtype(np.float32(radius)) * dtype(np.float32(radius))
                near = (f_in >= 0) & (d_in <= r2)
                d_out, f_out, p_out = np.where(near, d_in, dtype(np.inf)), np.where(near, f_in, -1), np.where(near[:, None], p_in, 0)
                up = ins & (f_in >= 0) & (d_in > deepest)
                deepest[up] = d_in[up]
                in_d2[t, n][up], in_idx[t, n][up], in_pt[t, n][up] = d_in[up], m * F + f_in[up], p_in[up]
                up = ~ins & (f_out >= 0) & ((out_idx[t, n] < 0) | (d_out < out_d2[t, n]))
                out_d2[t, n][up], out_idx[t, n][up], out_pt[t, n][up] = d_out[up], m * F + f_out[up], p_out[up]
    return dict(out_d2=out_d2, out_idx=out_idx, in_d2=in_d2, in_idx=in_idx, out_pt=out_pt, in_pt=in_pt)


def pairs_ref(out_d2, out_idx, in_d2, in_idx, part, P, contact, F):
    """the tables of mh_surface_pairs from (T,N,V) inputs: pair_depth_d2 (-1 = none), pair_min_d2 (inf = none) (T,N,N) float32,
    pair_contact (T,N,N) int32, and part_depth_d2, part_min_d2, part_contact (T,N,P)"""
    out_d2, in_d2 = np.asarray(out_d2, np.float32), np.asarray(in_d2, np.float32)
    T, N, V = out_d2.shape
    part = np.asarray(part).astype(np.int64)
    c2 = np.float32(contact) * np.float32(contact)
    out = dict(pair_depth_d2=np.full((T, N, N), -1, np.float32), pair_min_d2=np.full((T, N, N), np.inf, np.float32),
               pair_contact=np.zeros((T, N, N), np.int32), part_depth_d2=np.full((T, N, P), -1, np.float32),
               part_min_d2=np.full((T, N, P), np.inf, np.float32), part_contact=np.zeros((T, N, P), np.int32))
    for t in range(T):
        for n in range(N):
            oi, ii = out_idx[t, n], in_idx[t, n]
            has_o = (oi >= 0) & (oi // F < N)
            has_i = (ii >= 0) & (ii // F < N)
            with np.errstate(invalid='ignore'):
                rank_o, rank_i = has_o & (out_d2[t, n] >= 0), has_i & (in_d2[t, n] >= 0)
                touch = has_o & (out_d2[t, n] <= c2)
            for keys, size, po, pi, names in ((oi // F, N, has_o, has_i, ('pair_depth_d2', 'pair_min_d2', 'pair_contact')),
                                              (part, P, part < P, part < P, ('part_depth_d2', 'part_min_d2', 'part_contact'))):
                key_i = ii // F if names[0].startswith('pair') else part
                for k in range(size):
                    sel = rank_i & pi & (key_i == k)
                    if sel.any():
                        out[names[0]][t, n, k] = in_d2[t, n][sel].max()
                    sel = rank_o & po & (keys == k)
                    if sel.any():
                        out[names[1]][t, n, k] = out_d2[t, n][sel].min()
                    out[names[2]][t, n, k] = (touch & po & (keys == k)).sum()
    return out
