"""The points-inside-mesh test's definition in numpy int64 (include/mhmocap_hip.h: mh_mesh_bins, mh_mesh_winding,
mh_person_inside): every face against every query, no grid, plus a pure-Python-int version of the same rules for tiny cases.
A restatement of the definitions, not of the kernels; the device results are compared with it bit for bit
(tests/test_inside_gpu.py)."""
import numpy as np

SCALE = np.float32(65536.0)
RANGE = np.float32(8192.0)
MAX_EXT = 1 << 19
NOT_LIVE, NOT_TESTABLE, ALL_FACES = 1, 2, 4


def lattice(x):
    """float coordinates -> (int64 lattice coordinates, usable): usable where finite and |x| < 8192 (0 elsewhere)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid='ignore'):
        ok = np.abs(x) < RANGE                              # (false for NaN and inf)
    X = np.rint(np.where(ok, x, np.float32(0)) * SCALE)     # exact scaling, half to even
    return X.astype(np.int64), ok


def body_ref(verts, live=True):
    """verts (V,3) float32 -> (status, X (V,3) int64, finite (V) bool, box (2,3) int64): status has bit 1 for a dead body, bit
    2 for a live body that is not testable; the box is that of the finite vertices"""
    verts = np.asarray(verts, np.float32)
    X, ok = lattice(verts)
    finite = np.isfinite(verts).all(1)
    box = np.zeros((2, 3), np.int64)
    if not live:
        return NOT_LIVE, X, finite, box
    if not finite.any() or (np.isfinite(verts) & ~ok).any():
        return NOT_TESTABLE, X, finite, box
    box = np.stack([X[finite].min(0), X[finite].max(0)])
    if ((box[1] - box[0]) > MAX_EXT).any():
        return NOT_TESTABLE, X, finite, box
    return 0, X, finite, box


def _sign(a):
    return np.sign(a).astype(np.int64)


def _edge(P0, P1, Q):
    """P0, P1 (F,1,3), Q (1,Q,3) int64 -> (E, sgn) (F,Q)"""
    dx, dy = P1[..., 0] - P0[..., 0], P1[..., 1] - P0[..., 1]
    E = dx * (Q[..., 1] - P0[..., 1]) - dy * (Q[..., 0] - P0[..., 0])
    tie = np.where(dy != 0, -_sign(dy), _sign(dx))
    return E, np.where(E != 0, _sign(E), np.broadcast_to(tie, E.shape))


def faces_ref(X, valid, Q, block=256):
    """X (F,3,3) int64 lattice corners of the faces, valid (F) bool, Q (Q,3) int64 -> (winding, up, down, below) (Q) int64 over
    ALL valid faces; ``below`` is the count taken below the query with the sign reversed (not a device output)"""
    nq = Q.shape[0]
    wind, below = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    big = np.int64(1) << 62
    up, down = np.full(nq, big), np.full(nq, big)
    X = X[valid]
    for f0 in range(0, X.shape[0], block):
        P = X[f0:f0 + block, :, None, :]                    # (f,3,1,3)
        q = Q[None]
        w0, s0 = _edge(P[:, 1], P[:, 2], q)
        w1, s1 = _edge(P[:, 2], P[:, 0], q)
        w2, s2 = _edge(P[:, 0], P[:, 1], q)
        A = w0 + w1 + w2
        cover = (A != 0) & (s0 == s1) & (s1 == s2) & (s0 != 0)
        Nn = w0 * (P[:, 0, :, 2] - q[..., 2]) + w1 * (P[:, 1, :, 2] - q[..., 2]) + w2 * (P[:, 2, :, 2] - q[..., 2])
        above = cover & (Nn != 0) & (_sign(Nn) == _sign(A))
        under = cover & (Nn != 0) & (_sign(Nn) != _sign(A))
        dz = np.abs(Nn) // np.where(A != 0, np.abs(A), 1)   # (non-negative operands: floor = truncation)
        wind += np.where(above, _sign(A), 0).sum(0)
        below += np.where(under, -_sign(A), 0).sum(0)
        up = np.minimum(up, np.where(above, dz, big).min(0))
        down = np.minimum(down, np.where(under, dz, big).min(0))
    return wind, np.where(up == big, -1, up), np.where(down == big, -1, down), below


def winding_ref(verts, faces, points, live=True, with_below=False):
    """verts (V,3), faces (F,3), points (Q,3) -> (winding, up, down (Q) int32, status)"""
    verts, points = np.asarray(verts, np.float32), np.asarray(points, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, nq = verts.shape[0], points.shape[0]
    status, X, finite, box = body_ref(verts, live)
    wind, up, down, below = np.zeros(nq, np.int64), np.full(nq, -1, np.int64), np.full(nq, -1, np.int64), np.zeros(nq, np.int64)
    if status == 0:
        Q, ok = lattice(points)
        inbox = ok.all(1) & (Q >= box[0]).all(1) & (Q <= box[1]).all(1)
        named = ((faces >= 0) & (faces < V)).all(1)
        fc = np.where(named[:, None], faces, 0)
        valid = named & finite[fc].all(1)
        if inbox.any():
            w, u, d, bl = faces_ref(X[fc], valid, Q[inbox])
            wind[inbox], up[inbox], down[inbox], below[inbox] = w, u, d, bl
    out = (wind.astype(np.int32), up.astype(np.int32), down.astype(np.int32), status)
    return out + (below.astype(np.int32),) if with_below else out


def person_inside_ref(verts, faces, part, P, live=None):
    """verts (T,N,V,3), faces (F,3), part (V), live (T,N) or None -> dict of mask (T,N,V) uint32, depth, other (T,N,V) int32,
    pair_verts, pair_depth (T,N,N) int32, part_verts, part_depth (T,N,P) int32, status (T,N) int32"""
    verts = np.asarray(verts, np.float32)
    T, N, V = verts.shape[:3]
    part = np.asarray(part).astype(np.int64)
    live = np.ones((T, N), bool) if live is None else np.asarray(live) != 0
    mask = np.zeros((T, N, V), np.uint32)
    depth, other = np.full((T, N, V), -1, np.int32), np.full((T, N, V), -1, np.int32)
    pair_verts, pair_depth = np.zeros((T, N, N), np.int32), np.full((T, N, N), -1, np.int32)
    part_verts, part_depth = np.zeros((T, N, P), np.int32), np.full((T, N, P), -1, np.int32)
    status = np.zeros((T, N), np.int32)
    for t in range(T):
        for m in range(N):
            status[t, m] = body_ref(verts[t, m], live[t, m])[0]
        for n in range(N):
            if not live[t, n]:
                continue
            for m in range(N):
                if m == n or status[t, m]:
                    continue
                w, u, d, _ = winding_ref(verts[t, m], faces, verts[t, n])
                ins = w != 0
                ex = np.where((u >= 0) & (d >= 0), np.minimum(u, d), np.maximum(u, d))
                mask[t, n][ins] |= np.uint32(1 << m)
                better = ins & (ex > depth[t, n])           # ascending m: the smallest m on a tie
                depth[t, n][better], other[t, n][better] = ex[better], m
                pair_verts[t, n, m] = ins.sum()
                pair_depth[t, n, m] = ex[ins].max() if ins.any() else -1
            anyone = mask[t, n] != 0
            for k in range(P):
                sel = anyone & (part == k)
                part_verts[t, n, k] = sel.sum()
                part_depth[t, n, k] = depth[t, n][sel].max() if sel.any() else -1
    return dict(mask=mask, depth=depth, other=other, pair_verts=pair_verts, pair_depth=pair_depth, part_verts=part_verts,
                part_depth=part_depth, status=status)


# ---- the same rules in Python integers: one face, one query at a time (tiny cases only) --------------------------------------
def _sgn(a):
    return (a > 0) - (a < 0)


def _edge_py(p0, p1, q):
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    E = dx * (q[1] - p0[1]) - dy * (q[0] - p0[0])
    if E != 0:
        return E, _sgn(E)
    if dy != 0:
        return E, -_sgn(dy)
    return E, _sgn(dx)


def winding_py(X, faces, q):
    """X: list of lattice vertices (three Python ints each), faces: index triples, q: lattice query -> (winding, up, down, below).
    No box, no range rules: the face rules alone."""
    wind = below = 0
    up = down = -1
    for i0, i1, i2 in faces:
        p0, p1, p2 = X[i0], X[i1], X[i2]
        w0, s0 = _edge_py(p1, p2, q)
        w1, s1 = _edge_py(p2, p0, q)
        w2, s2 = _edge_py(p0, p1, q)
        A = w0 + w1 + w2
        if A == 0 or s0 == 0 or s0 != s1 or s1 != s2:
            continue
        Nn = w0 * (p0[2] - q[2]) + w1 * (p1[2] - q[2]) + w2 * (p2[2] - q[2])
        if Nn == 0:
            continue
        dz = abs(Nn) // abs(A)
        if _sgn(Nn) == _sgn(A):
            wind += _sgn(A)
            up = dz if up < 0 else min(up, dz)
        else:
            below -= _sgn(A)
            down = dz if down < 0 else min(down, dz)
    return wind, up, down, below


# ---- meshes --------------------------------------------------------------------------------------------------------------------
def cube(lo, hi):
    """an axis-aligned cube of 8 vertices and 12 outward-oriented faces (counter-clockwise seen from outside, right-handed)"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.float32)       # bit a of i: axis a at hi
    quads = [(0, 2, 3, 1), (4, 5, 7, 6),                    # z = lo (seen from -z), z = hi
             (0, 1, 5, 4), (2, 6, 7, 3),                    # y = lo, y = hi
             (0, 4, 6, 2), (1, 3, 7, 5)]                    # x = lo, x = hi
    faces = []
    for a, b, c, d in quads:
        faces += [(a, b, c), (a, c, d)]
    return v, np.asarray(faces, np.int32)


U_PRISM_INSIDE = np.array([0] * 8 + [1] * 6 + [0] * 2, bool)
U_PRISM_BEHIND = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], bool)


def u_prism():
    """a concave body: the U-shaped polygon (0,0) (3,0) (3,3) (2,3) (2,1) (1,1) (1,3) (0,3), in decimetres, extruded from
    z = 2.0 m to 2.1 m -> (verts (16,3) float32, faces (28,3) int32, closed and outward-oriented, probes (16,3) float32):
    eight probes in the slot between the prongs (outside the solid), six in the solid, two beside it, all at z = 2.04 m.
    U_PRISM_INSIDE is what the winding number says about the probes, U_PRISM_BEHIND what the local side test of
    tests/proximity_ref.py says with a radius of 0.3 m"""
    poly = np.array([(0, 0), (3, 0), (3, 3), (2, 3), (2, 1), (1, 1), (1, 3), (0, 3)], np.float64)
    cap = [(0, 1, 4), (0, 4, 5), (1, 2, 3), (1, 3, 4), (0, 5, 6), (0, 6, 7)]              # three convex quads, no new vertex
    faces = [(a + 8, b + 8, c + 8) for a, b, c in cap] + [(c, b, a) for a, b, c in cap]
    for i in range(8):
        j = (i + 1) % 8
        faces += [(i, j, j + 8), (i, j + 8, i + 8)]
    verts = np.concatenate([np.c_[poly, np.full(8, 20.0)], np.c_[poly, np.full(8, 21.0)]]) * 0.1
    xy = np.array([(1.05, 2.9), (1.5, 2.0), (1.5, 1.05), (1.95, 2.9), (1.1, 1.1), (1.9, 1.1), (1.5, 2.95), (1.05, 1.5),
                   (0.5, 0.5), (1.5, 0.5), (2.5, 2.5), (0.5, 2.9), (0.05, 0.05), (2.95, 2.95), (-0.05, -0.05), (3.05, 1.5)])
    probes = np.c_[xy, np.full(16, 20.4)] * 0.1
    return verts.astype(np.float32), np.asarray(faces, np.int32), probes.astype(np.float32)


def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts (10 4^level + 2, 3) float32, faces (20 4^level, 3) int32), outward-oriented; level 3: 642 and 1280"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.asarray(v) * radius + np.asarray(center, np.float64)
    return v.astype(np.float32), np.asarray(f, np.int32)
