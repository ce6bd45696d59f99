"""Inputs and float64 reference for the contact term's neighbour searches (csrc/mh_scene.hip: k_contact_knn,
k_contact_knn_grid and the bucket grid behind it) at their edges: k below 32, clouds around k / the 64-point chunk /
the four-wave split, degenerate extents and the cell clamps, one cell with thousands of points, the 2^20-cell cap,
and queries on points, on the bounding box and outside it.

Plain module (no pytest): tests/test_scene_knn_cases.py checks these inputs against the reference alone,
tests/test_scene_knn_edges_gpu.py runs the kernels on them.

dy of a query = mean y of its min(k, M) nearest cloud points - the query's y.  The kernels order candidates by a
float32 d^2, the reference by a float64 one, so a query whose k-th and (k+1)-th neighbour are closer in d^2 than
float32 can tell apart has no single right answer.  The rule that sorts those out does not fix a band in advance:

  e_q      = largest |f32(dx*dx + dy*dy + dz*dz) - f64(same)| over the k+1 nearest points, both from the float32
             differences the kernels form
  decided  : d2[k] - d2[k-1] > 8 * e_q   (4x for operation order and FMA contraction in the kernel, 2x because both
             neighbours carry the error); always when M <= k
  checked  : decided, or every point of the tie band [d2[k-1] - 8 e_q, d2[k] + 8 e_q] has the same y (any choice
             among them gives the same dy: the cloud of identical points relies on this)
  skipped  : everything else

Every case keeps |y| <= 4 for points and queries, so the tolerance of tests/test_scene_knn_gpu.py applies unchanged.
"""
import functools
from collections import namedtuple

import numpy as np

ATOL, RTOL = 2e-5, 1e-5          # on dy, as in tests/test_scene_knn_gpu.py
GRID_MAX_CELLS = 1 << 20         # csrc/mh_scene.hip

Case = namedtuple('Case', 'name pts q k')
Ref = namedtuple('Ref', 'dy d2 swap decided checked')


def tolerance(dy_ref):
    return ATOL + RTOL * np.abs(dy_ref)


def reference(pts, q, k):
    """Brute force in float64, query chunks of at most ~50 MB.  Per query: dy; the sorted d^2 of the min(k, M) + 1
    nearest points (+inf where the cloud has no such point); swap = the dy that results when the k-th neighbour is
    replaced by the (k+1)-th (M <= k: by nothing -- an empty slot adds 0 to the sum); decided / checked as above."""
    pts = np.asarray(pts)
    q = np.asarray(q)
    assert pts.dtype == np.float32 and q.dtype == np.float32
    M, B = pts.shape[0], q.shape[0]
    kk = min(k, M)
    p64 = pts.astype(np.float64)
    y64 = p64[:, 1]
    dy = np.empty(B)
    swap = np.empty(B)
    d2s = np.full((B, kk + 1), np.inf)
    decided = np.ones(B, bool)
    checked = np.ones(B, bool)
    step = max(1, min(B, 2_000_000 // M))
    for b0 in range(0, B, step):
        qc = q[b0:b0 + step].astype(np.float64)
        diff = p64[None] - qc[:, None]
        d2c = np.einsum('bmc,bmc->bm', diff, diff)
        del diff
        order = np.argsort(d2c, axis=1, kind='stable')[:, :kk + 1]
        for j in range(qc.shape[0]):
            b = b0 + j
            idx = order[j]
            d2 = d2c[j, idx]
            d2s[b, :d2.size] = d2
            ysum = y64[idx[:kk]].sum()
            dy[b] = ysum / kk - qc[j, 1]
            if M <= k:
                swap[b] = (ysum - y64[idx[kk - 1]]) / kk - qc[j, 1]
                continue
            swap[b] = (ysum - y64[idx[kk - 1]] + y64[idx[kk]]) / kk - qc[j, 1]
            e32 = pts[idx] - q[b]                                             # the kernels' float32 differences
            f32 = e32[:, 0] * e32[:, 0] + e32[:, 1] * e32[:, 1] + e32[:, 2] * e32[:, 2]
            e64 = e32.astype(np.float64)
            f64 = e64[:, 0] * e64[:, 0] + e64[:, 1] * e64[:, 1] + e64[:, 2] * e64[:, 2]
            band = 8.0 * np.abs(f32.astype(np.float64) - f64).max()
            decided[b] = d2[kk] - d2[kk - 1] > band
            if not decided[b]:
                tie = (d2c[j] >= d2[kk - 1] - band) & (d2c[j] <= d2[kk] + band)
                ty = pts[tie, 1]
                checked[b] = bool((ty == ty[0]).all())
    return Ref(dy, d2s, swap, decided, checked)


def grid_sizing(pts):
    """The sizing rule documented in k_grid_setup, in float32 like the kernel: extents clamped to 1e-3, cell =
    clamp(sqrt(16 A / M), 0.02, 4) with A the largest face of the bounding box, then cell *= 1.26 until the grid has
    at most 2^20 cells.  -> dict(ext, cell0, ncells0, cell, dims, loops)"""
    f = np.float32
    pts = np.asarray(pts, np.float32)
    M = pts.shape[0]
    ext = np.maximum(pts.max(0) - pts.min(0), f(1e-3)).astype(np.float32)
    area = max(ext[0] * ext[1], ext[1] * ext[2], ext[0] * ext[2])
    cell0 = f(min(max(np.sqrt(f(area * f(16.0)) / f(M)), f(0.02)), f(4.0)))
    dims = lambda c: [int(f(e) / f(c)) + 1 for e in ext]
    cell, loops = cell0, 0
    while int(np.prod(dims(cell), dtype=np.int64)) > GRID_MAX_CELLS:
        cell = f(cell * f(1.26))
        loops += 1
    return dict(ext=ext, cell0=float(cell0), ncells0=int(np.prod(dims(cell0), dtype=np.int64)), cell=float(cell),
                dims=dims(cell), loops=loops)


# ---------------------------------------------------------------------------------------------------------------
# clouds and queries
# ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _queries_near(rng, pts, B, spread, n_out=8, out=(6.0, 0.0, 9.0)):
    """B queries scattered by `spread` around random cloud points, the first n_out pushed outside the cloud"""
    q = pts[rng.randint(0, pts.shape[0], B)].astype(np.float64) + rng.randn(B, 3) * spread
    q[:n_out] += np.asarray(out) * np.where(rng.rand(n_out, 1) < 0.5, -1.0, 1.0)
    q[:, 1] = np.clip(q[:, 1], -3.9, 3.9)
    return _f32(q)


def _sheet(rng, M):
    return _f32(np.stack([rng.uniform(-3, 3, M), 1.2 + 0.02 * rng.randn(M) + 0.05 * np.sin(rng.uniform(0, 6, M)),
                          rng.uniform(2, 8, M)], 1))


def _volume(rng, M, side=2.0, centre=(0.0, 0.0, 4.0)):
    return _f32(rng.uniform(-0.5 * side, 0.5 * side, (M, 3)) + np.asarray(centre))


K_SWEEP = (1, 2, 7, 31, 32)
M_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)
DEGENERATE = ('plane_x', 'plane_z', 'line_y', 'identical', 'speck', 'beam', 'outlier_span', 'two_clusters', 'cell_cap',
              'query_positions')
NAMES = tuple(['k_sweep_sheet_k%d' % k for k in K_SWEEP] + ['k_sweep_volume_k%d' % k for k in K_SWEEP] +
              ['m_edges_%d' % m for m in M_EDGES] + list(DEGENERATE))


def _build(name):
    if name.startswith('k_sweep_sheet_k'):
        rng = np.random.RandomState(11)
        pts = _sheet(rng, 3000)
        return pts, _queries_near(rng, pts, 128, 0.3), int(name[len('k_sweep_sheet_k'):])
    if name.startswith('k_sweep_volume_k'):
        rng = np.random.RandomState(12)
        pts = _volume(rng, 2000)
        return pts, _queries_near(rng, pts, 128, 0.3), int(name[len('k_sweep_volume_k'):])
    if name.startswith('m_edges_'):
        M = int(name[len('m_edges_'):])
        rng = np.random.RandomState(100 + M)
        pts = _volume(rng, M)
        return pts, _queries_near(rng, pts, 128, 0.4), 32
    if name in ('plane_x', 'plane_z'):
        # one coordinate exactly constant: its extent is clamped to 1e-3 and the grid is one cell thick there
        rng = np.random.RandomState(21 if name == 'plane_x' else 22)
        pts = np.stack([rng.uniform(-1, 1, 4000), rng.uniform(-1, 1, 4000), rng.uniform(2, 4, 4000)], 1)
        pts[:, 0 if name == 'plane_x' else 2] = 0.7 if name == 'plane_x' else 3.1
        pts = _f32(pts)
        return pts, _queries_near(rng, pts, 128, 0.25), 32
    if name == 'line_y':
        # x and z constant: two clamped extents, sqrt(16 A / M) falls below the 0.02 cell clamp
        rng = np.random.RandomState(23)
        pts = _f32(np.stack([np.full(1500, 0.4), rng.uniform(-3.9, 3.9, 1500), np.full(1500, 2.5)], 1))
        return pts, _queries_near(rng, pts, 128, 0.2, out=(5.0, 0.0, 7.0)), 32
    if name == 'identical':
        rng = np.random.RandomState(24)
        pts = _f32(np.tile(np.array([[0.3, 0.9, 2.7]]), (500, 1)))
        return pts, _queries_near(rng, pts, 128, 0.5), 32
    if name == 'speck':
        # 1 cm^3: the 0.02 cell clamp leaves one cell, every run is far longer than the 64-entry insert buffer
        # For one wrong neighbour out of 32 to move dy by 4x the tolerance, the two candidates' y must differ by 2.6 mm
        # of the 10 mm there are.  The 32 nearest of a query inside the speck lie within 1.2 mm of it, so all but 12
        # queries sit 5..7.5 cm to the side (the nearest set then spans the speck's whole height), and y takes four
        # levels 3.3 mm apart (two uniform y differ by 2.6 mm in 55 % of the pairs, two levels differ in 75 %).
        rng = np.random.RandomState(25)
        p = rng.uniform(0.0, 0.01, (5000, 3))
        p[:, 1] = rng.randint(0, 4, 5000) * (0.01 / 3)
        pts = _f32(p + np.array([0.5, 1.0, 3.0]))
        ang = rng.uniform(0, 2 * np.pi, 116)
        side = np.stack([np.cos(ang), rng.uniform(-0.08, 0.08, 116), np.sin(ang)], 1) * rng.uniform(0.05, 0.075, (116, 1))
        q = np.concatenate([np.array([0.505, 1.005, 3.005]) + side, p[:12] + np.array([0.5, 1.0, 3.0]) + 1e-4])
        return pts, _f32(q), 32
    if name == 'beam':
        # 100 m x 0.2 m x 0.2 m, y short: sqrt(16 A / M) = 0.23 m, a grid one cell thick in y and z and hundreds of
        # cells long (the 4 m cell clamp needs A >= M and is not reached here: outlier_span below reaches it)
        rng = np.random.RandomState(26)
        pts = _f32(np.stack([rng.uniform(-50, 50, 6000), rng.uniform(0.9, 1.1, 6000), rng.uniform(3.0, 3.2, 6000)], 1))
        return pts, _queries_near(rng, pts, 128, 0.15, out=(8.0, 0.0, 6.0)), 32
    if name == 'outlier_span':
        # a dense 2 m patch plus a few outliers that stretch the box to 120 m x 120 m: sqrt(16 A / M) is far above the
        # 4 m cell clamp, and the patch lands in one or two 4 m cells -- runs of a thousand points and more per cell
        rng = np.random.RandomState(27)
        patch = np.stack([rng.uniform(-1, 1, 1950), 1.0 + 0.03 * rng.randn(1950), rng.uniform(4, 6, 1950)], 1)
        far = np.stack([rng.uniform(-60, 60, 50), rng.uniform(-3, 3, 50), rng.uniform(1, 121, 50)], 1)
        pts = _f32(np.concatenate([patch, far])[rng.permutation(2000)])
        q = np.concatenate([_queries_near(rng, _f32(patch), 96, 0.3, n_out=0),
                            _queries_near(rng, _f32(far), 32, 1.0, n_out=0)])
        return pts, q, 32
    if name == 'two_clusters':
        # 40 m apart: a query between them walks many empty shells before it meets a point
        rng = np.random.RandomState(28)
        a = rng.randn(1500, 3) * 0.4 + np.array([-20.0, 0.5, 5.0])
        b = rng.randn(1500, 3) * 0.4 + np.array([20.0, -0.5, 5.0])
        pts = _f32(np.concatenate([a, b])[rng.permutation(3000)])
        mid = np.array([0.0, 0.0, 5.0]) + rng.randn(40, 3) * np.array([1.5, 0.5, 0.5])
        q = np.concatenate([_queries_near(rng, _f32(a), 44, 0.3, n_out=0), _queries_near(rng, _f32(b), 44, 0.3, n_out=0),
                            _f32(mid)])
        return pts, q, 32
    if name == 'cell_cap':
        # sqrt(16 A / M) gives more than 2^20 cells for this cube: k_grid_setup has to enlarge the cell
        rng = np.random.RandomState(29)
        pts = _volume(rng, 170000, side=4.0, centre=(0.0, 0.0, 5.0))
        q = _queries_near(rng, pts, 96, 0.05, n_out=16, out=(0.4, 0.0, 0.5))
        return pts, q, 32
    if name == 'query_positions':
        rng = np.random.RandomState(30)
        pts = _volume(rng, 5000)
        mn, mx = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
        ctr = 0.5 * (mn + mx)
        groups = [pts[rng.randint(0, 5000, 40)].astype(np.float64)]                       # exactly on cloud points
        groups.append(np.array([[(mn, mx)[i >> c & 1][c] for c in range(3)] for i in range(8)]))   # bbox corners
        faces, near, far10 = [], [], []
        for c in range(3):
            for side, s in ((mn, -1.0), (mx, 1.0)):
                f = ctr.copy()
                f[c] = side[c]
                faces.append(f)
                # outside along this axis only, at three places over the face.  The far group goes 10 m out along x
                # and z; along y it goes 2.9 m out, the most that keeps |y| <= 4
                for _ in range(3):
                    o = mn + rng.rand(3) * (mx - mn)
                    o[c] = side[c] + s * 0.01
                    near.append(o)
                    o = mn + rng.rand(3) * (mx - mn)
                    o[c] = side[c] + s * (2.9 if c == 1 else 10.0)
                    far10.append(o)
        groups += [np.array(faces), np.array(near), np.array(far10)]
        groups.append(np.array([[ctr[0] + sx * 26.0, ctr[1] + sy * 3.9, ctr[2] + sz * 41.0]           # far along all three
                                for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]))
        return pts, _f32(np.concatenate(groups)), 32
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    pts, q, k = _build(name)
    assert pts.dtype == np.float32 and q.dtype == np.float32 and q.shape[0] <= 130
    assert np.abs(pts[:, 1]).max() <= 4.0 and np.abs(q[:, 1]).max() <= 4.0, name
    if name == 'cell_cap':
        g = grid_sizing(pts)
        assert g['ncells0'] > GRID_MAX_CELLS and g['loops'] >= 1, g     # the premise: the enlarging loop runs
    pts.setflags(write=False)
    q.setflags(write=False)
    return Case(name, pts, q, k)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the reference of a case, computed once per process and shared (its arrays are read-only)"""
    c = case(name)
    r = reference(c.pts, c.q, c.k)
    for a in r:
        a.setflags(write=False)
    return r
