"""The points-inside-mesh definition (include/mhmocap_hip.h) on cases whose answer is known by construction or by hand:
tests/inside_ref.py is what the device is compared with, so it is checked here against geometry, not against itself."""
import itertools

import numpy as np
import pytest

import inside_ref as ir

U = 2.0 ** -16                      # metres per lattice unit: lattice-aligned coordinates are k * U


def _block(lo, hi):
    """every lattice point of [lo, hi]^3 as float32 metres and as integers"""
    g = np.arange(lo, hi + 1)
    q = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    return (q * U).astype(np.float32), q


@pytest.fixture(scope='module')
def cube_block():
    v, f = ir.cube(0.0, 8 * U)
    pts, q = _block(-2, 10)
    w, up, down, status, below = ir.winding_ref(v, f, pts, with_below=True)
    return v, f, pts, q, w, up, down, status, below


def test_cube_every_lattice_query_of_a_block_around_it(cube_block):
    v, f, pts, q, w, up, down, status, below = cube_block
    assert status == 0 and f.shape == (12, 3)
    interior = ((q > 0) & (q < 8)).all(1)
    exterior = ((q < 0) | (q > 8)).any(1)
    half_open = ((q >= 0) & (q < 8)).all(1)
    assert interior.sum() == 343 and (w[interior] == 1).all()
    assert (w[exterior] == 0).all() and (up[exterior] == -1).all() and (down[exterior] == -1).all()
    # the surface is decided by the perturbation Q + (eps, eps^2) in x and y and by "on the face is neither" in z
    assert np.array_equal(w != 0, half_open) and half_open.sum() == 512
    assert set(np.unique(w)) == {0, 1}
    # up / down by hand: the top is at z = 8, the bottom at z = 0
    inside = w != 0
    assert np.array_equal(up[inside], 8 - q[inside, 2])
    strictly = interior
    assert np.array_equal(down[strictly], q[strictly, 2])
    assert (down[inside & (q[:, 2] == 0)] == -1).all()      # on the bottom face: nothing below
    # off the surface the count below, sign reversed, is the same number
    off = interior | exterior
    assert np.array_equal(below[off], w[off])
    on = ~off
    assert (below[on] != w[on]).any()                       # and on it they differ somewhere: the rule matters


def test_numpy_equals_python_ints_on_the_cube(cube_block):
    v, f, pts, q, w, up, down, status, below = cube_block
    X = [tuple(int(c) for c in p) for p in np.rint(v.astype(np.float64) / U).astype(np.int64)]
    inbox = ((q >= 0) & (q <= 8)).all(1)
    for i in np.nonzero(inbox)[0]:
        assert ir.winding_py(X, f.tolist(), tuple(int(c) for c in q[i])) == (w[i], up[i], down[i], below[i]), q[i]
    # outside the box the face rules alone count 0 as well: a ray misses the cube, or enters and leaves it (the box only
    # spares the work)
    for i in np.nonzero(~inbox)[0][::7]:
        wp, _, _, bp = ir.winding_py(X, f.tolist(), tuple(int(c) for c in q[i]))
        assert wp == 0 and bp == 0, q[i]


def test_flipped_orientation_gives_minus_one():
    v, f = ir.cube(0.0, 8 * U)
    pts, q = _block(-1, 9)
    w = ir.winding_ref(v, f, pts)[0]
    wf = ir.winding_ref(v, f[:, ::-1], pts)[0]
    assert np.array_equal(wf, -w) and (wf == -1).sum() == 512


def test_nested_and_overlapping_cubes():
    va, fa = ir.cube(0.0, 16 * U)
    vb, fb = ir.cube(4 * U, 12 * U)
    pts, q = _block(-1, 17)
    in_a = ((q >= 0) & (q < 16)).all(1)
    in_b = ((q >= 4) & (q < 12)).all(1)
    # two nested, both outward: 2 in the inner one, 1 between
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + 8])
    w, up, down, _ = ir.winding_ref(v, f, pts)
    assert np.array_equal(w, in_a.astype(np.int32) + in_b) and (w == 2).sum() == 512
    assert np.array_equal(up[in_b], 12 - q[in_b, 2])        # the nearest face above is the inner cube's top
    # the inner one flipped: a cavity
    w = ir.winding_ref(v, np.concatenate([fa, fb[:, ::-1] + 8]), pts)[0]
    assert np.array_equal(w, in_a.astype(np.int32) - in_b)
    # a self-overlapping pair: [0,8]^3 and [4,12]^3 share [4,8)^3 with winding 2
    vc, fc = ir.cube(0.0, 8 * U)
    vd, fd = ir.cube(4 * U, 12 * U)
    w = ir.winding_ref(np.concatenate([vc, vd]), np.concatenate([fc, fd + 8]), pts)[0]
    in_c, in_d = ((q >= 0) & (q < 8)).all(1), ((q >= 4) & (q < 12)).all(1)
    assert np.array_equal(w, in_c.astype(np.int32) + in_d) and (w == 2).sum() == 64


def test_open_mesh_counts_the_faces_above():
    v, f = ir.cube(0.0, 8 * U)
    v = np.concatenate([v, [[0, 0, -2 * U]]]).astype(np.float32)             # in no face: it widens the box to z = -2
    pts, q = _block(-1, 9)
    col = ((q[:, :2] >= 0) & (q[:, :2] < 8)).all(1)
    assert np.array_equal(ir.winding_ref(v, f, pts)[0], (col & (q[:, 2] >= 0) & (q[:, 2] < 8)).astype(np.int32))
    # without the top (faces 2, 3): under the bottom only the bottom is above (-1), inside nothing is
    w = ir.winding_ref(v, np.delete(f, [2, 3], 0), pts)[0]
    assert np.array_equal(w, -(col & (q[:, 2] < 0)).astype(np.int32)) and (w == -1).sum() == 64
    # without the bottom (faces 0, 1): everything under the top, the space under the cube included, counts +1
    w = ir.winding_ref(v, np.delete(f, [0, 1], 0), pts)[0]
    assert np.array_equal(w, (col & (q[:, 2] < 8)).astype(np.int32))


def test_degenerate_faces_contribute_nothing():
    v, f = ir.cube(0.0, 8 * U)
    pts, q = _block(-1, 9)
    want = ir.winding_ref(v, f, pts)
    # A = 0: a repeated vertex, three collinear vertices, and a vertical face whose projection is a segment (the cube has
    # eight of those already); a zero-length projected edge: 0 -> 4 is vertical
    extra = np.array([[0, 0, 7], [0, 3, 3], [0, 4, 4], [0, 4, 7]], np.int32)
    v2 = np.concatenate([v, [[4 * U, 4 * U, 4 * U]]]).astype(np.float32)      # vertex 8: the middle of the diagonal 0 - 7
    extra2 = np.array([[0, 8, 7], [7, 8, 0]], np.int32)
    got = ir.winding_ref(v2, np.concatenate([f, extra, extra2]), pts)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    # faces that name a vertex outside [0, V) or one that is not finite are skipped; the box ignores such a vertex
    v3 = np.concatenate([v, [[np.nan, 0, 0]], [[0, np.inf, 0]]]).astype(np.float32)
    bad = np.array([[0, 1, 8], [9, 3, 7], [0, 1, 10], [-1, 2, 3]], np.int32)
    got = ir.winding_ref(v3, np.concatenate([f, bad]), pts)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert got[3] == 0


def test_z_tie_and_hand_values():
    """one triangle z = x over (0,0), (8,0), (0,8), counter-clockwise seen from +z: A = 64"""
    v = np.array([[0, 0, 0], [8, 0, 8], [0, 8, 0], [0, 0, -4], [0, 0, 12]], np.float32) * np.float32(U)     # 3, 4: widen the box in z
    f = np.array([[0, 1, 2]], np.int32)
    q = np.array([[2, 2, 2], [2, 2, 1], [2, 2, 3], [1, 3, -4], [3, 1, 12], [5, 5, 0], [0, 0, -1], [8, 0, 0], [0, 8, -1], [4, 4, 0]])
    w, up, down, status = ir.winding_ref(v, f, (q * U).astype(np.float32))
    assert status == 0
    #                  on    under  over  under  over  outside (0,0): covered  (8,0) (0,8): not  hypotenuse: not
    assert w.tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 0, 0]
    assert up.tolist() == [-1, 1, -1, 5, -1, -1, 1, -1, -1, -1]
    assert down.tolist() == [-1, -1, 1, -1, 9, -1, -1, -1, -1, -1]
    # truncation: z = x / 3 over (0,0), (9,0), (0,9) -> at x = 1 the face is 1/3 above z = 0: dz = 0, yet ABOVE
    v = np.array([[0, 0, 0], [9, 0, 3], [0, 9, 0], [0, 0, -1]], np.float32) * np.float32(U)
    w, up, down, _ = ir.winding_ref(v, f, (np.array([[1, 1, 0], [1, 1, 1], [2, 2, 0], [2, 2, -1]]) * U).astype(np.float32))
    assert w.tolist() == [1, 0, 1, 1] and up.tolist() == [0, -1, 0, 1] and down.tolist() == [-1, 0, -1, -1]


def test_range_rules():
    v, f = ir.cube(0.0, 1.0)
    pts = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [9000.0, 0.5, 0.5], [0.5, 0.5, 1e30]], np.float32)
    w, up, down, status = ir.winding_ref(v, f, pts)
    assert status == 0 and w.tolist() == [1, 0, 0, 0, 0] and up.tolist() == [32768, -1, -1, -1, -1]
    assert ir.winding_ref(v, f, pts, live=False)[3] == 1 and not ir.winding_ref(v, f, pts, live=False)[0].any()
    for vv in (v * 8.001, v + 9000.0, v * np.nan, np.concatenate([v, [[0, 8192.0, 0]]]), np.concatenate([v, [[np.nan, -1e4, 0]]])):
        w, up, down, status = ir.winding_ref(vv.astype(np.float32), f, pts)
        assert status == 2 and not w.any() and (up == -1).all() and (down == -1).all()
    # exactly 8 m across is testable, and 8191 m out is
    assert ir.winding_ref(v * 8, f, pts)[3] == 0 and ir.winding_ref(v + 8190.0, f, pts)[3] == 0
    # half to even on the lattice
    X, ok = ir.lattice(np.array([0.5 * U, 1.5 * U, 2.5 * U, -0.5 * U, -1.5 * U, 8192.0, np.nan], np.float32))
    assert X[:5].tolist() == [0, 2, 2, 0, -2] and ok.tolist() == [True] * 5 + [False, False]


def test_icosphere_by_construction():
    """points under the inscribed radius are inside, points over the circumscribed radius outside: chosen so, none filtered"""
    r = 0.5
    v, f = ir.icosphere(3, r, (0.1, -0.2, 2.0))
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    c = np.array([0.1, -0.2, 2.0])
    vd = v.astype(np.float64) - c
    # the inscribed radius: the smallest distance of a face's plane from the centre (the faces are inside the sphere)
    n = np.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r_in = np.abs((n * vd[f[:, 0]]).sum(1)).min() - 1e-4    # (the lattice moves a vertex by at most 2^-17 m per axis)
    r_out = np.linalg.norm(vd, axis=1).max() + 1e-4
    assert 0.97 * r < r_in < r < r_out
    rng = np.random.default_rng(5)
    d = rng.normal(size=(600, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inner = c + d[:300] * (r_in * rng.uniform(0.0, 1.0, (300, 1)))
    outer = c + d[300:] * (r_out * rng.uniform(1.0, 1.4, (300, 1)))
    pts = np.concatenate([inner, outer]).astype(np.float32)
    w, up, down, status, below = ir.winding_ref(v, f, pts, with_below=True)
    assert status == 0
    assert (w[:300] == 1).all() and (w[300:] == 0).all()
    assert np.array_equal(below, w)                         # none of them is on the surface
    assert (up[:300] >= 0).all() and (down[:300] >= 0).all()
    # up + down is the chord through the point: at most the diameter, and for the centre about that
    assert ((up[:300] + down[:300]) * U <= 2 * r_out).all()
    w0, up0, down0, _ = ir.winding_ref(v, f, c[None].astype(np.float32))
    assert w0[0] == 1 and 2 * r_in < (up0[0] + down0[0]) * U < 2 * r_out
    # queries exactly over vertices and edge midpoints (the same x and y, 0.1 m lower): each ray is counted exactly once
    planted = np.concatenate([v[:40], (v[f[:40, 0]] + v[f[:40, 1]]) / 2]).astype(np.float32)
    upper = planted[:, 2] > 2.0 + 0.2                        # well on the upper half: 0.1 m lower is inside
    planted[:, 2] -= np.float32(0.1)
    wp = ir.winding_ref(v, f, planted)[0]
    assert upper.sum() > 10 and (wp[upper] == 1).all()


def test_concave_prism_where_the_local_side_test_fails():
    """the winding number gets every probe of the U-shaped prism right; the side test at the nearest vertex (``behind`` of
    tests/proximity_ref.py) calls seven of the eight probes in the slot, and the two beside the prism, behind the surface"""
    import proximity_ref as pr
    v, f, probes = ir.u_prism()
    edges = {}
    for tri in f.tolist():
        for k in range(3):
            edges[(tri[k], tri[(k + 1) % 3])] = edges.get((tri[k], tri[(k + 1) % 3]), 0) + 1
    assert all(c == 1 and edges.get((b, a)) == 1 for (a, b), c in edges.items())             # closed, consistently oriented
    w, up, down, status = ir.winding_ref(v, f, probes)
    assert status == 0 and np.array_equal(w, ir.U_PRISM_INSIDE.astype(np.int32))
    # the solid is 0.1 m thick and the probes sit 0.04 m above its bottom; in the slot there is nothing above or below
    # (each of the two lattice roundings moves a coordinate by at most half a unit)
    assert (np.abs(up[w == 1] * U - 0.06) < 2 * U).all()
    assert (np.abs(down[w == 1] * U - 0.04) < 2 * U).all() and (up[:8] == -1).all() and (down[:8] == -1).all()
    verts = np.stack([v, probes])[None]
    d2, idx = pr.nearest_ref(verts, 0.3)
    start, adj = pr.vertex_faces_ref(f, 16)
    normals = pr.normals_ref(verts[0], f, start, adj)[None]
    behind = pr.pairs_ref(verts, normals, d2, idx, np.zeros(16, np.uint8), 24, 0.02)['behind'][0, 1] != 0
    assert np.array_equal(behind, ir.U_PRISM_BEHIND)
    assert (behind[:8] & ~ir.U_PRISM_INSIDE[:8]).sum() == 7


def test_person_inside_ref_on_two_cubes():
    """body 0 = [0,8]^3, body 1 = [4,12]^3 (in lattice units): vertex 0 of body 1, (4,4,4), is inside body 0; vertex 7 of body
    0, (8,8,8), is inside body 1"""
    va, f = ir.cube(0.0, 8 * U)
    vb, _ = ir.cube(4 * U, 12 * U)
    verts = np.stack([va, vb])[None]
    part = np.array([0, 1, 2, 3, 4, 5, 6, 40], np.uint8)
    r = ir.person_inside_ref(verts, f, part, 24)
    assert r['mask'][0, 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and r['mask'][0, 0].tolist() == [0] * 7 + [2]
    assert r['depth'][0, 1, 0] == 4 and r['other'][0, 1, 0] == 0 and r['depth'][0, 0, 7] == 4 and r['other'][0, 0, 7] == 1
    assert r['pair_verts'][0].tolist() == [[0, 1], [1, 0]] and r['pair_depth'][0].tolist() == [[-1, 4], [4, -1]]
    assert r['part_verts'][0, 1, 0] == 1 and r['part_depth'][0, 1, 0] == 4
    assert r['part_verts'][0, 0].sum() == 0                 # part 40 >= P counts nowhere
    dead = ir.person_inside_ref(verts, f, part, 24, live=[[1, 0]])
    assert not dead['mask'].any() and dead['status'].tolist() == [[0, 1]]
