"""The numpy reference of the contact map (tests/contact_ref.py) against a float64 brute force on clouds where float32 can
tell the nearest point from the second nearest, against hand cases of the definition's edges (the inclusive radius, the tie
rule, a duplicate, a NaN query, nothing in reach), and ``body_parts`` on a hand-made weight matrix.  No GPU."""
import numpy as np

import contact_ref as cr

F = np.float32


def test_against_float64_on_decided_clouds():
    rng = np.random.RandomState(7)
    for M, Q, radius in ((1, 5, 0.5), (50, 200, 0.3), (600, 300, 0.1), (600, 300, 0.6)):
        pts = rng.uniform(-1, 1, (M, 3)).astype(F)
        q = (pts[rng.randint(0, M, 2 * Q)] + rng.uniform(-0.4, 0.4, (2 * Q, 3))).astype(F)
        r2 = float(radius) ** 2
        # keep the queries the inputs decide: nearest and second nearest differ by more than 1e-4 relative, and the nearest
        # is not within 1e-4 relative of the radius
        d64, i64, second = cr.nearest_ref64(pts, q, np.inf)
        keep = (second - d64 > 1e-4 * d64) & (np.abs(d64 - r2) > 1e-4 * r2)
        assert keep.sum() >= Q
        q = q[keep]
        d64, i64, second = cr.nearest_ref64(pts, q, radius)
        best = ((pts[None].astype(np.float64) - q[:, None]) ** 2).sum(-1).min(1)
        assert (second - best > 1e-4 * best).all() and (np.abs(best - r2) > 1e-4 * r2).all()
        d2, near = cr.nearest_ref(pts, q, radius)
        has = i64 >= 0
        assert has.any()
        assert np.array_equal(np.isfinite(d2), has)
        assert np.array_equal(near[has], pts[i64[has]])
        assert (near[~has] == 0).all()
        # three differences, three squares and two sums, each within 2^-24 relative: 2 + 1 + 2 half-ulps, and one to spare
        assert (np.abs(d2[has].astype(np.float64) - d64[has]) <= 6 * 2.0 ** -24 * d64[has] + 1e-12).all()


def test_radius_is_inclusive():
    pts = np.zeros((1, 3), F)              # at the origin, so that q = +-r along an axis is exact whatever r is
    r = F(0.3)
    for axis in range(3):
        for sign in (-1, 1):
            q = pts.copy()
            q[0, axis] = sign * r
            d2, near = cr.nearest_ref(pts, q, r)
            assert d2[0] == r * r and np.array_equal(near[0], pts[0])
            far = pts.copy()
            far[0, axis] = sign * np.nextafter(r, F(1))
            d2, near = cr.nearest_ref(pts, far, r)
            assert np.isinf(d2[0]) and (near == 0).all()


def test_ties_go_to_the_smallest_x_then_y_then_z():
    q = np.zeros((1, 3), F)
    for first in (0, 1):                   # in either order of the cloud
        mirror = np.array([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0]], F)[::1 if first == 0 else -1]
        d2, near = cr.nearest_ref(mirror, q, 1.0)
        assert d2[0] == F(0.25) and np.array_equal(near[0], [-0.5, 0.0, 0.0])
        on_y = np.array([[0.25, 0.5, 0.0], [0.25, -0.5, 0.0], [0.5, 0.25, 0.0]], F)[::1 if first == 0 else -1]
        d2, near = cr.nearest_ref(on_y, q, 1.0)
        assert d2[0] == F(0.3125) and np.array_equal(near[0], [0.25, -0.5, 0.0])
        on_z = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.5]], F)[::1 if first == 0 else -1]
        d2, near = cr.nearest_ref(on_z, q, 1.0)
        assert np.array_equal(near[0], [0.25, 0.25, -0.5])


def test_duplicate_nan_and_empty():
    pts = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [2.0, 2.0, 2.0]], F)
    q = np.array([[0.5, 0.5, 0.25], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [9.0, 9.0, 9.0]], F)
    d2, near = cr.nearest_ref(pts, q, 0.5)
    assert d2[0] == F(0.0625) and np.array_equal(near[0], pts[0])
    assert np.isinf(d2[1:]).all() and (d2[1:] > 0).all() and (near[1:] == 0).all()
    d2, near = cr.nearest_ref(np.zeros((0, 3), F), q, 0.5)
    assert np.isinf(d2).all() and (near == 0).all()


def test_parts_reference():
    d2 = np.array([[0.0, 0.01, 0.04, np.inf, 0.0009, np.nan],
                   [np.inf] * 6], F)
    part = np.array([0, 0, 2, 2, 3, 3], np.uint8)
    counts, mins = cr.parts_ref(d2, part, 4, 0.1)           # thr^2 = float32(0.1)^2 >= float32(0.01): the value is ON it
    assert F(0.1) * F(0.1) >= F(0.01)
    assert counts.tolist() == [[2, 0, 0, 1], [0, 0, 0, 0]]
    assert np.array_equal(mins[0], np.array([0.0, np.inf, 0.04, 0.0009], F))
    assert np.isinf(mins[1]).all()
    counts, _ = cr.parts_ref(d2, part, 4, 0.2)
    assert counts.tolist() == [[2, 0, 1, 1], [0, 0, 0, 0]]


def test_body_parts_first_index_on_ties():
    from mhhip import contact
    w = np.array([[0.1, 0.7, 0.2], [0.5, 0.5, 0.0], [0.0, 0.4, 0.4], [0.0, 0.0, 1.0]], np.float64)
    got = contact.body_parts(w)
    assert got.dtype == np.uint8 and got.tolist() == [1, 0, 1, 2]

    class Model:
        lbs_weights = w.astype(np.float32)
    assert contact.body_parts(Model()).tolist() == [1, 0, 1, 2]
    assert len(contact.PART_NAMES) == 24 and contact.PART_NAMES[10] == 'left_foot' and contact.PART_NAMES[15] == 'head'
