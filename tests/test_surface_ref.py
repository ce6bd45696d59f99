"""The reference of the point-to-surface distance (tests/surface_ref.py) pinned against geometry: numbers written out by hand,
the tie rule, degenerate faces, and what float32 loses against float64 on the body model far from the origin."""
import numpy as np
import pytest

import surface_ref as sr

TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
# query, D2, weights: one query per region of the triangle (0,0,0) (4,0,0) (0,4,0), every number exactly representable
REGIONS = [((-1, -1, 0), 2.0, (1, 0, 0)),                   # vertex a
           ((6, -1, 0), 5.0, (0, 1, 0)),                    # vertex b
           ((2, -3, 1), 10.0, (0.5, 0.5, 0)),               # edge ab
           ((-1, 6, 0), 5.0, (0, 0, 1)),                    # vertex c
           ((-3, 2, 1), 10.0, (0.5, 0, 0.5)),               # edge ac
           ((3, 3, 1), 3.0, (0, 0.5, 0.5)),                 # edge bc
           ((1, 1, 2), 4.0, (0.5, 0.25, 0.25))]             # the face


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_one_triangle_seven_regions(dtype):
    q = np.array([r[0] for r in REGIONS], np.float32)
    d2, face, point, weights = sr.closest_ref(TRI, [[0, 1, 2]], q, dtype=dtype)
    assert d2.dtype == dtype and d2.tolist() == [r[1] for r in REGIONS] and (face == 0).all()
    assert weights.tolist() == [list(map(float, r[2])) for r in REGIONS]
    assert np.array_equal(point, weights @ TRI.astype(dtype))
    # each query lands in its own region: the conditions of the earlier regions fail for it
    D2, x, v, w = sr.tri_ref(q, TRI[None, 0], TRI[None, 1], TRI[None, 2], dtype)
    assert np.array_equal(v[:, 0], [r[2][1] for r in REGIONS]) and np.array_equal(w[:, 0], [r[2][2] for r in REGIONS])


def test_unit_cube_and_the_tie_on_a_shared_edge():
    v, faces = sr.cube(0.0, 1.0)
    d2, face, point, weights = sr.closest_ref(v, faces, [[0.5, 0.5, 0.25]])
    assert d2[0] == np.float32(0.0625) and point[0].tolist() == [0.5, 0.5, 0.0]
    assert (v[faces[face[0]]][:, 2] == 0).all()             # a face of the z = 0 side
    # the foot (0.5, 0.5, 0) lies on the diagonal the two faces of that side share: the smaller index
    assert np.array_equal(faces[0], [0, 2, 3]) and np.array_equal(faces[1], [0, 3, 1]) and face[0] == 0
    flipped = faces[[1, 0] + list(range(2, 12))]
    assert sr.closest_ref(v, flipped, [[0.5, 0.5, 0.25]])[1][0] == 0
    # two triangles over one edge, the query above the edge's midpoint
    quad = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], np.float32)
    for fs in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 3], [0, 1, 2]], [[2, 0, 1], [3, 0, 2]]):
        d2, face, _, _ = sr.closest_ref(quad, fs, [[1, 1, 3]])
        assert d2[0] == 9.0 and face[0] == 0
    # beyond the radius there is no candidate; exactly at it there is
    assert sr.closest_ref(quad, [[0, 1, 2]], [[1, 1, 3]], radius=3.0)[1][0] == 0
    d2, face, point, weights = sr.closest_ref(quad, [[0, 1, 2]], [[1, 1, 3]], radius=np.nextafter(np.float32(3), np.float32(0)))
    assert np.isinf(d2[0]) and face[0] == -1 and not point.any() and not weights.any()


def test_degenerate_faces_and_faces_that_drop_out():
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]):
        assert sr.closest_ref(line, [order], [[0.5, 1, 0]])[0][0] == 1.0
        assert sr.closest_ref(line, [order], [[3, 0, 1]])[0][0] == 2.0
    dot = np.array([[1, 1, 1]] * 3, np.float32)
    assert sr.closest_ref(dot, [[0, 1, 2]], [[1, 1, 3]])[0][0] == 4.0
    # a face with a NaN corner or an index out of range is no candidate, the others stay; a query that is not finite finds nothing
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 5], [0, 0, 5], [1, 0, 5]], np.float32)
    d2, face, _, _ = sr.closest_ref(v, [[3, 4, 5], [4, 5, 9], [0, 1, 2]], [[0.25, 0.25, 4], [np.inf, 0, 0], [np.nan, 0, 0]])
    assert d2.tolist() == [16.0, np.inf, np.inf] and face.tolist() == [2, -1, -1]
    assert sr.closest_ref(v, [[0, 1, 2]], [[0.25, 0.25, 4]], live=False)[1][0] == -1


def test_float32_against_float64_on_the_body_far_from_the_origin(smpl_struct):
    """|sqrt(D2_32) - d_64| <= 1e-6 m with the body 3 m and 50 m out: the query-centred form subtracts first, so the
    differences near the surface are exact whatever the distance from the origin (measured: below 1e-8 m)."""
    faces = np.asarray(smpl_struct.f).astype(np.int64)
    rng = np.random.RandomState(7)
    worst = 0.0
    for offset in ((0.3, -0.2, 3.0), (-1.0, 0.5, 50.0)):
        v = (np.asarray(smpl_struct.v_template) + np.asarray(offset)).astype(np.float32)
        sub = np.arange(rng.randint(16), v.shape[0], 37)
        for jitter in (0.03, 0.0005):
            step = rng.normal(size=(len(sub), 3))
            q = (v[sub].astype(np.float64) + jitter * step / np.linalg.norm(step, axis=1, keepdims=True)).astype(np.float32)
            d32, f32, _, _ = sr.closest_ref(v, faces, q, dtype=np.float32)
            d64, f64, _, _ = sr.closest_ref(v, faces, q, dtype=np.float64)
            assert (f32 >= 0).all() and (f64 >= 0).all()
            err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64))
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-6, (offset, jitter, err.max())
            assert (np.sqrt(d64) <= jitter * (1 + 1e-6) + 1e-6).all()   # the vertex it was moved from is on the surface
    print('largest |sqrt(D2_32) - d_64|: %.3g m' % worst)


def test_person_and_pair_tables_on_two_cubes():
    """a unit cube and a copy moved by (0.25, 0, 0), nobody marked inside: the corners of each against the other's surface"""
    v, faces = sr.cube(0.0, 1.0)
    verts = np.stack([v, v + np.float32([0.25, 0, 0])])[None]
    got = sr.person_surface_ref(verts, faces, None, 0.5)
    # person 0's corners at x = 0 are 0.25 from the copy; those at x = 1 lie on the copy's y and z sides
    assert np.array_equal(got['out_d2'][0, 0], np.where(v[:, 0] == 1, 0.0, 0.0625).astype(np.float32))
    assert (got['in_idx'] == -1).all() and np.isinf(got['in_d2']).all()
    tab = sr.pairs_ref(got['out_d2'], got['out_idx'], got['in_d2'], got['in_idx'], np.zeros(8, np.uint8), 2, 0.1, 12)
    assert tab['pair_contact'][0].tolist() == [[0, 4], [0, 4][::-1]] and tab['part_contact'][0].tolist() == [[4, 0], [4, 0]]
    assert tab['pair_min_d2'][0, 0, 1] == 0 and np.isinf(tab['pair_min_d2'][0, 0, 0]) and (tab['pair_depth_d2'] == -1).all()
    # planted depths: the tables take the largest per deepest body and per part
    in_d2 = np.full((1, 2, 8), np.inf, np.float32)
    in_idx = np.full((1, 2, 8), -1, np.int32)
    in_d2[0, 1, :3], in_idx[0, 1, :3] = [0.01, 0.04, 0.02], [3, 5, 7]
    tab = sr.pairs_ref(got['out_d2'], got['out_idx'], in_d2, in_idx, np.array([0, 1, 1, 0, 0, 0, 0, 0]), 2, 0.1, 12)
    assert tab['pair_depth_d2'][0, 1].tolist() == [np.float32(0.04), -1.0] and tab['part_depth_d2'][0, 1].tolist() == [np.float32(0.01), np.float32(0.04)]
