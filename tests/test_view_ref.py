"""Hand-computed cases that pin tests/view_ref.py, the numpy restatement the free-viewpoint renderer's kernels are compared
with bit for bit: inclusive edges, both windings, zero area, the owner of a shared edge, mesh against point at one depth,
and the footprint of a point.  Coordinates are 1/64 pixel: the centre of pixel (px, py) is (64 px + 32, 64 py + 32)."""
import numpy as np

import view_ref as vr

H, W = 6, 7
C = lambda px, py, z: (64 * px + 32, 64 * py + 32, z)          # a vertex ON a pixel centre
# legs along row 0 and column 0 of the pixel centres; the hypotenuse runs through the centres (4,0) (3,1) (2,2) (1,3) (0,4)
TRI = np.asarray([[C(0, 0, 4096), C(4, 0, 4096 + 64), C(0, 4, 4096 + 128)]], np.int64)
INSIDE = {(px, py) for px in range(5) for py in range(5) if px + py <= 4}


def _covered(keys):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(keys[0] != vr.EMPTY))}


def test_right_triangle_with_the_hypotenuse_through_pixel_centres():
    keys = vr.raster(vr.clear(1, H, W), TRI, [[0, 1, 2]], 1)
    assert _covered(keys) == INSIDE and len(INSIDE) == 15      # the three edges are inclusive
    for px, py in INSIDE:                                      # barycentrics px / 4 and py / 4: depth is linear and integer
        assert int(keys[0, py, px]) == ((4096 + 16 * px + 32 * py) << 32 | 0)


def test_reversed_winding_gives_the_same_pixels():
    a = vr.raster(vr.clear(1, H, W), TRI, [[0, 1, 2]], 1)
    b = vr.raster(vr.clear(1, H, W), TRI, [[0, 2, 1]], 1)
    assert np.array_equal(a, b)


def test_zero_area_face_draws_nothing():
    line = np.asarray([[C(0, 0, 4096), C(2, 2, 4096), C(4, 4, 4096)]], np.int64)
    assert (vr.raster(vr.clear(1, H, W), line, [[0, 1, 2]], 1) == vr.EMPTY).all()
    assert (vr.raster(vr.clear(1, H, W), line, [[0, 0, 1]], 1) == vr.EMPTY).all()


def test_invalid_vertex_drops_the_face():
    v = TRI.copy()
    v[0, 1] = (vr.INVALID, 0, 0)
    assert (vr.raster(vr.clear(1, H, W), v, [[0, 1, 2]], 1) == vr.EMPTY).all()


def test_shared_edge_at_equal_depth_goes_to_the_lower_payload():
    quad = np.asarray([[C(0, 0, 5000), C(4, 0, 5000), C(0, 4, 5000), C(4, 4, 5000)]], np.int64)
    keys = vr.raster(vr.clear(1, H, W), quad, [[0, 1, 2], [1, 3, 2]], 1)
    out = vr.resolve(keys, 1, 2)
    assert _covered(keys) == {(px, py) for px in range(5) for py in range(5)}
    for px in range(5):
        for py in range(5):
            assert out['face'][0, py, px] == (0 if px + py <= 4 else 1)       # the diagonal px + py = 4 is face 0's
    assert (out['depth'][0, :5, :5] == np.float32(5000 / 4096)).all() and out['depth'][0, 5, 6] == -1
    assert out['coverage'].tolist() == [[25, 0]]
    # the same with the faces in the other order: the diagonal changes hands, payload 0 is now the lower triangle
    keys = vr.raster(vr.clear(1, H, W), quad, [[1, 3, 2], [0, 1, 2]], 1)
    assert vr.resolve(keys, 1, 2)['face'][0, 2, 2] == 0 and vr.resolve(keys, 1, 2)['face'][0, 0, 0] == 1


def test_a_lower_person_wins_an_exact_tie():
    two = np.concatenate([TRI, TRI])                          # the same triangle for person 0 and person 1
    keys = vr.raster(vr.clear(1, H, W), two, [[0, 1, 2]], 2)
    assert (vr.resolve(keys, 2, 1)['label'][0][keys[0] != vr.EMPTY] == 0).all()


def test_face_beats_point_at_equal_depth():
    flat = TRI.copy()
    flat[0, :, 2] = 5000
    keys = vr.raster(vr.clear(1, H, W), flat, [[0, 1, 2]], 1)
    pq = np.asarray([[[64 * 1 + 5, 64 * 1 + 60, 5000], [64 * 6 + 1, 64 * 5 + 1, 5000], [64 * 1 + 9, 64 * 1 + 9, 4999]]], np.int64)
    vr.splat(keys, pq[:, :2], None, 6400, 3)
    out = vr.resolve(keys, 1, 1)
    assert out['label'][0, 1, 1] == 0 and out['face'][0, 1, 1] == 0           # the face keeps pixel (1,1) ...
    assert out['label'][0, 5, 6] == -2 and out['face'][0, 5, 6] == 1          # ... the point beside it is drawn
    vr.splat(keys, pq, None, 6400, 3)                                         # one unit nearer, the point wins
    out = vr.resolve(keys, 1, 1)
    assert out['label'][0, 1, 1] == -2 and out['face'][0, 1, 1] == 2 and out['depth'][0, 1, 1] == np.float32(4999 / 4096)
    assert out['coverage'].tolist() == [[14, 2]]


def test_two_points_in_one_pixel_the_lower_index_wins():
    keys = vr.splat(vr.clear(1, H, W), np.asarray([[[70, 70, 4096], [100, 90, 4096]]]), None, 6400, 3)
    assert int(keys[0, 1, 1]) == (4096 << 32 | 0x80000000 | 0) and (keys != vr.EMPTY).sum() == 1


def test_point_half():
    fq = 100 * 64                                              # fx = 100 px
    assert vr.point_half(41, fq, 4096, 3) == 0                 # 1 cm at 1 m: 41 * 6400 // 4096 = 64 -> 64 // 128 = 0
    assert vr.point_half(410, fq, 8192, 3) == 2                # 10 cm at 2 m: 2624000 // 8192 = 320 -> 320 // 128 = 2
    assert vr.point_half(4096, fq, 4096, 3) == 3               # 1 m at 1 m: 6400 // 128 = 50, clamped to max_half
    assert vr.point_half(-5, fq, 4096, 3) == 0
    # the footprint: 2 half + 1 pixels around the pixel that contains the point, clipped to the image
    keys = vr.splat(vr.clear(1, H, W), np.asarray([[[64 * 6 + 63, 64 * 0 + 0, 8192]]]), [410], fq, 3)
    assert _covered(keys) == {(px, py) for px in (4, 5, 6) for py in (0, 1, 2)}


def test_projection_snaps_and_flags():
    K = np.asarray([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]])
    xyz = np.asarray([[0.5, -0.25, 1.0], [0, 0, 0.25], [0, 0, 0.5], [64.0, 0, 1.0], [64.0 - 1 / 4096, 0, 1.0], [0, 0, 256.0], [0, 0, 256 - 2.0 ** -12]])
    q, valid, _ = vr.project(xyz, np.eye(3), np.zeros(3), K, 0.5)
    assert valid.tolist() == [True, False, True, False, True, False, True]
    assert q[0].tolist() == [2048, -1024, 4096] and q[1].tolist() == [vr.INVALID, 0, 0] and q[2].tolist() == [0, 0, 2048]
    assert q[4].tolist() == [2 ** 18 - 1, 0, 4096] and q[6].tolist() == [0, 0, 2 ** 20 - 1]
