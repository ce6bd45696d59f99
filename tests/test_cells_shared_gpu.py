"""The cell-list build the grids share (csrc/mh_cells_p.h: workspace layout, box reduction, the 1024-thread scan with its carry,
the face lists and their clamped read) in ONE call per grid over four bodies that take every way through it:

  0  an icosphere of 5120 faces: more than 1024 cells in every grid, so the scan carries from pass to pass (surface 13^3 =
     2197 cells: three passes; inside 33 x 33 = 1089: two; proximity 13^3 = 2197: three);
  1  the same squashed to a needle, (1, 1/64, 1/64): at most 1024 cells everywhere, one pass (surface 64 x 2 x 2, inside 33 x 1,
     proximity 51 x 1 x 1);
  2  a dead body: the scan's early-out before any barrier;
  3  the sphere with one vertex at x = +3e38 and one at x = -3e38: the surface grid's extent overflows (all faces, the other
     early-out), the inside test finds the body not testable, the proximity grid is one cell.

Everything is compared bit for bit with the host references, and the face grids with themselves on the forced all-faces path.
The cell counts are asserted from the host (``surface_ref.grid_ref``; the shape rules of the other two grids are restated
below, since their references are defined on the SET of candidates and know no grid), so the edge cannot move silently."""
import numpy as np
import pytest
import torch

import inside_ref as ir
import proximity_ref as pr
import surface_ref as sr

pytestmark = pytest.mark.gpu

F32 = np.float32
Q = 300
RADIUS = 0.1


def _bodies():
    v, f = ir.icosphere(4, 0.5)
    v = (v.astype(np.float64) + [0.1, -0.2, 3.0]).astype(F32)
    needle = ((v.astype(np.float64) - [0.1, -0.2, 3.0]) * [1.0, 1.0 / 64, 1.0 / 64] + [0.1, -0.2, 3.0]).astype(F32)
    far = v.copy()
    far[7, 0], far[1900, 0] = F32(3e38), F32(-3e38)
    return np.stack([v, needle, v, far]), f, np.array([1, 1, 0, 1], np.uint8)


def _inside_cells(verts, F):
    """the shape rule of mh_mesh_bins for a testable body: (cells along x, along y)"""
    status, X, finite, box = ir.body_ref(verts)
    assert status == 0
    ex, ey = int(box[1, 0] - box[0, 0]), int(box[1, 1] - box[0, 1])
    most = max(F // 4, 256)
    for shift in range(32):
        dx, dy = (ex >> shift) + 1, (ey >> shift) + 1
        if dx <= 64 and dy <= 64 and dx * dy <= most:
            return dx, dy


def _proximity_cells(verts):
    """the shape rule of mh_person_nearest for a body of finite extent: cells per axis"""
    ext = np.maximum(verts.max(0) - verts.min(0), F32(1e-3)).astype(F32)
    cell = max(F32(np.cbrt(ext[0]) * np.cbrt(ext[1]) * np.cbrt(ext[2]) / F32(16)), F32(0.02))
    while True:
        d = np.minimum(ext / cell, F32(4096)).astype(np.int64) + 1
        if d.prod() <= 4096:
            return tuple(int(x) for x in d)
        cell = F32(cell * F32(1.26))


def _assert_the_edge(verts, f):
    """from the host: body 0 needs more than one pass of the 1024-thread scan in every grid, body 1 exactly one"""
    assert verts.shape == (4, 2562, 3) and f.shape == (5120, 3)
    big, small = (sr.grid_ref(verts[b], f) for b in (0, 1))
    assert big[0] == 0 and small[0] == 0                                      # both on the grid path
    assert tuple(big[1]) == (13, 13, 13) and tuple(small[1]) == (64, 2, 2)
    assert big[1].prod() > 2048 and small[1].prod() <= 1024                   # three passes, and one
    assert _inside_cells(verts[0], 5120) == (33, 33) and _inside_cells(verts[1], 5120) == (33, 1)
    assert _proximity_cells(verts[0]) == (13, 13, 13) and _proximity_cells(verts[1]) == (51, 1, 1)
    assert sr.grid_ref(verts[3], f)[0] == sr.ALL_FACES and ir.body_ref(verts[3])[0] == ir.NOT_TESTABLE
    assert sr.grid_ref(verts[2], f, live=False)[0] == sr.NOT_LIVE and ir.body_ref(verts[2], live=False)[0] == ir.NOT_LIVE


def test_face_grids_across_the_edge():
    """(a) mh_mesh_bins + mh_mesh_winding and mh_surface_grid + mh_mesh_closest, B = 4"""
    from mhhip import inside
    from test_inside_gpu import _check_winding, _sphere_queries
    from test_surface_gpu import _check_closest, _queries
    verts, f, live = _bodies()
    _assert_the_edge(verts, f)
    rng = np.random.RandomState(5)
    src = [verts[0], verts[1], verts[0], verts[0]]                            # (the far-out body: queries about the sphere it was)
    wq = np.stack([_sphere_queries(v, f, rng, n_random=169)[::3][:Q] for v in src])
    assert wq.shape == (4, Q, 3)
    want = _check_winding(verts, f, wq, live)
    assert want[3].tolist() == [0, 0, ir.NOT_LIVE, ir.NOT_TESTABLE]
    assert (want[0][0] == 1).sum() > 20 and (want[0][1] == 1).sum() > 5 and not want[0][2:].any()
    status = inside.mesh_winding(torch.tensor(verts, device='cuda:0'), f, torch.tensor(wq, device='cuda:0'), live)[3]
    assert status.tolist() == [0, 0, ir.NOT_LIVE, ir.NOT_TESTABLE]            # the two testable bodies are on the grid path
    cq = np.stack([_queries(v, f, rng, Q) for v in src])
    want = _check_closest(verts, f, cq, live=live)
    assert want[4].tolist() == [0, 0, sr.NOT_LIVE, sr.ALL_FACES]
    assert np.isfinite(want[0][[0, 1, 3]]).all() and np.isinf(want[0][2]).all() and (want[0][[0, 1, 3]] == 0).any()
    near = _check_closest(verts, f, cq, radius=0.05, live=live)               # the ring walk ends at the radius
    assert np.isinf(near[0][0]).any() and np.isfinite(near[0][0]).any()


def test_vertex_grid_across_the_edge():
    """(b) mh_person_nearest, T = 1, N = 4, on the same bodies"""
    from mhhip import proximity
    verts, f, live = _bodies()
    _assert_the_edge(verts, f)
    want_d2, want_idx = pr.nearest_ref(verts[None], RADIUS, live[None])
    d2, idx = proximity.person_nearest(torch.tensor(verts[None], device='cuda:0'), RADIUS, live=live[None])
    assert np.array_equal(pr.bits(d2.cpu().numpy()), pr.bits(want_d2)) and np.array_equal(idx.cpu().numpy(), want_idx)
    other = np.where(want_idx >= 0, want_idx // verts.shape[1], -1)[0]
    # the sphere finds the needle and, where the needle is not nearer, its far-out twin; those two find the sphere (the smaller
    # index of two equal candidates) or nobody; the dead body finds nobody
    assert [set(np.unique(o).tolist()) for o in other] == [{1, 3}, {-1, 0}, {-1}, {-1, 0}]
