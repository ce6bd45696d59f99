"""``SMPLDepthSequenceOptimizer.clearance_map`` on the small sequence of tests/test_scene_pen_fit_gpu.py (4 frames, 2 people,
48 x 32).  No scene and no staged images are needed: the method reads the leaves only.

The two people of the sequence stand metres apart, so person 1 is PLANTED as a copy of person 0 moved 5 cm along x by editing
the leaves, which are restored afterwards.  Every vertex of the copy is then 5 cm from its own original, a point of the other
surface, and the other way round: no signed distance can exceed 5 cm in magnitude, which the depth along z does not obey.  The
reference (tests/surface_ref.py) walks every face for every query, so it is asked about every 16th vertex of one frame: the
device's answer for those vertices must be the reference's, exactly."""
import numpy as np
import pytest

import surface_ref as sr
from test_scene_pen_fit_gpu import T, N, _optimiser
from test_proximity_map_gpu import LEAVES, _verts, _live

pytestmark = pytest.mark.gpu

U = 2.0 ** -16
STEP = 16
SHIFT = 0.05
RADIUS, CONTACT = 0.1, 0.02


@pytest.fixture(scope='module')
def fitted(smpl_struct, smpl_regs, tmp_path_factory):
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path_factory.mktemp('clearance_map'), 61)
    return opt


class _Planted:
    """person 1 becomes person 0 shifted by ``shift`` metres, everybody is there; the leaves come back on exit"""
    names = ['poses_T', 'poses_smpl', 'betas', 'xscale']

    def __init__(self, opt, shift):
        self.opt, self.shift = opt, shift

    def __enter__(self):
        import torch
        e = self.opt.engine
        self.saved = {k: e.leaf(k).clone() for k in self.names}
        self.live = self.opt._valid.copy()
        e.leaf('poses_smpl').view(T, N, 72)[:, 1] = e.leaf('poses_smpl').view(T, N, 72)[:, 0]
        e.leaf('betas').view(N, 10)[1] = e.leaf('betas').view(N, 10)[0]
        e.leaf('xscale').view(N)[1] = e.leaf('xscale').view(N)[0]
        pT = e.leaf('poses_T').view(T, N, 3)
        pT[:, 1] = pT[:, 0] + torch.tensor(self.shift, device=pT.device, dtype=pT.dtype)
        self.opt._valid[...] = 1.0
        torch.cuda.synchronize()
        return self

    def __exit__(self, *exc):
        import torch
        for k in self.names:
            self.opt.engine.leaf(k).copy_(self.saved[k])
        self.opt._valid[...] = self.live
        torch.cuda.synchronize()


def _faces(opt):
    from mhhip import bodies
    return bodies.faces_of(opt.SMPLPY.body_model).astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


@pytest.fixture(scope='module')
def planted(fitted):
    """the three maps of the planted copy, and the vertices they were computed on"""
    opt = fitted
    before = {k: opt.engine.leaf(k).clone() for k in LEAVES}
    with _Planted(opt, [SHIFT, 0.0, 0.0]):
        got = opt.clearance_map(radius=RADIUS, contact=CONTACT, nearest=True)
        pen = opt.penetration_map()
        prox = opt.proximity_map(radius=RADIUS, contact=CONTACT)
        verts = _verts(opt).cpu().numpy()
    for k in LEAVES:
        assert (opt.engine.leaf(k) == before[k]).all(), k   # the leaves are unchanged afterwards
    return got, pen, prox, verts


def test_method_equals_module_on_the_vertices_of_predict(fitted):
    from mhhip import surface
    opt = fitted
    before = {k: opt.engine.leaf(k).clone() for k in LEAVES}
    live0 = _live(opt).copy()
    with _Planted(opt, [SHIFT, 0.0, 0.0]):
        opt._valid[...] = live0.reshape(opt._valid.shape)   # the sequence's own gaps: a person that is not there takes no part
        got = opt.clearance_map(nearest=True)
        want = surface.clearance_map(opt.SMPLPY.body_model, _verts(opt), live=live0, nearest=True)
        assert sorted(got) == sorted(list(want) + ['frames']) and got['frames'].tolist() == list(range(T))
        V = opt.engine.V
        f32, i32 = np.float32, np.int32
        cols = dict(signed_m=((T, N, V), f32), dist_m=((T, N, V), f32), depth_m=((T, N, V), f32), other=((T, N, V), i32), face=((T, N, V), i32),
                    inside=((T, N, V), np.bool_), mask=((T, N, V), i32), pair_depth_m=((T, N, N), f32), pair_min_dist_m=((T, N, N), f32),
                    pair_contact_verts=((T, N, N), i32), part_depth_m=((T, N, 24), f32), part_min_dist_m=((T, N, 24), f32),
                    part_contact_verts=((T, N, 24), i32), status=((T, N), i32), point=((T, N, V, 3), f32))
        assert sorted(cols) == sorted(want)
        for k, w in want.items():
            w = w.cpu().numpy()
            assert (got[k].shape, got[k].dtype) == cols[k], k
            assert np.array_equal(_bits(got[k]), _bits(w)), k
        assert 'point' not in opt.clearance_map(frames=[0])
        both = live0.all(1)
        assert both.any() and got['inside'][both].any() and np.isfinite(got['dist_m'][both]).any()
        assert not got['inside'][~both].any() and (got['other'][~both] == -1).all() and np.isinf(got['signed_m'][~both]).all()
        assert np.array_equal(got['status'] & 1, (~live0).astype(np.int32)) and not (got['status'] & 6).any()      # SMPL bodies: the grids
        # chunked: the same; one frame is its row of the full call
        small = opt.clearance_map(nearest=True, chunk=1)
        one = opt.clearance_map(frames=[2], nearest=True)
        assert one['frames'].tolist() == [2]
        for k in want:
            assert np.array_equal(_bits(small[k]), _bits(got[k])), k
            assert one[k].shape == (1,) + got[k].shape[1:] and np.array_equal(_bits(one[k][0]), _bits(got[k][2])), k
    for k in LEAVES:
        assert (opt.engine.leaf(k) == before[k]).all(), k


def test_every_sixteenth_vertex_equals_the_reference(fitted, planted):
    got, pen, prox, verts = planted
    V, faces = fitted.engine.V, _faces(fitted)
    F = faces.shape[0]
    sub = np.arange(0, V, STEP)
    t = 1
    want = sr.person_surface_ref(verts[t:t + 1], faces, got['mask'][t:t + 1], RADIUS, sub=sub)
    ins = got['inside'][t][:, sub]
    assert ins.any() and not ins.all()
    dist, depth = np.sqrt(want['out_d2'][0]), np.sqrt(want['in_d2'][0])
    idx = np.where(ins, want['in_idx'][0], want['out_idx'][0])
    assert np.array_equal(_bits(got['dist_m'][t][:, sub]), _bits(dist)) and np.array_equal(_bits(got['depth_m'][t][:, sub]), _bits(depth))
    assert np.array_equal(_bits(got['signed_m'][t][:, sub]), _bits(np.where(ins, -depth, dist)))
    assert np.array_equal(got['other'][t][:, sub], np.where(idx >= 0, idx // F, -1)) and np.array_equal(got['face'][t][:, sub], np.where(idx >= 0, idx % F, -1))
    assert np.array_equal(_bits(got['point'][t][:, sub]), _bits(np.where(ins[..., None], want['in_pt'][0], want['out_pt'][0])))
    assert (idx >= 0).all() and np.array_equal(ins, want['in_idx'][0] >= 0)
    # the closest point is where it says, for EVERY vertex: in the box of the other body's face, at the distance reported
    # (the point is q + x rounded to float32 at up to 8 m: half an ulp of 4.8e-7 m per coordinate)
    other, face, point = got['other'][t], got['face'][t], got['point'][t]
    for n in range(N):
        assert (other[n] == 1 - n).all() and (face[n] >= 0).all()
        corners = verts[t, 1 - n][faces[face[n]]].astype(np.float64)                                 # (V,3,3)
        gap = np.linalg.norm(point[n].astype(np.float64) - verts[t, n], axis=1)
        assert np.abs(gap - np.abs(got['signed_m'][t, n])).max() < 4e-6
        lo, hi = corners.min(1), corners.max(1)
        assert ((point[n] >= lo - 4e-6) & (point[n] <= hi + 4e-6)).all()


def test_a_copy_shifted_by_five_centimetres(fitted, planted):
    """|signed_m| <= 0.05 + 1e-5 for EVERY vertex of both people: a vertex of the copy is 5 cm from its own original, which
    lies on the other surface (the slack covers the two bodies' separate float32 skinning).  The depth along z does not obey
    the bound.  Where a vertex is inside, the shortest way out is no longer than the way out along z: depth_m <= depth_z_m +
    4 x 2^-16 -- one lattice unit for the truncation of depth_z_m, the rest for the half-unit lattice rounding of the query
    and the mesh (the two references on the CPU, rest shape, every 8th vertex: at most 1.12 units)."""
    got, pen, prox, verts = planted
    assert np.isfinite(got['signed_m']).all()
    print('largest |signed_m| %.6f m; largest depth_z_m %.6f m; inside %d of %d' % (
        np.abs(got['signed_m']).max(), pen['depth_z_m'][pen['inside']].max(), got['inside'].sum(), got['inside'].size))
    assert (np.abs(got['signed_m']) <= SHIFT + 1e-5).all()
    assert (pen['depth_z_m'][pen['inside']] > SHIFT + 1e-5).any()
    assert np.array_equal(got['inside'], pen['inside']) and np.array_equal(got['mask'], pen['mask'])
    ins = got['inside']
    assert ins.any() and (~ins).any()
    excess = got['depth_m'][ins].astype(np.float64) - pen['depth_z_m'][ins]
    print('largest depth_m - depth_z_m where inside: %.3f lattice units' % (excess.max() / U))
    assert (excess <= 4 * U).all()
    assert np.isinf(got['depth_m'][~ins]).all() and np.array_equal(got['signed_m'][ins], -got['depth_m'][ins])
    assert np.array_equal(got['signed_m'][~ins], got['dist_m'][~ins]) and np.isinf(got['dist_m'][ins]).all()      # two people: no third surface
    # the tables: per pair the largest depth and the smallest distance of the columns
    for n, m in ((0, 1), (1, 0)):
        assert np.array_equal(got['pair_depth_m'][:, n, m], np.where(ins[:, n], got['depth_m'][:, n], -np.inf).max(-1).astype(np.float32))
        assert np.array_equal(got['pair_min_dist_m'][:, n, m], got['dist_m'][:, n].min(-1))
        # (counted on the squares in float32: a root within a rounding of the threshold may fall either way)
        assert ((got['dist_m'][:, n] <= CONTACT - 1e-7).sum(-1) <= got['pair_contact_verts'][:, n, m]).all()
        assert (got['pair_contact_verts'][:, n, m] <= (got['dist_m'][:, n] <= CONTACT + 1e-7).sum(-1)).all()
        assert (got['pair_contact_verts'][:, n, m] > 0).all()
        assert np.isinf(got['pair_depth_m'][:, n, n]).all() and (got['pair_contact_verts'][:, n, n] == 0).all()
    assert np.array_equal(got['part_contact_verts'].sum(-1), got['pair_contact_verts'].sum(-1))
    assert np.array_equal(got['part_depth_m'].max(-1, initial=-np.inf, where=np.isfinite(got['part_depth_m'])), got['pair_depth_m'].max(-1, initial=-np.inf, where=np.isfinite(got['pair_depth_m'])))


def test_the_surface_is_no_farther_than_the_nearest_vertex(planted):
    """every vertex of the other body lies on its surface, so the distance to the surface cannot exceed ``proximity_map``'s
    distance to the nearest vertex by more than float32 rounding.  The bound: both are float32 evaluations from the same
    coordinates; the closest point x = A + ab v + ac w carries an absolute error of a few eps (|A| + |ab| + |ac|) <=
    8 x 2^-24 x (0.1 + 2 x 0.075) m = 1.2e-7 m (radius 0.1 m, longest edge 7.5 cm), the vertex distance 3 eps relative:
    1e-6 m covers both eight times over.  On average the surface is millimetres nearer."""
    got, pen, prox, verts = planted
    near = np.isfinite(prox['dist_m'])
    assert near.any()
    surf = np.where(got['inside'], got['depth_m'], got['dist_m']).astype(np.float64)
    print('nearest vertex minus surface: mean %.5f m, largest %.5f m, smallest %.3g m' % (
        (prox['dist_m'][near] - surf[near]).mean(), (prox['dist_m'][near] - surf[near]).max(), (prox['dist_m'][near] - surf[near]).min()))
    assert (surf[near] <= prox['dist_m'][near].astype(np.float64) + 1e-6).all()
    assert (prox['dist_m'][near] - surf[near]).mean() > 1e-4


def test_refusals(fitted, smpl_struct, smpl_regs, tmp_path):
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import synthetic
    from test_scene_pen_fit_gpu import W, H
    opt = fitted
    K = synthetic.default_cam_K((W, H), 60.0)
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'), ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(str(tmp_path / fn), smpl_regs[k])
    fresh = SMPLDepthSequenceOptimizer(image_size=(W, H), num_frames=T, fov=60, device='cuda:0', smpl_model_parameters_path=str(tmp_path),
                                       smpl_data_struct=smpl_struct, cam_K=K, scene_update='none')
    with pytest.raises(RuntimeError, match='init_optimized_variables'):
        fresh.clearance_map()
    opt._world = lambda: (2, 0)
    try:
        with pytest.raises(RuntimeError, match='frame-sharded'):
            opt.clearance_map()
    finally:
        del opt._world
    with pytest.raises(ValueError, match='frames'):
        opt.clearance_map(frames=[T])
    with pytest.raises(ValueError, match='frames'):
        opt.clearance_map(frames=[])
    with pytest.raises(ValueError, match='radius'):
        opt.clearance_map(radius=0.7)
