"""``SMPLDepthSequenceOptimizer.penetration_map`` on the small sequence of tests/test_scene_pen_fit_gpu.py (4 frames, 2 people,
48 x 32).  No scene and no staged images are needed: the method reads the leaves only.

The two people of the sequence stand metres apart, so penetration is PLANTED by editing the leaves (person 1 becomes a shifted
copy of person 0) and the leaves are restored afterwards.  The reference (tests/inside_ref.py) walks every face for every
query, so it is asked about every 16th vertex: the device's answer for those vertices must be the reference's, exactly."""
import numpy as np
import pytest

import inside_ref as ir
from test_scene_pen_fit_gpu import T, N, _optimiser
from test_proximity_map_gpu import LEAVES, _verts, _live

pytestmark = pytest.mark.gpu

U = 2.0 ** -16
STEP = 16


@pytest.fixture(scope='module')
def fitted(smpl_struct, smpl_regs, tmp_path_factory):
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path_factory.mktemp('penetration_map'), 61)
    return opt


class _Copy:
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


def _metres(lat):
    return np.where(lat < 0, np.inf, lat.astype(np.float64) * U).astype(np.float32)


def test_method_equals_module_on_the_vertices_of_predict(fitted):
    import torch
    from mhhip import inside
    opt = fitted
    before = {k: opt.engine.leaf(k).clone() for k in LEAVES}
    live0 = _live(opt).copy()
    with _Copy(opt, [0.05, 0.0, 0.0]):
        opt._valid[...] = live0.reshape(opt._valid.shape)   # the sequence's own gaps: a person that is not there takes no part
        got = opt.penetration_map()
        want = inside.penetration_map(opt.SMPLPY.body_model, _verts(opt), live=live0)
        assert sorted(got) == sorted(list(want) + ['frames']) and got['frames'].tolist() == list(range(T))
        V = opt.engine.V
        shapes = dict(inside=(T, N, V), mask=(T, N, V), depth_z_m=(T, N, V), other=(T, N, V), pair_verts=(T, N, N), pair_depth_z_m=(T, N, N),
                      part_verts=(T, N, 24), part_depth_z_m=(T, N, 24), inside_verts=(T, N), status=(T, N))
        types = dict(inside=np.bool_, mask=np.int32, depth_z_m=np.float32, other=np.int32, pair_verts=np.int32, pair_depth_z_m=np.float32,
                     part_verts=np.int32, part_depth_z_m=np.float32, inside_verts=np.int32, status=np.int32)
        assert sorted(shapes) == sorted(want)
        for k, w in want.items():
            w = w.cpu().numpy()
            assert got[k].shape == shapes[k] and got[k].dtype == types[k], k
            assert np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k], w.view(np.int32) if w.dtype == np.float32 else w), k
        both = live0.all(1)
        assert both.any() and got['inside'][both].any()
        assert not got['inside'][~both].any() and (got['other'][~both] == -1).all() and np.isinf(got['depth_z_m'][~both]).all()
        assert np.array_equal(got['status'] & 1, (~live0).astype(np.int32)) and not (got['status'] & 6).any()      # SMPL bodies: the grid path
        # chunked: the same; one frame is its row of the full call
        small = opt.penetration_map(chunk=1)
        one = opt.penetration_map(frames=[2])
        assert one['frames'].tolist() == [2]
        for k in want:
            assert np.array_equal(small[k], got[k]), k
            assert one[k].shape == (1,) + got[k].shape[1:] and np.array_equal(one[k][0], got[k][2]), k
        # consistent with itself (two people: whoever is inside is inside the other one)
        assert np.array_equal(got['inside'].sum(-1), got['inside_verts']) and np.array_equal(got['pair_verts'].sum(-1), got['inside_verts'])
        assert np.array_equal(got['part_verts'].sum(-1), got['inside_verts'])
        assert np.array_equal(got['inside'], got['mask'] != 0) and np.array_equal(got['inside'], got['other'] >= 0)
        assert np.array_equal(got['inside'], np.isfinite(got['depth_z_m']))
        assert np.array_equal(got['pair_depth_z_m'].max(-1, initial=-np.inf, where=np.isfinite(got['pair_depth_z_m'])),
                              np.where(got['inside'], got['depth_z_m'], -np.inf).max(-1))
    for k in LEAVES:
        assert (opt.engine.leaf(k) == before[k]).all(), k


def test_a_copy_shifted_by_five_centimetres(fitted):
    """Person 1 is person 0 moved 5 cm along +x.  A vertex of the copy is inside the original where the surface faces against
    the shift, a vertex of the original inside the copy where it faces along it: for a closed surface about half of the
    vertices each way, less what the shift carries out of thin parts -- tests/inside_ref.py gives 46.4 % both ways for the
    body model's rest shape on the CPU.  Asserted: between a quarter and 55 % in every frame; the device's answer for every
    16th vertex is the reference's; and the two directions of the pair table differ by what the reference says they do."""
    opt = fitted
    with _Copy(opt, [0.05, 0.0, 0.0]):
        got = opt.penetration_map()
        verts = _verts(opt).cpu().numpy()
    V = opt.engine.V
    faces = _faces(opt)
    share = got['pair_verts'] / float(V)
    print('inside: %s of person 0 in 1, %s of person 1 in 0' % (share[:, 0, 1], share[:, 1, 0]))
    assert (share[:, 0, 1] > 0.25).all() and (share[:, 0, 1] < 0.55).all() and (share[:, 1, 0] > 0.25).all() and (share[:, 1, 0] < 0.55).all()
    assert (got['pair_verts'][:, 0, 0] == 0).all() and (got['pair_verts'][:, 1, 1] == 0).all()
    sub = np.arange(0, V, STEP)
    t = 1
    ref = {}
    for n, m in ((0, 1), (1, 0)):
        w, up, down, status = ir.winding_ref(verts[t, m], faces, verts[t, n, sub])
        assert status == 0
        ins = w != 0
        ex = np.where((up >= 0) & (down >= 0), np.minimum(up, down), np.maximum(up, down))
        assert np.array_equal(got['inside'][t, n, sub], ins)
        assert np.array_equal(got['mask'][t, n, sub], np.where(ins, 1 << m, 0))
        assert np.array_equal(got['other'][t, n, sub], np.where(ins, m, -1))
        assert np.array_equal(got['depth_z_m'][t, n, sub], _metres(np.where(ins, ex, -1)))
        ref[n] = int(ins.sum())
    dev = {n: int(got['inside'][t, n, sub].sum()) for n in (0, 1)}
    assert dev == ref and abs(dev[0] - dev[1]) == abs(ref[0] - ref[1])
    # a shift of 5 cm: nobody is deeper than that along x, and along z not deeper than the body is thick
    assert np.isfinite(got['pair_depth_z_m'][:, 0, 1]).all() and (got['pair_depth_z_m'][:, 0, 1] < 0.5).all()


def test_three_metres_apart(fitted):
    opt = fitted
    with _Copy(opt, [3.0, 0.0, 0.0]):
        far = opt.penetration_map()
    assert not far['inside'].any() and not far['mask'].any() and (far['other'] == -1).all() and np.isinf(far['depth_z_m']).all()
    for k in ('pair_verts', 'part_verts', 'inside_verts', 'status'):
        assert (far[k] == 0).all(), k
    assert np.isinf(far['pair_depth_z_m']).all() and np.isinf(far['part_depth_z_m']).all()


def test_behind_is_not_inside():
    """``proximity_map``'s ``behind`` is a local side test at the nearest vertex, ``inside`` the winding number: near a concave
    region they differ.  The case is built on the CPU (tests/inside_ref.py: ``u_prism``; tests/test_inside_ref.py holds what
    the two references say about it): a U-shaped prism as person 0, and as person 1 sixteen probes -- eight in the slot
    between the prongs (outside the solid), six in the solid, two beside it.  The winding number gets all sixteen right; the
    side test calls seven of the eight in the slot, and the two beside the prism, behind the surface.  Here the device must
    give both answers as the references do."""
    import torch
    import proximity_ref as pr
    from mhhip import inside, proximity
    v, faces, probes = ir.u_prism()

    class Model:
        pass
    model = Model()
    model.faces = faces
    model.lbs_weights = np.ones((16, 1), np.float32)
    verts = np.stack([v, probes])[None]
    tv = torch.tensor(verts, device='cuda:0')
    pen = {k: t.cpu().numpy() for k, t in inside.penetration_map(model, tv).items()}
    prox = {k: t.cpu().numpy() for k, t in proximity.proximity_map(model, tv, radius=0.3, contact=0.02).items()}
    want = ir.person_inside_ref(verts, faces, np.zeros(16, np.uint8), 24)
    assert np.array_equal(pen['mask'].view(np.uint32), want['mask']) and np.array_equal(pen['other'], want['other'])
    assert np.array_equal(pen['inside'][0, 1], ir.U_PRISM_INSIDE)
    d2, idx = pr.nearest_ref(verts, 0.3)
    start, adj = pr.vertex_faces_ref(faces, 16)
    normals = pr.normals_ref(verts[0], faces, start, adj)[None]
    behind = pr.pairs_ref(verts, normals, d2, idx, np.zeros(16, np.uint8), 24, 0.02)['behind'] != 0
    assert np.array_equal(prox['behind'], behind) and np.array_equal(prox['behind'][0, 1], ir.U_PRISM_BEHIND)
    differ = pen['inside'][0, 1] != prox['behind'][0, 1]
    assert differ[:8].sum() == 7 and differ.sum() == 9 and not (pen['inside'][0, 1] & ~prox['behind'][0, 1]).any()


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
        fresh.penetration_map()
    opt._world = lambda: (2, 0)
    try:
        with pytest.raises(RuntimeError, match='frame-sharded'):
            opt.penetration_map()
    finally:
        del opt._world
    with pytest.raises(ValueError, match='frames'):
        opt.penetration_map(frames=[T])
    with pytest.raises(ValueError, match='frames'):
        opt.penetration_map(frames=[])
