"""``SMPLDepthSequenceOptimizer.proximity_map`` on the small sequence of tests/test_scene_pen_fit_gpu.py (4 frames, 2 people,
48 x 32).  No scene and no staged images are needed: the method reads the leaves only.

The two people of the sequence stand metres apart, so contact is PLANTED by editing the translation leaf (a translation
moves every vertex of a body by the same amount up to float32 rounding) and the leaf is restored afterwards."""
import numpy as np
import pytest

import proximity_ref as pr
from test_scene_pen_fit_gpu import T, N, _optimiser

pytestmark = pytest.mark.gpu

CHEST, HAND = 9, 22             # spine3, left_hand of mhhip.contact.PART_NAMES
LEAVES = ['poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale']


def _verts(opt, frames=None):
    """the vertices of ``predict`` from the leaves as they are, on the device"""
    import torch
    e = opt.engine
    fr = torch.arange(T, device=e.dev) if frames is None else torch.as_tensor(frames, device=e.dev)
    nb = len(fr) * N
    verts, _, _, _ = opt.SMPLPY.body_model.lbs_forward(e.leaf('betas').view(N, 10), e.leaf('poses_smpl').view(T, N, 72)[fr].reshape(nb, 72),
                                                       e.leaf('xscale').view(N), e.leaf('poses_T').view(T, N, 3)[fr].reshape(nb, 3),
                                                       want_vposed=False)
    return verts.view(len(fr), N, -1, 3)


@pytest.fixture(scope='module')
def fitted(smpl_struct, smpl_regs, tmp_path_factory):
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path_factory.mktemp('proximity_map'), 61)
    return opt


def _live(opt):
    return opt._valid.reshape(T, N) > 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def test_method_equals_module_on_the_vertices_of_predict(fitted):
    import torch
    from mhhip import proximity
    opt = fitted
    assert opt.scene_pcd is None or int(opt.scene_pcd.numel()) == 0           # no scene was ever handed in
    before = {k: opt.engine.leaf(k).clone() for k in LEAVES}
    # bring the people within reach of each other first, or every column is trivially empty
    pT = opt.engine.leaf('poses_T').view(T, N, 3)
    saved = pT.clone()
    try:
        v = _verts(opt)
        pT[:, 1] += v[:, 0].mean(1) - v[:, 1].mean(1) + torch.tensor([0.25, 0.0, 0.0], device=v.device)
        torch.cuda.synchronize()
        got = opt.proximity_map(radius=0.3, contact=0.1, nearest=True)
        want = proximity.proximity_map(opt.SMPLPY.body_model, _verts(opt), live=_live(opt), radius=0.3, contact=0.1, nearest=True)
        assert sorted(got) == sorted(list(want) + ['frames']) and got['frames'].tolist() == list(range(T))
        V = opt.engine.V
        shapes = dict(dist_m=(T, N, V), contact=(T, N, V), behind=(T, N, V), other=(T, N, V), pair_verts=(T, N, N), pair_behind=(T, N, N),
                      pair_min_m=(T, N, N), part_verts=(T, N, 24), part_min_m=(T, N, 24), part_other=(T, N, 24), part_other_part=(T, N, 24),
                      contact_verts=(T, N), behind_verts=(T, N), other_vert=(T, N, V), nearest=(T, N, V, 3))
        types = dict(dist_m=np.float32, contact=np.bool_, behind=np.bool_, other=np.int32, pair_verts=np.int32, pair_behind=np.int32,
                     pair_min_m=np.float32, part_verts=np.int32, part_min_m=np.float32, part_other=np.int32, part_other_part=np.int32,
                     contact_verts=np.int32, behind_verts=np.int32, other_vert=np.int32, nearest=np.float32)
        assert sorted(shapes) == sorted(want)
        for k, w in want.items():
            w = w.cpu().numpy()
            assert got[k].shape == shapes[k] and got[k].dtype == types[k], k
            assert np.array_equal(_bits(got[k]), _bits(w)), k
        both = _live(opt).all(1)
        assert both.any() and got['contact'][both].any() and np.isfinite(got['dist_m'][both]).any()
        assert (got['other'][~_live(opt)] == -1).all()
        plain = opt.proximity_map(radius=0.3, contact=0.1)
        assert 'nearest' not in plain and 'other_vert' not in plain
        # chunked: the same
        small = opt.proximity_map(radius=0.3, contact=0.1, nearest=True, chunk=1)
        for k in want:
            assert np.array_equal(_bits(small[k]), _bits(got[k])), k
        # one frame is its row of the full call
        one = opt.proximity_map(frames=[2], radius=0.3, contact=0.1, nearest=True)
        assert one['frames'].tolist() == [2]
        for k in want:
            assert one[k].shape == (1,) + got[k].shape[1:] and np.array_equal(_bits(one[k][0]), _bits(got[k][2])), k
        # consistent with itself
        assert np.array_equal(got['contact'].sum(-1), got['contact_verts']) and np.array_equal(got['pair_verts'].sum(-1), got['contact_verts'])
        assert np.array_equal(got['behind'].sum(-1), got['behind_verts'])
        has = got['other'] >= 0
        vv = _verts(opt).cpu().numpy()
        assert np.array_equal(got['nearest'][has], vv.reshape(T, N * V, 3)[np.nonzero(has)[0], (got['other'] * V + got['other_vert'])[has]])
        assert (got['nearest'][~has] == 0).all() and (got['other_vert'][~has] == -1).all()
    finally:
        pT.copy_(saved)
        torch.cuda.synchronize()
    # read-only
    for k in LEAVES:
        assert (opt.engine.leaf(k) == before[k]).all(), k


def test_planted_contact_and_three_metres_apart(fitted):
    import torch
    from mhhip import contact
    opt = fitted
    part = contact.body_parts(opt.SMPLPY.body_model)
    chest, hand = int(np.nonzero(part == CHEST)[0][0]), int(np.nonzero(part == HAND)[0][0])
    both = _live(opt).all(1)
    assert both.any()
    pT = opt.engine.leaf('poses_T').view(T, N, 3)
    saved = pT.clone()
    try:
        v = _verts(opt)
        assert float(v.abs().max()) < 8.0
        pT[:, 1] += v[:, 0, chest] - v[:, 1, hand]          # person 1's hand vertex onto person 0's chest vertex
        torch.cuda.synchronize()
        got = opt.proximity_map()
        # Each coordinate of the two vertices passes through at most four roundings of half an ulp on the way (the
        # difference, the new translation, and the translation added to either vertex); coordinates below 8 m have an ulp of at
        # most 2^-21 m, so they agree within 4 * 2^-22 = 2^-20 m per axis, sqrt(3) * 2^-20 < 2^-19 m in distance.
        bound = 2.0 ** -19
        d01, d10 = got['dist_m'][both, 0, chest], got['dist_m'][both, 1, hand]
        print('planted: chest -> hand %s m, hand -> chest %s m (bound %.3g)' % (d01, d10, bound))
        assert (d01 <= bound).all() and (d10 <= bound).all()
        assert (got['pair_min_m'][both, 0, 1] <= bound).all() and (got['pair_min_m'][both, 1, 0] <= bound).all()
        assert (got['pair_verts'][both, 0, 1] >= 1).all() and (got['pair_verts'][both, 1, 0] >= 1).all()
        assert (got['part_min_m'][both, 0, CHEST] <= bound).all() and (got['part_min_m'][both, 1, HAND] <= bound).all()
        assert (got['part_other'][both, 0, CHEST] == 1).all() and (got['part_other_part'][both, 0, CHEST] == HAND).all()
        assert (got['part_other'][both, 1, HAND] == 0).all() and (got['part_other_part'][both, 1, HAND] == CHEST).all()
        assert (got['part_verts'][both, 0, CHEST] >= 1).all() and (got['part_verts'][both, 1, HAND] >= 1).all()
        # a frame in which one of the two is not there reports nothing
        assert np.isinf(got['dist_m'][~both]).all() and (got['pair_verts'][~both] == 0).all()
        # 3 m of air between the two: nothing within reach, whatever the radius
        v = _verts(opt)
        pT[:, 1, 0] += v[:, 0, :, 0].amax(1) - v[:, 1, :, 0].amin(1) + 3.0
        torch.cuda.synchronize()
        far = opt.proximity_map(radius=0.64, contact=0.64)
        assert np.isinf(far['dist_m']).all() and np.isinf(far['pair_min_m']).all() and np.isinf(far['part_min_m']).all()
        for k in ('pair_verts', 'pair_behind', 'part_verts', 'contact_verts', 'behind_verts'):
            assert (far[k] == 0).all(), k
        assert not far['contact'].any() and not far['behind'].any()
        assert (far['other'] == -1).all() and (far['part_other'] == -1).all() and (far['part_other_part'] == -1).all()
    finally:
        pT.copy_(saved)
        torch.cuda.synchronize()


def test_side_test_on_a_shifted_copy(fitted):
    """Person 1 becomes an exact copy of person 0 shifted by delta = 2 mm along +x.  Where a vertex's nearest vertex of the
    other body is its own copy, the side test reduces to the sign of the x component of that copy's normal: the copy of a
    vertex of person 1 lies at -x of it, so it is behind iff the normal there has x < 0; for person 0 the other way round.
    The test proves something only if most vertices are such vertices: with tests/proximity_ref.py on the CPU oracle's bodies
    in the poses and shapes the sequence is made from, delta = 2 mm leaves 99.5 % to 99.7 % of the vertices nearest to their
    own copy (1 mm: 99.9 %), the rest sit at the capsule mesh's poles where rings of vertices are closer than 2 mm; the
    condition asserted below is 90 %."""
    import torch
    from mhhip import proximity
    opt = fitted
    e = opt.engine
    delta = 0.002
    names = ['poses_T', 'poses_smpl', 'betas', 'xscale']
    saved = {k: e.leaf(k).clone() for k in names}
    live_saved = opt._valid.copy()
    try:
        e.leaf('poses_smpl').view(T, N, 72)[:, 1] = e.leaf('poses_smpl').view(T, N, 72)[:, 0]
        e.leaf('betas').view(N, 10)[1] = e.leaf('betas').view(N, 10)[0]
        e.leaf('xscale').view(N)[1] = e.leaf('xscale').view(N)[0]
        pT = e.leaf('poses_T').view(T, N, 3)
        pT[:, 1] = pT[:, 0]
        pT[:, 1, 0] += delta
        opt._valid[...] = 1.0                               # everybody is there
        torch.cuda.synchronize()
        got = opt.proximity_map(nearest=True)
        verts = _verts(opt)
        normals = proximity.vertex_normals(opt.SMPLPY.body_model, verts).cpu().numpy()
        V = e.V
        # the condition, from the definition alone (frame 0), and the device's answer against it
        d2, idx = pr.nearest_ref(verts[:1].cpu().numpy(), 0.1)
        own_ref = (idx[0] >= 0) & (idx[0] % V == np.arange(V))
        print('nearest vertex is the own copy: %.2f%% / %.2f%% of the vertices (reference, frame 0)' % tuple(100 * own_ref.mean(1)))
        assert (own_ref.mean(1) >= 0.9).all()
        assert np.array_equal(got['other_vert'][0], np.where(idx[0] >= 0, idx[0] % V, -1))
        own = got['other_vert'] == np.arange(V)
        assert (own.mean(-1) >= 0.9).all()
        nx = normals[..., 0]
        assert np.array_equal(got['behind'][:, 1][own[:, 1]], (nx[:, 0] < 0)[own[:, 1]])        # person 1 against person 0's normals
        assert np.array_equal(got['behind'][:, 0][own[:, 0]], (nx[:, 1] > 0)[own[:, 0]])        # person 0 against person 1's
        share = got['behind'][own].mean()
        print('behind: %.1f%% of the vertices paired with their copy' % (100 * share))
        assert 0.25 < share < 0.75                          # about half of a closed surface faces either way
    finally:
        for k in names:
            e.leaf(k).copy_(saved[k])
        opt._valid[...] = live_saved
        torch.cuda.synchronize()


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
        fresh.proximity_map()
    opt._world = lambda: (2, 0)
    try:
        with pytest.raises(RuntimeError, match='frame-sharded'):
            opt.proximity_map()
    finally:
        del opt._world
    with pytest.raises(ValueError, match='frames'):
        opt.proximity_map(frames=[T])
    with pytest.raises(ValueError, match='contact'):
        opt.proximity_map(radius=0.1, contact=0.2)
    with pytest.raises(ValueError, match='radius'):
        opt.proximity_map(radius=1.0)
