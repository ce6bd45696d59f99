"""``SMPLDepthSequenceOptimizer.contact_map`` on the small sequence of tests/test_scene_pen_fit_gpu.py (4 frames, 2 people,
48 x 32) with a horizontal floor handed in by ``update_scene_pointcloud``.

The cloud of a 32-row depth map is coarse on a floor seen at a grazing angle (rows 0.2 to 0.4 m apart), so "standing on
the floor" is made exact: every body of every frame is slid over the floor and lowered until its lowest vertex lies ON a
point of the cloud (the translation leaf is edited; a translation moves every vertex by the same amount up to float32
rounding, a few 1e-7 m at these coordinates).  The lowest vertex then has distance ~0, it belongs to a foot or ankle part
(asserted), and every other vertex is above the floor."""
import numpy as np
import pytest

from test_scene_pen_fit_gpu import T, N, W, H, _optimiser, _floor_under

pytestmark = pytest.mark.gpu

FEET = [7, 8, 10, 11]           # left_ankle, right_ankle, left_foot, right_foot
HEAD = 15
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
def standing(smpl_struct, smpl_regs, tmp_path_factory):
    import torch
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path_factory.mktemp('contact_map'), 61)
    opt.update_scene_pointcloud(*_floor_under(opt, depth=0.0))
    cloud = opt.scene_pcd.view(-1, 3)
    v = _verts(opt)
    low = v.view(T * N, -1, 3)[torch.arange(T * N), v.view(T * N, -1, 3)[..., 1].argmax(1)]       # y points down
    to = cloud[torch.cdist(low, cloud).argmin(1)]
    opt.engine.leaf('poses_T').view(T * N, 3).add_(to - low)
    torch.cuda.synchronize()
    return opt


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def test_method_equals_module_on_the_vertices_of_predict(standing):
    from mhhip import contact
    opt = standing
    before = {k: opt.engine.leaf(k).clone() for k in LEAVES}
    got = opt.contact_map(nearest=True)
    want = contact.contact_map(opt.SMPLPY.body_model, _verts(opt), opt.scene_pcd.view(-1, 3), nearest=True)
    assert sorted(got) == sorted(list(want) + ['frames']) and got['frames'].tolist() == list(range(T))
    V = opt.engine.V
    shapes = dict(dist_m=(T, N, V), contact=(T, N, V), part_verts=(T, N, 24), part_min_m=(T, N, 24), contact_verts=(T, N), nearest=(T, N, V, 3))
    types = dict(dist_m=np.float32, contact=np.bool_, part_verts=np.int32, part_min_m=np.float32, contact_verts=np.int32, nearest=np.float32)
    for k, w in want.items():
        w = w.cpu().numpy()
        assert got[k].shape == shapes[k] and got[k].dtype == types[k], k
        assert np.array_equal(_bits(got[k]), _bits(w)), k
    assert 'nearest' not in opt.contact_map()
    # chunked: the same
    small = opt.contact_map(nearest=True, chunk=1)
    for k in want:
        assert np.array_equal(_bits(small[k]), _bits(got[k])), k
    # one frame is its row of the full call
    one = opt.contact_map(frames=[2], nearest=True)
    assert one['frames'].tolist() == [2]
    for k in want:
        assert one[k].shape == (1,) + got[k].shape[1:] and np.array_equal(_bits(one[k][0]), _bits(got[k][2])), k
    # the nearest points are rows of the cloud (or the zero row where there is none)
    cloud = opt.scene_pcd.view(-1, 3).cpu().numpy()
    rows = {r.tobytes() for r in cloud}
    has = np.isfinite(got['dist_m'])
    assert has.any() and all(r.tobytes() in rows for r in got['nearest'][has][::7])
    assert (got['nearest'][~has] == 0).all()
    # consistent with itself
    assert np.array_equal(got['contact'].sum(-1), got['contact_verts'])
    assert np.array_equal(got['part_verts'].sum(-1), got['contact_verts'])
    # read-only
    for k in LEAVES:
        assert (opt.engine.leaf(k) == before[k]).all(), k


def test_feet_touch_the_floor_and_the_head_does_not(standing):
    import torch
    from mhhip import contact
    opt = standing
    part = contact.body_parts(opt.SMPLPY.body_model)
    v = _verts(opt).view(T * N, -1, 3)
    lowest = v[..., 1].argmax(1).cpu().numpy()
    assert np.isin(part[lowest], FEET).all(), 'the lowest vertex of every body is a foot or ankle vertex'
    got = opt.contact_map(radius=0.6)                        # contact: the default, 0.03 m
    feet, head = got['part_verts'][..., FEET].sum(-1), got['part_verts'][..., HEAD]
    print('contact vertices per body: feet %s, head %s; smallest foot distance %s' % (feet.ravel(), head.ravel(), got['part_min_m'][..., FEET].min(-1).ravel()))
    assert (feet >= 1).all() and (head == 0).all()
    # the lowest vertex was put on a cloud point: within the rounding of one translation (coordinates below 8 m: 2^-21 m a step)
    old = got['part_min_m'][..., FEET].min(-1)
    assert (old <= 4 * 2.0 ** -21).all()
    # 0.5 m up (y points down): nothing touches any more, and the feet are 0.5 m from the point they stood on -- every
    # vertex is at least 0.5 m above the floor all cloud points lie on, and the lowest vertex exactly 0.5 m above its point
    opt.engine.leaf('poses_T').view(T * N, 3)[:, 1] -= 0.5
    torch.cuda.synchronize()
    try:
        up = opt.contact_map(radius=0.6)
    finally:
        opt.engine.leaf('poses_T').view(T * N, 3)[:, 1] += 0.5
        torch.cuda.synchronize()
    assert (up['part_verts'] == 0).all() and (up['contact_verts'] == 0).all() and not up['contact'].any()
    new = up['part_min_m'][..., FEET].min(-1)
    print('smallest foot distance after raising the bodies by 0.5 m: %s' % new.ravel())
    assert (np.abs((new - old) - 0.5) <= 1e-3).all()


def test_refusals(standing, smpl_struct, smpl_regs, tmp_path):
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import synthetic
    opt = standing
    K = synthetic.default_cam_K((W, H), 60.0)
    no_scene, _ = _optimiser(smpl_struct, smpl_regs, tmp_path, 62)          # (writes the regressor files into tmp_path)
    with pytest.raises(RuntimeError, match='update_scene_pointcloud'):
        no_scene.contact_map()
    fresh = SMPLDepthSequenceOptimizer(image_size=(W, H), num_frames=T, fov=60, device='cuda:0', smpl_model_parameters_path=str(tmp_path),
                                       smpl_data_struct=smpl_struct, cam_K=K, scene_update='none')
    with pytest.raises(RuntimeError, match='init_optimized_variables'):
        fresh.contact_map()
    opt._world = lambda: (2, 0)
    try:
        with pytest.raises(RuntimeError, match='frame-sharded'):
            opt.contact_map()
    finally:
        del opt._world
    with pytest.raises(ValueError, match='frames'):
        opt.contact_map(frames=[T])
    with pytest.raises(ValueError, match='contact'):
        opt.contact_map(radius=0.1, contact=0.2)
    with pytest.raises(ValueError, match='radius'):
        opt.contact_map(radius=1.0)


def test_module_refusals(standing):
    import torch
    from mhhip import contact
    opt = standing
    m, v, cloud = opt.SMPLPY.body_model, _verts(opt), opt.scene_pcd.view(-1, 3)
    with pytest.raises(ValueError, match='verts'):
        contact.contact_map(m, v[0], cloud)
    with pytest.raises(ValueError, match='vertices'):
        contact.contact_map(m, v[:, :, :100], cloud)
    with pytest.raises(ValueError, match='scene_points'):
        contact.contact_map(m, v, cloud.view(-1))
    with pytest.raises(ValueError, match='empty'):
        contact.contact_map(m, v, cloud[:0])
    with pytest.raises(ValueError, match='contact'):
        contact.contact_map(m, v, cloud, radius=0.1, contact=0.11)
    d2, near = contact.scene_nearest(cloud, v[0, 0], 0.6)
    full = contact.contact_map(m, v[:1, :1], cloud, radius=0.6, nearest=True)
    assert torch.equal(d2.sqrt(), full['dist_m'][0, 0]) and torch.equal(near, full['nearest'][0, 0])
