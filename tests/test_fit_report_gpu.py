"""The fit report on the device (``mh_fit_report_pixels``, ``mh_fit_report_verts``, ``mhhip.report.fit_report``,
``SMPLDepthSequenceOptimizer.fit_report``) against the numpy reference of tests/fit_report_ref.py.

Counts are exact.  The two depth sums: the tolerance is not chosen in advance -- the formula is evaluated in numpy float32 and
float64 on the cases of this file and the kernel may be off by 4x the largest float32 error of a sum, relative to sum |d|
(operation order, fused multiply-adds, the division's rounding).  Vertices: undecided ones (fit_report_ref.py) may be counted
or not; ``pen_max`` is bit-equal to a float32 difference, no tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_report_ref as fr

pytestmark = pytest.mark.gpu

LEAVES = ['poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale']


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda:0')


def _run_pixels(c, with_disp, with_scene):
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    T, N, H, W = c['T'], c['N'], c['H'], c['W']
    person, depth, bits = _dev(c['person']), _dev(c['depth']), _dev(c['bits'].view(np.int32))
    disp, min_z, max_z = (_dev(c[k]) if with_disp else None for k in ('disp', 'min_z', 'max_z'))
    sd, sm = (_dev(c[k]) if with_scene else None for k in ('scene_depth', 'scene_mask'))
    counts = torch.full((T, N, 4), 77, dtype=torch.int32, device='cuda:0')           # the kernel zeroes its outputs itself
    dsum = torch.full((T, N, 2), 77.0, dtype=torch.float32, device='cuda:0')
    check(_lib.lib().mh_fit_report_pixels(T, N, H, W, ptr(person), ptr(depth), ptr(bits), ptr(disp), ptr(min_z), ptr(max_z), ptr(sd),
                                          ptr(sm), fr.DEPTH_OFFSET, fr.MARGIN, ptr(counts), ptr(dsum), _lib.stream_ptr(counts.device)))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), dsum.cpu().numpy()


@pytest.fixture(scope='module')
def pixel_cases():
    cases = {s: fr.pixel_case(*s) for s in fr.PIXEL_SHAPES}
    return cases, fr.sum_budget(cases.values())


@pytest.mark.parametrize('shape', fr.PIXEL_SHAPES)
def test_pixel_kernel(pixel_cases, shape):
    cases, budget = pixel_cases
    c = cases[shape]
    for with_disp in (True, False):
        for with_scene in (True, False):
            kw = dict(disp=c['disp'], min_z=c['min_z'], max_z=c['max_z']) if with_disp else {}
            if with_scene:
                kw.update(scene_depth=c['scene_depth'], scene_mask=c['scene_mask'])
            want, s64 = fr.pixels_ref(c['person'], c['depth'], c['bits'], c['N'], **kw)
            counts, dsum = _run_pixels(c, with_disp, with_scene)
            assert np.array_equal(counts, want), (with_disp, with_scene)
            if not with_scene:
                assert (counts[..., 3] == 0).all()
            if not with_disp:
                assert (dsum == 0).all()
                continue
            err = float((np.abs(dsum.astype(np.float64) - s64) / np.maximum(s64[..., 1:2], 1e-300)).max())
            print('%s scene=%d: kernel sums off by %.3e of sum |d|, numpy float32 (all cases) %.3e' % (shape, with_scene, err, budget))
            assert err <= 4 * budget
            again = _run_pixels(c, with_disp, with_scene)[1]
            assert np.array_equal(dsum.view(np.int32), again.view(np.int32)), 'two launches, different bits'


@pytest.mark.parametrize('name', fr.VERTEX_CASES)
def test_vertex_kernel(name):
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    c = fr.vertex_case(name)
    ref = fr.verts_ref(c['verts'], c['K'], c['scene_depth'], c['scene_mask'], c['margin'])
    B = c['B']
    n = torch.full((B,), 77, dtype=torch.int32, device='cuda:0')
    m = torch.full((B,), 77.0, dtype=torch.float32, device='cuda:0')
    K = np.ascontiguousarray(c['K'], np.float32).reshape(9)
    verts, sd, sm = _dev(c['verts']), _dev(c['scene_depth']), _dev(c['scene_mask'])
    check(_lib.lib().mh_fit_report_verts(B, c['V'], c['H'], c['W'], K.ctypes.data_as(_lib.c_float_p), ptr(verts), ptr(sd), ptr(sm),
                                         c['margin'], ptr(n), ptr(m), _lib.stream_ptr(n.device)))
    torch.cuda.synchronize()
    n, m = n.cpu().numpy(), m.cpu().numpy()
    print('%s: pen_count %s, decided inside %s, undecided %s' % (name, n.tolist(), ref['inside'].sum(-1).tolist(),
                                                                 ref['undecided'].sum(-1).tolist()))
    fr.check_verts(ref, n, m, c['margin'])
    if name in ('zero_mask', 'none_inside'):
        assert (n == 0).all() and (m == 0).all()


def _engine_for_scene(smpl_struct, smpl_regs, W, H):
    from mhhip import engine, synthetic
    from mhhip.sequence import SequenceEngine
    model = engine.BodyModel(smpl_struct, smpl_regs)
    K = synthetic.default_cam_K((W, H), 60.0)
    return SequenceEngine(model, (W, H), 1, 1, K), K


def test_round_trip_with_the_projects_own_unprojection(smpl_struct, smpl_regs):
    """the pixel-centre convention: every masked pixel of a depth map, unprojected by ``scene_from_depth`` and pushed 0.10 m
    behind the surface, lands in its own pixel"""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    W, H = 97, 55
    e, K = _engine_for_scene(smpl_struct, smpl_regs, W, H)
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (2.5 + 0.01 * xx + 0.015 * yy + rng.uniform(-0.05, 0.05, (H, W))).astype(np.float32)
    mask = rng.rand(H, W) < 0.7
    pts = e.scene_from_depth(depth, mask).clone()
    M = int(mask.sum())
    assert tuple(pts.shape) == (M, 3)
    sd, sm = _dev(depth), _dev(mask.astype(np.uint8))
    Kp = np.ascontiguousarray(K, np.float32).reshape(9).ctypes.data_as(_lib.c_float_p)
    for dz, want_n in ((0.10, M), (-0.10, 0)):
        v = pts.clone()
        # along the ray: the pixel of the point does not change
        v *= ((v[:, 2:3] + dz) / v[:, 2:3])
        n = torch.zeros(1, dtype=torch.int32, device='cuda:0')
        m = torch.zeros(1, dtype=torch.float32, device='cuda:0')
        check(_lib.lib().mh_fit_report_verts(1, M, H, W, Kp, ptr(v.contiguous()), ptr(sd), ptr(sm), 0.05, ptr(n), ptr(m),
                                             _lib.stream_ptr(n.device)))
        torch.cuda.synchronize()
        print('z %+.2f: pen_count %d of %d masked pixels, pen_max %.7f' % (dz, int(n), M, float(m)))
        assert int(n) == want_n
        assert abs(float(m) - 0.10) <= 1e-5 if dz > 0 else float(m) == 0.0


# ---- through the optimiser -------------------------------------------------------------------------------------------------

def _floor_scene(K, W, H, height=1.15):
    """a floor ``height`` m below the camera axis (y down), seen by the lower half of the image"""
    ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
    depth = np.minimum(np.where(ys[:, None] > 1e-3, height / np.maximum(ys[:, None], 1e-3), 10.0), 10.0)
    return np.tile(depth, (1, W)).astype(np.float32), np.tile(ys[:, None] > 1e-3, (1, W))


def _optimiser(smpl_struct, smpl_regs, oracle_model, tmp_path, seed):
    from test_fit_full_gpu import _setup
    T, N, W, H, batch = 4, 2, 96, 54, 2
    opt, dl, _, _, seq = _setup(smpl_struct, smpl_regs, oracle_model, tmp_path, T, N, W, H, batch, seed, False)
    return opt, dl, seq


def _reference_report(opt, seq, frames, scene):
    """every column from the reference, evaluated on render_scene's maps, the staged masks and disparity and the vertices of
    the leaves"""
    import torch
    e = opt.engine
    T, N = 4, 2
    g = opt.get_optimized_variables()
    img = opt.render_scene(frames=frames, outputs=('person', 'depth', 'coverage'))
    bits = e.bits.cpu().numpy().view(np.uint32)[frames]
    disp = e.depths.cpu().numpy()[frames]
    min_z, max_z = g['min_z'].reshape(T)[frames].astype(np.float32), g['max_z'].reshape(T)[frames].astype(np.float32)
    kw = {} if scene is None else dict(scene_depth=scene[0], scene_mask=scene[1])
    counts, s64 = fr.pixels_ref(img['person'], img['depth'], bits, N, disp=disp, min_z=min_z, max_z=max_z, **kw)
    _, s32 = fr.pixels_ref(img['person'], img['depth'], bits, N, disp=disp, min_z=min_z, max_z=max_z, dtype=np.float32)
    m = opt.SMPLPY.body_model
    verts, _, _, _ = m.lbs_forward(e.leaf('betas'), e.leaf('poses_smpl').view(T * N, 72), e.leaf('xscale'), e.leaf('poses_T').view(T * N, 3),
                                   want_vposed=False)
    joints = m.joints_regress(opt._joints_reg[0], verts, corr=e.leaf('poses_T').view(T * N, 3).contiguous(), root=opt._joints_reg[1])
    verts, joints = verts.view(T, N, -1, 3).cpu().numpy(), joints.view(T, N, 17, 3).cpu().numpy()
    return dict(img=img, counts=counts, s64=s64, s32=s32, verts=verts, joints=joints)


def test_optimiser_fit_report(smpl_struct, smpl_regs, oracle_model, tmp_path):
    import torch
    opt, dl, seq = _optimiser(smpl_struct, smpl_regs, oracle_model, tmp_path, 41)
    T, N, W, H = 4, 2, 96, 54
    with pytest.raises(ValueError):
        opt.fit_report(frames=[0, 4])
    with pytest.raises(ValueError):
        opt.fit_report(frames=[-1])
    early = opt.fit_report()                       # before staging: no images, no scene
    assert (early['mask_rendered'] == -1).all() and np.isnan(early['mask_iou']).all() and np.isnan(early['depth_abs_m']).all()
    assert (early['pen_verts'] == -1).all() and (early['behind_scene_px'] == -1).all()
    assert np.isnan(early['pen_max_m']).all() and np.isnan(early['contact_dy_m']).all()
    assert np.isfinite(early['reproj_px']).all() and (early['joints_used'] > 0).all()
    scene = _floor_scene(opt.cam_K, W, H)
    opt.update_scene_pointcloud(*scene)
    opt.fit(dl, num_iter=3)
    e = opt.engine
    before = {k: e.leaf(k).clone() for k in LEAVES}
    grads = e.grads.clone()
    got = opt.fit_report()
    torch.cuda.synchronize()
    for k in LEAVES:
        assert torch.equal(e.leaf(k), before[k]), k
    assert torch.equal(e.grads, grads)
    frames = np.arange(T)
    ref = _reference_report(opt, seq, frames, scene)
    for k in got:
        assert got[k].shape == ((T, N) if k != 'frames' else (T,)), k
    assert np.array_equal(got['frames'], frames) and np.array_equal(got['valid'], opt._valid.reshape(T, N))
    # ---- pixels: counts exact, sums within 4x the float32 formula's own error
    for j, k in enumerate(['mask_rendered', 'mask_seg', 'mask_inter', 'behind_scene_px']):
        assert np.array_equal(got[k], ref['counts'][..., j]), k
    assert np.array_equal(got['mask_rendered'], ref['img']['coverage'])
    assert got['mask_inter'].sum() > 100
    iou, bias, absd = fr.derived_ref(ref['counts'], ref['s64'])
    assert np.allclose(got['mask_iou'], iou, rtol=1e-6, atol=0, equal_nan=True)
    scale = np.maximum(ref['s64'][..., 1], 1e-300)
    budget = float((np.abs(ref['s32'].astype(np.float64) - ref['s64']) / scale[..., None]).max())
    budget = max(budget, fr.sum_budget([fr.pixel_case(*s) for s in fr.PIXEL_SHAPES]))
    inter = np.maximum(ref['counts'][..., 2], 1)
    some = ref['counts'][..., 2] > 0
    for k, want, j in (('depth_bias_m', bias, 0), ('depth_abs_m', absd, 1)):
        assert np.array_equal(np.isnan(got[k]), ~some), k
        err = float((np.abs(got[k].astype(np.float64) * inter - ref['s64'][..., j])[some] / scale[some]).max())
        print('%s: off by %.3e of sum |d| (budget %.3e, plus one float32 rounding of the quotient)' % (k, err, budget))
        assert err <= 4 * budget + 2.0 ** -23
    # ---- vertices against the scene
    vr = fr.verts_ref(ref['verts'].reshape(T * N, -1, 3), opt.cam_K, scene[0], scene[1], 0.05)
    fr.check_verts(vr, got['pen_verts'].reshape(-1), got['pen_max_m'].reshape(-1), 0.05)
    # ---- key-points: float64 from the same 3D joints
    mean, worst, used = fr.reproj_ref(ref['joints'], opt.cam_K, opt.cam_dist_coef, seq['pose2d'], opt.joint_confidence_thr)
    assert np.array_equal(got['joints_used'], used)
    assert np.nanmax(np.abs(got['reproj_px'] - mean)) <= 1e-3 and np.nanmax(np.abs(got['reproj_max_px'] - worst)) <= 1e-3
    assert np.array_equal(np.isnan(got['reproj_px']), np.isnan(mean))
    # ---- contact and foot slide: float32 kernels of the cycle against float64 (tests/test_scene_knn_gpu.py holds the search itself)
    cloud = opt.scene_pcd.view(-1, 3).cpu().numpy()
    assert np.abs(got['contact_dy_m'] - fr.contact_ref(ref['verts'], cloud)).max() <= 1e-4
    assert np.isnan(got['foot_slide_m'][0]).all()
    assert np.abs(got['foot_slide_m'][1:] - fr.foot_slide_ref(ref['verts'][1:], ref['verts'][:-1])).max() <= 1e-5
    # ---- rows follow ``frames``; frame 3 needs the forward of frame 2, which is not asked for
    part = opt.fit_report(frames=[3, 0], chunk=1)
    assert np.array_equal(part['frames'], [3, 0])
    for k in got:
        if k == 'frames':
            continue
        # (the two calls run the forward on other batches of frames: the counts must agree, the floats to rounding)
        if np.issubdtype(got[k].dtype, np.integer):
            assert np.array_equal(part[k], got[k][[3, 0]]), k
        else:
            assert np.allclose(part[k], got[k][[3, 0]], rtol=1e-5, atol=1e-6, equal_nan=True), k
    # ---- a planted failure: person 1 of frame 2 pushed half a metre into the floor
    opt.engine.leaf('poses_T')[2, 1, 1] += 0.5
    bad = opt.fit_report()
    others = np.ones((T, N), bool)
    others[2, 1] = False
    print('planted: pen_verts %s\npen_max_m %s\ncontact_dy_m %s' % (bad['pen_verts'].tolist(), bad['pen_max_m'].tolist(),
                                                                    bad['contact_dy_m'].tolist()))
    assert bad['pen_verts'][2, 1] > bad['pen_verts'][others].max()
    assert bad['pen_max_m'][2, 1] > bad['pen_max_m'][others].max()
    assert bad['contact_dy_m'][2, 1] < 0
    opt.engine.leaf('poses_T')[2, 1, 1] -= 0.5
    # ---- the three errors
    opt._world = lambda: (2, 0)
    with pytest.raises(RuntimeError, match='shard'):
        opt.fit_report()
    del opt._world
    opt.engine = None
    with pytest.raises(RuntimeError, match='init_optimized_variables'):
        opt.fit_report()


def test_optimiser_fit_report_without_a_scene(smpl_struct, smpl_regs, oracle_model, tmp_path):
    opt, dl, seq = _optimiser(smpl_struct, smpl_regs, oracle_model, tmp_path, 42)
    opt.fit(dl, num_iter=3)
    got = opt.fit_report(frames=[1, 2])
    assert (got['behind_scene_px'] == -1).all() and (got['pen_verts'] == -1).all()
    assert np.isnan(got['pen_max_m']).all() and np.isnan(got['contact_dy_m']).all()
    assert (got['mask_rendered'] > 0).any() and np.isfinite(got['foot_slide_m']).all()
    ref = _reference_report(opt, seq, np.asarray([1, 2]), None)
    for j, k in enumerate(['mask_rendered', 'mask_seg', 'mask_inter']):
        assert np.array_equal(got[k], ref['counts'][..., j]), k


def _child(out_path, tmp_root):
    """fit(k) -> fit(k) and fit(k) -> fit_report() -> fit(k) on two optimisers with the same start (the process was started
    with MHHIP_DETERMINISTIC=1): log rows and leaves of the second fit of both, for the parent to compare"""
    import pathlib
    import conftest  # noqa: F401  (the suite's import paths)
    import torch
    from mhhip import synthetic
    from oracle import lbs_oracle
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    omodel = lbs_oracle.BodyModel(struct, regs)
    res = {}
    for tag in ('plain', 'report'):
        tmp = pathlib.Path(tmp_root) / tag
        tmp.mkdir()
        opt, dl, _ = _optimiser(struct, regs, omodel, tmp, 43)
        opt.update_scene_pointcloud(*_floor_scene(opt.cam_K, 96, 54))
        opt.fit(dl, num_iter=3)
        if tag == 'report':
            assert (opt.fit_report()['mask_rendered'] > 0).any()
        log = opt.fit(dl, num_iter=3)
        torch.cuda.synchronize()
        keys = sorted(log[0])
        res[tag + '_log'] = np.asarray([[row[k] for k in keys] for row in log], np.float64)
        for k in LEAVES:
            res[tag + '_' + k] = opt.engine.leaf(k).cpu().numpy()
    np.savez(out_path, **res)


def test_fit_is_the_same_with_a_report_in_between(tmp_path):
    """under MHHIP_DETERMINISTIC=1, set for a fresh child process: a report between two fits changes no bit of the second"""
    out = str(tmp_path / 'runs.npz')
    env = dict(os.environ, MHHIP_DETERMINISTIC='1')
    p = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out, str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = np.load(out)
    assert r['plain_log'].shape[0] == 3 and np.isfinite(r['plain_log']).all()
    assert np.array_equal(r['plain_log'], r['report_log'])
    for k in LEAVES:
        assert np.array_equal(r['plain_' + k].view(np.int32), r['report_' + k].view(np.int32)), k


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2])
