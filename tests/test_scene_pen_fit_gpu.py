"""The scene-penetration term inside the fit (``reg_scene_pen_coef`` of ``SMPLDepthSequenceOptimizer``,
``SequenceEngine._scene_pen``): the engine's gradient chain against the plain kernel, the term at work, the default of 0
changing no bit, captured against eager cycles, the device-built scene behind the selector, and the refusal of sharding.

A small sequence: 4 frames, 2 people, 48 x 32.  The scene is a horizontal floor handed in by ``update_scene_pointcloud``,
0.3 m above the lowest vertex of the shallowest body: every body stands at least 0.3 m deep in it.  A horizontal floor is
seen at a grazing angle -- 0.3 m below it are about 0.8 m behind it along the ray, and neighbouring rows of a 32-row map are
0.2 to 0.3 m apart in depth -- so the fits here run with ``scene_pen_band`` = ``scene_pen_edge`` = 2 m.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, N, W, H, BATCH = 4, 2, 48, 32, 2
LEAVES = ['poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale']
NINE = ['loss_pose24j', 'loss_depth', 'loss_silhouette', 'reg_ref_poses', 'reg_scale', 'reg_contact', 'reg_foot_sliding', 'reg_vel',
        'reg_filter_verts']
WIDE = dict(scene_pen_band=2.0, scene_pen_edge=2.0)


def _optimiser(struct, regs, tmp_path, seed, coefs=None, **kw):
    import torch
    import golden_inputs as gi
    from mhhip import synthetic, synthetic_seq
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'),
                  ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(os.path.join(str(tmp_path), fn), regs[k])
    c = gi.COEFS if coefs is None else coefs
    K = synthetic.default_cam_K((W, H), 60.0)
    kw.setdefault('scene_update', 'none')
    opt = SMPLDepthSequenceOptimizer(
        image_size=(W, H), num_frames=T, fov=60, device='cuda:0', smpl_model_parameters_path=str(tmp_path),
        smpl_data_struct=struct, cam_K=K,
        proj2d_loss_coef=c['proj2d'], depth_loss_coef=c['depth'], silhouette_loss_coef=c['silhouette'],
        reg_velocity_coef=c['reg_velocity'], reg_verts_filter_coef=c['reg_verts_filter'], reg_poses_coef=c['reg_poses'],
        reg_scales_coef=c['reg_scales'], reg_contact_coef=c['reg_contact'], reg_foot_sliding_coef=c['reg_foot_sliding'], **kw)
    seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, N, T, (W, H), seed, cam_K=K, z_range=(2.6, 3.6))
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=30)
    dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=BATCH, shuffle=False)
    return opt, dl


def _floor_under(opt, depth=0.3):
    """(scene depth, scene mask) of the horizontal floor ``depth`` m above the lowest vertex (y down) of the shallowest body"""
    import torch
    e = opt.engine
    e.forward(regress=False)
    torch.cuda.synchronize()
    height = float(e.verts[..., 1].amax(dim=1).min()) - depth
    assert height > 0.2, 'the floor must lie below the optical axis to be seen'
    K = opt.cam_K
    ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
    d = np.where(ys[:, None] > 1e-3, height / np.maximum(ys[:, None], 1e-3), 10.0)
    mask = np.tile((ys[:, None] > 1e-3) & (d <= 10.0), (1, W))
    return np.tile(np.minimum(d, 10.0), (1, W)).astype(np.float32), mask


ZERO = dict(proj2d=0.0, depth=0.0, silhouette=0.0, reg_poses=0.0, reg_scales=0.0, reg_velocity=0.0, reg_verts_filter=0.0,
            reg_contact=0.0, reg_foot_sliding=0.0)


def test_engine_gradient_chain(smpl_struct, smpl_regs, tmp_path):
    """(a) every other coefficient 0, no images: the translation gradient of one cycle is the per-body sum of the vertex
    gradients of the plain kernel on the cycle's vertices.  Tolerance: a float32 sum of V terms in any order is within
    V 2^-24 sum |g| of the exact one."""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path, 51, coefs=ZERO, reg_scene_pen_coef=1.0, **WIDE)
    opt.update_scene_pointcloud(*_floor_under(opt))
    opt._stage_from_dataloader(dl)
    e = opt.engine
    assert e.scene_zmap is not None
    e.cycle(0, use_images=False)
    torch.cuda.synchronize()
    got = e.leaf('poses_T', e.grads).double().cpu().numpy().reshape(T * N, 3)
    B, V = e.B, e.V
    gv = torch.zeros(B, V, 3, device='cuda:0')
    body = torch.zeros(B, device='cuda:0')
    check(_lib.lib().mh_scene_pen_term(B, V, H, W, e.K.ctypes.data_as(_lib.c_float_p), ptr(e.verts), ptr(e.scene_zmap), 1.0, 0.05, 2.0, 2.0,
                                       ptr(gv), ptr(body), None, _lib.stream_ptr(gv.device)))
    torch.cuda.synchronize()
    want = gv.double().sum(1).cpu().numpy()
    tol = V * 2.0 ** -24 * gv.double().abs().sum(1).cpu().numpy()
    print('poses_T gradient against the summed vertex gradients: worst |difference| / tolerance %.3f; largest entry %.3e'
          % (float((np.abs(got - want) / np.maximum(tol, 1e-300)).max()), np.abs(want).max()))
    assert (np.abs(want).max(axis=1) > 0).all(), 'every body stands in the floor'
    assert (np.abs(got - want) <= tol).all()
    log = e.read_log(1)[0]
    assert list(log) == NINE + ['reg_scene_pen']
    assert abs(float(log['reg_scene_pen']) - float(body.double().sum())) <= 1e-6 * float(body.double().sum())
    assert float(log['reg_scene_pen']) > 0


def test_term_pushes_bodies_out_of_the_floor(smpl_struct, smpl_regs, tmp_path):
    """(b) 30 cycles: the logged term of the last cycle is below the first, and fewer vertices are inside the scene than in a
    twin run with the coefficient at 0 (``fit_report``'s ``pen_verts``)"""
    runs = {}
    for tag, kw in (('on', dict(reg_scene_pen_coef=100.0, **WIDE)), ('off', {})):
        sub = tmp_path / tag
        sub.mkdir()
        opt, dl = _optimiser(smpl_struct, smpl_regs, sub, 52, **kw)
        opt.update_scene_pointcloud(*_floor_under(opt))
        before = opt.fit_report()['pen_verts'].sum()
        log = opt.fit(dl, num_iter=30)
        runs[tag] = (before, opt.fit_report()['pen_verts'].sum(), log)
    (b_on, a_on, log_on), (b_off, a_off, log_off) = runs['on'], runs['off']
    print('vertices inside the scene before / after 30 cycles: %d / %d with the term, %d / %d without; term %.4g -> %.4g'
          % (b_on, a_on, b_off, a_off, log_on[0]['reg_scene_pen'], log_on[-1]['reg_scene_pen']))
    assert b_on > 0 and b_off > 0
    assert list(log_off[0]) == NINE
    assert log_on[-1]['reg_scene_pen'] < log_on[0]['reg_scene_pen']
    assert a_on < a_off


def test_graph_replay_matches_eager(smpl_struct, smpl_regs, tmp_path):
    """(d) captured against eager cycles with the term on: the tolerance of tests/test_fit_full_gpu.py's graph tests"""
    import torch
    runs = []
    for graphs in (False, True):
        sub = tmp_path / str(graphs)
        sub.mkdir()
        opt, dl = _optimiser(smpl_struct, smpl_regs, sub, 53, use_graphs=graphs, reg_scene_pen_coef=10.0, **WIDE)
        opt.update_scene_pointcloud(*_floor_under(opt))
        log = opt.fit(dl, num_iter=6)
        torch.cuda.synchronize()
        runs.append((opt.engine.params.cpu().numpy().copy(), log))
    (p0, l0), (p1, l1) = runs
    np.testing.assert_allclose(p1, p0, atol=2e-4 * np.abs(p0).max())
    for c in range(6):
        assert l0[c]['reg_scene_pen'] > 0
        for k in ['loss_depth', 'loss_silhouette', 'loss_pose24j', 'reg_scene_pen']:
            np.testing.assert_allclose(l1[c][k], l0[c][k], rtol=2e-3, atol=1e-6, err_msg='%s cycle %d' % (k, c))


@pytest.mark.parametrize('graphs', [True, False])
def test_device_built_scene(smpl_struct, smpl_regs, tmp_path, graphs):
    """the scene the fit builds itself from cycle 30 on (two sets, each with its own z-map; captured cycles read the live one
    through the selector, eager ones through the front set): the term is 0 while no scene is live and at work afterwards.
    The bodies are pushed 0.3 m into the ground the synthetic depth maps show."""
    import torch
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path, 54, use_graphs=graphs, scene_update='device', reg_scene_pen_coef=10.0, **WIDE)
    opt.engine.leaf('poses_T')[..., 1] += 0.3
    log = opt.fit(dl, num_iter=36)
    torch.cuda.synchronize()
    vals = np.asarray([row['reg_scene_pen'] for row in log], np.float64)
    print('term per cycle from cycle 28: %s' % ' '.join('%.4g' % v for v in vals[28:]))
    assert np.isfinite(vals).all() and (vals[:31] == 0).all()          # the first update is launched in cycle 30, read from 31 on
    assert (vals[31:] > 0).all()
    for k in LEAVES:
        assert torch.isfinite(opt.engine.leaf(k)).all(), k
    sets = opt.engine._scene_dev['sets']
    depth, mask, _ = opt.engine.scene_device_result()
    zm = [s['zmap'].cpu().numpy() for s in sets]
    assert any(np.array_equal(z, np.where(mask, depth, np.float32(0))) for z in zm)      # the last update's set holds its maps


def test_sharding_is_refused(smpl_struct, smpl_regs, tmp_path):
    """(e)"""
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from mhhip import sharded
    with pytest.raises(ValueError, match='shard'):
        SMPLDepthSequenceOptimizer(image_size=(W, H), num_frames=T, device='cuda:0', smpl_model_parameters_path=str(tmp_path),
                                   smpl_data_struct=smpl_struct, shard_frames=True, reg_scene_pen_coef=1.0)
    opt, _ = _optimiser(smpl_struct, smpl_regs, tmp_path, 55, reg_scene_pen_coef=1.0)
    with pytest.raises(ValueError, match='shard'):
        sharded.ShardedSequence(opt.engine, 0, T, enabled=True)


# ---- (c) the default changes nothing ------------------------------------------------------------------------------------------

def _child(out_path, tmp_root):
    """two optimisers from the same inputs, one constructed without the new keywords and one with reg_scene_pen_coef=0.0
    (the process was started with MHHIP_DETERMINISTIC=1): leaves and log rows of a fit of both, for the parent to compare"""
    import pathlib
    import conftest  # noqa: F401  (the suite's import paths)
    import torch
    from mhhip import synthetic
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    res = {}
    for tag, kw in (('plain', {}), ('zero', dict(reg_scene_pen_coef=0.0))):
        tmp = pathlib.Path(tmp_root) / tag
        tmp.mkdir()
        opt, dl = _optimiser(struct, regs, tmp, 56, **kw)
        opt.update_scene_pointcloud(*_floor_under(opt))
        log = opt.fit(dl, num_iter=5)
        torch.cuda.synchronize()
        res[tag + '_keys'] = np.asarray(list(log[0]))
        res[tag + '_log'] = np.asarray([[row[k] for k in row] for row in log], np.float64)
        for k in LEAVES:
            res[tag + '_' + k] = opt.engine.leaf(k).cpu().numpy()
    np.savez(out_path, **res)


def test_coefficient_zero_changes_nothing(tmp_path):
    """under MHHIP_DETERMINISTIC=1, set for a fresh child process: bit-identical leaves and logs, and the nine reference keys"""
    out = str(tmp_path / 'runs.npz')
    env = dict(os.environ, MHHIP_DETERMINISTIC='1')
    p = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out, str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = np.load(out)
    assert list(r['plain_keys']) == NINE and list(r['zero_keys']) == NINE
    assert r['plain_log'].shape == (5, 9) and np.isfinite(r['plain_log']).all()
    assert np.array_equal(r['plain_log'], r['zero_log'])
    for k in LEAVES:
        assert np.array_equal(r['plain_' + k].view(np.int32), r['zero_' + k].view(np.int32)), k


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2])
