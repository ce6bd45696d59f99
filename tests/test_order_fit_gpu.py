"""The depth-ordering term inside the fit (``reg_order_coef`` of ``SMPLDepthSequenceOptimizer``, ``SequenceEngine._order_term``):
the engine's launch against the plain kernel, the term at work, captured against eager cycles, the default of 0 changing no
bit, and both opt-in terms together.

A small sequence: 4 frames, 2 people, 48 x 32, batches of 2.  Person 1 stands at 1.6 m, person 0 at 2.2 m on a ray four
pixels to its right: person 1 hides most of person 0, and the data set's instance masks, depths and key-points are rendered
from that arrangement.  The fit then STARTS with the two depths exchanged -- every root translation scaled along its ray, so
that the roots' projections stay -- which puts person 0 in front of the pixels the masks give to person 1.
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
ZERO = dict(proj2d=0.0, depth=0.0, silhouette=0.0, reg_poses=0.0, reg_scales=0.0, reg_velocity=0.0, reg_verts_filter=0.0,
            reg_contact=0.0, reg_foot_sliding=0.0)
Z_FRONT, Z_BACK = 1.6, 2.2
CYCLES = 8          # the twin restores the order through its key-points as well, more slowly: 144 violated pairs become 24
                    # with the term and 54 without after 8 cycles, 0 and 1 after 12


def _arrangement():
    """root translations (T,N,3) of the data: person 1 in front"""
    pT = np.zeros((T, N, 3), np.float32)
    drift = 0.01 * np.arange(T, dtype=np.float32)
    pT[:, 1] = np.float32([-0.05, 0.0, 1.0]) * Z_FRONT
    pT[:, 0] = np.float32([-0.05 + 4.0 / 27.7, 0.0, 1.0]) * Z_BACK
    pT[:, :, 0] += drift[:, None]
    return pT


def _optimiser(struct, regs, tmp_path, seed, coefs=None, **kw):
    """the optimiser, staged, with the two depths exchanged"""
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
    # the data: make_sequence with the translations of _arrangement() instead of its random walk
    plain = synthetic.make_sequence_params

    def arranged(*a, **k):
        sp = plain(*a, **k)
        sp['trans_gt'] = _arrangement()
        sp['valid'] = np.ones_like(sp['valid'])
        return sp
    synthetic.make_sequence_params = arranged
    try:
        seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, N, T, (W, H), seed, cam_K=K)
    finally:
        synthetic.make_sequence_params = plain
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=30)
    dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=BATCH, shuffle=False)
    opt._stage_from_dataloader(dl)
    pT = opt.engine.leaf('poses_T')
    want = torch.tensor([Z_FRONT, Z_BACK], device=pT.device).view(1, N, 1)           # person 0 in front
    pT.mul_(want / pT[..., 2:3])
    torch.cuda.synchronize()
    return opt, dl


def _reduce_sum_multi_ref(x):
    """``k_reduce_sum_multi`` (csrc/mh_image.hip) in numpy float32: lane j of 256 adds x[j], x[j + 256], ... in turn, then a
    binary tree over the 256 lanes, s[j] += s[j + o] for o = 128, 64, ..., 1"""
    s = np.zeros(256, np.float32)
    for i, v in enumerate(np.asarray(x, np.float32)):
        s[i % 256] = s[i % 256] + v
    o = 128
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o >>= 1
    return np.float32(s[0])


def test_one_cycle_against_the_plain_kernel(smpl_struct, smpl_regs, tmp_path):
    """(a) every other coefficient 0.  ``reg_order`` is the float32 sum of the T N ``body_loss`` values in the fixed order of
    ``k_reduce_sum_multi`` (``_reduce_sum_multi_ref``): bit equality."""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path, 61, coefs=ZERO, reg_order_coef=2.0)
    e = opt.engine
    raster = e.raster_terms(opt.znear, opt.zfar)
    e.cycle(0, use_images=True, raster=raster)
    torch.cuda.synchronize()
    g = e.leaf('poses_T', e.grads).cpu().numpy().reshape(T, N, 3)
    print('poses_T gradient, z: %s' % g[..., 2].tolist())
    assert not g[..., :2].any()
    assert (g[:, 1, 2] > 0).all() and (g[:, 0, 2] < 0).all()          # the owner (seen in front) positive, the occluder negative
    assert np.array_equal(g[:, 0, 2].view(np.int32), (-g[:, 1, 2]).view(np.int32))
    assert e.order_gate is not None and (e.order_gate != 0).all()
    gt = torch.zeros(T * N, 3, device='cuda:0')
    body = torch.zeros(T * N, device='cuda:0')
    count = torch.zeros(T * N, dtype=torch.int32, device='cuda:0')
    check(_lib.lib().mh_order_term(*raster.dims, ptr(raster.ws), ptr(e.bits), ptr(e.ebits), ptr(e.order_gate), 2.0, 0.05, 0.5, ptr(gt),
                                   ptr(body), ptr(count), None, None, _lib.stream_ptr(gt.device)))
    torch.cuda.synchronize()
    assert np.array_equal(gt.cpu().numpy().reshape(T, N, 3)[..., 2].view(np.int32), g[..., 2].view(np.int32))
    assert (count.cpu().numpy().reshape(T, N)[:, 1] > 0).all() and not count.cpu().numpy().reshape(T, N)[:, 0].any()
    log = e.read_log(1)[0]
    assert list(log) == NINE + ['reg_order']
    total = float(body.double().sum())
    print('reg_order %.9g, sum of body_loss %.9g' % (float(log['reg_order']), total))
    assert total > 0
    want = _reduce_sum_multi_ref(body.cpu().numpy())
    assert np.float32(log['reg_order']).view(np.int32) == want.view(np.int32), (log['reg_order'], want)


def test_term_restores_the_order(smpl_struct, smpl_regs, tmp_path):
    """(b) CYCLES cycles: fewer violated pixels than at the start and a smaller logged term; a twin run with the coefficient
    at 0 keeps its violations and has the nine keys"""
    runs = {}
    for tag, kw in (('on', dict(reg_order_coef=100.0)), ('off', {})):
        sub = tmp_path / tag
        sub.mkdir()
        opt, dl = _optimiser(smpl_struct, smpl_regs, sub, 62, **kw)
        before = opt.order_report()
        log = opt.fit(dl, num_iter=CYCLES)
        after = opt.order_report()
        assert before['order_px'].shape == (T, N) and before['order_pairs'].shape == (T, N, N) and before['order_loss'].shape == (T, N)
        assert (before['order_pairs'].sum(2) == before['order_px']).all()
        runs[tag] = (int(before['order_px'].sum()), int(after['order_px'].sum()), log)
    (b_on, a_on, log_on), (b_off, a_off, log_off) = runs['on'], runs['off']
    print('violated (pixel, person) pairs before / after %d cycles: %d / %d with the term, %d / %d without; term %.4g -> %.4g'
          % (CYCLES, b_on, a_on, b_off, a_off, log_on[0]['reg_order'], log_on[-1]['reg_order']))
    assert b_on > 0 and b_on == b_off
    assert list(log_off[0]) == NINE and list(log_on[0]) == NINE + ['reg_order']
    assert a_on < b_on
    assert log_on[-1]['reg_order'] < log_on[0]['reg_order']
    assert a_off > 0 and a_on < a_off


def test_graph_replay_matches_eager(smpl_struct, smpl_regs, tmp_path):
    """(c) captured against eager cycles with the term on: the tolerances of tests/test_scene_pen_fit_gpu.py's graph test"""
    import torch
    runs = []
    for graphs in (False, True):
        sub = tmp_path / str(graphs)
        sub.mkdir()
        opt, dl = _optimiser(smpl_struct, smpl_regs, sub, 63, use_graphs=graphs, reg_order_coef=10.0)
        log = opt.fit(dl, num_iter=6)
        torch.cuda.synchronize()
        runs.append((opt.engine.params.cpu().numpy().copy(), log))
    (p0, l0), (p1, l1) = runs
    np.testing.assert_allclose(p1, p0, atol=2e-4 * np.abs(p0).max())
    for c in range(6):
        assert l0[c]['reg_order'] > 0
        for k in ['loss_depth', 'loss_silhouette', 'loss_pose24j', 'reg_order']:
            np.testing.assert_allclose(l1[c][k], l0[c][k], rtol=2e-3, atol=1e-6, err_msg='%s cycle %d' % (k, c))


def test_both_opt_in_terms(smpl_struct, smpl_regs, tmp_path):
    """(e) the scene-penetration term and the ordering term together: two more keys, in this order"""
    import torch
    opt, dl = _optimiser(smpl_struct, smpl_regs, tmp_path, 64, reg_order_coef=10.0, reg_scene_pen_coef=10.0, scene_pen_band=2.0,
                         scene_pen_edge=2.0)
    K = opt.cam_K
    ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
    d = np.where(ys[:, None] > 1e-3, 0.7 / np.maximum(ys[:, None], 1e-3), 10.0)          # a floor 0.2 m above the feet
    opt.update_scene_pointcloud(np.tile(np.minimum(d, 10.0), (1, W)).astype(np.float32), np.tile((ys[:, None] > 1e-3) & (d <= 10.0), (1, W)))
    log = opt.fit(dl, num_iter=3)
    torch.cuda.synchronize()
    assert list(log[0]) == NINE + ['reg_scene_pen', 'reg_order']
    assert all(row['reg_order'] > 0 and np.isfinite(row['reg_scene_pen']) for row in log)
    for k in LEAVES:
        assert torch.isfinite(opt.engine.leaf(k)).all(), k


def test_sharding_is_refused(smpl_struct, smpl_regs, tmp_path):
    from mhhip import sharded
    opt, _ = _optimiser(smpl_struct, smpl_regs, tmp_path, 65, reg_order_coef=1.0)
    with pytest.raises(ValueError, match='shard'):
        sharded.ShardedSequence(opt.engine, 0, T, enabled=True)


# ---- (d) the default changes nothing ------------------------------------------------------------------------------------------

def _child(out_path, tmp_root):
    """two optimisers from the same inputs, one constructed without the new keywords and one with reg_order_coef=0.0 (the
    process was started with MHHIP_DETERMINISTIC=1): leaves and log rows of a fit of both, for the parent to compare"""
    import pathlib
    import conftest  # noqa: F401  (the suite's import paths)
    import torch
    from mhhip import synthetic
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    res = {}
    for tag, kw in (('plain', {}), ('zero', dict(reg_order_coef=0.0, order_margin=0.1, order_delta=0.25))):
        tmp = pathlib.Path(tmp_root) / tag
        tmp.mkdir()
        opt, dl = _optimiser(struct, regs, tmp, 66, **kw)
        log = opt.fit(dl, num_iter=6)
        torch.cuda.synchronize()
        res[tag + '_keys'] = np.asarray(list(log[0]))
        res[tag + '_log'] = np.asarray([[row[k] for k in row] for row in log], np.float64)
        res[tag + '_graphs'] = np.asarray(sorted(repr(k) for k in opt.engine._graphs))
        for k in LEAVES:
            res[tag + '_' + k] = opt.engine.leaf(k).cpu().numpy()
    np.savez(out_path, **res)


def test_coefficient_zero_changes_nothing(tmp_path):
    """under MHHIP_DETERMINISTIC=1, set for a fresh child process: bit-identical leaves and logs after six cycles, equal key
    lists, and graph keys of the same shape (no element more)"""
    out = str(tmp_path / 'runs.npz')
    env = dict(os.environ, MHHIP_DETERMINISTIC='1')
    p = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out, str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = np.load(out)
    assert list(r['plain_keys']) == NINE and list(r['zero_keys']) == NINE
    assert r['plain_log'].shape == (6, 9) and np.isfinite(r['plain_log']).all()
    assert np.array_equal(r['plain_log'], r['zero_log'])
    assert len(r['plain_graphs']) == len(r['zero_graphs']) == 1 and 'order' not in r['zero_graphs'][0]
    for k in LEAVES:
        assert np.array_equal(r['plain_' + k].view(np.int32), r['zero_' + k].view(np.int32)), k


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2])
