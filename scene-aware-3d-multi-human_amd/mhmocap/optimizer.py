"""Drop-in for the reference's ``mhmocap.optimizer`` on MI355X.

``SMPLDepthSequenceOptimizer`` keeps the constructor / ``init_optimized_variables`` / ``fit`` /
``get_optimized_variables`` / ``update_scene_pointcloud`` / ``one_euro_filter`` signatures of
reference ``mhmocap/optimizer.py:146-770`` so that ``predict.py:290-306, 332-344`` keeps working,
but the work is organised for the GPU instead of for autograd:

* the constant per-frame inputs are staged to HBM once (first pass over the dataloader) instead
  of every batch of every cycle (reference optimizer.py:396-400);
* one cycle = ONE pass over all frames: LBS forward -> residual kernels -> hand-written LBS
  backward -> one fused RMSprop launch over a flat parameter buffer.  The reference's per-batch
  ``backward()`` only accumulates gradients (optimizer.py:394-544), so the sums are identical;
  the two batch-structure-dependent terms (in-batch foot-sliding pairs :512-518, per-batch scale
  regulariser :531-539) are evaluated with the same batch partition (contiguous batches of the
  dataloader's batch size, i.e. ``shuffle=False`` semantics);
* losses are logged on the device and read back once per ``fit``.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from mhhip import _lib, engine
from mhhip.sequence import SequenceEngine, COEF_KEYS
from .smpl import SMPL
from .transforms import get_focal, softplus_np

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None


def frames_arg(frames, T):
    """The ``frames`` argument of the diagnostics as int64 indices into a sequence of ``T`` frames: all of them for None,
    else the caller's, in the caller's order and with its duplicates."""
    idx = np.arange(T) if frames is None else np.asarray(frames).reshape(-1)
    if idx.size == 0 or not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= T:
        raise ValueError('frames must be indices in [0, %d), got %r' % (T, frames))
    return idx.astype(np.int64)


class SMPLOptimizerBase(object):
    """reference optimizer.py:32-143"""
    _needs_hip = True          # there is no CPU path (tests/cpu_shard_engine.py subclasses this for the gloo orchestration tests)

    def __init__(self, device=None, smpl_model_parameters_path='model_data/parameters',
                 smpl_J_reg_extra_path='J_regressor_extra.npy', smpl_J_reg_h37m_path='J_regressor_h36m.npy',
                 smpl_J_reg_alphapose_path='SMPL_AlphaPose_Regressor_RMSprop_6.npy',
                 smpl_sparse_joints_key='joints_alphapose', pose24j_weights=None, pose17j_weights=None,
                 smpl_data_struct=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('the MI355X build of mhmocap.optimizer needs a HIP device (no CPU fallback)')
            device = 'cuda:0'
        self.device = torch.device(device)
        if self.device.type != 'cuda' and self._needs_hip:
            raise RuntimeError('the MI355X build of mhmocap.optimizer needs a HIP device, got %s' % device)
        self.smpl_model_parameters_path = os.path.abspath(smpl_model_parameters_path)
        p = lambda f: os.path.join(smpl_model_parameters_path, f)
        self.SMPLPY = SMPL(smpl_model_parameters_path, J_reg_extra9_path=p(smpl_J_reg_extra_path),
                           J_reg_h36m17_path=p(smpl_J_reg_h37m_path), J_reg_alphapose_path=p(smpl_J_reg_alphapose_path),
                           data_struct=smpl_data_struct).to(self.device)
        self.faces_smpl = torch.tensor(np.asarray(self.SMPLPY.faces)[np.newaxis, :].astype(np.int32), device=self.device)
        self.smpl_sparse_joints_key = smpl_sparse_joints_key
        # the joint set the 2D term compares with the 17 detected key-points (reference :41, 75, 695-696): any 17-joint
        # regressor the body model holds; joints_h36m17 is root-relative to joint 14 like SMPL.forward makes it (smpl.py:371-372)
        regs = {'joints_alphapose': (engine.REG_ALPHAPOSE, -1), 'joints_h36m17': (engine.REG_H36M17, 14),
                'joints_mupots': (engine.REG_MUPOTS, -1)}
        if smpl_sparse_joints_key not in regs:
            raise ValueError('smpl_sparse_joints_key must name a 17-joint set (%s), got %r' % (', '.join(regs), smpl_sparse_joints_key))
        self._joints_reg = regs[smpl_sparse_joints_key]
        w17 = np.ones(17, np.float32) if pose17j_weights is None else np.asarray(pose17j_weights, np.float32)
        assert w17.shape == (17,), 'pose17j_weights must hold one weight per key-point'
        w17 = (len(w17) * w17 / np.sum(w17)).astype(np.float32)            # normalised to mean 1 (reference :128-130)
        self._joint_w = None if np.allclose(w17, 1.0) else w17
        self.pose17j_weights = torch.tensor(w17[np.newaxis, :, np.newaxis], device=self.device)
        if pose24j_weights is not None:                                  # kept for call compatibility (:118-126)
            w24 = np.asarray(pose24j_weights, np.float32)
            self.pose24j_weights = torch.tensor((len(w24) * w24 / np.sum(w24))[np.newaxis, :, np.newaxis], device=self.device)

    def predict(self, poses_T, poses_smpl, betas_smpl, scale_factor):
        res = self.SMPLPY(betas=torch.as_tensor(betas_smpl), poses=torch.as_tensor(poses_smpl))
        verts = scale_factor * res['verts'].detach().cpu().numpy() + poses_T
        joints = scale_factor * res[self.smpl_sparse_joints_key].detach().cpu().numpy() + poses_T
        return verts, joints


class SMPLDepthSequenceOptimizer(SMPLOptimizerBase):
    """reference optimizer.py:146-770"""

    def __init__(self, image_size, num_frames, fov=60, focal_length=None, znear=1.0, zfar=100.0, cam_K=None,
                 cam_dist_coef=None, proj2d_loss_coef=1.0, depth_loss_coef=1.0, silhouette_loss_coef=1.0,
                 reg_velocity_coef=1.0, reg_verts_filter_coef=1.0, reg_poses_coef=1.0, reg_scales_coef=1.0,
                 reg_contact_coef=1.0, reg_foot_sliding_coef=1.0, joint_confidence_thr=0.5, eps=1e-3, **kargs):
        self.use_rasteriser = kargs.pop('use_rasteriser', True)
        self.scene_update = kargs.pop('scene_update', 'device')      # 'device' | 'none'
        if self.scene_update not in ('device', 'none'):
            raise ValueError("scene_update must be 'device' or 'none' (the numpy restatement of the reference's host path "
                             "lives with the test infrastructure, not in the product), got %r" % (self.scene_update,))
        self.use_graphs = kargs.pop('use_graphs', True)              # replay each cycle as a captured hipGraph
        # frame sharding is OPT-IN: ``shard_frames=True``, a ``process_group=``, or MHHIP_SHARD_FRAMES=1 in
        # the environment (for an unmodified predict.py under torchrun).  Every rank is then handed the SAME
        # full-sequence inputs and keeps the frames of its contiguous block.  Without the opt-in an initialised
        # torch.distributed changes nothing: every process optimises its own sequence, no collective is issued.
        self.process_group = kargs.pop('process_group', None)
        shard = kargs.pop('shard_frames', None)
        if shard is None:
            shard = self.process_group is not None or os.environ.get('MHHIP_SHARD_FRAMES') == '1'
        self.shard_frames = bool(shard)
        # opt-in scene-penetration term (no counterpart in the reference: keywords only, the positional signature stays):
        # every vertex against the scene's depth map, pushed out along the surface normal (mh_scene_pen_term)
        self.reg_scene_pen_coef = float(kargs.pop('reg_scene_pen_coef', 0.0))
        self.scene_pen_margin = float(kargs.pop('scene_pen_margin', 0.05))
        self.scene_pen_band = float(kargs.pop('scene_pen_band', 0.5))
        self.scene_pen_edge = float(kargs.pop('scene_pen_edge', 0.25))
        if self.reg_scene_pen_coef != 0.0 and self.shard_frames:
            raise ValueError('reg_scene_pen_coef != 0 is not available with frame sharding (shard_frames / process_group / '
                             'MHHIP_SHARD_FRAMES=1)')
        # opt-in depth-ordering term between the people of a frame (no counterpart in the reference either): where the instance
        # masks say who occludes whom, the occluded body is pushed behind the other one (mh_order_term)
        self.reg_order_coef = float(kargs.pop('reg_order_coef', 0.0))
        self.order_margin = float(kargs.pop('order_margin', 0.05))
        self.order_delta = float(kargs.pop('order_delta', 0.5))
        if self.reg_order_coef != 0.0 and self.shard_frames:
            raise ValueError('reg_order_coef != 0 is not available with frame sharding (shard_frames / process_group / '
                             'MHHIP_SHARD_FRAMES=1)')
        self._global_cache = None
        super().__init__(**kargs)
        if focal_length is None:
            focal_length = get_focal(min(image_size), fov)
        if cam_K is None:                                           # (sic) reference :194-197 swaps W/H here
            self.cam_K = np.array([[focal_length, 0, image_size[1] / 2.0], [0, focal_length, image_size[0] / 2.0],
                                   [0, 0, 1]], dtype=np.float32)
        else:
            self.cam_K = np.asarray(cam_K).astype(np.float32)
        self.cam_dist_coef = cam_dist_coef
        self.znear, self.zfar = znear, zfar
        self.coefs = dict(proj2d=proj2d_loss_coef, depth=depth_loss_coef, silhouette=silhouette_loss_coef,
                          reg_velocity=reg_velocity_coef, reg_verts_filter=reg_verts_filter_coef,
                          reg_poses=reg_poses_coef, reg_scales=reg_scales_coef, reg_contact=reg_contact_coef,
                          reg_foot_sliding=reg_foot_sliding_coef)
        if self.reg_scene_pen_coef != 0.0:          # (at 0 the engine is handed exactly the reference's nine)
            self.coefs.update(reg_scene_pen=self.reg_scene_pen_coef, scene_pen_margin=self.scene_pen_margin,
                              scene_pen_band=self.scene_pen_band, scene_pen_edge=self.scene_pen_edge)
        if self.reg_order_coef != 0.0:              # (likewise)
            self.coefs.update(reg_order=self.reg_order_coef, order_margin=self.order_margin, order_delta=self.order_delta)
        for k in COEF_KEYS:
            setattr(self, {'proj2d': 'proj2d_loss_coef', 'depth': 'depth_loss_coef',
                           'silhouette': 'silhouette_loss_coef'}.get(k, k + '_coef'), self.coefs[k])
        self.joint_confidence_thr = joint_confidence_thr
        self.eps = eps
        self.num_frames = num_frames
        self.img_w, self.img_h = image_size
        self.min_delta_z = 1.0
        self.engine = None
        self.scene_depth = None
        self.scene_pcd = None
        self.poses_T_filtered = None
        self.verts_filtered = None

    # -- leaves, exposed with the reference's shapes ------------------------------------------------
    # (frame-sharded run: the per-frame leaves are the LOCAL frames [self.first_frame, self.last_frame);
    # get_optimized_variables() returns the whole sequence on every rank)
    @property
    def poses_T(self):
        return self.engine.leaf('poses_T').view(self.engine.T, self.num_people, 1, 3)

    @property
    def poses_smpl(self):
        return self.engine.leaf('poses_smpl')

    @property
    def betas_smpl(self):
        return self.engine.leaf('betas').view(1, self.num_people, 10)

    @property
    def xscale_factor(self):
        return self.engine.leaf('xscale').view(1, self.num_people, 1, 1)

    @property
    def zmin_lin(self):
        return self.engine.leaf('zmin_lin').view(self.engine.T, 1, 1)

    @property
    def zmax_lin(self):
        return self.engine.leaf('zmax_lin').view(self.engine.T, 1, 1)

    # -- frame sharding ---------------------------------------------------------------------------------
    def _world(self):
        if self.shard_frames and dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.process_group), dist.get_rank(self.process_group)
        return 1, 0

    def _bcast(self, arr, src=0):
        """numpy array -> the same array on every rank (replicas must start bit-identical)"""
        world, _ = self._world()
        if world == 1:
            return arr
        t = torch.as_tensor(np.ascontiguousarray(arr)).to(self.device)
        dist.broadcast(t, src=dist.get_global_rank(self.process_group, src) if self.process_group is not None else src,
                       group=self.process_group)
        return t.cpu().numpy()

    def _gather_frames(self, local):
        """(T_local, ...) tensor of this rank -> (T, ...) numpy array of the whole sequence, on every rank"""
        world, _ = self._world()
        local = local.detach().contiguous()
        if world == 1:
            return local.cpu().numpy().copy()
        tmax = max(b - a for a, b in self._bounds)
        pad = torch.zeros((tmax,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        pad[:local.shape[0]] = local
        outs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(outs, pad, group=self.process_group)
        return torch.cat([o[:b - a] for o, (a, b) in zip(outs, self._bounds)]).cpu().numpy()

    def refresh_global_leaves(self):
        """collective: re-gather the whole-sequence leaves get_optimized_variables() serves (frame-sharded run only)"""
        self._global_cache = None
        self.sh.leaves_changed()
        self.sh.refresh_halo()            # (every rank is here: the neighbours' boundary leaves are stale too -- ADVICE r05)
        return self._global_leaves()

    def check_replicas(self):
        """Debug aid (MHHIP_CHECK_REPLICAS=1 runs it every 25 cycles): the shared leaves betas | xscale and their
        RMSprop state must be bit-identical on every rank."""
        world, rank = self._world()
        if world == 1:
            return True
        e = self.engine
        mine = torch.cat([e.params[e.shared_lo:], e.sq[e.shared_lo:], e.buf[e.shared_lo:]]).contiguous()
        outs = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(outs, mine, group=self.process_group)
        for r, o in enumerate(outs):
            if not torch.equal(o, outs[0]):
                raise RuntimeError('replicated shape/scale leaves diverged between rank 0 and rank %d (max |diff| %.3e)'
                                   % (r, float((o - outs[0]).abs().max())))
        return True

    # -- reference optimizer.py:262-321 ---------------------------------------------------------------
    def init_optimized_variables(self, pose2d, poses_smpl, betas_smpl, valid_smpl, scale_factor=None, num_iter=100):
        assert (pose2d.shape[:2] == poses_smpl.shape[:2] == betas_smpl.shape[:2] == valid_smpl.shape[:2]), (
            f'Error: invalid inputs {pose2d.shape}, {poses_smpl.shape}, {betas_smpl.shape}, {valid_smpl.shape}')
        T, N = pose2d.shape[0:2]
        assert T == self.num_frames, f'expected {self.num_frames} frames, got {T}'
        self.num_people = N
        if scale_factor is not None:
            xscale = (np.log(scale_factor) / np.log(1.1)).astype(np.float32).reshape(N)
            self.optim_scale_factor = False
        else:
            xscale = np.zeros(N, np.float32)
            self.optim_scale_factor = True
        self._pose2d_init = np.asarray(pose2d, np.float32)
        self._poses_ref = np.asarray(poses_smpl, np.float32)
        self._valid = (np.asarray(valid_smpl) > 0.7).astype(np.float32)       # :299
        init_log, poses_T = self.__init_global_poses(pose2d, poses_smpl, betas_smpl, xscale, num_iter)
        poses_T = self._bcast(poses_T)           # frame-sharded run: every rank starts from rank 0's warm-up result
        max_z = np.clip(np.max(poses_T[..., 2], axis=1), 2, None)            # (T,)  :292
        avg_betas = np.mean(betas_smpl, axis=0).astype(np.float32)            # (N,10) :296
        self._betas_ref = avg_betas
        self._init_leaves = dict(poses_T=poses_T, poses_smpl=self._poses_ref, betas=avg_betas,
                                 zmin_lin=np.ones_like(max_z), zmax_lin=2.0 * max_z, xscale=xscale)
        # the dataloader's batch size is only known in fit(): provisional blocks now (every rank must own frames for
        # get_optimized_variables() to work before fit, predict.py:333), re-sharded at staging if the batch differs
        bs0 = 10
        while self._world()[0] > 1 and bs0 > 1 and (T + bs0 - 1) // bs0 < self._world()[0]:
            bs0 -= 1
        self._build_engine(batch_size=bs0)
        self._global_leaves()                     # sharded: gathered once here, served locally until fit() ends
        self.scene_depth = None
        self.scene_pcd = None
        self._report_scene = None
        self.poses_T_filtered = None
        self.verts_filtered = None
        return init_log

    def _make_engine(self, **kw):
        """the device-resident state of this rank's frames.  (The gloo tests of the frame-sharded orchestration subclass the
        optimiser in tests/cpu_shard_engine.py and return a torch-CPU stand-in with the same interface here; nothing in the
        product does.)"""
        return SequenceEngine(self.SMPLPY.body_model, **kw)

    def _build_engine(self, batch_size, leaves=None):
        """(Re)build the engine for this rank's frames.  ``leaves``: whole-sequence arrays (default: the initial ones)."""
        from mhhip import sharded
        leaves = self._init_leaves if leaves is None else leaves
        world, rank = self._world()
        self._bounds = sharded.shard_bounds(self.num_frames, world, int(batch_size))
        self.first_frame, self.last_frame = self._bounds[rank]
        if world > 1 and self.last_frame <= self.first_frame:
            raise RuntimeError('rank %d owns no frames: %d frames in batches of %d over %d ranks' %
                               (rank, self.num_frames, batch_size, world))
        sl = slice(self.first_frame, self.last_frame)
        kw = dict(image_size=(self.img_w, self.img_h), num_frames=self.last_frame - self.first_frame,
                  num_people=self.num_people, cam_K=self.cam_K, cam_dist_coef=self.cam_dist_coef, coefs=self.coefs,
                  joint_confidence_thr=self.joint_confidence_thr, eps=self.eps, batch_size=int(batch_size),
                  joint_weights=self._joint_w)
        if self._joints_reg[0] != engine.REG_ALPHAPOSE:
            kw['joints_reg'] = self._joints_reg
        self.engine = self._make_engine(**kw)
        self.engine.set_leaves(poses_T=np.asarray(leaves['poses_T'])[sl], poses_smpl=np.asarray(leaves['poses_smpl'])[sl],
                               betas=self._bcast(np.asarray(leaves['betas'], np.float32)),
                               zmin_lin=np.asarray(leaves['zmin_lin'])[sl], zmax_lin=np.asarray(leaves['zmax_lin'])[sl],
                               xscale=self._bcast(np.asarray(leaves['xscale'], np.float32)))
        self.sh = sharded.ShardedSequence(self.engine, self.first_frame, self.num_frames, group=self.process_group,
                                          enabled=self.shard_frames)
        # the whole-sequence leaves this engine was built from ARE the gathered copy until the next fit refreshes it (no
        # collective needed: every rank was handed the same arrays)
        self._global_cache = None
        if world > 1:
            T, N = self.num_frames, self.num_people
            self._global_cache = dict(
                poses_T=np.array(leaves['poses_T'], np.float32).reshape(T, N, 1, 3), poses_smpl=np.array(leaves['poses_smpl'], np.float32),
                betas=np.array(self.engine.leaf('betas').cpu().numpy()), zmin_lin=np.array(leaves['zmin_lin'], np.float32),
                zmax_lin=np.array(leaves['zmax_lin'], np.float32), xscale=np.array(self.engine.leaf('xscale').cpu().numpy()))
        self._engine_batch = int(batch_size)
        self.valid_smpl = torch.tensor(self._valid, device=self.device)
        self._staged = False

    def _global_leaves(self, cached=False):
        """Whole-sequence leaves.  In a frame-sharded run this is a COLLECTIVE (all_gather over the group): ``fit`` and
        ``init_optimized_variables`` call it on every rank and keep the result, so that ``get_optimized_variables()``
        (``cached=True``) is a local read -- the usual ``if rank == 0: save(opt.get_optimized_variables())`` works."""
        if cached and self._world()[0] > 1:
            if self._global_cache is not None:
                return self._global_cache
            # no gathered copy (the engine was rebuilt since the last fit / init): gathering HERE would be a collective
            # inside what is documented as a local read -- a rank-0-only call would hang the job
            raise RuntimeError('get_optimized_variables() in a frame-sharded run reads the copy gathered at the end of '
                               'init_optimized_variables() / fit(); there is none since the engine was rebuilt -- call '
                               'refresh_global_leaves() on EVERY rank first (a collective)')
        g = self._gather_global()
        if self._world()[0] > 1:
            self._global_cache = g
        return g

    def _gather_global(self):
        e = self.engine
        return dict(poses_T=self._gather_frames(e.leaf('poses_T')).reshape(self.num_frames, self.num_people, 1, 3),
                    poses_smpl=self._gather_frames(e.leaf('poses_smpl')), betas=e.leaf('betas').cpu().numpy().copy(),
                    zmin_lin=self._gather_frames(e.leaf('zmin_lin')), zmax_lin=self._gather_frames(e.leaf('zmax_lin')),
                    xscale=e.leaf('xscale').cpu().numpy().copy())

    # -- reference optimizer.py:710-770: only poses_T is a leaf, so SMPL runs once --------------------
    def __init_global_poses(self, pose2d, poses_smpl, betas_smpl, xscale, num_iter, joints_thr=0.15):
        T, N = pose2d.shape[0:2]
        B = T * N
        if num_iter <= 0:
            return [], np.tile(np.array([[[[0, 0, 1]]]], np.float32), (T, N, 1, 1))          # :729
        m = self.SMPLPY.body_model
        dev = self.device
        L = _lib.lib()
        st = _lib.stream_ptr(dev)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        verts, _, _, _ = m.lbs_forward(f32(betas_smpl).view(B, 10), f32(poses_smpl).view(B, 72), want_vposed=False)
        local = m.joints_regress(self._joints_reg[0], verts, root=self._joints_reg[1])   # (B,17,3), constant during warm-up
        del verts
        pT = f32(np.tile(np.array([[0, 0, 1]], np.float32), (B, 1)))          # :729
        p2d, xs = f32(pose2d).view(B, 17, 3), f32(xscale)
        g = torch.zeros_like(pT)
        mom, var = torch.zeros_like(pT), torch.zeros_like(pT)
        body_loss = torch.zeros(B, device=dev)
        log_dev = torch.zeros(max(num_iter, 1), device=dev)
        vel = torch.zeros(1, device=dev)
        Kp = np.ascontiguousarray(self.cam_K.reshape(9)).ctypes.data_as(_lib.c_float_p)
        Kd = None if self.cam_dist_coef is None else np.ascontiguousarray(self.cam_dist_coef, np.float32)
        Kdp = None if Kd is None else Kd.ctypes.data_as(_lib.c_float_p)
        lr = 0.5
        jwp = None if self._joint_w is None else self._joint_w.ctypes.data_as(_lib.c_float_p)
        for it in range(num_iter):
            _lib.check(L.mh_warmup_project_w(B, N, _lib.ptr(local), _lib.ptr(xs), _lib.ptr(pT), Kp, Kdp, jwp, _lib.ptr(p2d),
                                             joints_thr, float(self.coefs['proj2d']), _lib.ptr(g), _lib.ptr(body_loss), st))
            _lib.check(L.mh_velocity_term(T, N, _lib.ptr(pT), None, None, float(self.coefs['reg_velocity']),
                                          _lib.ptr(g), _lib.ptr(vel), st))
            _lib.check(L.mh_reduce_sum(_lib.ptr(body_loss), B, 1.0, _lib.ptr(log_dev[it:it + 1]), st))
            engine.adam_step(pT, g, mom, var, it + 1, lr)                     # Adam(lr=.5, betas=(.5,.5), eps=1e-6) :738
            lr *= 0.95                                                        # ExponentialLR(0.95) :739
        log = log_dev.cpu().numpy()
        return [{'loss_2d': np.float32(v)} for v in log[:num_iter]], pT.view(T, N, 1, 3).cpu().numpy()

    # -- staging the constant inputs (first pass over the dataloader) ---------------------------------
    def _stage_from_dataloader(self, dataloader):
        T, N = self.num_frames, self.num_people
        H, W = self.img_h, self.img_w
        bs = getattr(dataloader, 'batch_size', None)
        if getattr(dataloader, 'drop_last', False) and len(getattr(dataloader, 'dataset', ())) % int(bs or 1) != 0:
            # the reference would never show the dropped tail frames to the data terms; staging reads every frame once and
            # the cycle covers all of them -- refuse rather than optimise something else silently
            raise ValueError('dataloader drops its last, incomplete batch (drop_last=True with %d frames in batches of %s): '
                             'not supported by the staged optimisation loop' % (len(dataloader.dataset), bs))
        if self._is_shuffled(dataloader) and self._world()[0] > 1:
            import warnings
            warnings.warn('dataloader has shuffle=True (configs/predict_mupots.yml:14) in a FRAME-SHARDED run: a random batch '
                          'mixes frames of different ranks, so the foot-sliding term (optimizer.py:512-518) pairs CONSECUTIVE '
                          'frames inside contiguous batches of %s frames instead (shuffle=False semantics; the single-process '
                          'run reproduces the shuffled pairing).  Every other term is independent of the batch order.' % bs)
        first = True
        have_img = True
        store = {}
        keep = {}
        world, _ = self._world()
        ds = getattr(dataloader, 'dataset', None)
        direct = self._dataset_is_plain(dataloader, ds)
        own = None                      # frame range of the per-pixel inputs kept on this rank (None: the whole sequence)
        if direct and world > 1:
            # the batch size is known up front: fix the shard first, keep the big per-pixel inputs of the own frames only
            if int(bs) != self._engine_batch:
                self._build_engine(int(bs), leaves=self._global_leaves())
            own = (self.first_frame, self.last_frame)
        LOCAL = ('depths', 'seg_mask', 'images', 'backmasks')     # per-pixel inputs: only the own frames are kept
        PINNED = ('depths', 'seg_mask')          # uploaded once at PCIe speed; images / backmasks stay pageable (they are
        # only read again for the scene update's set-up and the scene image) -- and never more than this many bytes
        pin_budget = [int(float(os.environ.get('MHHIP_STAGE_PINNED_MAX_GB', '8')) * (1 << 30))]

        def alloc(k, shape, dtype):
            n = T if own is None or k not in LOCAL else own[1] - own[0]
            nbytes = int(np.prod((n,) + tuple(shape))) * np.dtype(dtype).itemsize
            pin = (k in PINNED and torch.cuda.is_available() and os.environ.get('MHHIP_STAGE_PINNED', '1') == '1'
                   and nbytes <= pin_budget[0])
            if pin:
                try:
                    t = torch.zeros((n,) + tuple(shape), dtype=torch.from_numpy(np.zeros(0, dtype)).dtype, pin_memory=True)
                    pin_budget[0] -= nbytes
                    keep[k] = t
                    store[k] = t.numpy()
                    return
                except (RuntimeError, TypeError):
                    pass
            store[k] = np.zeros((n,) + tuple(shape), dtype)

        def put(idx, data, lead):
            nonlocal have_img
            for k in ['depths', 'seg_mask', 'pose2d', 'poses_smpl', 'images', 'backmasks']:
                if k not in data:
                    if k in ('depths', 'seg_mask'):
                        have_img = False
                    continue
                if own is not None and k in LOCAL:
                    if not own[0] <= idx < own[1]:
                        continue
                    a = data[k].numpy() if isinstance(data[k], torch.Tensor) else np.asarray(data[k])
                    if k == 'backmasks' and a.dtype != np.uint8:
                        a = a != 0
                    if k not in store:
                        alloc(k, a.shape[lead:], np.uint8 if k == 'backmasks' else a.dtype)
                    store[k][idx - own[0]] = a
                    continue
                a = data[k].numpy() if isinstance(data[k], torch.Tensor) else np.asarray(data[k])
                if k == 'backmasks' and a.dtype != np.uint8:
                    a = a != 0          # only "background or not" is ever read (fhsog.py:190-197): one byte per pixel from here on
                if k not in store:
                    alloc(k, a.shape[lead:], np.uint8 if k == 'backmasks' else a.dtype)
                store[k][idx] = a

        # this extra pass must not advance the shuffle of cycle 0: the global generator AND the loader's / sampler's own
        # generators (a DataLoader built with generator= draws its base seed, a RandomSampler with generator= its
        # permutation, from those -- ADVICE r03)
        rng_state = None if direct else torch.get_rng_state()
        own_gens = []
        if not direct:
            for holder in (dataloader, getattr(dataloader, 'sampler', None), getattr(dataloader, 'batch_sampler', None),
                           getattr(getattr(dataloader, 'batch_sampler', None), 'sampler', None)):
                gen = getattr(holder, 'generator', None)
                if isinstance(gen, torch.Generator) and all(gen is not g0 for g0, _ in own_gens):
                    own_gens.append((gen, gen.get_state()))
        if direct:
            # A plain map-style dataset behind the stock collate function: the frames are read from the dataset itself,
            # straight into the staging buffers.  Going through the loader costs a torch.stack per key and batch plus
            # the profiler hooks of every __next__ (250 of the 350 ms this pass took at C3) for batches that are taken
            # apart again right here.
            for i in range(len(ds)):
                item = ds[i]
                put(int(np.asarray(item['idxs']).reshape(-1)[0]), item, 0)
        else:
            for data in dataloader:
                idx = np.asarray(data['idxs']).reshape(-1).astype(np.int64)
                if bs is None and first:
                    bs = len(idx)
                put(idx, data, 1)
                first = False
        if rng_state is not None:
            torch.set_rng_state(rng_state)
        for gen, state in own_gens:
            gen.set_state(state)
        if world > 1 and int(bs) != self._engine_batch:
            # block boundaries are multiples of the batch size: re-shard with the dataloader's
            self._build_engine(int(bs), leaves=self._global_leaves())
        self.engine.set_batch_size(int(bs))
        sl = slice(self.first_frame, self.last_frame)
        loc = (lambda k: store[k]) if own is not None else (lambda k: store[k][sl])
        self.engine.stage(store['pose2d'][sl], store.get('poses_smpl', self._poses_ref)[sl], self._valid[sl], self._betas_ref,
                          loc('seg_mask') if have_img else None, loc('depths') if have_img else None)
        # own frames only (scene update set-up, colour median of the scene image once per fit); copied out of the staging
        # buffers so that no page-locked memory outlives this call
        self._images = None if 'images' not in store else np.array(loc('images'))
        self._backmasks = None if 'backmasks' not in store else np.ascontiguousarray(loc('backmasks'))   # uint8, never pinned: no copy
        keep.clear()
        self._staged = True
        try:
            import weakref
            self._staged_from = weakref.ref(dataloader)
        except TypeError:
            self._staged_from = None

    @staticmethod
    def _is_shuffled(dataloader):
        """does the loader deliver anything but contiguous batches in order?"""
        sampler = getattr(dataloader, 'sampler', None)
        return (getattr(dataloader, 'batch_sampler', None) is not None and sampler is not None
                and type(sampler).__name__ != 'SequentialSampler')

    def _cycle_batch_tables(self, dataloader, num_iter):
        """The index batches of ``num_iter`` passes over a shuffling dataloader, as a (num_iter, nbatches * batch) int32
        device table (-1 = empty position).  Indices only -- the inputs stay staged.  Consumes the random number
        generators exactly like the reference's ``for data in dataloader`` (optimizer.py:394) does once per cycle: the
        ``_base_seed`` draw of ``DataLoader.__iter__`` from the loader's generator, then whatever the batch sampler
        draws (RandomSampler: one seed from the global generator) -- so under one ``torch.manual_seed`` both sides see
        the same batches.  Nothing else on this path draws random numbers, so drawing all cycles up front is the same
        sequence."""
        e = self.engine
        nb, bs = e.nbatches, e.batch
        tab = np.full((num_iter, nb, bs), -1, np.int32)
        for c in range(num_iter):
            torch.empty((), dtype=torch.int64).random_(generator=getattr(dataloader, 'generator', None))
            seen = 0
            for b, idx in enumerate(dataloader.batch_sampler):
                idx = [int(i) for i in idx]
                assert b < nb and len(idx) <= bs, 'batch sampler delivers more / larger batches than len(dataset) / batch_size'
                tab[c, b, :len(idx)] = idx
                seen += len(idx)
            assert seen == self.num_frames and len(np.unique(tab[c][tab[c] >= 0])) == seen, \
                'every frame must appear exactly once per pass over the dataloader'
        return torch.as_tensor(tab.reshape(num_iter, nb * bs)).to(self.device)

    @staticmethod
    def _dataset_is_plain(dataloader, ds):
        """True when reading ``dataloader.dataset[i]`` for every i yields exactly the frames the loader would deliver
        (stock DataLoader, stock collate, stock batch sampler over a sequential or random sampler, no dropped tail)."""
        if os.environ.get('MHHIP_STAGE_VIA_LOADER') == '1' or ds is None:
            return False
        try:
            from torch.utils.data import DataLoader, IterableDataset
            from torch.utils.data._utils.collate import default_collate
        except ImportError:
            return False
        return (type(dataloader) is DataLoader and dataloader.collate_fn is default_collate
                and not isinstance(ds, IterableDataset) and hasattr(ds, '__getitem__') and hasattr(ds, '__len__')
                and dataloader.batch_size is not None and not dataloader.drop_last
                and type(dataloader.batch_sampler).__name__ == 'BatchSampler'
                and type(dataloader.sampler).__name__ in ('SequentialSampler', 'RandomSampler'))

    # -- reference optimizer.py:324-602 ---------------------------------------------------------------
    def fit(self, dataloader, num_iter=250, min_cutoff1=0.01, min_cutoff2=0.001, beta1=0.02, beta2=0.5,
            update_filters_every=25, verbose=False):
        # the inputs are read once; a DIFFERENT dataloader object means different inputs (the reference reads whatever it is
        # handed in every cycle), so it is staged afresh -- the same object is trusted to deliver the same frames
        other = self._staged and getattr(self, '_staged_from', None) is not None and self._staged_from() is not dataloader
        if not self._staged or other:
            self._stage_from_dataloader(dataloader)
        e, sh = self.engine, self.sh
        world, rank = self._world()
        if not self.optim_scale_factor:
            print('WARNING!!! Not optimizing scale_factor!')
        if num_iter > e.log.shape[0]:
            e._flush_log()
            e.log = torch.zeros(num_iter, 16, device=self.device)
        raster = None
        if self.use_rasteriser and e.has_images:
            raster = e.raster_terms(self.znear, self.zfar)        # one per engine: captured graphs bake its addresses
        scene_mode = self.scene_update
        # shuffle: True (the shipped config): the in-batch pairs of the foot-sliding term follow the loader's batches
        tables = None
        if world == 1 and self._is_shuffled(dataloader):
            tables = self._cycle_batch_tables(dataloader, num_iter)
        else:
            e.set_batch_table(None)
        self.batch_tables = tables
        check_every = 25 if os.environ.get('MHHIP_CHECK_REPLICAS') == '1' else 0
        lr = 0.01                                                             # a new RMSprop + ExponentialLR per fit (:355-356):
        e.sq.zero_()                                                          # ... its running squares and momentum buffers
        e.buf.zero_()                                                         # start at zero in EVERY call
        sh.leaves_changed()                                                   # (sharded: the neighbours' boundary leaves are gathered
        sh.refresh_halo()                                                     #  here, by every rank: the cycles issue no hidden collective)
        # ONE captured graph for the whole fit (single process): what changes between the phases of a fit -- no scene before
        # cycle 30 (:578-584), no filtered trajectories before the first filter update (:383-392, 571-573) -- is switched by
        # device-resident words the captured launches read, so the buffers those launches touch must exist from cycle 0 on
        if (self.use_graphs and world == 1 and os.environ.get('MHHIP_UNIFORM') != '0' and hasattr(e, 'enable_filter_gate')):
            if (num_iter > 30 and scene_mode == 'device' and e.has_images and self._backmasks is not None and e._scene_dev is None):
                sh.scene_setup(self._backmasks)
            if any(c % update_filters_every == 0 for c in range(30, num_iter)):
                e.enable_filter_gate()
        # the per-person sums of the shape / scale gradients ride in the update's launch (single process, captured cycles: the
        # step follows every cycle at once and nothing reads the gradients in between)
        deferring = bool(self.use_graphs and world == 1 and hasattr(e, 'defer_person'))
        if deferring:
            defer_before = e.defer_person
            e.defer_person, e.freeze_xscale = True, not self.optim_scale_factor
        cycles = range(num_iter)
        if verbose and tqdm is not None and rank == 0:
            cycles = tqdm(cycles)
        for cycle in cycles:
            if cycle >= 30 and cycle % update_filters_every == 0:            # :383-392
                if world > 1:
                    sh.update_filters(min_cutoff1, beta1, min_cutoff2, beta2)    # state handed rank k -> k+1
                else:
                    e.update_filters(min_cutoff1, beta1, min_cutoff2, beta2)
                self.poses_T_filtered = e.pT_filt.view(e.T, self.num_people, 1, 3)
                self.verts_filtered = e.verts_filt
            if tables is not None:
                e.set_batch_table(tables[cycle])
            scene_now = cycle >= 30 and e.has_images and self._backmasks is not None      # :578-584
            dev_scene = scene_now and scene_mode == 'device'
            if dev_scene and e._scene_dev is None:
                # the update only reads the depth-range leaves as they are before this cycle's step and is first used by
                # the NEXT cycle's contact term: launched on its own stream during this cycle, swapped in after it
                sh.scene_setup(self._backmasks)
            if world > 1:
                # frame-sharded: the cycle is one graph; ONE all-reduce per cycle in sh.step (mhhip/sharded.py);
                # the median of the scene update runs pixel-sharded over all ranks' frames
                if dev_scene:
                    sh.scene_update()
                sh.cycle(cycle, raster=raster, graphs=self.use_graphs)
            else:
                # single process: one captured graph per cycle (the device scene update is issued after the first replay)
                sh.cycle(cycle, raster=raster, graphs=self.use_graphs, scene_update=dev_scene)
            if dev_scene:
                e.scene_device_swap()
            if not self.optim_scale_factor:
                e.leaf('xscale', e.grads).zero_()
            sh.step(lr)            # RMSprop(lr=.01, alpha=.5, momentum=.9) :355; launched outside the captured cycle, lr by value
                                   # (frame-sharded: per-frame leaves, THE all-reduce of the cycle, shared leaves -- mhhip/sharded.py)
            lr *= 0.99                                                        # ExponentialLR(0.99) :356
            if check_every and cycle % check_every == 0:
                self.check_replicas()
        if deferring:
            e._flush_person()
            e.defer_person = defer_before
        self._finish_scene()
        self._global_cache = None
        self._global_leaves()                     # sharded: the one gather of the result (collective, every rank is here)
        return sh.read_log(num_iter)

    def _finish_scene(self):
        """results of the device scene aggregation back on the host + the scene image (optimizer.py:595-600), once per fit"""
        e = self.engine
        if self.scene_update != 'device' or e._scene_dev is None:
            return
        self.scene_depth, ma_mask, pts = e.scene_device_result()
        self.scene_pcd = pts.unsqueeze(0).unsqueeze(0)
        self._report_scene = (self.scene_depth, ma_mask)
        if self._images is not None:
            # colour median + looped 11x11 fill on the device (independent of the optimised variables: once per fit);
            # frame-sharded: pixel-sharded over the ranks like the depth median
            self.scene_img, self.scene_mask = self.sh.scene_image(self._images)

    # -- reference optimizer.py:605-616 ---------------------------------------------------------------
    def update_scene_pointcloud(self, scene_depth, scene_mask):
        pts = self.engine.scene_from_depth(np.asarray(scene_depth, np.float32), np.asarray(scene_mask))
        self.scene_pcd = pts.unsqueeze(0).unsqueeze(0)                        # (1,1,M,3)
        # the maps the cloud came from, for fit_report (body against scene is measured per pixel of the depth map)
        self._report_scene = (np.array(scene_depth, np.float32), np.asarray(scene_mask, np.float32) > 0.5)
        if self.reg_scene_pen_coef != 0.0:          # ... and, packed into one z-map, for the penetration term
            self.engine.set_scene_depth(self._report_scene[0], self._report_scene[1])

    # -- reference optimizer.py:619-636 ---------------------------------------------------------------
    def get_optimized_variables(self):
        e = self.engine
        T, N = self.num_frames, self.num_people
        # frame-sharded run: the whole sequence as gathered at the end of init_optimized_variables() / fit() -- a local
        # read, NOT a collective (leaves edited by hand in between: call refresh_global_leaves() on every rank)
        g = self._global_leaves(cached=True)
        zmin, zmax = g['zmin_lin'].reshape(T, 1, 1), g['zmax_lin'].reshape(T, 1, 1)
        min_z = softplus_np(zmin)
        max_z = min_z + self.min_delta_z + softplus_np(zmax)
        return {
            'scale_factor': np.power(np.float32(1.1), g['xscale']).reshape(1, N, 1, 1),
            'poses_T': g['poses_T'].reshape(T, N, 1, 3),
            'poses_smpl': g['poses_smpl'].reshape(T, N, 72),
            'betas_smpl': g['betas'].reshape(1, N, 10),
            'valid_smpl': self._valid.copy(),
            'min_z': min_z, 'max_z': max_z,
            'scene_depth': self.scene_depth if hasattr(self, 'scene_depth') else None,
            'scene_img': self.scene_img if hasattr(self, 'scene_img') else None,
            'scene_mask': self.scene_mask if hasattr(self, 'scene_mask') else None,
        }

    # -- what the diagnostics below share: their checks, and their loop over the frames -----------------------------------
    def _diag_frames(self, name, verb, frames, chunk, need=None):
        """What every diagnostic checks first, in this order: there is an engine, the run is not frame-sharded, the method's
        own precondition (``need()`` raises), ``frames``.  ``verb`` is 'render from' / 'report on' / 'measure on'.  Returns
        the frame indices (``frames_arg``) and ``chunk`` as at least 1."""
        if self.engine is None:
            raise RuntimeError('%s: nothing to %s before init_optimized_variables()' % (name, verb.split()[0]))
        if self._world()[0] > 1:
            raise RuntimeError('%s is not available in a frame-sharded run (world > 1): %s the gathered '
                               'result of get_optimized_variables() in one process' % (name, verb))
        if need is not None:
            need()
        return frames_arg(frames, self.num_frames), max(1, int(chunk))

    def _diag_chunks(self, idx, chunk, call, prev=False):
        """The loop of every diagnostic over the frames ``idx``, ``chunk`` at a time: the vertices of ``predict`` (LBS, scale,
        translation) of the current leaves at ``idx[sl]`` as (n, N, V, 3), ``call(sl, verts)`` -> dict of tensors, the dicts
        concatenated as numpy arrays, plus ``'frames'``.  ``prev=True``: ``call(sl, verts, before)`` with the vertices of
        every frame's predecessor in the SEQUENCE as well (frame 0: its own); each frame's forward is computed once."""
        e, m = self.engine, self.SMPLPY.body_model
        T, N = self.num_frames, self.num_people
        parts = []
        with torch.cuda.device(self.device), torch.no_grad():
            pT_all, pose_all = e.leaf('poses_T').view(T, N, 3), e.leaf('poses_smpl').view(T, N, 72)
            for f0 in range(0, len(idx), chunk):
                sl = slice(f0, min(len(idx), f0 + chunk))
                fr = idx[sl]
                need = np.unique(np.concatenate([fr, fr[fr > 0] - 1])) if prev else fr      # with predecessors: each once
                sel = torch.as_tensor(need, device=self.device)
                nb = len(need) * N
                verts, _, _, _ = m.lbs_forward(e.leaf('betas').view(N, 10), pose_all[sel].reshape(nb, 72), e.leaf('xscale').view(N),
                                               pT_all[sel].reshape(nb, 3), want_vposed=False)
                verts = verts.view(len(need), N, -1, 3)
                if prev:
                    at = torch.as_tensor(np.searchsorted(need, fr), device=self.device)
                    before = torch.as_tensor(np.searchsorted(need, np.maximum(fr - 1, 0)), device=self.device)
                    got = call(sl, verts[at].contiguous(), verts[before].contiguous())
                else:
                    got = call(sl, verts)
                parts.append({k: v.cpu().numpy() for k, v in got.items()})
                del verts, got
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        out['frames'] = idx
        return out

    # -- the fit as images (the reference looks at it with scatter plots of projected vertices, predict.py:195-243) ------
    def render_scene(self, frames=None, images=True, **kw):
        """Render the current leaves at ``frames`` (default: all): the vertices of ``predict`` (LBS, scale, translation)
        composited over the people of every frame by ``mhhip.raster.render_scene`` -- depth, person and face labels,
        normals, a shaded overlay on the staged input images (``images=True`` and images were staged; else on black),
        vertex visibility and per-person pixel counts, as numpy arrays, plus ``'frames'``.  ``kw`` goes to
        ``mhhip.raster.render_scene`` (palette, light, ambient, alpha, outputs, chunk).  Reads the leaves only: buffers
        and rasteriser workspace of its own, nothing of the engine's state is written."""
        from mhhip import raster
        idx, chunk = self._diag_frames('render_scene', 'render from', frames, kw.pop('chunk', 32))
        T = self.num_frames
        imgs = None
        if images and getattr(self, '_staged', False) and getattr(self, '_images', None) is not None:
            imgs = np.asarray(self._images)
            if imgs.shape != (T, self.img_h, self.img_w, 3):
                raise ValueError('staged images are %s, not (T,H,W,3) = (%d,%d,%d,3)' % (imgs.shape, T, self.img_h, self.img_w))
            imgs = np.ascontiguousarray(imgs[idx]).astype(np.uint8)
        return self._diag_chunks(idx, chunk, lambda sl, verts: raster.render_scene(
            self.SMPLPY.body_model, verts, self.cam_K, (self.img_w, self.img_h), images=None if imgs is None else imgs[sl],
            chunk=chunk, **kw))

    # -- the fit from the side or from above (the reference opens an Open3D window, visualization.py) ---------------------
    def render_view(self, view, frames=None, image_size=None, K=None, scene=True, splat=1.0, **kw):
        """Render the current leaves at ``frames`` (default: all) from ANOTHER camera: ``view`` = (R (3,3), t (3)) or
        ((len(frames),3,3), (len(frames),3)) with x_view = R x + t in the fit camera's space (``mhhip.view.look_at``, ``orbit``,
        ``top_down``), ``image_size`` (W,H) and ``K`` of the view (default: the fit's).  The vertices of ``predict`` are drawn
        by ``mhhip.view.render_view`` into one z-buffer with the scene (``scene=True`` and there is one: the depth map and
        mask ``fit_report`` uses -- the last ``update_scene_pointcloud`` / scene update, else ``scene_depth`` with
        ``scene_mask``): its masked pixels unprojected under the fit camera (pixel centres at +0.5), coloured by ``scene_img``
        (mid-grey without one), every point ``splat`` * depth / fx metres wide, so that a depth pixel keeps its metric
        footprint.  Returns numpy arrays -- image, depth, label (person, -2 = scene, -1 = empty), face, coverage (people,
        then the scene) -- plus ``'frames'``.  ``kw`` goes to ``mhhip.view.render_view`` (palette, light, ambient, background,
        near, max_half, outputs, chunk).  Reads the leaves only: buffers of its own, nothing of the engine's state is written."""
        from mhhip import view as mhview
        idx, chunk = self._diag_frames('render_view', 'render from', frames, kw.pop('chunk', 32))
        size = (self.img_w, self.img_h) if image_size is None else (int(image_size[0]), int(image_size[1]))
        K = self.cam_K if K is None else K
        R, t = mhview._views(view, len(idx))
        cloud = rgb = extent = None
        found = getattr(self, '_report_scene', None)
        if found is None and self.scene_depth is not None and getattr(self, 'scene_mask', None) is not None:
            found = (self.scene_depth, self.scene_mask)
        if scene and found is not None:
            img = getattr(self, 'scene_img', None)
            if img is not None:
                img = np.asarray(img)
                img = (img if img.dtype == np.uint8 else np.clip(np.rint(img), 0, 255).astype(np.uint8)).reshape(self.img_h, self.img_w, 3)
            cloud, rgb, extent, _ = mhview.cloud_from_depth(np.asarray(found[0], np.float32).reshape(self.img_h, self.img_w),
                                                            np.asarray(found[1]).reshape(self.img_h, self.img_w), self.cam_K, img, splat)
            if len(cloud) == 0:
                cloud = rgb = extent = None
        if cloud is not None:
            cloud, rgb, extent = (torch.as_tensor(a).to(self.device) for a in (cloud, rgb, extent))
        return self._diag_chunks(idx, chunk, lambda sl, verts: mhview.render_view(
            self.SMPLPY.body_model, verts, (R[sl], t[sl]), K, size, cloud=cloud, cloud_rgb=rgb, cloud_size_m=extent,
            chunk=chunk, **kw))

    # -- the fit in numbers (the reference has scatter plots to look at, predict.py:141-257) -----------------------------
    def fit_report(self, frames=None, margin=0.05, chunk=32):
        """Per frame and per person, how well the current leaves fit at ``frames`` (default: all): dict of numpy arrays of
        shape (len(frames), N) -- the columns of ``mhhip.report.fit_report`` (reproj_px, reproj_max_px, joints_used,
        mask_rendered, mask_seg, mask_inter, mask_iou, depth_bias_m, depth_abs_m, behind_scene_px, pen_verts, pen_max_m,
        contact_dy_m, foot_slide_m) and ``valid`` (``valid_smpl`` of the inputs, thresholded as the fit does) -- plus
        ``'frames'``.  The scene is the depth map and mask the last ``update_scene_pointcloud`` was handed or the last fit's
        scene update left (``scene_depth`` with the mask of its point cloud; else ``scene_depth`` / ``scene_mask``) with the
        cloud ``scene_pcd``; without one the scene columns are -1 (counts) / NaN.  Without staged images (no fit yet, or a
        dataloader without masks and depths) the mask and depth columns are -1 / NaN.  ``min_z`` / ``max_z`` are those of
        ``get_optimized_variables``; ``foot_slide_m`` pairs frame t with frame t - 1 of the SEQUENCE (NaN for frame 0), whose
        forward is computed when it is not among ``frames``.  At most ``chunk`` frames are on the device at a time.  Reads
        the leaves only: buffers and rasteriser workspace of its own, nothing of the engine's state is written."""
        from mhhip import report
        idx, chunk = self._diag_frames('fit_report', 'report on', frames, chunk)
        e = self.engine
        T, N = self.num_frames, self.num_people
        H, W = self.img_h, self.img_w
        scene = getattr(self, '_report_scene', None)
        if scene is None and self.scene_depth is not None and getattr(self, 'scene_mask', None) is not None:
            scene = (self.scene_depth, self.scene_mask)
        cloud = None if scene is None or self.scene_pcd is None else self.scene_pcd.view(-1, 3)
        staged = bool(getattr(self, '_staged', False))
        imgs = staged and e.has_images
        g = self.get_optimized_variables()
        min_z, max_z = g['min_z'].reshape(T).astype(np.float32), g['max_z'].reshape(T).astype(np.float32)
        pose2d = e.pose2d.view(T, N, 17, 3) if staged else torch.as_tensor(self._pose2d_init).to(self.device)
        m = self.SMPLPY.body_model

        def report_chunk(sl, verts, prev):
            fr = idx[sl]
            cur = torch.as_tensor(fr, device=self.device)
            joints = m.joints_regress(self._joints_reg[0], verts.view(len(fr) * N, -1, 3),
                                      corr=e.leaf('poses_T').view(T, N, 3)[cur].reshape(len(fr) * N, 3), root=self._joints_reg[1])
            return report.fit_report(
                m, verts, self.cam_K, (W, H), bits=e.bits[cur] if imgs else None, disp=e.depths[cur] if imgs else None,
                min_z=min_z[fr] if imgs else None, max_z=max_z[fr] if imgs else None,
                scene_depth=None if scene is None else np.asarray(scene[0], np.float32),
                scene_mask=None if scene is None else np.asarray(scene[1]) != 0, scene_points=cloud,
                joints=joints.view(len(fr), N, 17, 3), pose2d=pose2d[cur], cam_dist_coef=self.cam_dist_coef,
                joint_confidence_thr=self.joint_confidence_thr, verts_prev=prev, has_prev=fr > 0, margin=margin, chunk=chunk)

        out = self._diag_chunks(idx, chunk, report_chunk, prev=True)
        out['valid'] = self._valid.reshape(T, N)[idx].copy()
        out['frames'] = out.pop('frames')          # stays the last key
        return out

    # -- who stands in front of whom, against the instance masks ----------------------------------------------------------
    def order_report(self, frames=None, margin=None, delta=None, chunk=32):
        """Per frame and per person, where the current leaves put somebody in front of the person the instance masks show
        at ``frames`` (default: all): dict of numpy arrays -- the columns of ``mhhip.order.order_terms``, ``order_px``
        (len(frames), N) violating (pixel, other person) pairs the person owns, ``order_pairs`` (len(frames), N, N) the same by
        the other person, ``order_loss`` (len(frames), N) the term's value at coefficient 1 -- plus ``'frames'``.  The masks
        and the gate are the staged ones (a fit, or ``_stage_from_dataloader``, must have run); ``margin`` / ``delta`` default
        to the optimiser's ``order_margin`` / ``order_delta``.  Reads the leaves only, on a rasteriser workspace of its own."""
        from mhhip import order

        def staged_masks():
            if not (bool(getattr(self, '_staged', False)) and self.engine.has_images):
                raise RuntimeError('order_report needs the staged instance masks: run fit() (or stage a dataloader with masks) first')

        idx, chunk = self._diag_frames('order_report', 'report on', frames, chunk, need=staged_masks)
        e = self.engine
        margin = self.order_margin if margin is None else float(margin)
        delta = self.order_delta if delta is None else float(delta)
        gate = (e.p2d_valid * e.mask_valid).view(self.num_frames, self.num_people)

        def order_chunk(sl, verts):
            cur = torch.as_tensor(idx[sl], device=self.device)
            return order.order_terms(self.SMPLPY.body_model, verts, self.cam_K, (self.img_w, self.img_h), e.bits[cur], e.ebits[cur],
                                     gate=gate[cur], margin=margin, delta=delta, chunk=chunk)

        return self._diag_chunks(idx, chunk, order_chunk)

    # -- which part of a body touches the scene (the reference has its interactive viewer to look at) ----------------------
    def contact_map(self, frames=None, radius=0.1, contact=0.03, nearest=False, chunk=32):
        """Per vertex, how far the current leaves put every body from the scene at ``frames`` (default: all): dict of numpy
        arrays -- the columns of ``mhhip.contact.contact_map``, ``dist_m`` (len(frames), N, V) distance to the nearest point of
        the scene cloud ``scene_pcd`` within ``radius`` (inf beyond it), ``contact`` the same thresholded at ``contact``,
        ``part_verts`` / ``part_min_m`` (len(frames), N, 24) vertices in contact and smallest distance per body part
        (``mhhip.contact.PART_NAMES``), ``contact_verts`` (len(frames), N), with ``nearest=True`` also ``nearest``
        (len(frames), N, V, 3) the scene points themselves -- plus ``'frames'``.  The vertices are those of ``predict``; at
        most ``chunk`` frames are on the device at a time.  Reads the leaves only: a grid and buffers of its own, nothing of
        the engine's state is written."""
        from mhhip import contact as mhcontact

        def a_scene():
            if self.scene_pcd is None or int(self.scene_pcd.numel()) == 0:
                raise RuntimeError('contact_map needs a scene: hand one in with update_scene_pointcloud(scene_depth, scene_mask), or '
                                   "run fit() with scene_update='device' for more than 30 cycles")

        idx, chunk = self._diag_frames('contact_map', 'measure on', frames, chunk, need=a_scene)
        cloud = self.scene_pcd.view(-1, 3)
        return self._diag_chunks(idx, chunk, lambda sl, verts: mhcontact.contact_map(
            self.SMPLPY.body_model, verts, cloud, radius=radius, contact=contact, nearest=nearest, chunk=chunk))

    # -- which people touch, where and with which parts (again the reference has its viewer only) --------------------------
    def proximity_map(self, frames=None, radius=0.1, contact=0.02, nearest=False, chunk=8):
        """Per vertex, how far the current leaves put every body from the OTHER people of its frame at ``frames`` (default:
        all): dict of numpy arrays -- the columns of ``mhhip.proximity.proximity_map``: ``dist_m`` (len(frames), N, V) distance
        to the nearest vertex of another person within ``radius`` (inf beyond it), ``contact`` the same thresholded at
        ``contact``, ``behind`` the local side test against that vertex's normal, ``other`` the other person, the per-pair
        tables ``pair_verts`` / ``pair_behind`` / ``pair_min_m`` (len(frames), N, N), the per-part tables ``part_verts`` /
        ``part_min_m`` / ``part_other`` / ``part_other_part`` (len(frames), N, 24), ``contact_verts`` / ``behind_verts``
        (len(frames), N), with ``nearest=True`` also ``other_vert`` and ``nearest`` -- plus ``'frames'``.  The vertices are
        those of ``predict``; a person counts where the fit's thresholded ``valid_smpl`` says it is there; at most ``chunk``
        frames are on the device at a time.  Needs no scene and no staged images.  Reads the leaves only: a workspace and
        buffers of its own, nothing of the engine's state is written."""
        from mhhip import proximity as mhprox
        idx, chunk = self._diag_frames('proximity_map', 'measure on', frames, chunk)
        live = self._valid.reshape(self.num_frames, self.num_people) > 0
        return self._diag_chunks(idx, chunk, lambda sl, verts: mhprox.proximity_map(
            self.SMPLPY.body_model, verts, live=live[idx[sl]], radius=radius, contact=contact, nearest=nearest, chunk=chunk))

    # -- is one body inside another (the reference has a nearest-face-normal heuristic, unused) -------------------------------
    def penetration_map(self, frames=None, chunk=8):
        """Per vertex, which OTHER people of its frame the current leaves put it inside at ``frames`` (default: all), by the
        exact winding-number test: dict of numpy arrays -- the columns of ``mhhip.inside.penetration_map``: ``inside``
        (len(frames), N, V) bool, ``mask`` the containing bodies as bits, ``depth_z_m`` how far along the camera axis the vertex
        is from leaving the body it is deepest in (inf outside), ``other`` that body, the per-pair tables ``pair_verts`` /
        ``pair_depth_z_m`` (len(frames), N, N), the per-part tables ``part_verts`` / ``part_depth_z_m`` (len(frames), N, 24),
        ``inside_verts`` and ``status`` (len(frames), N) -- plus ``'frames'``.  The vertices are those of ``predict``; a person
        counts where the fit's thresholded ``valid_smpl`` says it is there; at most ``chunk`` frames are on the device at a time.
        Needs no scene and no staged images.  Reads the leaves only: a workspace and buffers of its own, nothing of the
        engine's state is written."""
        from mhhip import inside as mhinside
        idx, chunk = self._diag_frames('penetration_map', 'measure on', frames, chunk)
        live = self._valid.reshape(self.num_frames, self.num_people) > 0
        return self._diag_chunks(idx, chunk, lambda sl, verts: mhinside.penetration_map(
            self.SMPLPY.body_model, verts, live=live[idx[sl]], chunk=chunk))

    # -- how deep along the shortest way out, and how much room between bodies that do not overlap -------------------------------
    def clearance_map(self, frames=None, radius=0.1, contact=0.02, nearest=False, chunk=8):
        """Per vertex, the signed distance the current leaves put between it and the SURFACE of the other people of its frame
        at ``frames`` (default: all): dict of numpy arrays -- the columns of ``mhhip.surface.clearance_map``: ``signed_m``
        (len(frames), N, V) minus the distance to the surface of the body the vertex is deepest in where the exact inside
        test says it is inside one, else ``dist_m``, the distance to the nearest surface within ``radius`` (inf beyond it);
        ``depth_m``; ``other`` and ``face`` that decide ``signed_m``; ``inside`` and ``mask`` as ``penetration_map`` gives them;
        the per-pair tables ``pair_depth_m`` / ``pair_min_dist_m`` / ``pair_contact_verts`` (len(frames), N, N), the per-part
        tables ``part_depth_m`` / ``part_min_dist_m`` / ``part_contact_verts`` (len(frames), N, 24), ``status``
        (len(frames), N), with ``nearest=True`` also ``point`` (len(frames), N, V, 3), the closest surface point: the way out
        or the way to contact -- plus ``'frames'``.  The vertices are those of ``predict``; a person counts where the fit's
        thresholded ``valid_smpl`` says it is there; at most ``chunk`` frames are on the device at a time.  Needs no scene and
        no staged images.  Reads the leaves only: workspaces and buffers of its own, nothing of the engine's state is
        written."""
        from mhhip import surface as mhsurface
        idx, chunk = self._diag_frames('clearance_map', 'measure on', frames, chunk)
        live = self._valid.reshape(self.num_frames, self.num_people) > 0
        return self._diag_chunks(idx, chunk, lambda sl, verts: mhsurface.clearance_map(
            self.SMPLPY.body_model, verts, live=live[idx[sl]], radius=radius, contact=contact, nearest=nearest, chunk=chunk))

    # -- reference optimizer.py:664-675 ---------------------------------------------------------------
    def one_euro_filter(self, x, min_cutoff=0.1, beta=0.02, frame_rate=25):
        x = torch.as_tensor(x).detach().to(self.device).float()
        return engine.one_euro_scan(x, min_cutoff, beta, frame_rate)

    # -- reference optimizer.py:639-661 (not called by any shipped entry point) ------------------------
    def get_filtered_vertices_by_smpl(self, min_cutoff_T=0.004, min_cutoff_angles=0.1, beta_T=0.7, beta_angles=0.1,
                                      frame_rate=25):
        from .one_euro_filter import OneEuroFilter
        poses_T = self.poses_T.cpu().numpy().copy()
        pose = self.poses_smpl.cpu().numpy().copy()
        fT = OneEuroFilter(0, poses_T[0], dx0=0 * poses_T[0], min_cutoff=min_cutoff_T, beta=beta_T, d_cutoff=1.0)
        fP = OneEuroFilter(0, pose[0], dx0=0 * pose[0], min_cutoff=min_cutoff_angles, beta=beta_angles, d_cutoff=1.0)
        for i in range(1, len(pose)):
            poses_T[i] = fT(i / frame_rate, poses_T[i])
            pose[i] = fP(i / frame_rate, pose[i])
        T, N = self.num_frames, self.num_people
        m = self.SMPLPY.body_model
        verts, _, _, _ = m.lbs_forward(self.engine.leaf('betas'), torch.tensor(pose, device=self.device).view(-1, 72),
                                       self.engine.leaf('xscale'), torch.tensor(poses_T, device=self.device).view(-1, 3),
                                       want_vposed=False)
        return verts.view(T, N, -1, 3)
