"""What the map tools (contact_map.py, proximity_map.py, penetration_map.py, clearance_map.py) share: the synthetic sequence
and its optimiser, the vertices the maps are computed on, the ``--together`` slide, and the two ways they time a call."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def add_arguments(ap, chunk, together=True):
    """the arguments every map tool has"""
    ap.add_argument('--people', type=int, default=2)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(240, 135), metavar=('W', 'H'))
    ap.add_argument('--cycles', type=int, default=40, help='fit cycles before the map (0: the initial variables)')
    ap.add_argument('--init-iter', type=int, default=30)
    ap.add_argument('--chunk', type=int, default=chunk)
    if together:
        ap.add_argument('--together', type=float, default=None, metavar='D',
                        help="slide the people along x until neighbours' centres are D metres apart, at the depth of person 0")
    ap.add_argument('--repeat', type=int, default=1, help='calls (the last one is written, all are timed)')
    ap.add_argument('--ply', action='store_true', help='one coloured mesh per frame')
    ap.add_argument('--seed', type=int, default=5)


def setup(a):
    """the library built, an optimiser over a synthetic sequence of ``a.people`` x ``a.frames``, its variables initialised ->
    (opt, seq, K)"""
    from mhhip import build, synthetic, synthetic_seq
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    build.build()
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    tmp = tempfile.mkdtemp()
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'),
                  ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(os.path.join(tmp, fn), regs[k])
    (W, H), T, N = a.size, a.frames, a.people
    K = synthetic.default_cam_K((W, H), 60.0)
    opt = SMPLDepthSequenceOptimizer(
        image_size=(W, H), num_frames=T, cam_K=K, device='cuda:0', smpl_model_parameters_path=tmp, smpl_data_struct=struct,
        scene_update='none', proj2d_loss_coef=1.0, depth_loss_coef=0.05, silhouette_loss_coef=0.1, reg_velocity_coef=0.05,
        reg_verts_filter_coef=0.002, reg_poses_coef=0.002, reg_scales_coef=1e-4, reg_contact_coef=0.001, reg_foot_sliding_coef=0.01)
    seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, N, T, (W, H), a.seed, cam_K=K)
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=a.init_iter)
    return opt, seq, K


def fit(opt, seq, a):
    """``a.cycles`` cycles of the fit, if any"""
    import torch
    from mhhip import synthetic_seq
    if a.cycles > 0:
        dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=min(10, a.frames), shuffle=False)
        opt.fit(dl, num_iter=a.cycles)


def forward(opt, frames):
    """the vertices the map is computed on: (len(frames), N, V, 3) on the device"""
    import torch
    e, m = opt.engine, opt.SMPLPY.body_model
    T, N = opt.num_frames, opt.num_people
    fr = torch.as_tensor(list(frames), device=e.dev)
    nb = len(fr) * N
    verts, _, _, _ = m.lbs_forward(e.leaf('betas').view(N, 10), e.leaf('poses_smpl').view(T, N, 72)[fr].reshape(nb, 72),
                                   e.leaf('xscale').view(N), e.leaf('poses_T').view(T, N, 3)[fr].reshape(nb, 3), want_vposed=False)
    return verts.view(len(fr), N, -1, 3)


def forward_all(opt, of=lambda verts: verts):
    """``of(forward(...))`` of the whole sequence, 32 frames at a time: (T, N, ...)"""
    import torch
    T = opt.num_frames
    return torch.cat([of(forward(opt, range(t0, min(T, t0 + 32)))) for t0 in range(0, T, 32)])


def slide_together(opt, D):
    """``--together D``: the translation leaf edited so that neighbouring people's centres are D metres apart along x"""
    import torch
    e = opt.engine
    T, N = opt.num_frames, opt.num_people
    pT = e.leaf('poses_T').view(T, N, 3)
    centre = forward_all(opt, lambda verts: verts.mean(2))                        # (T,N,3)
    want = centre[:, :1] + torch.tensor([D, 0.0, 0.0], device=e.dev) * torch.arange(N, device=e.dev).view(1, N, 1)
    pT += want - centre


def wall_times(call, repeat):
    """``call()`` ``repeat`` times (at least once) -> (the last result, the wall time of each in seconds)"""
    import torch
    wall = []
    for _ in range(max(1, repeat)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        wall.append(time.perf_counter() - t0)
    return got, wall


def timed(fn):
    """``fn()`` between device events, in ms"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])
