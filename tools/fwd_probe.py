"""developer tool (GPU box): stand-alone time of the "LBS + projection" forward at C3 (k_pose_fwd + the skinning kernel, eager
launches with events around them) for each form of the kernel: mh_lbs_set_forward_pipeline 0 (tile after tile) / 1 (software
pipeline over a wave's tiles).  python tools/fwd_probe.py [modes]"""
import os, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd')]
import bench
from mhhip import synthetic, synthetic_seq, _lib

T = 200
struct = synthetic.make_smpl_struct(1); regs = synthetic.make_extra_regressors(1, struct)
K = synthetic.default_cam_K(bench.IMG, 60.0)
opt = bench.build_optimizer(struct, regs, tempfile.mkdtemp(), T, 'cuda:0', K)
seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, 4, T, bench.IMG, 1003, cam_K=K)
dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=10, shuffle=False)
opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=100)
opt._stage_from_dataloader(dl)
e = opt.engine
raster = e.raster_terms()
for c in range(3):
    e.cycle(0, raster=raster); e.step(0.01)
L = _lib.lib()


def timed(n=40):
    for _ in range(5):
        e.forward(regress=False, raster=raster)
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); e.forward(regress=False, raster=raster); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


modes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else '0,1').split(',')]
for m in modes:
    _lib.check(L.mh_lbs_set_forward_pipeline(m))
    med, mn = timed()
    print('pipe %d: forward (pose + skinning) median %.1f us, min %.1f us' % (m, med, mn), flush=True)
