"""Fit a synthetic sequence and write the shaded overlay of a few frames as PNG (developer tool): what
``SMPLDepthSequenceOptimizer.render_scene`` gives a user in place of the reference's scatter plots (predict.py:195-243).

  python tools/render_sequence.py --out render_out                         # 2 people x 8 frames, 240x135, 40 cycles
  python tools/render_sequence.py --people 4 --frames 200 --cycles 0 --repeat 3 --png 0
        # the C3 shape, rendering only: under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> --` this is
        # the measurement of DESIGN section 3 (k_scene_composite and the k_raster_strip launches in front of it)

Prints one JSON line: frames, people, pixels every person owns (first rendered frame), wall time of the render calls.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--people', type=int, default=2)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(240, 135), metavar=('W', 'H'))
    ap.add_argument('--cycles', type=int, default=40, help='fit cycles before rendering (0: the initial variables)')
    ap.add_argument('--init-iter', type=int, default=30)
    ap.add_argument('--png', type=int, default=4, help='frames written as PNG (evenly spaced)')
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--repeat', type=int, default=1, help='render calls (the last one is reported and written)')
    ap.add_argument('--out', default='render_out')
    ap.add_argument('--seed', type=int, default=5)
    a = ap.parse_args()
    import torch
    from mhhip import build, synthetic, synthetic_seq
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    build.build()
    W, H = a.size
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    tmp = tempfile.mkdtemp()
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'),
                  ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(os.path.join(tmp, fn), regs[k])
    K = synthetic.default_cam_K((W, H), 60.0)
    opt = SMPLDepthSequenceOptimizer(
        image_size=(W, H), num_frames=a.frames, cam_K=K, device='cuda:0', smpl_model_parameters_path=tmp, smpl_data_struct=struct,
        scene_update='none', proj2d_loss_coef=1.0, depth_loss_coef=0.05, silhouette_loss_coef=0.1, reg_velocity_coef=0.05,
        reg_verts_filter_coef=0.002, reg_poses_coef=0.002, reg_scales_coef=1e-4, reg_contact_coef=0.001, reg_foot_sliding_coef=0.01)
    seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, a.people, a.frames, (W, H), a.seed, cam_K=K)
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=a.init_iter)
    dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=min(10, a.frames), shuffle=False)
    if a.cycles > 0:
        opt.fit(dl, num_iter=a.cycles)
    else:
        opt._stage_from_dataloader(dl)           # the frames the overlay is drawn on
    wall = []
    for _ in range(max(1, a.repeat)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = opt.render_scene(light=(0.0, 0.0, 1.0), chunk=a.chunk)      # a head-light
        wall.append(time.perf_counter() - t0)
    written = []
    if a.png > 0:
        from PIL import Image
        os.makedirs(a.out, exist_ok=True)
        for f in sorted(set(np.linspace(0, a.frames - 1, min(a.png, a.frames)).astype(int).tolist())):
            path = os.path.join(a.out, 'overlay_%04d.png' % f)
            Image.fromarray(out['overlay'][f]).save(path)
            written.append(path)
    print(json.dumps(dict(frames=a.frames, people=a.people, image=[W, H], cycles=a.cycles, chunk=a.chunk,
                          coverage_frame0=out['coverage'][0].tolist(), covered_fraction=float((out['person'] >= 0).mean()),
                          render_scene_wall_s=[round(w, 4) for w in wall], png=written)))


if __name__ == '__main__':
    main()
