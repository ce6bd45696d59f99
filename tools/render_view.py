"""Fit a synthetic sequence with a scene and write free-viewpoint renders of it as PNG (developer tool): what
``SMPLDepthSequenceOptimizer.render_view`` gives a user in place of the reference's interactive Open3D window
(mhmocap/visualization.py) -- the people ON the reconstructed scene, seen from the side, from above or on an orbit.

  python tools/render_view.py --out view_out                               # 2 people x 8 frames, 240x135: side and top views
  python tools/render_view.py --orbit 20 --png 8                           # one turn around the scene, 20 degrees up
  python tools/render_view.py --people 4 --frames 200 --cycles 0 --png 0 --time
        # the C3 shape, rendering only: milliseconds per frame of project, raster, splat and resolve

Prints one JSON line: frames, people, views, pixels of every person and of the scene (first frame), stage times with --time.
"""
import argparse
import json
import os
import sys
import tempfile

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
    ap.add_argument('--orbit', type=float, default=None, metavar='ELEVATION', help='one turn around the scene over the frames, degrees up')
    ap.add_argument('--top', action='store_true', help='from above')
    ap.add_argument('--side', action='store_true', help='from the right-hand side, 10 degrees up (with --top: both; neither: both)')
    ap.add_argument('--radius', type=float, default=4.0, help='distance of the camera from the centre of the people')
    ap.add_argument('--splat', type=float, default=1.5)
    ap.add_argument('--png', type=int, default=4, help='frames written as PNG per view (evenly spaced)')
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--time', action='store_true', help='milliseconds per frame of the four stages (second of two calls)')
    ap.add_argument('--out', default='view_out')
    ap.add_argument('--seed', type=int, default=5)
    a = ap.parse_args()
    import torch
    from mhhip import build, synthetic, synthetic_seq, view
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    build.build()
    W, H = a.size
    T, N = a.frames, a.people
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    tmp = tempfile.mkdtemp()
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'),
                  ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(os.path.join(tmp, fn), regs[k])
    K = synthetic.default_cam_K((W, H), 60.0)
    opt = SMPLDepthSequenceOptimizer(
        image_size=(W, H), num_frames=T, cam_K=K, device='cuda:0', smpl_model_parameters_path=tmp, smpl_data_struct=struct,
        scene_update='none', proj2d_loss_coef=1.0, depth_loss_coef=0.05, silhouette_loss_coef=0.1, reg_velocity_coef=0.05,
        reg_verts_filter_coef=0.002, reg_poses_coef=0.002, reg_scales_coef=1e-4, reg_contact_coef=0.001, reg_foot_sliding_coef=0.01)
    seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, N, T, (W, H), a.seed, cam_K=K)
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=a.init_iter)
    # the scene: a floor 1.15 m below the camera and a wall at 10 m, where no frame has a person
    ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
    scene_depth = np.tile(np.minimum(np.where(ys[:, None] > 1e-3, 1.15 / np.maximum(ys[:, None], 1e-3), 10.0), 10.0), (1, W)).astype(np.float32)
    opt.scene_depth = scene_depth
    opt.update_scene_pointcloud(scene_depth, seq['backmasks'].min(axis=0) > 0)
    dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=min(10, T), shuffle=False)
    if a.cycles > 0:
        opt.fit(dl, num_iter=a.cycles)
    centre = opt.poses_T.detach().cpu().numpy().reshape(-1, 3).mean(0)
    views = {}
    if a.orbit is not None:
        views['orbit'] = view.orbit(centre, a.radius, a.orbit, np.linspace(0.0, 360.0, T, endpoint=False))
    if a.top or (a.orbit is None and not a.side):
        views['top'] = view.top_down(centre, a.radius)
    if a.side or (a.orbit is None and not a.top):
        views['side'] = view.orbit(centre, a.radius, 10.0, 90.0)
    res = dict(frames=T, people=N, image=[W, H], cycles=a.cycles, chunk=a.chunk, views=sorted(views), png=[])
    for name, v in views.items():
        for _ in range(2 if a.time else 1):               # (the first call pays for allocations and code loading)
            timings = {} if a.time else None
            out = opt.render_view(v, splat=a.splat, chunk=a.chunk, timings=timings)
        res['coverage_frame0_' + name] = out['coverage'][0].tolist()
        if a.time:
            res['ms_per_frame_' + name] = {k: round(ms / T, 5) for k, ms in timings.items()}
        if a.png > 0:
            from PIL import Image
            os.makedirs(a.out, exist_ok=True)
            for f in sorted(set(np.linspace(0, T - 1, min(a.png, T)).astype(int).tolist())):
                path = os.path.join(a.out, '%s_%04d.png' % (name, f))
                Image.fromarray(out['image'][f]).save(path)
                res['png'].append(path)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
