"""Fit a synthetic sequence (or a pickle of inputs) and write the per-frame, per-person fit report as CSV plus a JSON summary
(developer tool): ``SMPLDepthSequenceOptimizer.fit_report`` in place of paging through images.

  python tools/fit_report.py --out report_out                              # 2 people x 8 frames, 240x135, 40 cycles
  python tools/fit_report.py --people 4 --frames 200 --cycles 0 --repeat 3 # the C3 shape: the cost of the report
  python tools/fit_report.py --inputs seq.pkl                              # a pickled dict with the keys of
        # mhhip.synthetic_seq.make_sequence (pose2d, poses_smpl, betas_smpl, valid_smpl, seg_mask, depths, images, backmasks,
        # optional cam_K, scene_depth, scene_mask); the body model is the synthetic one

Writes <out>/fit_report.csv (one row per frame and person) and <out>/fit_report.json: per person the median and the worst frame
of every column, the ten worst (frame, person) pairs by mask_iou and by pen_max_m, and the wall time of the report beside that
of the render_scene(outputs=('person', 'depth')) it contains.  Prints the JSON's timing part as one line.
"""
import argparse
import csv
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

# columns where a LOW value is the bad one; for every other column the worst frame is the one with the largest value
LOW_IS_BAD = ('mask_iou', 'contact_dy_m', 'joints_used', 'mask_inter', 'valid')


def summarise(rep):
    """per person the median and worst frame of every column, and the ten worst pairs by mask_iou and pen_max_m"""
    frames = rep['frames']
    cols = [k for k in rep if k != 'frames']
    N = rep[cols[0]].shape[1]
    people = []
    for n in range(N):
        row = {}
        for k in cols:
            v = rep[k][:, n].astype(np.float64)
            ok = np.isfinite(v) & (v != -1 if np.issubdtype(rep[k].dtype, np.integer) else True)
            if not ok.any():
                row[k] = None
                continue
            key = np.where(ok, np.abs(v) if k == 'depth_bias_m' else v, np.inf if k in LOW_IS_BAD else -np.inf)
            w = int(np.argmin(key) if k in LOW_IS_BAD else np.argmax(key))
            row[k] = dict(median=float(np.median(v[ok])), worst=float(v[w]), worst_frame=int(frames[w]))
        people.append(row)

    def ten(k, low):
        v = rep[k].astype(np.float64)
        key = np.where(np.isfinite(v), v if low else -v, np.inf).reshape(-1)
        order = [i for i in np.argsort(key, kind='stable')[:10] if np.isfinite(key[i])]
        return [dict(frame=int(frames[i // N]), person=int(i % N), value=float(v.reshape(-1)[i])) for i in order]

    return dict(people=people, worst_mask_iou=ten('mask_iou', True), worst_pen_max_m=ten('pen_max_m', False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--people', type=int, default=2)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(240, 135), metavar=('W', 'H'))
    ap.add_argument('--cycles', type=int, default=40, help='fit cycles before the report (0: the initial variables)')
    ap.add_argument('--init-iter', type=int, default=30)
    ap.add_argument('--inputs', default=None, help='pickle of inputs instead of the synthetic sequence')
    ap.add_argument('--floor', type=float, default=1.15, help='synthetic sequence: height of the injected floor below the camera '
                    'axis in metres (0: no scene)')
    ap.add_argument('--margin', type=float, default=0.05)
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--repeat', type=int, default=1, help='report calls (the last one is written, all are timed)')
    ap.add_argument('--out', default='report_out')
    ap.add_argument('--seed', type=int, default=5)
    a = ap.parse_args()
    import torch
    from mhhip import build, synthetic, synthetic_seq
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    build.build()
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    tmp = tempfile.mkdtemp()
    for k, fn in [('extra9', 'J_regressor_extra.npy'), ('h36m', 'J_regressor_h36m.npy'),
                  ('alphapose', 'SMPL_AlphaPose_Regressor_RMSprop_6.npy')]:
        np.save(os.path.join(tmp, fn), regs[k])
    seq = None
    if a.inputs:
        with open(a.inputs, 'rb') as f:
            seq = pickle.load(f)
        T, N = seq['pose2d'].shape[:2]
        H, W = seq['depths'].shape[-2:]
    else:
        (W, H), T, N = a.size, a.frames, a.people
    K = np.asarray(seq['cam_K'], np.float32) if seq is not None and 'cam_K' in seq else synthetic.default_cam_K((W, H), 60.0)
    opt = SMPLDepthSequenceOptimizer(
        image_size=(W, H), num_frames=T, cam_K=K, device='cuda:0', smpl_model_parameters_path=tmp, smpl_data_struct=struct,
        scene_update='none', proj2d_loss_coef=1.0, depth_loss_coef=0.05, silhouette_loss_coef=0.1, reg_velocity_coef=0.05,
        reg_verts_filter_coef=0.002, reg_poses_coef=0.002, reg_scales_coef=1e-4, reg_contact_coef=0.001, reg_foot_sliding_coef=0.01)
    if seq is None:
        seq = synthetic_seq.make_sequence(opt.SMPLPY.body_model, N, T, (W, H), a.seed, cam_K=K)
        if a.floor > 0:
            ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
            depth = np.minimum(np.where(ys[:, None] > 1e-3, a.floor / np.maximum(ys[:, None], 1e-3), 10.0), 10.0)
            seq['scene_depth'] = np.tile(depth, (1, W)).astype(np.float32)
            seq['scene_mask'] = np.tile(ys[:, None] > 1e-3, (1, W))
    opt.init_optimized_variables(seq['pose2d'], seq['poses_smpl'], seq['betas_smpl'], seq['valid_smpl'], num_iter=a.init_iter)
    if seq.get('scene_depth') is not None:
        opt.update_scene_pointcloud(seq['scene_depth'], seq['scene_mask'])
    dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=min(10, T), shuffle=False)
    if a.cycles > 0:
        opt.fit(dl, num_iter=a.cycles)
    else:
        opt._stage_from_dataloader(dl)
    wall, wall_render = [], []
    for _ in range(max(1, a.repeat)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = opt.fit_report(margin=a.margin, chunk=a.chunk)
        wall.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        opt.render_scene(outputs=('person', 'depth'), chunk=a.chunk)
        wall_render.append(time.perf_counter() - t0)
    os.makedirs(a.out, exist_ok=True)
    cols = [k for k in rep if k != 'frames']
    with open(os.path.join(a.out, 'fit_report.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person'] + cols)
        for i, fr in enumerate(rep['frames']):
            for n in range(N):
                w.writerow([int(fr), n] + [repr(rep[k][i, n].item()) for k in cols])
    timing = dict(frames=T, people=N, image=[W, H], cycles=a.cycles, chunk=a.chunk, fit_report_wall_s=[round(x, 4) for x in wall],
                  render_scene_person_depth_wall_s=[round(x, 4) for x in wall_render])
    with open(os.path.join(a.out, 'fit_report.json'), 'w') as f:
        json.dump(dict(timing, **summarise(rep)), f, indent=1)
    print(json.dumps(timing))


if __name__ == '__main__':
    main()
