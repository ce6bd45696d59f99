"""Fit a synthetic sequence and write which people touch, where and with which body parts (developer tool):
``SMPLDepthSequenceOptimizer.proximity_map`` as a table, and optionally as coloured meshes to look at.

  python tools/proximity_map.py --out proximity_out                         # 2 people x 8 frames, 240x135, 40 cycles
  python tools/proximity_map.py --people 4 --frames 200 --cycles 0 --repeat 3
  python tools/proximity_map.py --ply --radius 0.3 --together 0.3           # + one ASCII PLY per frame

Writes <out>/proximity_map.csv: one row per frame, person and other person with the number of the person's vertices within
``--contact`` metres of the other, how many of those lie behind the other's surface (the local side test), the smallest
distance between the two (inf beyond ``--radius``) and the pair of body parts (``mhhip.contact.PART_NAMES``) that come
closest.  ``--together D`` first slides everybody along x until neighbouring people's centres are D metres apart (the synthetic
people stand metres apart; the translation leaf is edited), so that there is something to see.  With ``--ply``,
<out>/proximity_<frame>.ply holds the vertices and faces of all bodies of the frame, coloured by distance to the other people:
red in contact, fading to blue at the radius, grey beyond it.  Prints one JSON line: the wall time of the calls, the time of
``mhhip.proximity.proximity_map`` alone on the sequence's vertices between device events, and the share of (vertex, other
body) pairs that end at the bounding-box test.
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def box_share(verts, live, radius):
    """share of the (vertex of a live person, other person) pairs whose vertex lies outside the other's bounding box grown by
    the radius (a dead other counts: its header ends the visit just the same) -- what ``k_person_nearest`` drops after
    reading a header.  verts (T,N,V,3) finite, live (T,N) bool, both on the device."""
    import torch
    T, N, V = verts.shape[:3]
    mn, mx = verts.amin(2), verts.amax(2)                                        # (T,N,3)
    out = ((verts[:, :, None] + radius < mn[:, None, :, None]) | (verts[:, :, None] - radius > mx[:, None, :, None])).any(-1)   # (T,n,m,V)
    out = out | ~live[:, None, :, None]
    pairs = live[:, :, None, None] & ~torch.eye(N, dtype=torch.bool, device=verts.device)[None, :, :, None]
    return float((out & pairs).sum()) / max(1, int(pairs.sum()) * V)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--people', type=int, default=2)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(240, 135), metavar=('W', 'H'))
    ap.add_argument('--cycles', type=int, default=40, help='fit cycles before the map (0: the initial variables)')
    ap.add_argument('--init-iter', type=int, default=30)
    ap.add_argument('--radius', type=float, default=0.1)
    ap.add_argument('--contact', type=float, default=0.02)
    ap.add_argument('--chunk', type=int, default=8)
    ap.add_argument('--together', type=float, default=None, metavar='D',
                    help="slide the people along x until neighbours' centres are D metres apart, at the depth of person 0")
    ap.add_argument('--repeat', type=int, default=1, help='calls (the last one is written, all are timed)')
    ap.add_argument('--ply', action='store_true', help='one coloured mesh per frame')
    ap.add_argument('--out', default='proximity_out')
    ap.add_argument('--seed', type=int, default=5)
    a = ap.parse_args()
    import torch
    from contact_map import colours, write_ply
    from mhhip import build, contact, proximity, synthetic, synthetic_seq
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
    if a.cycles > 0:
        dl = torch.utils.data.DataLoader(synthetic_seq.SequenceDataset(seq), batch_size=min(10, T), shuffle=False)
        opt.fit(dl, num_iter=a.cycles)
    e, m = opt.engine, opt.SMPLPY.body_model

    def forward(frames):
        """the vertices the map is computed on: (len(frames), N, V, 3) on the device"""
        fr = torch.as_tensor(list(frames), device=e.dev)
        nb = len(fr) * N
        verts, _, _, _ = m.lbs_forward(e.leaf('betas').view(N, 10), e.leaf('poses_smpl').view(T, N, 72)[fr].reshape(nb, 72),
                                       e.leaf('xscale').view(N), e.leaf('poses_T').view(T, N, 3)[fr].reshape(nb, 3), want_vposed=False)
        return verts.view(len(fr), N, -1, 3)

    if a.together is not None:
        pT = e.leaf('poses_T').view(T, N, 3)
        centre = torch.cat([forward(range(t0, min(T, t0 + 32))).mean(2) for t0 in range(0, T, 32)])        # (T,N,3)
        want = centre[:, :1] + torch.tensor([a.together, 0.0, 0.0], device=e.dev) * torch.arange(N, device=e.dev).view(1, N, 1)
        pT += want - centre
    wall = []
    for _ in range(max(1, a.repeat)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = opt.proximity_map(radius=a.radius, contact=a.contact, chunk=a.chunk)
        wall.append(time.perf_counter() - t0)
    # the module alone on the whole sequence's vertices, outputs left on the device: between device events
    live = torch.as_tensor(opt._valid.reshape(T, N) > 0, device=e.dev)
    verts = torch.cat([forward(range(t0, min(T, t0 + 32))) for t0 in range(0, T, 32)])
    module_ms = []
    for _ in range(max(1, a.repeat) + 1):                   # (the first call builds the model's tables: not reported)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        proximity.proximity_map(m, verts, live=live, radius=a.radius, contact=a.contact, chunk=a.chunk)
        ev[1].record()
        torch.cuda.synchronize()
        module_ms.append(ev[0].elapsed_time(ev[1]))
    share = box_share(verts, live, a.radius)
    del verts
    os.makedirs(a.out, exist_ok=True)
    names = contact.PART_NAMES
    with open(os.path.join(a.out, 'proximity_map.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'other', 'contact_verts', 'behind_verts', 'min_dist_m', 'closest_part', 'closest_other_part'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                for o in range(N):
                    if o == n:
                        continue
                    # the part of n that comes closest to o, and the part of o it comes closest to
                    d = np.where(got['part_other'][i, n] == o, got['part_min_m'][i, n], np.inf)
                    k = int(d.argmin())
                    pair = (names[k], names[got['part_other_part'][i, n, k]]) if np.isfinite(d[k]) else ('', '')
                    w.writerow([int(fr), n, o, int(got['pair_verts'][i, n, o]), int(got['pair_behind'][i, n, o]),
                                repr(float(got['pair_min_m'][i, n, o])), pair[0], pair[1]])
    if a.ply:
        faces = np.asarray(m.faces).astype(np.int64)
        rgb = colours(got['dist_m'], a.contact, a.radius)
        for i, fr in enumerate(got['frames']):                  # the vertices the map was computed on, a frame at a time
            write_ply(os.path.join(a.out, 'proximity_%04d.ply' % fr), forward([int(fr)])[0].cpu().numpy(), faces, rgb[i])
    print(json.dumps(dict(frames=T, people=N, radius=a.radius, contact=a.contact, chunk=a.chunk, together=a.together,
                          contact_verts=int(got['contact_verts'].sum()), behind_verts=int(got['behind_verts'].sum()),
                          in_reach_verts=int(np.isfinite(got['dist_m']).sum()), box_rejected_share=round(share, 4),
                          proximity_map_wall_s=[round(x, 4) for x in wall], module_ms=[round(x, 3) for x in module_ms[1:]])))


if __name__ == '__main__':
    main()
