"""Fit a synthetic sequence and write which part of every body touches the scene (developer tool):
``SMPLDepthSequenceOptimizer.contact_map`` as a table, and optionally as coloured meshes to look at.

  python tools/contact_map.py --out contact_out                           # 2 people x 8 frames, 240x135, 40 cycles
  python tools/contact_map.py --people 4 --frames 200 --cycles 0 --repeat 3
  python tools/contact_map.py --ply --radius 0.3                          # + one ASCII PLY per frame

Writes <out>/contact_map.csv: one row per frame, person and body part (``mhhip.contact.PART_NAMES``) with the number of
vertices within ``--contact`` metres of the scene cloud and the part's smallest distance (inf beyond ``--radius``).  With
``--ply``, <out>/contact_<frame>.ply holds the vertices and faces of all bodies of the frame, coloured by distance: red in
contact, fading to blue at the radius, grey beyond it.  Prints the wall time of the calls as one JSON line.
"""
import argparse
import csv
import json
import os

import numpy as np

import map_common as mc                                    # (puts the packages on sys.path)


def colours(dist, contact, radius):
    """(..., V) distances -> (..., V, 3) uint8: red at <= contact, to blue at the radius, grey where there is no scene point"""
    t = np.clip((np.where(np.isfinite(dist), dist, radius) - contact) / max(radius - contact, 1e-9), 0.0, 1.0)
    rgb = np.stack([255 * (1 - t), 40 + 0 * t, 255 * t], -1)
    rgb[~np.isfinite(dist)] = 128
    return np.rint(rgb).astype(np.uint8)


def write_ply(path, verts, faces, rgb):
    """verts (N,V,3), faces (F,3), rgb (N,V,3) -> one ASCII PLY with the N bodies"""
    N, V = verts.shape[:2]
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
                'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n'
                'property list uchar int vertex_indices\nend_header\n' % (N * V, N * len(faces)))
        for p, c in zip(verts.reshape(-1, 3), rgb.reshape(-1, 3)):
            f.write('%.6f %.6f %.6f %d %d %d\n' % (p[0], p[1], p[2], c[0], c[1], c[2]))
        for n in range(N):
            for a, b, c in faces + n * V:
                f.write('3 %d %d %d\n' % (a, b, c))


def main():
    ap = argparse.ArgumentParser()
    mc.add_arguments(ap, chunk=32, together=False)
    ap.add_argument('--floor', type=float, default=1.15, help='height of the injected floor below the camera axis in metres')
    ap.add_argument('--radius', type=float, default=0.1)
    ap.add_argument('--contact', type=float, default=0.03)
    ap.add_argument('--out', default='contact_out')
    a = ap.parse_args()
    from mhhip import contact
    opt, seq, K = mc.setup(a)
    (W, H), T, N = a.size, a.frames, a.people
    ys = (np.arange(H, dtype=np.float32) + 0.5 - K[1, 2]) / K[1, 1]
    depth = np.minimum(np.where(ys[:, None] > 1e-3, a.floor / np.maximum(ys[:, None], 1e-3), 10.0), 10.0)
    opt.update_scene_pointcloud(np.tile(depth, (1, W)).astype(np.float32), np.tile(ys[:, None] > 1e-3, (1, W)))
    mc.fit(opt, seq, a)
    got, wall = mc.wall_times(lambda: opt.contact_map(radius=a.radius, contact=a.contact, chunk=a.chunk), a.repeat)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'contact_map.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'part', 'contact_verts', 'min_dist_m'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                for k, name in enumerate(contact.PART_NAMES):
                    w.writerow([int(fr), n, name, int(got['part_verts'][i, n, k]), repr(float(got['part_min_m'][i, n, k]))])
    if a.ply:
        faces = np.asarray(opt.SMPLPY.body_model.faces).astype(np.int64)
        rgb = colours(got['dist_m'], a.contact, a.radius)
        for i, fr in enumerate(got['frames']):                  # the vertices the map was computed on, a frame at a time
            write_ply(os.path.join(a.out, 'contact_%04d.ply' % fr), mc.forward(opt, [int(fr)])[0].cpu().numpy(), faces, rgb[i])
    print(json.dumps(dict(frames=T, people=N, image=[W, H], cloud_points=int(opt.scene_pcd.numel() // 3), radius=a.radius,
                          contact=a.contact, contact_verts=int(got['contact_verts'].sum()),
                          contact_map_wall_s=[round(x, 4) for x in wall])))


if __name__ == '__main__':
    main()
