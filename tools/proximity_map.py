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

import numpy as np

import map_common as mc                                    # (puts the packages on sys.path)


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
    mc.add_arguments(ap, chunk=8)
    ap.add_argument('--radius', type=float, default=0.1)
    ap.add_argument('--contact', type=float, default=0.02)
    ap.add_argument('--out', default='proximity_out')
    a = ap.parse_args()
    import torch
    from contact_map import colours, write_ply
    from mhhip import contact, proximity
    opt, seq, _ = mc.setup(a)
    mc.fit(opt, seq, a)
    T, N = a.frames, a.people
    e, m = opt.engine, opt.SMPLPY.body_model
    if a.together is not None:
        mc.slide_together(opt, a.together)
    got, wall = mc.wall_times(lambda: opt.proximity_map(radius=a.radius, contact=a.contact, chunk=a.chunk), a.repeat)
    # the module alone on the whole sequence's vertices, outputs left on the device: between device events
    live = torch.as_tensor(opt._valid.reshape(T, N) > 0, device=e.dev)
    verts = mc.forward_all(opt)
    # (the first call builds the model's tables: not reported)
    module_ms = [mc.timed(lambda: proximity.proximity_map(m, verts, live=live, radius=a.radius, contact=a.contact, chunk=a.chunk))
                 for _ in range(max(1, a.repeat) + 1)]
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
            write_ply(os.path.join(a.out, 'proximity_%04d.ply' % fr), mc.forward(opt, [int(fr)])[0].cpu().numpy(), faces, rgb[i])
    print(json.dumps(dict(frames=T, people=N, radius=a.radius, contact=a.contact, chunk=a.chunk, together=a.together,
                          contact_verts=int(got['contact_verts'].sum()), behind_verts=int(got['behind_verts'].sum()),
                          in_reach_verts=int(np.isfinite(got['dist_m']).sum()), box_rejected_share=round(share, 4),
                          proximity_map_wall_s=[round(x, 4) for x in wall], module_ms=[round(x, 3) for x in module_ms[1:]])))


if __name__ == '__main__':
    main()
