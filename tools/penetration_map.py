"""Fit a synthetic sequence and write which people are inside each other, with which body parts and how deep (developer
tool): ``SMPLDepthSequenceOptimizer.penetration_map`` as tables, and optionally as coloured meshes to look at.

  python tools/penetration_map.py --out penetration_out --together 0.2     # 2 people x 8 frames, 240x135, 40 cycles
  python tools/penetration_map.py --people 4 --frames 200 --cycles 0 --repeat 3 --together 0.3 --all-faces
  python tools/penetration_map.py --ply --together 0.2                      # + one ASCII PLY per frame

Writes <out>/penetration_pairs.csv: one row per frame, person and other person with the number of the person's vertices
inside the other's body and the largest distance along z (the camera axis) such a vertex is from leaving it;
<out>/penetration_parts.csv: one row per frame, person and body part (``mhhip.contact.PART_NAMES``) that has a vertex inside
anybody; <out>/penetration_frames.csv: per frame and person the vertices inside anybody and the body's status word.
``--together D`` first slides everybody along x until neighbouring people's centres are D metres apart (the synthetic people
stand metres apart; the translation leaf is edited), so that there is something to see.  With ``--ply``,
<out>/penetration_<frame>.ply holds the vertices and faces of all bodies of the frame: red where a vertex is inside another
body (darker the shallower), grey elsewhere.  Prints one JSON line: the wall time of the calls; between device events the time
of ``mhhip.inside.penetration_map`` alone on the sequence's vertices and, summed over its chunks, of ``mh_mesh_bins`` and of
``mh_person_inside``; the share of (vertex, other body) pairs that end at the box test; over ``--stat-frames`` frames the mean
number of faces a surviving pair looks at; the share of bodies that walk all faces; and with ``--all-faces`` the same times
with every body forced onto that path.
"""
import argparse
import csv
import json
import os

import numpy as np

import map_common as mc                                    # (puts the packages on sys.path)


def lattice(verts):
    import torch
    return torch.round(verts.double() * 65536.0).to(torch.int64)               # (half to even, as the kernel)


def box_share(X, live):
    """share of the (vertex of a live person, other person) pairs whose vertex lies outside the other's lattice box (a dead
    other counts: its header ends the visit just the same) -- what ``k_person_inside`` drops after reading a header.
    X (T,N,V,3) lattice, live (T,N) bool, both on the device; also the mask (T,n,m,V) of the pairs that survive"""
    import torch
    T, N, V = X.shape[:3]
    mn, mx = X.amin(2), X.amax(2)                                                # (T,N,3)
    out = ((X[:, :, None] < mn[:, None, :, None]) | (X[:, :, None] > mx[:, None, :, None])).any(-1)             # (T,n,m,V)
    out = out | ~live[:, None, :, None]
    pairs = live[:, :, None, None] & ~torch.eye(N, dtype=torch.bool, device=X.device)[None, :, :, None]
    return float((out & pairs).sum()) / max(1, int(pairs.sum()) * V), pairs & ~out


def faces_per_pair(X, faces, survive):
    """mean length of the cell list a surviving (vertex, other body) pair walks, by the grid rule of include/mhmocap_hip.h
    evaluated on the host: X (T,N,V,3) lattice, faces (F,3), survive (T,n,m,V) bool, numpy.  (0, 0) without such a pair."""
    T, N, V = X.shape[:3]
    F = faces.shape[0]
    total = pairs = 0
    for t in range(T):
        for m in range(N):
            q = survive[t, :, m]                                                  # (n,V)
            if not q.any():
                continue
            B = X[t, m]
            mn, ext = B.min(0), B.max(0) - B.min(0)
            s = 0
            while True:
                dx, dy = (int(ext[0]) >> s) + 1, (int(ext[1]) >> s) + 1
                if dx <= 64 and dy <= 64 and dx * dy <= max(F // 4, 256):
                    break
                s += 1
            P = (B[faces][:, :, :2] - mn[:2]) >> s                                # (F,3,2) cells of the corners
            lo, hi = P.min(1), P.max(1)
            counts = np.zeros((dy, dx), np.int64)
            for ox in range(int((hi[:, 0] - lo[:, 0]).max()) + 1):
                for oy in range(int((hi[:, 1] - lo[:, 1]).max()) + 1):
                    ok = (lo[:, 0] + ox <= hi[:, 0]) & (lo[:, 1] + oy <= hi[:, 1])
                    np.add.at(counts, (lo[ok, 1] + oy, lo[ok, 0] + ox), 1)
            c = (X[t][q][:, :2] - mn[:2]) >> s
            total += int(counts[c[:, 1], c[:, 0]].sum())
            pairs += int(q.sum())
    return total, pairs


def main():
    ap = argparse.ArgumentParser()
    mc.add_arguments(ap, chunk=8)
    ap.add_argument('--all-faces', action='store_true', help='time the module once more with every body walking all faces')
    ap.add_argument('--stat-frames', type=int, default=8, help='frames (evenly spread) the faces-per-pair figure is taken over')
    ap.add_argument('--out', default='penetration_out')
    a = ap.parse_args()
    import torch
    from contact_map import write_ply
    from mhhip import _lib, bodies, contact, inside
    opt, seq, _ = mc.setup(a)
    mc.fit(opt, seq, a)
    T, N = a.frames, a.people
    e, m = opt.engine, opt.SMPLPY.body_model
    if a.together is not None:
        mc.slide_together(opt, a.together)
    got, wall = mc.wall_times(lambda: opt.penetration_map(chunk=a.chunk), a.repeat)
    # the module alone on the whole sequence's vertices, outputs left on the device: between device events
    live = torch.as_tensor(opt._valid.reshape(T, N) > 0, device=e.dev)
    verts = mc.forward_all(opt).contiguous()
    V = int(verts.shape[2])

    timed = mc.timed

    def module_times(repeat):
        return [timed(lambda: inside.penetration_map(m, verts, live=live, chunk=a.chunk)) for _ in range(repeat + 1)][1:]

    def entry_times():
        """(mh_mesh_bins, mh_person_inside) in ms, each summed over the chunks of the sequence"""
        L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(e.dev)
        faces = bodies.faces(m, e.dev)
        F = int(faces.shape[0])
        part = torch.as_tensor(contact.body_parts(m)).to(e.dev)
        chunk = max(1, min(a.chunk, T))
        nbytes = L.mh_mesh_bins_bytes(chunk * N, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=e.dev)
        lv = live.to(torch.uint8).contiguous()
        o3 = [torch.empty(chunk, N, V, dtype=torch.int32, device=e.dev) for _ in range(3)]
        o2 = [torch.empty(chunk, N, N, dtype=torch.int32, device=e.dev) for _ in range(2)]
        op = [torch.empty(chunk, N, 24, dtype=torch.int32, device=e.dev) for _ in range(2)]
        status = torch.empty(chunk, N, dtype=torch.int32, device=e.dev)
        bins = query = 0.0
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nt = sl.stop - sl.start
            bins += timed(lambda: _lib.check(L.mh_mesh_bins(nt * N, V, F, ptr(verts[sl]), ptr(faces), ptr(lv[sl]), ptr(ws), nbytes,
                                                             ptr(status), st)))
            query += timed(lambda: _lib.check(L.mh_person_inside(nt, N, V, F, ptr(faces), ptr(ws), ptr(verts[sl]), ptr(part), 24,
                                                                 *[ptr(o) for o in o3 + o2 + op], st)))
        return bins, query

    module_ms = module_times(max(1, a.repeat))
    entry_times()                                           # (warm)
    bins_ms, query_ms = entry_times()
    forced = None
    if a.all_faces:
        was = inside.force_all_faces(True)
        try:
            forced_module = module_times(1)
            fb, fq = entry_times()
            forced = dict(module_ms=[round(x, 3) for x in forced_module], mesh_bins_ms=round(fb, 3), person_inside_ms=round(fq, 3))
        finally:
            inside.force_all_faces(was)
    X = lattice(verts)
    share, survive = box_share(X, live)
    pick = np.unique(np.linspace(0, T - 1, max(1, min(a.stat_frames, T))).astype(np.int64))
    tot, npairs = faces_per_pair(X[pick].cpu().numpy(), np.asarray(m.faces).astype(np.int64), survive[pick].cpu().numpy())
    del verts, X, survive
    os.makedirs(a.out, exist_ok=True)
    names = contact.PART_NAMES
    with open(os.path.join(a.out, 'penetration_pairs.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'other', 'inside_verts', 'max_depth_z_m'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                for o in range(N):
                    if o != n:
                        w.writerow([int(fr), n, o, int(got['pair_verts'][i, n, o]), repr(float(got['pair_depth_z_m'][i, n, o]))])
    with open(os.path.join(a.out, 'penetration_parts.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'part', 'inside_verts', 'max_depth_z_m'])
        for i, n, k in zip(*np.nonzero(got['part_verts'])):
            w.writerow([int(got['frames'][i]), n, names[k], int(got['part_verts'][i, n, k]), repr(float(got['part_depth_z_m'][i, n, k]))])
    with open(os.path.join(a.out, 'penetration_frames.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'inside_verts', 'status'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                w.writerow([int(fr), n, int(got['inside_verts'][i, n]), int(got['status'][i, n])])
    if a.ply:
        faces = np.asarray(m.faces).astype(np.int64)
        deep = np.where(got['inside'], got['depth_z_m'], 0.0)
        tone = 0.4 + 0.6 * deep / max(float(deep.max()), 1e-9)
        rgb = np.where(got['inside'][..., None], np.stack([255 * tone, 30 * tone, 30 * tone], -1), 128.0)
        rgb = np.rint(rgb).astype(np.uint8)
        for i, fr in enumerate(got['frames']):                  # the vertices the map was computed on, a frame at a time
            write_ply(os.path.join(a.out, 'penetration_%04d.ply' % fr), mc.forward(opt, [int(fr)])[0].cpu().numpy(), faces, rgb[i])
    testable = (got['status'] & 3) == 0
    print(json.dumps(dict(frames=T, people=N, chunk=a.chunk, together=a.together, inside_verts=int(got['inside_verts'].sum()),
                          max_depth_z_m=float(np.where(got['inside'], got['depth_z_m'], 0.0).max()),
                          box_rejected_share=round(share, 4), faces_per_surviving_pair=round(tot / max(1, npairs), 2),
                          surviving_pairs_sampled=npairs, all_faces_bodies_share=round(float(((got['status'] & 4) != 0).sum()) / max(1, int(testable.sum())), 4),
                          penetration_map_wall_s=[round(x, 4) for x in wall], module_ms=[round(x, 3) for x in module_ms],
                          mesh_bins_ms=round(bins_ms, 3), person_inside_ms=round(query_ms, 3), forced_all_faces=forced)))


if __name__ == '__main__':
    main()
