"""Fit a synthetic sequence and write how deep people are inside each other along the shortest way out, and how much room is
between those that do not overlap (developer tool): ``SMPLDepthSequenceOptimizer.clearance_map`` as tables, and optionally as
coloured meshes to look at.

  python tools/clearance_map.py --out clearance_out --together 0.2     # 2 people x 8 frames, 240x135, 40 cycles
  python tools/clearance_map.py --people 4 --frames 200 --cycles 0 --repeat 3 --together 0.3 --all-faces
  python tools/clearance_map.py --ply --together 0.2                    # + one ASCII PLY per frame

Writes <out>/clearance_pairs.csv: one row per frame, person and other person with the largest depth of the person's vertices
that are deepest in the other, the smallest distance of those whose nearest surface outside is the other's, and how many of
them are within ``--contact``; <out>/clearance_parts.csv: the same three per frame, person and body part
(``mhhip.contact.PART_NAMES``) that has anything to report; <out>/clearance_frames.csv: per frame and person the vertices
inside anybody, the deepest and the nearest vertex, and the body's status word.  ``--together D`` first slides everybody along
x until neighbouring people's centres are D metres apart (the synthetic people stand metres apart; the translation leaf is
edited), so that there is something to see.  With ``--ply``, <out>/clearance_<frame>.ply holds the vertices and faces of all
bodies of the frame coloured by ``signed_m``: red inside (darker the shallower), blue within the radius outside (lighter the
farther), grey beyond it.  Prints one JSON line: the wall time of the calls; between device events the time of
``mhhip.surface.clearance_map`` alone on the sequence's vertices and, summed over its chunks, of ``mh_surface_grid``, of
``mh_person_surface`` and of the inside test before them; the share of (vertex, other body) pairs that end at the box test;
the mean number of faces a surviving pair evaluates; the share of bodies that walk all faces; and with ``--all-faces`` the
same times with every body forced onto that path.
"""
import argparse
import csv
import json
import os

import numpy as np

import map_common as mc                                    # (puts the packages on sys.path)


def main():
    ap = argparse.ArgumentParser()
    mc.add_arguments(ap, chunk=8)
    ap.add_argument('--radius', type=float, default=0.1)
    ap.add_argument('--contact', type=float, default=0.02)
    ap.add_argument('--all-faces', action='store_true', help='time the module once more with every body walking all faces')
    ap.add_argument('--out', default='clearance_out')
    a = ap.parse_args()
    import torch
    from contact_map import write_ply
    from mhhip import _lib, bodies, contact, surface
    opt, seq, _ = mc.setup(a)
    mc.fit(opt, seq, a)
    T, N = a.frames, a.people
    e, m = opt.engine, opt.SMPLPY.body_model
    if a.together is not None:
        mc.slide_together(opt, a.together)
    got, wall = mc.wall_times(lambda: opt.clearance_map(radius=a.radius, contact=a.contact, chunk=a.chunk), a.repeat)
    # the module alone on the whole sequence's vertices, outputs left on the device: between device events
    live = torch.as_tensor(opt._valid.reshape(T, N) > 0, device=e.dev)
    verts = mc.forward_all(opt).contiguous()
    V = int(verts.shape[2])

    timed = mc.timed

    def module_times(repeat):
        return [timed(lambda: surface.clearance_map(m, verts, live=live, radius=a.radius, contact=a.contact, chunk=a.chunk))
                for _ in range(repeat + 1)][1:]

    def entry_times():
        """(inside test, mh_surface_grid, mh_person_surface, mh_surface_pairs) in ms, each summed over the chunks"""
        L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(e.dev)
        faces = bodies.faces(m, e.dev)
        F = int(faces.shape[0])
        part = torch.as_tensor(contact.body_parts(m)).to(e.dev)
        chunk = max(1, min(a.chunk, T))
        nb_in, nb_sf = L.mh_mesh_bins_bytes(chunk * N, F), L.mh_surface_grid_bytes(chunk * N, F)
        ws_in = torch.empty(nb_in, dtype=torch.uint8, device=e.dev)
        ws_sf = torch.empty(nb_sf, dtype=torch.uint8, device=e.dev)
        lv = live.to(torch.uint8).contiguous()
        mask = torch.empty(chunk, N, V, dtype=torch.int32, device=e.dev)
        oi, ii = torch.empty_like(mask), torch.empty_like(mask)
        od, idd = torch.empty(chunk, N, V, device=e.dev), torch.empty(chunk, N, V, device=e.dev)
        pf = [torch.empty(chunk, N, N, device=e.dev) for _ in range(2)] + [torch.empty(chunk, N, N, dtype=torch.int32, device=e.dev)]
        cf = [torch.empty(chunk, N, 24, device=e.dev) for _ in range(2)] + [torch.empty(chunk, N, 24, dtype=torch.int32, device=e.dev)]
        status = torch.empty(chunk, N, dtype=torch.int32, device=e.dev)
        ms = [0.0] * 4

        def both(v, l, nt):
            _lib.check(L.mh_mesh_bins(nt * N, V, F, v, ptr(faces), l, ptr(ws_in), nb_in, ptr(status), st))
            _lib.check(L.mh_person_inside(nt, N, V, F, ptr(faces), ptr(ws_in), v, ptr(part), 24, ptr(mask), None, None, None, None, None, None, st))
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nt = sl.stop - sl.start
            v, l = ptr(verts[sl]), ptr(lv[sl])
            ms[0] += timed(lambda: both(v, l, nt))
            ms[1] += timed(lambda: _lib.check(L.mh_surface_grid(nt * N, V, F, v, ptr(faces), l, ptr(ws_sf), nb_sf, ptr(status), st)))
            ms[2] += timed(lambda: _lib.check(L.mh_person_surface(nt, N, V, F, ptr(faces), ptr(ws_sf), v, ptr(mask), a.radius, ptr(od), ptr(oi),
                                                                  ptr(idd), ptr(ii), None, None, None, st)))
            ms[3] += timed(lambda: _lib.check(L.mh_surface_pairs(nt, N, V, F, ptr(od), ptr(oi), ptr(idd), ptr(ii), ptr(part), 24, a.contact,
                                                                 *[ptr(x) for x in pf + cf], st)))
        return dict(zip(('inside_test_ms', 'surface_grid_ms', 'person_surface_ms', 'surface_pairs_ms'), [round(x, 3) for x in ms]))

    module_ms = module_times(max(1, a.repeat))
    entry_times()                                           # (warm)
    entries = entry_times()
    st = surface._clearance(m, verts, live, a.radius, a.contact, False, a.chunk, True)
    pairs = int(live.sum(1).clamp(min=1).sub(1).mul(live.sum(1)).sum()) * V       # (vertex of a live person, other live person)
    searched, visited = int(st['searched'].sum()), int(st['faces_visited'].sum())
    inside_searched = int((st['mask'] != 0).sum())          # (two people: one body each; more: a lower bound)
    forced = None
    if a.all_faces:
        was = surface.force_all_faces(True)
        try:
            forced_module = module_times(1)
            forced = dict(module_ms=[round(x, 3) for x in forced_module], **entry_times())
        finally:
            surface.force_all_faces(was)
    del verts, st
    os.makedirs(a.out, exist_ok=True)
    names = contact.PART_NAMES
    with open(os.path.join(a.out, 'clearance_pairs.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'other', 'max_depth_m', 'min_dist_m', 'contact_verts'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                for o in range(N):
                    if o != n:
                        w.writerow([int(fr), n, o, repr(float(got['pair_depth_m'][i, n, o])), repr(float(got['pair_min_dist_m'][i, n, o])),
                                    int(got['pair_contact_verts'][i, n, o])])
    with open(os.path.join(a.out, 'clearance_parts.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'part', 'max_depth_m', 'min_dist_m', 'contact_verts'])
        for i, n, k in zip(*np.nonzero(np.isfinite(got['part_depth_m']) | np.isfinite(got['part_min_dist_m']))):
            w.writerow([int(got['frames'][i]), n, names[k], repr(float(got['part_depth_m'][i, n, k])), repr(float(got['part_min_dist_m'][i, n, k])),
                        int(got['part_contact_verts'][i, n, k])])
    with open(os.path.join(a.out, 'clearance_frames.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['frame', 'person', 'inside_verts', 'min_signed_m', 'status'])
        for i, fr in enumerate(got['frames']):
            for n in range(N):
                w.writerow([int(fr), n, int(got['inside'][i, n].sum()), repr(float(got['signed_m'][i, n].min())), int(got['status'][i, n])])
    if a.ply:
        faces = np.asarray(m.faces).astype(np.int64)
        s = got['signed_m']
        deep = np.where(got['inside'], -s, 0.0)
        tone = 0.4 + 0.6 * deep / max(float(deep.max()), 1e-9)
        far = np.clip(np.where(np.isfinite(s), s, a.radius) / a.radius, 0.0, 1.0)
        rgb = np.where(got['inside'][..., None], np.stack([255 * tone, 30 * tone, 30 * tone], -1),
                       np.where(np.isfinite(s)[..., None], np.stack([40 + 160 * far, 40 + 160 * far, 255 + 0 * far], -1), 128.0))
        rgb = np.rint(rgb).astype(np.uint8)
        for i, fr in enumerate(got['frames']):                  # the vertices the map was computed on, a frame at a time
            write_ply(os.path.join(a.out, 'clearance_%04d.ply' % fr), mc.forward(opt, [int(fr)])[0].cpu().numpy(), faces, rgb[i])
    live_bodies = (got['status'] & 1) == 0
    print(json.dumps(dict(frames=T, people=N, chunk=a.chunk, radius=a.radius, contact=a.contact, together=a.together,
                          inside_verts=int(got['inside'].sum()), max_depth_m=float(np.where(got['inside'], got['depth_m'], 0.0).max()),
                          contact_verts=int(got['pair_contact_verts'].sum()), vertex_body_pairs=pairs,
                          box_rejected_share=round(1.0 - searched / max(1, pairs), 4), surviving_pairs=searched,
                          faces_per_surviving_pair=round(visited / max(1, searched), 2), pairs_searched_unbounded_at_least=inside_searched,
                          all_faces_bodies_share=round(float(((got['status'] & 4) != 0).sum()) / max(1, int(live_bodies.sum())), 4),
                          clearance_map_wall_s=[round(x, 4) for x in wall], module_ms=[round(x, 3) for x in module_ms], **entries,
                          forced_all_faces=forced)))


if __name__ == '__main__':
    main()
