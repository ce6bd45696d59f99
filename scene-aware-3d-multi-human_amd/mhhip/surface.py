"""How far is a point from the SURFACE of a mesh, and how deep is one body inside another along the shortest way out: the exact
point-to-triangle distance over a mesh (``mh_surface_grid``, ``mh_mesh_closest``) and, built on it and on the inside test of
``mhhip.inside``, for every vertex of every person the signed distance to the other people of its frame -- negative where it is
inside one of them -- with the closest surface point and the tables per pair of people and per body part
(``mh_person_surface``, ``mh_surface_pairs``).  The distance is defined in float32 in a fixed order, so it is the same on every
launch and equal bit for bit to a float32 evaluation on the host.  Read-only: a workspace and buffers of its own, nothing of an
engine's state is written.  include/mhmocap_hip.h has the definitions; the parts are those of ``mhhip.contact``."""
import torch

from . import _lib
from ._lib import check, ptr
from .bodies import (PART_NAMES, any_radius, batch_shape, body_parts, cell_radius, contact_within, faces as model_faces,  # noqa: F401
                     live_mask, part_table, shape)

NOT_LIVE, NOT_TESTABLE, ALL_FACES = 1, 2, 4     # bits of the status word
INF = float('inf')


def force_all_faces(on):
    """send every live body of later calls down the all-faces path (a yardstick and a test: the results do not change);
    returns the previous setting"""
    return bool(_lib.lib().mh_surface_set_all_faces(1 if on else 0))


def mesh_closest(verts, faces, points, radius=INF, live=None):
    """verts (B,V,3), points (B,Q,3) on the device, faces (F,3) integers (or a body model), live (B) or None -> the raw
    results of ``mh_surface_grid`` and ``mh_mesh_closest``: (d2 (B,Q) float32, face (B,Q) int32, point, weights (B,Q,3)
    float32, status (B) int32)"""
    B, V, Q = batch_shape(verts, points)
    radius = any_radius(radius)
    lv = live_mask(live, B)
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        fc = model_faces(faces, dev)
        F = int(fc.shape[0])
        lv = None if lv is None else lv.to(dev).contiguous()
        v = verts.contiguous().float()
        p = points.to(dev).contiguous().float()
        nbytes = L.mh_surface_grid_bytes(B, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        d2 = torch.empty(B, Q, dtype=torch.float32, device=dev)
        face = torch.empty(B, Q, dtype=torch.int32, device=dev)
        point = torch.empty(B, Q, 3, dtype=torch.float32, device=dev)
        weights = torch.empty_like(point)
        check(L.mh_surface_grid(B, V, F, ptr(v), ptr(fc), ptr(lv), ptr(ws), nbytes, ptr(status), st))
        check(L.mh_mesh_closest(B, V, F, ptr(fc), ptr(ws), Q, ptr(p), radius, ptr(d2), ptr(face), ptr(point), ptr(weights), st))
    return d2, face, point, weights, status


def closest_point_on_mesh(verts, faces, points, radius=INF):
    """verts (V,3) or (B,V,3) on the device, faces (F,3) integers (or a body model), points (Q,3) or (B,Q,3) on the device:
    points of row b against body b -> (d2 float32, face int32 (Q) or (B,Q), point, weights float32 (Q,3) or (B,Q,3)): the
    squared distance to the nearest point of the mesh's surface within ``radius`` (inf: anywhere), the face it lies on (the
    smallest index on a tie: a point over a shared edge), the point itself and its barycentric weights on the face's three
    vertices.  inf / -1 / zeros where there is none, for a point that is not finite, and for a mesh without a finite face."""
    single = verts.dim() == 2
    if single:
        verts = verts.unsqueeze(0)
        if points.dim() == 2:
            points = points.unsqueeze(0)
    out = mesh_closest(verts, faces, points, radius)[:4]
    return tuple(o[0] for o in out) if single else out


def signed_distance(verts, faces, points, radius=INF):
    """as ``closest_point_on_mesh`` -> float32 metres (Q) or (B,Q): the distance to the surface, NEGATIVE where
    ``inside.points_inside_mesh`` says the point is inside (winding number != 0), inf (never -inf) where no surface lies
    within ``radius``.  The sign is the lattice test's (coordinates rounded to 2^-16 m), the distance float32's: closer
    than one lattice unit (15 um) to the surface the two come from two roundings of the same geometry, and a point that is
    that close may carry either sign."""
    from .inside import points_inside_mesh
    d2 = closest_point_on_mesh(verts, faces, points, radius)[0]
    ins = points_inside_mesh(verts, faces, points)[1]
    with torch.cuda.device(d2.device), torch.no_grad():
        d = _root(d2)
        return torch.where(ins & torch.isfinite(d), -d, d)


def _root(d2):
    """float32 D2 -> metres, the CORRECTLY ROUNDED float32 square root whatever the device's own float32 root does: taken in
    float64 and rounded (53 bits >= 2 x 24 + 2: the double rounding is harmless), so the metres equal the host's bit for bit"""
    return d2.double().sqrt().float()


def _depth(bits_d2):
    """largest squared depth, -1 = none -> metres, inf where none"""
    return torch.where(bits_d2 < 0, torch.full_like(bits_d2, INF), _root(bits_d2.clamp(min=0)))


def clearance_map(model, verts, live=None, radius=0.1, contact=0.02, nearest=False, chunk=8):
    """verts (T,N,V,3) on the device, in the frame ``inside.penetration_map`` wants (the inside test is its own); live (T,N):
    the people that are there -> dict of device tensors:

    signed_m (T,N,V) f32 -- ``-depth_m`` where the vertex is inside another person of its frame, else ``dist_m``;
    dist_m (T,N,V) f32 -- distance to the nearest surface, within ``radius``, among the bodies that do not contain the vertex,
      inf where there is none;
    depth_m (T,N,V) f32 -- the distance to the surface of the body the vertex is deepest in (the largest, over the bodies
      that contain it, of the distance to that body's surface: the shortest way out of it, however deep), inf outside;
    other, face (T,N,V) i32 -- the person and the face of its mesh that decide ``signed_m``, -1 where it is inf;
    inside (T,N,V) bool, mask (T,N,V) i32 -- as ``inside.penetration_map`` gives them (bit m: inside person m);
    pair_depth_m (T,N,N) f32 -- largest depth over the vertices of n that are deepest in m, inf if none;
    pair_min_dist_m (T,N,N) f32, pair_contact_verts (T,N,N) i32 -- over the vertices of n whose nearest surface outside is
      m's: the smallest ``dist_m`` (inf if none), and how many have ``dist_m`` <= ``contact`` (compared squared in float32);
    part_depth_m, part_min_dist_m (T,N,24) f32, part_contact_verts (T,N,24) i32 -- the same per part of ``PART_NAMES``;
    status (T,N) i32 -- bit 1: not live, 2: not testable for the inside test (contains nothing), 4: its distance queries
      walk all faces;
    point (T,N,V,3) f32 -- only with ``nearest=True``: the closest surface point of the body that decides ``signed_m``, so
      the way out or the way to contact; zeros where there is none.

    ``chunk`` frames go into one call; memory beyond the inputs and outputs is the two workspaces of one chunk.  One person
    per frame is not an error: everything is inf / -1 / 0."""
    return _clearance(model, verts, live, radius, contact, nearest, chunk, False)


def _clearance(model, verts, live, radius, contact, nearest, chunk, stats):
    """``clearance_map``; ``stats`` adds ``searched`` and ``faces_visited`` (T,N,V) i32: the other bodies a vertex searched (not
    dropped at their box) and the faces it evaluated (tools/clearance_map.py reports them)"""
    T, N, V = shape(verts)
    radius = cell_radius(radius)
    contact = contact_within(contact, radius)
    dev = verts.device
    part, P = part_table(model, V, dev)
    lv = live_mask(live, T, N)
    chunk = max(1, min(int(chunk), T))
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        lv = None if lv is None else lv.to(dev).contiguous()
        verts = verts.contiguous().float()
        faces = model_faces(model, dev)
        F = int(faces.shape[0])
        nb_in, nb_sf = L.mh_mesh_bins_bytes(chunk * N, F), L.mh_surface_grid_bytes(chunk * N, F)
        ws_in = torch.empty(nb_in, dtype=torch.uint8, device=dev)
        ws_sf = torch.empty(nb_sf, dtype=torch.uint8, device=dev)
        mask = torch.empty(T, N, V, dtype=torch.int32, device=dev)
        out_idx, in_idx = torch.empty_like(mask), torch.empty_like(mask)
        out_d2 = torch.empty(T, N, V, dtype=torch.float32, device=dev)
        in_d2 = torch.empty_like(out_d2)
        out_pt = torch.empty(T, N, V, 3, dtype=torch.float32, device=dev) if nearest else None
        in_pt = torch.empty_like(out_pt) if nearest else None
        st2 = torch.empty(T, N, V, 2, dtype=torch.int32, device=dev) if stats else None
        pair_depth = torch.empty(T, N, N, dtype=torch.float32, device=dev)
        pair_min = torch.empty_like(pair_depth)
        pair_contact = torch.empty(T, N, N, dtype=torch.int32, device=dev)
        part_depth = torch.empty(T, N, P, dtype=torch.float32, device=dev)
        part_min = torch.empty_like(part_depth)
        part_contact = torch.empty(T, N, P, dtype=torch.int32, device=dev)
        status_in = torch.empty(T, N, dtype=torch.int32, device=dev)
        status_sf = torch.empty_like(status_in)

        def at(x, sl):
            return None if x is None else ptr(x[sl])
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nt = sl.stop - sl.start
            v, l = ptr(verts[sl]), at(lv, sl)
            check(L.mh_mesh_bins(nt * N, V, F, v, ptr(faces), l, ptr(ws_in), nb_in, ptr(status_in[sl]), st))
            check(L.mh_person_inside(nt, N, V, F, ptr(faces), ptr(ws_in), v, ptr(part), P, ptr(mask[sl]), None, None, None, None, None,
                                     None, st))
            check(L.mh_surface_grid(nt * N, V, F, v, ptr(faces), l, ptr(ws_sf), nb_sf, ptr(status_sf[sl]), st))
            check(L.mh_person_surface(nt, N, V, F, ptr(faces), ptr(ws_sf), v, ptr(mask[sl]), radius, ptr(out_d2[sl]), ptr(out_idx[sl]),
                                      ptr(in_d2[sl]), ptr(in_idx[sl]), at(out_pt, sl), at(in_pt, sl), at(st2, sl), st))
            check(L.mh_surface_pairs(nt, N, V, F, ptr(out_d2[sl]), ptr(out_idx[sl]), ptr(in_d2[sl]), ptr(in_idx[sl]), ptr(part), P, contact,
                                     ptr(pair_depth[sl]), ptr(pair_min[sl]), ptr(pair_contact[sl]), ptr(part_depth[sl]), ptr(part_min[sl]),
                                     ptr(part_contact[sl]), st))
        inside = mask != 0
        dist, depth = _root(out_d2), _root(in_d2)
        idx = torch.where(inside, in_idx, out_idx)
        minus = torch.full_like(idx, -1)
        out = dict(signed_m=torch.where(inside, -depth, dist), dist_m=dist, depth_m=depth,
                   other=torch.where(idx >= 0, idx // F, minus), face=torch.where(idx >= 0, idx % F, minus), inside=inside, mask=mask,
                   pair_depth_m=_depth(pair_depth), pair_min_dist_m=_root(pair_min), pair_contact_verts=pair_contact,
                   part_depth_m=_depth(part_depth), part_min_dist_m=_root(part_min), part_contact_verts=part_contact,
                   status=(status_in & (NOT_LIVE | NOT_TESTABLE)) | (status_sf & (NOT_LIVE | ALL_FACES)))
        if nearest:
            out['point'] = torch.where(inside.unsqueeze(-1), in_pt, out_pt)
        if stats:
            out['searched'], out['faces_visited'] = st2[..., 0], st2[..., 1]
    return out
