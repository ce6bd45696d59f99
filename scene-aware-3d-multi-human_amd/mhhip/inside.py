"""Is one body inside another: the exact points-inside-mesh test (``mh_mesh_bins``, ``mh_mesh_winding``) and, built on it, for
every vertex of every person the other people of its frame that contain it, how deep along the camera axis, and the counts
per pair of people and per body part (``mh_person_inside``).  The test is defined on an integer lattice of 2^-16 m, so it is
exact and the same on every launch.  Read-only: a workspace and buffers of its own, nothing of an engine's state is written.
include/mhmocap_hip.h has the definitions; the parts are those of ``mhhip.contact``."""
import torch

from . import _lib
from ._lib import check, ptr
from .bodies import MAX_PEOPLE, PART_NAMES, batch_shape, body_parts, faces as model_faces, live_mask, part_table, shape  # noqa: F401

LATTICE_M = 2.0 ** -16                  # metres per lattice unit
NOT_LIVE, NOT_TESTABLE, ALL_FACES = 1, 2, 4     # bits of the status word


def _metres(lat):
    """lattice units (int32, -1 = none) -> metres in float32 (exact: below 2^24 units), inf where none"""
    m = lat.to(torch.float32) * LATTICE_M
    return torch.where(lat < 0, torch.full_like(m, float('inf')), m)


def force_all_faces(on):
    """send every testable body of later calls down the all-faces path (a yardstick and a test: the results do not change);
    returns the previous setting"""
    return bool(_lib.lib().mh_mesh_set_all_faces(1 if on else 0))


def mesh_winding(verts, faces, points, live=None):
    """verts (B,V,3), points (B,Q,3) on the device, faces (F,3) integers (or a body model), live (B) or None -> the raw
    results of ``mh_mesh_bins`` and ``mh_mesh_winding``: (winding, up, down (B,Q) int32 in lattice units, -1 = none,
    status (B) int32)"""
    B, V, Q = batch_shape(verts, points)
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
        nbytes = L.mh_mesh_bins_bytes(B, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        wind = torch.empty(B, Q, dtype=torch.int32, device=dev)
        up, down = torch.empty_like(wind), torch.empty_like(wind)
        check(L.mh_mesh_bins(B, V, F, ptr(v), ptr(fc), ptr(lv), ptr(ws), nbytes, ptr(status), st))
        check(L.mh_mesh_winding(B, V, F, ptr(fc), ptr(ws), Q, ptr(p), ptr(wind), ptr(up), ptr(down), st))
    return wind, up, down, status


def points_inside_mesh(verts, faces, points):
    """verts (V,3) or (B,V,3) on the device, faces (F,3) integers (or a body model), points (Q,3) or (B,Q,3) on the device:
    points of row b against body b -> (winding int32, inside bool, up_m, down_m float32), each (Q) or (B,Q): the winding
    number (+1 inside an outward-oriented closed mesh), winding != 0, and the distance along +z / -z to the nearest face of
    the mesh over / under the point in metres (a multiple of 2^-16), inf where there is none.  A body that is not testable
    (no finite vertex, a coordinate at or beyond 8192 m, more than 8 m across) contains nothing."""
    single = verts.dim() == 2
    if single:
        verts = verts.unsqueeze(0)
        if points.dim() == 2:
            points = points.unsqueeze(0)
    wind, up, down, _ = mesh_winding(verts, faces, points)
    with torch.cuda.device(verts.device), torch.no_grad():
        out = (wind, wind != 0, _metres(up), _metres(down))
    return tuple(o[0] for o in out) if single else out


def penetration_map(model, verts, live=None, chunk=8):
    """verts (T,N,V,3) on the device, any frame whose z is the axis depth is to be measured along (the fit's camera frame);
    live (T,N): the people that are there -> dict of device tensors:

    inside (T,N,V) bool -- the vertex is inside the body of another person of its frame (winding number != 0);
    mask (T,N,V) i32 -- the bits of a uint32: bit m is set iff the vertex is inside person m;
    depth_z_m (T,N,V) f32 -- how far the vertex has to move along z, either way, to leave the body it is deepest in
      (the largest, over the bodies that contain it, of the smaller distance to the surface over / under it), inf outside;
    other (T,N,V) i32 -- that body, the smallest m on a tie, -1 outside;
    pair_verts (T,N,N) i32, pair_depth_z_m (T,N,N) f32 -- vertices of n inside m, and the largest such distance, inf if none;
    part_verts (T,N,24) i32, part_depth_z_m (T,N,24) f32 -- per part of ``PART_NAMES``: vertices inside anybody, largest depth;
    inside_verts (T,N) i32 -- the body's vertices inside anybody;
    status (T,N) i32 -- bit 1: not live, 2: not testable (contains nothing), 4: its queries walk all faces.

    ``chunk`` frames go into one call; memory beyond the inputs and outputs is the workspace of one chunk.  One person per
    frame is not an error: everything is inf / -1 / 0."""
    T, N, V = shape(verts)
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
        nbytes = L.mh_mesh_bins_bytes(chunk * N, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mask = torch.empty(T, N, V, dtype=torch.int32, device=dev)
        depth, other = torch.empty_like(mask), torch.empty_like(mask)
        pair_verts = torch.empty(T, N, N, dtype=torch.int32, device=dev)
        pair_depth = torch.empty_like(pair_verts)
        part_verts = torch.empty(T, N, P, dtype=torch.int32, device=dev)
        part_depth = torch.empty_like(part_verts)
        status = torch.empty(T, N, dtype=torch.int32, device=dev)
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nt = sl.stop - sl.start
            check(L.mh_mesh_bins(nt * N, V, F, ptr(verts[sl]), ptr(faces), None if lv is None else ptr(lv[sl]), ptr(ws), nbytes,
                                 ptr(status[sl]), st))
            check(L.mh_person_inside(nt, N, V, F, ptr(faces), ptr(ws), ptr(verts[sl]), ptr(part), P, ptr(mask[sl]), ptr(depth[sl]),
                                     ptr(other[sl]), ptr(pair_verts[sl]), ptr(pair_depth[sl]), ptr(part_verts[sl]), ptr(part_depth[sl]), st))
        inside = mask != 0
        out = dict(inside=inside, mask=mask, depth_z_m=_metres(depth), other=other, pair_verts=pair_verts,
                   pair_depth_z_m=_metres(pair_depth), part_verts=part_verts, part_depth_z_m=_metres(part_depth),
                   inside_verts=inside.sum(-1).to(torch.int32), status=status)
    return out
