"""Is one body inside another: the exact points-inside-mesh test (``mh_mesh_bins``, ``mh_mesh_winding``) and, built on it, for
every vertex of every person the other people of its frame that contain it, how deep along the camera axis, and the counts
per pair of people and per body part (``mh_person_inside``).  The test is defined on an integer lattice of 2^-16 m, so it is
exact and the same on every launch.  Read-only: a workspace and buffers of its own, nothing of an engine's state is written.
include/mhmocap_hip.h has the definitions; the parts are those of ``mhhip.contact``."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .contact import PART_NAMES, body_parts

MAX_PEOPLE = 32
LATTICE_M = 2.0 ** -16                  # metres per lattice unit
NOT_LIVE, NOT_TESTABLE, ALL_FACES = 1, 2, 4     # bits of the status word


def _faces_of(model):
    for name in ('faces', 'f'):
        if hasattr(model, name):
            return np.asarray(getattr(model, name))
    return np.asarray(model)


def _faces(model, dev):
    """(F,3) int32 on ``dev``; kept on the model where it can keep them"""
    cache = getattr(model, '_inside_faces', None)
    if cache is not None and str(dev) in cache:
        return cache[str(dev)]
    faces = _faces_of(model)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError('faces must be (F,3), got %s' % (tuple(faces.shape),))
    tab = torch.as_tensor(np.ascontiguousarray(faces, dtype=np.int32)).to(dev)
    try:
        if cache is None:
            cache = model._inside_faces = {}
        cache[str(dev)] = tab
    except AttributeError:                                  # (an array of faces: nothing to keep them on)
        pass
    return tab


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
    if verts.dim() != 3 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (V,3) or (B,V,3), got %s' % (tuple(verts.shape),))
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if points.dim() != 3 or points.shape[-1] != 3 or 0 in points.shape or points.shape[0] != B:
        raise ValueError('points must be (Q,3) for verts (V,3) or (B,Q,3) for verts (B,V,3), got %s' % (tuple(points.shape),))
    Q = int(points.shape[1])
    lv = None
    if live is not None:
        lv = torch.as_tensor(live)
        if tuple(lv.shape) != (B,):
            raise ValueError('live must be (B) = (%d), got %s' % (B, tuple(lv.shape)))
        lv = (lv != 0).to(torch.uint8)
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        fc = _faces(faces, dev)
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


def _shape(verts):
    if verts.dim() != 4 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    if N > MAX_PEOPLE:
        raise ValueError('at most %d people per frame, got %d' % (MAX_PEOPLE, N))
    return T, N, V


def _live(live, T, N):
    """(T,N) uint8 on the host, or None"""
    if live is None:
        return None
    lv = torch.as_tensor(live)
    if tuple(lv.shape) != (T, N):
        raise ValueError('live must be (T,N) = (%d,%d), got %s' % (T, N, tuple(lv.shape)))
    return (lv != 0).to(torch.uint8)


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
    T, N, V = _shape(verts)
    part = body_parts(model)
    if part.shape[0] != V:
        raise ValueError('the model has %d vertices, verts %d' % (part.shape[0], V))
    P = len(PART_NAMES)
    if int(part.max()) >= P:
        raise ValueError('the model has more than %d parts' % P)
    lv = _live(live, T, N)
    chunk = max(1, min(int(chunk), T))
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        lv = None if lv is None else lv.to(dev).contiguous()
        verts = verts.contiguous().float()
        part = torch.as_tensor(part).to(dev)
        faces = _faces(model, dev)
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
