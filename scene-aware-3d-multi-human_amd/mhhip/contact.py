"""Which part of a body touches the scene, and how far the rest is from it: for every vertex the nearest point of the scene
cloud within a radius (``mh_scene_nearest``), and per body and body part the vertices in contact and the smallest distance
(``mh_contact_parts``).  Read-only: a grid and buffers of its own, nothing of an engine's state is written."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .bodies import MAX_RADIUS, PART_NAMES, body_parts, cell_radius, contact_within, part_table  # noqa: F401 (names of this module too)


def _grid(L, pts, st):
    M = int(pts.shape[0])
    grid = torch.empty(L.mh_scene_grid_bytes(M), dtype=torch.uint8, device=pts.device)
    check(L.mh_scene_grid_build(ptr(pts), M, ptr(grid), st))
    return grid, M


def _cloud(scene_points, dev):
    pts = torch.as_tensor(scene_points)
    if pts.dim() != 2 or pts.shape[-1] != 3:
        raise ValueError('scene_points must be (M,3), got %s' % (tuple(pts.shape),))
    if int(pts.shape[0]) == 0:
        raise ValueError('scene_points is empty: there is no scene to measure against')
    return pts.to(dev).float().contiguous()


def scene_nearest(points, queries, radius):
    """points (M,3), queries (Q,3) on the device -> (d2 (Q), nearest (Q,3)): squared distance to and position of the nearest
    point within ``radius`` (include/mhmocap_hip.h has the definition); +inf and (0,0,0) where there is none.  Builds a grid
    of its own over ``points``."""
    radius = cell_radius(radius)
    if queries.dim() != 2 or queries.shape[-1] != 3 or int(queries.shape[0]) == 0:
        raise ValueError('queries must be (Q,3) with Q > 0, got %s' % (tuple(queries.shape),))
    dev = queries.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        pts = _cloud(points, dev)
        q = queries.float().contiguous()
        Q = int(q.shape[0])
        grid, M = _grid(L, pts, st)
        d2 = torch.empty(Q, dtype=torch.float32, device=dev)
        near = torch.empty(Q, 3, dtype=torch.float32, device=dev)
        check(L.mh_scene_nearest(ptr(grid), M, ptr(q), Q, radius, ptr(d2), ptr(near), st))
    return d2, near


def contact_map(model, verts, scene_points, radius=0.1, contact=0.03, nearest=False, chunk=32):
    """verts (T,N,V,3) on the device, camera space; scene_points (M,3) -> dict of device tensors:

    dist_m (T,N,V) f32 -- distance of every vertex to the nearest scene point within ``radius``, inf where there is none;
    contact (T,N,V) bool -- that distance is at most ``contact`` (compared as d2 <= contact^2, the product in float32);
    part_verts (T,N,24) i32, part_min_m (T,N,24) f32 -- per part of ``PART_NAMES`` (``body_parts(model)``): the vertices in
      contact and the smallest distance (inf when no vertex of the part is within ``radius``);
    contact_verts (T,N) i32 -- the vertices in contact of the body;
    nearest (T,N,V,3) f32 -- only with ``nearest=True``: the scene point itself, (0,0,0) where there is none.

    ``chunk`` frames go into one launch; memory beyond the inputs and outputs is the grid over the cloud."""
    if verts.dim() != 4 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    radius = cell_radius(radius)
    contact = contact_within(contact, radius)
    dev = verts.device
    part, P = part_table(model, V, dev)
    chunk = max(1, min(int(chunk), T))
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        pts = _cloud(scene_points, dev)
        verts = verts.contiguous().float()
        grid, M = _grid(L, pts, st)
        d2 = torch.empty(T, N, V, dtype=torch.float32, device=dev)
        near = torch.empty(T, N, V, 3, dtype=torch.float32, device=dev) if nearest else None
        counts = torch.empty(T, N, P, dtype=torch.int32, device=dev)
        pmin = torch.empty(T, N, P, dtype=torch.float32, device=dev)
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nb = (sl.stop - sl.start) * N
            check(L.mh_scene_nearest(ptr(grid), M, ptr(verts[sl]), nb * V, radius, ptr(d2[sl]), None if near is None else ptr(near[sl]), st))
            check(L.mh_contact_parts(nb, V, ptr(d2[sl]), ptr(part), P, contact, ptr(counts[sl]), ptr(pmin[sl]), st))
        c2 = float(np.float32(contact) * np.float32(contact))
        out = dict(dist_m=d2.sqrt(), contact=d2 <= c2, part_verts=counts, part_min_m=pmin.sqrt(),
                   contact_verts=counts.sum(-1).to(torch.int32))
        if nearest:
            out['nearest'] = near
    return out
