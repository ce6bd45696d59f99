"""Do two people touch, where, and with which body parts: for every vertex the nearest vertex of the OTHER bodies of its frame
within a radius (``mh_person_nearest``), on which side of that body's surface it lies (``mh_vertex_normals`` and the side test
of ``mh_person_pairs``), and per pair of people and per body part the vertices in contact and the closest approach.
Read-only: a workspace and buffers of its own, nothing of an engine's state is written.  include/mhmocap_hip.h has the
definitions; the parts are those of ``mhhip.contact``."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .contact import MAX_RADIUS, PART_NAMES, _radius, body_parts

MAX_PEOPLE = 32


def vertex_faces(faces, V):
    """faces (F,3) integers, V -> (adj_start (V+1) int32, adj_face (A) int32): for vertex v the faces
    ``adj_face[adj_start[v]:adj_start[v+1]]`` that name it, in ascending face index, a face once per corner that names the
    vertex.  Corners that name a vertex outside [0, V) are left out (the kernel skips such a face altogether)."""
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or int(V) <= 0:
        raise ValueError('faces must be (F,3) and V positive, got %s and %r' % (tuple(faces.shape), V))
    V = int(V)
    corner = faces.astype(np.int64).reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    keep = (corner >= 0) & (corner < V)
    corner, face = corner[keep], face[keep]
    order = np.argsort(corner, kind='stable')             # stable: the faces of a vertex stay in ascending order
    adj_start = np.zeros(V + 1, np.int32)
    adj_start[1:] = np.cumsum(np.bincount(corner, minlength=V))
    return adj_start, face[order].astype(np.int32)


def _faces_of(model):
    for name in ('faces', 'f'):
        if hasattr(model, name):
            return np.asarray(getattr(model, name))
    return np.asarray(model)


def _tables(model, V, dev):
    """(faces (F,3) int32, adj_start, adj_face) on ``dev``; built once per model and device where the model can keep them"""
    key = (str(dev), V)
    cache = getattr(model, '_proximity_tables', None)
    if cache is not None and key in cache:
        return cache[key]
    faces = _faces_of(model)
    adj_start, adj_face = vertex_faces(faces, V)
    tabs = tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (faces, adj_start, adj_face))
    try:
        if cache is None:
            cache = model._proximity_tables = {}
        cache[key] = tabs
    except AttributeError:                                  # (an array of faces: nothing to keep them on)
        pass
    return tabs


def vertex_normals(model, verts):
    """verts (..., V, 3) on the device -> the area-weighted, NOT normalised vertex normals, same shape (``mh_vertex_normals``).
    ``model``: a body model (``faces``) or the (F,3) faces themselves."""
    if verts.dim() < 2 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (...,V,3), got %s' % (tuple(verts.shape),))
    V = int(verts.shape[-2])
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        faces, adj_start, adj_face = _tables(model, V, dev)
        v = verts.contiguous().float()
        out = torch.empty_like(v)
        check(L.mh_vertex_normals(v.numel() // (3 * V), V, int(faces.shape[0]), ptr(v), ptr(faces), ptr(adj_start), ptr(adj_face),
                                  int(adj_face.shape[0]), ptr(out), st))
    return out


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


def person_nearest(verts, radius, live=None):
    """verts (T,N,V,3) on the device -> (d2 (T,N,V) float32, idx (T,N,V) int32): squared distance to the nearest vertex of
    another live person of the same frame within ``radius`` and its index m V + u; +inf and -1 where there is none
    (``mh_person_nearest``).  ``live`` (T,N): people that are there, default all."""
    T, N, V = _shape(verts)
    radius = _radius(radius)
    lv = _live(live, T, N)
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        lv = None if lv is None else lv.to(dev).contiguous()
        v = verts.contiguous().float()
        nbytes = L.mh_person_nearest_bytes(T, N, V)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d2 = torch.empty(T, N, V, dtype=torch.float32, device=dev)
        idx = torch.empty(T, N, V, dtype=torch.int32, device=dev)
        check(L.mh_person_nearest(T, N, V, ptr(v), ptr(lv), radius, ptr(ws), nbytes, ptr(d2), ptr(idx), st))
    return d2, idx


def decode_keys(keys, V, part):
    """part_min_key (...) int64 (the uint64's bits), V, part (V) tensor -> (smallest d2 float32, other person int32, part of
    the other body's vertex int32): inf / -1 / -1 where the key is all ones"""
    none = keys < 0
    k = keys.clamp(min=0)
    d2 = (k >> 32).to(torch.int32).view(torch.float32)
    idx = k & 0xffffffff
    inf = torch.full_like(d2, float('inf'))
    minus = torch.full_like(idx, -1)
    return (torch.where(none, inf, d2), torch.where(none, minus, idx // V).to(torch.int32),
            torch.where(none, minus, part.to(torch.int64)[idx % V]).to(torch.int32))


def proximity_map(model, verts, live=None, radius=0.1, contact=0.02, nearest=False, chunk=8):
    """verts (T,N,V,3) on the device, any common frame; live (T,N): the people that are there -> dict of device tensors:

    dist_m (T,N,V) f32 -- distance of every vertex to the nearest vertex of another person of its frame within ``radius``,
      inf where there is none;
    contact (T,N,V) bool -- that distance is at most ``contact`` (compared as d2 <= contact^2, the product in float32);
    behind (T,N,V) bool -- the vertex lies on the inner side of the other body's surface at that body's nearest vertex (a
      local side test against the vertex normal, not a points-inside-mesh test), in contact or not;
    other (T,N,V) i32 -- the other person, -1 where there is none;
    pair_verts, pair_behind (T,N,N) i32 -- vertices of n in contact (and behind) whose nearest person is m;
    pair_min_m (T,N,N) f32 -- smallest distance over the vertices of n whose nearest person is m, inf when there is none;
    part_verts (T,N,24) i32, part_min_m (T,N,24) f32 -- per part of ``PART_NAMES``: vertices in contact, smallest distance;
    part_other, part_other_part (T,N,24) i32 -- the other person, and the part of its vertex, at the part's closest
      approach; -1 where there is none;
    contact_verts, behind_verts (T,N) i32 -- the body's vertices in contact / behind;
    other_vert (T,N,V) i32, nearest (T,N,V,3) f32 -- only with ``nearest=True``: the other body's vertex and its position,
      -1 and (0,0,0) where there is none.

    ``chunk`` frames go into one call; memory beyond the inputs and outputs is the workspace and normals of one chunk.  One
    person per frame is not an error: everything is inf / -1 / 0."""
    T, N, V = _shape(verts)
    radius = _radius(radius)
    contact = float(np.float32(contact))
    if not 0.0 <= contact <= radius:
        raise ValueError('contact must lie in [0, radius = %g]: beyond the radius no distance is known, got %g' % (radius, contact))
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
        faces, adj_start, adj_face = _tables(model, V, dev)
        nbytes = L.mh_person_nearest_bytes(chunk, N, V)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        normals = torch.empty(chunk, N, V, 3, dtype=torch.float32, device=dev)
        d2 = torch.empty(T, N, V, dtype=torch.float32, device=dev)
        idx = torch.empty(T, N, V, dtype=torch.int32, device=dev)
        behind = torch.empty(T, N, V, dtype=torch.uint8, device=dev)
        pair_verts = torch.empty(T, N, N, dtype=torch.int32, device=dev)
        pair_behind = torch.empty(T, N, N, dtype=torch.int32, device=dev)
        pair_min = torch.empty(T, N, N, dtype=torch.float32, device=dev)
        part_verts = torch.empty(T, N, P, dtype=torch.int32, device=dev)
        keys = torch.empty(T, N, P, dtype=torch.int64, device=dev)
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(T, t0 + chunk))
            nt = sl.stop - sl.start
            check(L.mh_person_nearest(nt, N, V, ptr(verts[sl]), None if lv is None else ptr(lv[sl]), radius, ptr(ws), nbytes,
                                      ptr(d2[sl]), ptr(idx[sl]), st))
            check(L.mh_vertex_normals(nt * N, V, int(faces.shape[0]), ptr(verts[sl]), ptr(faces), ptr(adj_start), ptr(adj_face),
                                      int(adj_face.shape[0]), ptr(normals), st))
            check(L.mh_person_pairs(nt, N, V, ptr(verts[sl]), ptr(normals), ptr(d2[sl]), ptr(idx[sl]), ptr(part), P, contact,
                                    ptr(behind[sl]), ptr(pair_verts[sl]), ptr(pair_min[sl]), ptr(pair_behind[sl]), ptr(part_verts[sl]),
                                    ptr(keys[sl]), st))
        c2 = float(np.float32(contact) * np.float32(contact))
        has = idx >= 0
        minus = torch.full_like(idx, -1)
        key_d2, part_other, part_other_part = decode_keys(keys, V, part)
        behind = behind != 0
        out = dict(dist_m=d2.sqrt(), contact=d2 <= c2, behind=behind, other=torch.where(has, idx // V, minus),
                   pair_verts=pair_verts, pair_behind=pair_behind, pair_min_m=pair_min.sqrt(),
                   part_verts=part_verts, part_min_m=key_d2.sqrt(), part_other=part_other, part_other_part=part_other_part,
                   contact_verts=pair_verts.sum(-1).to(torch.int32), behind_verts=behind.sum(-1).to(torch.int32))
        if nearest:
            out['other_vert'] = torch.where(has, idx % V, minus)
            pos = verts.view(T, N * V, 3).gather(1, idx.clamp(min=0).view(T, N * V, 1).expand(-1, -1, 3).to(torch.int64)).view(T, N, V, 3)
            out['nearest'] = torch.where(has.unsqueeze(-1), pos, torch.zeros_like(pos))
    return out
