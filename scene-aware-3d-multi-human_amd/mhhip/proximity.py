"""Do two people touch, where, and with which body parts: for every vertex the nearest vertex of the OTHER bodies of its frame
within a radius (``mh_person_nearest``), on which side of that body's surface it lies (``mh_vertex_normals`` and the side test
of ``mh_person_pairs``), and per pair of people and per body part the vertices in contact and the closest approach.
Read-only: a workspace and buffers of its own, nothing of an engine's state is written.  include/mhmocap_hip.h has the
definitions; the parts are those of ``mhhip.contact``."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .bodies import (MAX_PEOPLE, MAX_RADIUS, PART_NAMES, adjacency, body_parts, cell_radius, contact_within,  # noqa: F401
                     live_mask, part_table, shape, vertex_faces)


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
        faces, adj_start, adj_face = adjacency(model, V, dev)
        v = verts.contiguous().float()
        out = torch.empty_like(v)
        check(L.mh_vertex_normals(v.numel() // (3 * V), V, int(faces.shape[0]), ptr(v), ptr(faces), ptr(adj_start), ptr(adj_face),
                                  int(adj_face.shape[0]), ptr(out), st))
    return out


def person_nearest(verts, radius, live=None):
    """verts (T,N,V,3) on the device -> (d2 (T,N,V) float32, idx (T,N,V) int32): squared distance to the nearest vertex of
    another live person of the same frame within ``radius`` and its index m V + u; +inf and -1 where there is none
    (``mh_person_nearest``).  ``live`` (T,N): people that are there, default all."""
    T, N, V = shape(verts)
    radius = cell_radius(radius)
    lv = live_mask(live, T, N)
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
        faces, adj_start, adj_face = adjacency(model, V, dev)
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
