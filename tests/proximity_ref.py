"""The person-to-person contact map's definition in numpy (include/mhmocap_hip.h: mh_vertex_normals, mh_person_nearest,
mh_person_pairs): brute force over all pairs in float32, every operation rounded on its own and in the stated order, with the
tie rules.  A restatement of the definitions, not of the kernels; the device results are compared with it bit for bit
(tests/test_proximity_gpu.py)."""
import numpy as np

F = np.float32
ALL_ONES = np.uint64(0xffffffffffffffff)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def vertex_faces_ref(faces, V):
    """(adj_start (V+1), adj_face): for every vertex the faces that name it in ascending face index, once per corner"""
    lists = [[] for _ in range(V)]
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3)):
        for c in tri:
            if 0 <= c < V:
                lists[int(c)].append(f)
    start = np.zeros(V + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in lists])
    return start, np.asarray([f for l in lists for f in l], np.int32).reshape(-1)


def normals_ref(verts, faces, adj_start, adj_face):
    """verts (B,V,3) float32 -> (B,V,3): per vertex the sum, in the table's order and starting from +0, of the unnormalised
    face normals n(f) = e1 x e2; a face index outside [0, F) or a face naming a vertex outside [0, V) contributes nothing"""
    verts = np.ascontiguousarray(verts, F)
    B, V = verts.shape[:2]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    Fn = faces.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(1)
    fc = np.where(ok[:, None], faces, 0)
    v0, v1, v2 = verts[:, fc[:, 0]], verts[:, fc[:, 1]], verts[:, fc[:, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = v1 - v0, v2 - v0
        n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        assert n.dtype == F
        out = np.zeros((B, V, 3), F)
        adj_start, adj_face = np.asarray(adj_start, np.int64), np.asarray(adj_face, np.int64)
        for v in range(V):
            for k in range(max(adj_start[v], 0), min(adj_start[v + 1], len(adj_face))):
                f = adj_face[k]
                if 0 <= f < Fn and ok[f]:
                    out[:, v] = out[:, v] + n[:, f]
    return out


def nearest_ref(verts, radius, live=None, block=256):
    """verts (T,N,V,3) float32 -> d2 (T,N,V) float32, idx (T,N,V) int32: over the vertices p of the OTHER live people of the
    same frame with d2 = (dx dx + dy dy) + dz dz <= radius radius the smallest d2 and m V + u of the candidate that attains
    it, on equal d2 the smallest m, then u; +inf / -1 without a candidate, for a dead person, for a query that is not finite"""
    verts = np.ascontiguousarray(verts, F)
    T, N, V = verts.shape[:3]
    alive = np.ones((T, N), bool) if live is None else np.asarray(live).reshape(T, N) != 0
    r2 = F(radius) * F(radius)
    d2o = np.full((T, N, V), np.inf, F)
    idx = np.full((T, N, V), -1, np.int32)
    fin = np.isfinite(verts).all(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(T):
            pts = verts[t].reshape(N * V, 3)
            owner = np.repeat(np.arange(N), V)
            target = fin[t].reshape(-1) & alive[t][owner]
            for n in range(N):
                if not alive[t, n]:
                    continue
                allowed = target & (owner != n)
                for s in range(0, V, block):
                    q = verts[t, n, s:s + block]
                    dx = pts[None, :, 0] - q[:, None, 0]
                    dy = pts[None, :, 1] - q[:, None, 1]
                    dz = pts[None, :, 2] - q[:, None, 2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    assert d2.dtype == F
                    cand = (d2 <= r2) & allowed[None, :] & fin[t, n, s:s + block, None]
                    dm = np.where(cand, d2, F(np.inf)).min(1)
                    pick = (cand & (d2 == dm[:, None])).argmax(1)          # the first: smallest m, then smallest u
                    has = cand.any(1)
                    d2o[t, n, s:s + block] = np.where(has, dm, F(np.inf))
                    idx[t, n, s:s + block] = np.where(has, pick, -1)
    return d2o, idx


def make_key(d2, idx):
    """(bits of d2 << 32 | idx) as uint64"""
    return (np.asarray(bits(d2)).astype(np.uint64) << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def decode_key(key):
    """uint64 keys -> (d2 float32, idx int32): +inf / -1 for the all-ones key"""
    key = np.asarray(key, np.uint64)
    none = key == ALL_ONES
    d2 = (key >> np.uint64(32)).astype(np.uint32).view(F)
    idx = (key & np.uint64(0xffffffff)).astype(np.int64)
    return np.where(none, F(np.inf), d2).astype(F), np.where(none, -1, idx).astype(np.int32)


def pairs_ref(verts, normals, d2, idx, part, P, thr):
    """-> dict(behind (T,N,V) uint8, pair_verts, pair_behind (T,N,N) int32, pair_min_d2 (T,N,N) float32, part_verts (T,N,P)
    int32, part_min_key (T,N,P) uint64) by the definitions of mh_person_pairs"""
    verts = np.ascontiguousarray(verts, F)
    T, N, V = verts.shape[:3]
    d2 = np.asarray(d2, F).reshape(T, N, V)
    idx = np.asarray(idx).reshape(T, N, V)
    part = np.asarray(part).reshape(V)
    t2 = F(thr) * F(thr)
    has = idx >= 0
    safe = np.where(has, idx, 0)
    m = safe // V
    tt = np.arange(T)[:, None, None]
    p = verts.reshape(T, N * V, 3)[tt, safe]
    behind = np.zeros((T, N, V), bool)
    with np.errstate(invalid='ignore', over='ignore'):
        if normals is not None:
            w = np.ascontiguousarray(normals, F).reshape(T, N * V, 3)[tt, safe]
            e = verts - p
            s = (e[..., 0] * w[..., 0] + e[..., 1] * w[..., 1]) + e[..., 2] * w[..., 2]
            assert s.dtype == F
            behind = has & (s < 0)
        touch = has & (d2 <= t2)
    out = dict(behind=behind.astype(np.uint8), pair_verts=np.zeros((T, N, N), np.int32), pair_behind=np.zeros((T, N, N), np.int32),
               pair_min_d2=np.full((T, N, N), np.inf, F), part_verts=np.zeros((T, N, P), np.int32),
               part_min_key=np.full((T, N, P), ALL_ONES, np.uint64))
    key = make_key(d2, safe)
    for t in range(T):
        for n in range(N):
            for o in range(N):
                sel = has[t, n] & (m[t, n] == o)
                out['pair_verts'][t, n, o] = (sel & touch[t, n]).sum()
                out['pair_behind'][t, n, o] = (sel & touch[t, n] & behind[t, n]).sum()
                if sel.any():
                    out['pair_min_d2'][t, n, o] = d2[t, n][sel].min()
            for k in range(P):
                sel = has[t, n] & (part == k)
                out['part_verts'][t, n, k] = (sel & touch[t, n]).sum()
                if sel.any():
                    out['part_min_key'][t, n, k] = key[t, n][sel].min()
    return out
