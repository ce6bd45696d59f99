"""A numpy restatement of the free-viewpoint renderer's conventions (csrc/mh_view.hip): the projection in float64, and --
working from GIVEN snapped coordinates -- rasterisation, splatting, key composition and resolve in Python integers / int64.
Everything after the projection is exact: the kernels are compared with it bit for bit.

  screen  1/64 pixel, xq = rint(u 64), yq = rint(v 64); pixel (px, py) has its centre at (64 px + 32, 64 py + 32)
  depth   zq = rint(zc 4096), valid 1 <= zq < 2^20
  invalid zc < near, zq out of range, |xq| or |yq| >= 2^18: written (INT32_MIN, 0, 0)
  key     zpix << 32 | payload; payload = n F + f (face f of person n) or 0x80000000 | point; empty = all ones
"""
import numpy as np

EMPTY = np.uint64(0xffffffffffffffff)
INVALID = -2 ** 31
GUARD = 2 ** 18
ZLIM = 2 ** 20
POINT = 0x80000000


def project(xyz, R, t, K, near):
    """xyz (...,3) under ONE view in float64 -> (q (...,3) int64 with invalid rows (INVALID, 0, 0), valid (...) bool,
    distance (...): the smallest relative distance of the entry from a validity boundary)"""
    X = np.asarray(xyz, np.float64)
    R, t, K = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(K, np.float64).reshape(3, 3)
    c = X @ R.T + t
    zc = c[..., 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        u = K[0, 0] * c[..., 0] / zc + K[0, 2]
        v = K[1, 1] * c[..., 1] / zc + K[1, 2]
    xq, yq, zq = np.rint(u * 64), np.rint(v * 64), np.rint(zc * 4096)
    near = float(near)
    valid = (zc >= near) & (zq >= 1) & (zq < ZLIM) & (np.abs(xq) < GUARD) & (np.abs(yq) < GUARD)
    q = np.zeros(X.shape, np.int64)
    q[..., 0] = INVALID
    q[valid] = np.stack([xq, yq, zq], -1)[valid]
    # the boundaries: zc = near; zc 4096 = 0.5 and 2^20 - 0.5 (where rint changes side); |u 64|, |v 64| = 2^18 - 0.5
    with np.errstate(divide='ignore', invalid='ignore'):
        dist = np.minimum.reduce([np.abs(zc - near) / near, np.abs(zc * 4096 - 0.5) / 0.5, np.abs(zc * 4096 - (ZLIM - 0.5)) / ZLIM,
                                  np.abs(np.abs(u * 64) - (GUARD - 0.5)) / GUARD, np.abs(np.abs(v * 64) - (GUARD - 0.5)) / GUARD])
    return q, valid, dist


def point_half(size_q, fq, zq, max_half):
    return min(int(max_half), (max(int(size_q), 0) * int(fq) // int(zq)) // 128)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def face_pixels(v0, v1, v2, H, W):
    """pixels covered by the face with the snapped vertices v0, v1, v2 = (xq, yq, zq): (py, px, zpix) int64 arrays"""
    none = (np.zeros(0, np.int64),) * 3
    if INVALID in (v0[0], v1[0], v2[0]):
        return none
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = ([int(a) for a in v] for v in (v0, v1, v2))
    A = _edge(x0, y0, x1, y1, x2, y2)
    if A == 0:
        return none
    bx0, by0 = max(0, -((32 - min(x0, x1, x2)) // 64)), max(0, -((32 - min(y0, y1, y2)) // 64))        # ceil((min - 32) / 64)
    bx1, by1 = min(W - 1, (max(x0, x1, x2) - 32) // 64), min(H - 1, (max(y0, y1, y2) - 32) // 64)
    if bx1 < bx0 or by1 < by0:
        return none
    py, px = np.meshgrid(np.arange(by0, by1 + 1, dtype=np.int64), np.arange(bx0, bx1 + 1, dtype=np.int64), indexing='ij')
    qx, qy = px * 64 + 32, py * 64 + 32
    s = 1 if A > 0 else -1
    e0, e1, e2 = s * _edge(x1, y1, x2, y2, qx, qy), s * _edge(x2, y2, x0, y0, qx, qy), s * _edge(x0, y0, x1, y1, qx, qy)
    assert ((e0 + e1 + e2) == s * A).all()
    cov = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    z = (e0 * z0 + e1 * z1 + e2 * z2) // (s * A)           # < 2^61: int64 holds it
    return py[cov], px[cov], z[cov]


def clear(T, H, W):
    return np.full((T, H, W), EMPTY, np.uint64)


def _put(img, py, px, key):
    np.minimum.at(img, (py, px), key)


def raster(keys, vq, faces, N):
    """draws vq (T*N,V,3) int, faces (F,3) into keys (T,H,W) uint64, in place"""
    T, H, W = keys.shape
    vq, faces = np.asarray(vq, np.int64), np.asarray(faces, np.int64)
    F = len(faces)
    tri = vq[:, faces]                                     # (T*N,F,3 vertices,3)
    ok = (tri[..., 0] != INVALID).all(-1)
    lo, hi = tri[..., :2].min(2), tri[..., :2].max(2)      # (T*N,F,2)
    bx0, bx1 = np.maximum(0, -((32 - lo[..., 0]) // 64)), np.minimum(W - 1, (hi[..., 0] - 32) // 64)
    by0, by1 = np.maximum(0, -((32 - lo[..., 1]) // 64)), np.minimum(H - 1, (hi[..., 1] - 32) // 64)
    box = ok & (bx0 <= bx1) & (by0 <= by1)
    for b, f in zip(*np.nonzero(box)):                     # (faces without a pixel centre in their box draw nothing)
        py, px, z = face_pixels(tri[b, f, 0], tri[b, f, 1], tri[b, f, 2], H, W)
        if len(z):
            t, n = divmod(int(b), N)
            _put(keys[t], py, px, (z.astype(np.uint64) << np.uint64(32)) | np.uint64(n * F + int(f)))
    return keys


def splat(keys, pq, size_q, fq, max_half):
    """draws the points pq (T,P,3) int with extents size_q (P) (None: 0) into keys, in place"""
    T, H, W = keys.shape
    pq = np.asarray(pq, np.int64)
    for t in range(T):
        for i, (xq, yq, zq) in enumerate(pq[t].tolist()):
            if xq == INVALID or zq < 1:
                continue
            half = point_half(0 if size_q is None else size_q[i], fq, zq, max_half)
            px, py = xq // 64, yq // 64
            x0, x1, y0, y1 = max(0, px - half), min(W - 1, px + half), max(0, py - half), min(H - 1, py + half)
            if x1 < x0 or y1 < y0:
                continue
            key = np.uint64((zq << 32) | POINT | i)
            keys[t, y0:y1 + 1, x0:x1 + 1] = np.minimum(keys[t, y0:y1 + 1, x0:x1 + 1], key)
    return keys


def resolve(keys, N, F):
    """keys -> dict(depth f32, label i32, face i32, coverage (T,N+1) i32)"""
    keys = np.asarray(keys, np.uint64)
    T = keys.shape[0]
    empty = keys == EMPTY
    z = (keys >> np.uint64(32)).astype(np.int64)
    pay = (keys & np.uint64(0xffffffff)).astype(np.int64)
    point = (pay & POINT) != 0
    label = np.where(empty, -1, np.where(point, -2, pay // F)).astype(np.int32)
    face = np.where(empty, -1, np.where(point, pay & (POINT - 1), pay % F)).astype(np.int32)
    depth = np.where(empty, -1.0, z / 4096.0).astype(np.float32)
    cov = np.zeros((T, N + 1), np.int32)
    for t in range(T):
        for n in range(N):
            cov[t, n] = (label[t] == n).sum()
        cov[t, N] = (label[t] == -2).sum()
    return dict(depth=depth, label=label, face=face, coverage=cov)


def shade_image(label, face, verts_view, faces, palette, light, ambient, background, point_rgb):
    """the image formula in float64 from GIVEN labels: 255 palette shade, shade = ambient + (1 - ambient) max(0, -n.light),
    n = unit (v1 - v0) x (v2 - v0) flipped so that n_z <= 0 -> (T,H,W,3) float64 (not rounded)"""
    T, H, W = label.shape
    v = np.asarray(verts_view, np.float64)                 # (T,N,V,3)
    out = np.empty((T, H, W, 3), np.float64)
    out[:] = np.asarray(background, np.float64)
    sc = label == -2
    if sc.any():
        out[sc] = 128.0 if point_rgb is None else np.asarray(point_rgb, np.float64)[face[sc]]
    tt, yy, xx = np.nonzero(label >= 0)
    nn = label[tt, yy, xx]
    tri = np.asarray(faces)[face[tt, yy, xx]]
    v0, v1, v2 = (v[tt, nn, tri[:, k]] for k in range(3))
    c = np.cross(v1 - v0, v2 - v0)
    ln = np.sqrt((c * c).sum(-1))
    n = c / np.where(ln > 0, ln, 1)[:, None]
    n = np.where(n[:, 2:3] > 0, -n, n)
    shade = ambient + (1 - ambient) * np.maximum(0.0, -(n @ np.asarray(light, np.float64)))
    out[tt, yy, xx] = np.clip(255.0 * np.asarray(palette, np.float64)[nn] * shade[:, None], 0, 255)
    return out
