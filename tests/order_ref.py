"""The depth-ordering term between the people of a frame (``mh_order_term_keys``, include/mhmocap_hip.h) in numpy, on
explicit tables: float32 operations in the order the header states, Python integers for the fixed-point sums, one
conversion at the end.  The definition fixes every rounding, so a kernel is compared with this BIT FOR BIT."""
import numpy as np

EMPTY = np.uint64(0xffffffffffffffff)
FIX = 2 ** 24
RMAX = np.float32(1024.0)


def pack_keys(z, face):
    """key = float bits of z << 32 | face, as the selection pass stores it"""
    zb = np.asarray(z, np.float32).view(np.uint32).astype(np.uint64)
    return (zb << np.uint64(32)) | np.asarray(face, np.uint64)


def full_tables(z, face=None, empty=None):
    """tables of bodies whose windows are the whole image: z (T,N,H,W) float32 -> (win (T*N,4) int32, koff (T*N) int64,
    keys (T*N*H*W,5) uint64); face (same shape, default 0); empty (same shape, bool): all-ones keys"""
    z = np.asarray(z, np.float32)
    T, N, H, W = z.shape
    win = np.tile(np.asarray([0, 0, W, H], np.int32), (T * N, 1))
    koff = np.arange(T * N, dtype=np.int64) * (H * W)
    k0 = pack_keys(z, np.zeros(z.shape, np.uint64) if face is None else face)
    if empty is not None:
        k0 = np.where(empty, EMPTY, k0)
    keys = np.full((T * N * H * W, 5), EMPTY, np.uint64)
    keys[:, 0] = k0.reshape(-1)
    return win, koff, keys


def depths(T, N, F, H, W, win, koff, keys):
    """z_n(i) as k_scene_composite decides it: (z (T,N,H*W) float32, defined (T,N,H*W) bool)"""
    P = H * W
    kcap = T * N * P
    z = np.zeros((T, N, P), np.float32)
    ok = np.zeros((T, N, P), bool)
    yy, xx = np.divmod(np.arange(P), W)
    for b in range(T * N):
        x0, y0, ww, wh = (int(v) for v in win[b])
        ko = int(koff[b])
        if not (ww > 0 and wh > 0 and x0 >= 0 and y0 >= 0 and x0 <= W - ww and y0 <= H - wh and ko >= 0 and ko <= kcap - ww * wh):
            continue
        ins = (xx >= x0) & (xx < x0 + ww) & (yy >= y0) & (yy < y0 + wh)
        rec = ko + (yy[ins] - y0) * ww + (xx[ins] - x0)
        k = keys[rec, 0]
        zz = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
        f = (k & np.uint64(0xffffffff)).astype(np.int64)
        with np.errstate(invalid='ignore'):
            good = (k != EMPTY) & (f < F) & (zz > 0) & (zz < np.float32(np.inf))
        t, n = divmod(b, N)
        z[t, n, ins] = np.where(good, zz, np.float32(0))
        ok[t, n, ins] = good
    return z, ok


def order_ref(T, N, F, H, W, win, koff, keys, bits, ebits, gate, coef, margin, delta, gtransl=None):
    """-> dict: G, R, C (lists of T*N Python integers), body_loss (T*N) f32, count (T*N) i32, pairs (T,N,N) i32 and, when
    ``gtransl`` (T*N,3) f32 is given, ``gtransl``: a copy with the term's gradient added"""
    P = H * W
    bits = np.ascontiguousarray(bits).reshape(T, P).view(np.uint32)          # (int32 or uint32 words: read unsigned)
    ebits = np.ascontiguousarray(ebits).reshape(T, P).view(np.uint32)
    margin, delta = np.float32(margin), np.float32(delta)
    z, ok = depths(T, N, F, H, W, np.asarray(win).reshape(T * N, 4), np.asarray(koff).reshape(T * N), keys)
    if gate is not None:
        ok = ok & (np.asarray(gate, np.float32).reshape(T, N, 1) != 0)
    G, R, C = [0] * (T * N), [0] * (T * N), [0] * (T * N)
    pairs = np.zeros((T, N, N), np.int32)
    for t in range(T):
        for y in range(N):
            owner = ((ebits[t] >> np.uint32(y)) & np.uint32(1)).astype(bool) & ok[t, y]
            if not owner.any():
                continue
            for n in range(N):
                if n == y:
                    continue
                px = owner & ~((bits[t] >> np.uint32(n)) & np.uint32(1)).astype(bool) & ok[t, n]
                if not px.any():
                    continue
                with np.errstate(over='ignore'):
                    d = (z[t, y, px] - z[t, n, px]) + margin                 # float32 throughout
                    act = d > 0
                    d = d[act]
                    m = np.minimum(d, delta)
                    r = m * ((d + d) - m)
                    r = np.minimum(r, RMAX)
                assert d.dtype == np.float32 and m.dtype == np.float32 and r.dtype == np.float32
                qm = sum(int(v) for v in np.rint(m.astype(np.float64) * FIX))
                qr = sum(int(v) for v in np.rint(r.astype(np.float64) * FIX))
                G[t * N + y] += qm
                G[t * N + n] -= qm
                R[t * N + y] += qr
                C[t * N + y] += int(act.sum())
                pairs[t, y, n] += int(act.sum())
    c32 = np.float64(np.float32(coef))
    cl, cg = np.float32(c32 / P), np.float32(2.0 * c32 / P)
    tail = lambda v: np.float32(np.float64(float(v)) * 2.0 ** -24)            # int -> double (nearest even) -> float32
    out = dict(G=G, R=R, C=C, pairs=pairs, count=np.asarray(C, np.int32),
               body_loss=np.asarray([cl * tail(v) for v in R], np.float32))
    if gtransl is not None:
        g = np.array(gtransl, np.float32).reshape(T * N, 3).copy()
        if N > 1:
            for b in range(T * N):
                g[b, 2] = g[b, 2] + cg * tail(G[b])
        out['gtransl'] = g
    return out
