"""Plain references of the lowest-vertex and the contact / foot-sliding kernels (csrc/mh_scene.hip: k_lowest_vertex,
k_lowest_resolve, k_contact_foot) and the inputs their tests share: NumPy float64 computed from the float32 inputs, no GPU.

``contact_foot`` restates reference optimizer.py:502-518 the way oracle/fit_oracle.py:352-358 writes it, batch by batch;
tests/test_scene_terms_ref.py pins it to torch autograd of those formulas and asserts what the case builders promise.
"""
import numpy as np

C_OFFSET = float(np.float32(0.02))        # the kernel's float32 constants, widened
C_GATE = float(np.float32(-0.20))
V_CASE = 7                                # the contact kernel only indexes the vertices: a handful is enough


# ---- lowest vertex (optimizer.py:487-489) ----------------------------------------------------------------------------------------

def lowest_vertex(verts):
    """verts (B,V,3) float32 -> (idx (B,) int32, xyz (B,3) float32): argmax of y, first index on ties; a y that does not
    compare greater than -inf (NaN, -inf) never wins, and a body of nothing else gives index 0"""
    verts = np.asarray(verts, np.float32)
    y = verts[..., 1].astype(np.float64)
    idx = np.argmax(np.where(y > -np.inf, y, -np.inf), axis=1).astype(np.int32)      # -0.0 == +0.0: the first one
    return idx, verts[np.arange(verts.shape[0]), idx]


def lowest_key(verts, idx):
    """the key k_lowest_resolve writes back for a body it scanned: order-preserving bits of y + 0.0f in the high word (so that
    -0.0 and +0.0 share one key), ~index in the low word"""
    verts = np.asarray(verts, np.float32)
    y = verts[np.arange(verts.shape[0]), idx, 1] + np.float32(0.0)
    u = y.view(np.uint32).astype(np.uint64)
    hi = np.where(u >> np.uint64(31), u ^ np.uint64(0xffffffff), u ^ np.uint64(0x80000000))
    return (hi << np.uint64(32)) | ((~np.asarray(idx).astype(np.uint32)).astype(np.uint64))


# ---- contact + foot sliding ------------------------------------------------------------------------------------------------------

def batch_table(T, batch, table=None):
    """(nbatches, batch) int64 frame at every position; None: contiguous batches, positions past T - 1 empty"""
    if table is None:
        nb = (T + batch - 1) // batch
        return np.arange(nb * batch, dtype=np.int64).reshape(nb, batch)
    return np.asarray(table, np.int64).reshape(-1, batch)


def pairs_of(T, N, batch, table=None):
    """[(batch index, position k, person, item of position k, item of position k - 1)] of the in-batch pairs, in the order
    the kernel's loops visit them; item = frame * N + person.  An empty position (entry < 0 or >= T) is in no pair."""
    out = []
    for bt, row in enumerate(batch_table(T, batch, table)):
        for k in range(1, batch):
            t, tp = int(row[k]), int(row[k - 1])
            if 0 <= t < T and 0 <= tp < T:
                out += [(bt, k, n, t * N + n, tp * N + n) for n in range(N)]
    return out


def contact_foot(T, N, V, batch, table, verts, low_idx, low_xyz, dy, cc, cf, dtype=np.float64):
    """-> (gpT (B,3), gverts (B,V,3), batch_contact (nb,), batch_foot (nb,)): the INCREMENTS to the two gradients and the two
    sums per batch, float64.  ``dtype=np.float32``: the same terms summed one after the other in float32 (the sums only), what
    the GPU test measures its gates for the sums with."""
    B = T * N
    verts = np.asarray(verts, np.float32).reshape(B, V, 3).astype(dtype)
    low_xyz = np.asarray(low_xyz, np.float32).reshape(B, 3).astype(dtype)
    dy32 = np.asarray(dy, np.float32).reshape(B)
    dyw = dy32.astype(dtype)
    low_idx = np.asarray(low_idx).reshape(B)
    cc, cf = float(np.float32(cc)), float(np.float32(cf))
    rows = batch_table(T, batch, table)
    gpT, gverts = np.zeros((B, 3)), np.zeros((B, V, 3))
    bc, bf = np.zeros(len(rows)), np.zeros(len(rows))
    open_ = dy32.astype(np.float64) > C_GATE
    for bt, row in enumerate(rows):
        ok = [0 <= int(t) < T for t in row]
        acc = dtype(0)
        for k in range(batch):
            if ok[k]:
                for n in range(N):
                    i = int(row[k]) * N + n
                    r = -(dyw[i] + dtype(C_OFFSET))                  # pT - (detach(pT) + [0, dy + 0.02, 0]), :504-506
                    acc = dtype(acc + abs(r))
                    gpT[i, 1] += cc * np.sign(float(r))
        bc[bt] = acc
        pairs = [(int(row[k]) * N + n, int(row[k - 1]) * N + n) for k in range(1, batch) if ok[k] and ok[k - 1] for n in range(N)]
        cnt = max(sum(1 for i, _ in pairs if open_[i]), 1)          # clamp(sum(gate), 1), :518
        acc = dtype(0)
        for i, ip in pairs:
            if not open_[i]:
                continue
            vi = int(low_idx[i])
            for c in range(3):
                d = low_xyz[i, c] - verts[ip, vi, c]                 # :514-517
                acc = dtype(acc + abs(d))
                gverts[i, vi, c] += cf * np.sign(float(d)) / cnt
                gverts[ip, vi, c] -= cf * np.sign(float(d)) / cnt
        bf[bt] = float(acc * (dtype(1) / dtype(cnt))) if dtype is np.float32 else float(acc) / cnt
    return gpT, gverts, bc, bf


# ---- the cases of tests/test_scene_terms_gpu.py ----------------------------------------------------------------------------------

PERM13 = [7, 2, 11, 0, 9, 4, 12, 5, 1, 10, 3, 8, 6]
SHAPES = {                                 # name: (T, N, batch, table)
    'single': (1, 1, 1, None),                                    # no pair: foot 0, divisor clamped to 1
    'one_pair': (2, 1, 2, None),
    'ragged': (5, 2, 2, None),                                    # contiguous, the last batch one frame short
    'items256': (8, 32, 8, None),                                 # exactly 256 items: the last shape without a second stride
    'items260': (9, 26, 10, None),                                # the first shape into the stride loops (j += 256): empty positions
    'items260_full': (10, 26, 10, None),                          # the same with a frame at the last position: four items there
    'items320': (20, 32, 10, None),                               # two full batches of 320 items
    'positions320': (3, 32, 10, None),                            # 320 positions, frames 0..2 exist
    'permuted': (13, 3, 5, PERM13 + [-1, -1]),                    # a fixed permutation padded with -1
    'hole': (8, 3, 5, [4, 7, -1, 0, 5, 2, -1, 3, 1, 6]),          # an empty position in the middle of a batch
    'past_T': (8, 3, 6, [4, 7, 8, 0, 5, 6, 2, 3, 11, -3, 1, -1]),    # entries equal to T, above T and negative other than -1
}
SHUFFLED_FOR_ORACLE = {                    # empty positions at the end of the last batch only: what a dataloader hands out
    'permuted': SHAPES['permuted'],
    'permuted7': (7, 2, 3, [5, 0, 3, 6, 2, 4, 1, -1, -1]),
}
F_GATE = np.float32(-0.20)
F_OPEN = np.nextafter(np.float32(-0.20), np.float32(0))
F_ZERO = np.float32(-0.02)


def make_case(name, seed=0, shapes=SHAPES):
    """Inputs of one shape with everything the kernel can get wrong planted where the shape has room for it.

    -> dict(T, N, V, batch, table (or None), nb, verts, low_idx, low_xyz, dy, planted).  ``planted`` names the items (frame * N +
    person) that carry a planted value, so that a test can assert the condition from the data:
      at_gate      dy == -0.20f at the current item of a pair: the gate is closed
      above_gate   dy == nextafter(-0.20f, 0): open
      zero_sign    dy == -0.02f: dy + 0.02f == 0, no increment of gpT
      zero_d       (item, previous item, coordinate): low_xyz of the item equals the previous frame's vertex there
      closed       index of a batch with pairs and every gate closed (or None)
    Person 0 keeps one lowest vertex through the sequence, so that the element of a frame in the middle of three positions is
    written by both sweeps; the last person's changes with every position.  The first and the last pairs of batch 0 carry the
    planted values: the last ones are the items of the second stride where a shape has one."""
    T, N, batch, table = shapes[name]
    V = V_CASE
    B = T * N
    rng = np.random.RandomState(1000 + seed + sum(ord(c) for c in name))
    rows = batch_table(T, batch, table)
    verts = rng.uniform(-1, 1, (B, V, 3)).astype(np.float32)
    low_idx = rng.randint(0, V, B).astype(np.int32)
    low_idx[0::N] = 3
    for row in rows:
        for k, t in enumerate(row):
            if 0 <= t < T and N > 1:
                low_idx[int(t) * N + N - 1] = (3 * k + 1) % V
    dy = rng.uniform(-0.3, 0.1, B).astype(np.float32)
    pairs = pairs_of(T, N, batch, table)
    planted = dict(at_gate=[], above_gate=[], zero_sign=[], zero_d=[], closed=None)
    nb = len(rows)
    if nb >= 2:
        its = [i for bt, k, n, i, ip in pairs if bt == 1]
        if its:
            fr = sorted(set(int(t) for t in rows[1] if 0 <= t < T))
            for t in fr:
                dy[t * N:(t + 1) * N] = rng.uniform(-0.5, -0.21, N).astype(np.float32)
            dy[its[0]] = F_GATE
            planted['closed'] = 1
    p0 = [p for p in pairs if p[0] == 0]
    picks = p0[:4] + (p0[-4:] if len(p0) >= 8 else [])
    if len(p0) >= 4:
        for q, (bt, k, n, i, ip) in enumerate(picks):
            kind = q % 4
            if kind == 0:
                dy[i] = F_GATE
                planted['at_gate'].append(i)
            elif kind == 1:
                dy[i] = F_OPEN
                planted['above_gate'].append(i)
            elif kind == 2:
                dy[i] = F_ZERO
                planted['zero_sign'].append(i)
            else:
                dy[i] = np.float32(0.05)
                c = q % 3
                verts[ip, low_idx[i], c] = verts[i, low_idx[i], c]
                planted['zero_d'].append((i, ip, c))
    elif len(p0) == 1:                     # the one pair there is: the gate just open
        dy[p0[0][3]] = F_OPEN
        planted['above_gate'].append(p0[0][3])
    low_xyz = verts[np.arange(B), low_idx].copy()
    return dict(name=name, T=T, N=N, V=V, batch=batch, table=None if table is None else np.asarray(table, np.int32).reshape(nb, batch),
                nb=nb, verts=verts, low_idx=low_idx, low_xyz=low_xyz, dy=dy, planted=planted)


def reference(case, cc, cf, dtype=np.float64):
    c = case
    return contact_foot(c['T'], c['N'], c['V'], c['batch'], c['table'], c['verts'], c['low_idx'], c['low_xyz'], c['dy'], cc, cf, dtype)
