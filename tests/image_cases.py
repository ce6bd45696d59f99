"""Inputs and plain references for the image-space kernels of csrc/mh_image.hip at the edges of their dispatch: the mask
packing at bit 31 and around 0.5, the erosion on images smaller than its window and beyond both grid caps, the two
validity gates at equality, the occlusion ordering of the silhouette term at every instantiation (<4> / <8> / <16> /
<32>) and split (8 | 4 | 1 parts), the priors with their three gradient leaves, the fixed-order sums, and the
stand-alone losses and morphology.

Every reference is written from the definition in include/mhmocap_hip.h and the reference lines it cites, in numpy or
float64 torch on the CPU; none of them packs bits before it counts, ranks people by comparison counting or splits an
image into parts as the kernels do.  Plain module (no pytest, no GPU, nothing from the product tree):
tests/test_image_cases.py proves that the references reproduce the reference-generated fixtures and that every case has
the property it is built for, tests/test_image_gpu.py runs the kernels on them.
"""
import functools
import math
from collections import namedtuple

import numpy as np

F = np.float32
HALF = F(0.5)
BELOW_HALF = np.nextafter(F(0.5), F(0), dtype=np.float32)


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ---------------------------------------------------------------------------------------------------------------
# pack: (T,N,H,W) float masks -> one word per pixel, bit n = seg_n >= 0.5; area = number of set pixels
# ---------------------------------------------------------------------------------------------------------------
PACK_PEOPLE = (1, 5, 31, 32)                                # 32: bit 31, the sign bit of a signed word
PACK_IMAGES = ((1, 1), (1, 37), (37, 1))
PACK_LARGE = (2, 32, 130, 127)                              # 16510 pixels > 64 workgroups * 256: the grid-stride loop runs
PACK_VALUES = (F(0.0), BELOW_HALF, HALF, F(0.7))


@functools.lru_cache(maxsize=None)
def pack_input(T, N, H, W, binary=False):
    """every value of PACK_VALUES in every plane that has four pixels (binary: {0, 1} masks as the sequences have them)"""
    rng = np.random.RandomState(11 * N + H + 1000 * W + 7 * T)
    if binary:
        seg = (rng.rand(T, N, H, W) > 0.4).astype(np.float32)
    else:
        seg = np.asarray(PACK_VALUES, np.float32)[rng.randint(0, 4, (T, N, H, W))]
        if H * W >= 4:
            flat = seg.reshape(T, N, H * W)
            flat[:, :, :4] = np.asarray(PACK_VALUES, np.float32)[(np.arange(4)[None, None] + np.arange(N)[None, :, None]) % 4]
    _freeze(seg)
    return seg


def pack_reference(seg):
    """person by person: bit n = seg_n >= 0.5; area[t, n] = the number of set pixels.  On {0, 1} masks that number IS the
    reference's sum(seg_mask, dim=(2, 3)) (optimizer.py:408); on other values the kernel's definition is the count."""
    seg = np.asarray(seg, np.float32)
    T, N, H, W = seg.shape
    bits = np.zeros((T, H, W), np.uint32)
    area = np.zeros((T, N), np.float32)
    for n in range(N):
        on = seg[:, n] >= HALF
        bits |= on.astype(np.uint32) << np.uint32(n)
        area[:, n] = on.sum(axis=(1, 2))
    return bits, area


def planes(bits, N):
    """(T,H,W) words -> (T,N,H,W) float32 {0,1}"""
    bits = np.asarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, np.uint32)
    return ((bits[:, None] >> np.arange(N, dtype=np.uint32)[None, :, None, None]) & np.uint32(1)).astype(np.float32)


def words(seg01):
    """(T,N,H,W) {0,1} -> (T,H,W) uint32 (the inverse of planes)"""
    seg01 = np.asarray(seg01)
    out = np.zeros((seg01.shape[0],) + seg01.shape[2:], np.uint32)
    for n in range(seg01.shape[1]):
        out |= (seg01[:, n] > 0).astype(np.uint32) << np.uint32(n)
    return out


# ---------------------------------------------------------------------------------------------------------------
# erode / morph (morphology.py:21-34): threshold 0.5, k x k window, pixels outside the image do not count
# ---------------------------------------------------------------------------------------------------------------
MORPH_KSIZES = (1, 3, 5, 7)
MORPH_IMAGES = ((1, 1), (1, 7), (5, 1), (2, 2), (6, 9))     # all but the last are smaller than the 5 and 7 windows
ERODE_IMAGES = ((1, 1), (1, 37), (37, 1), (2, 2))
ERODE_LARGE = (2, 5, 182, 181)                              # 32942 pixels > 128 workgroups * 256


def morph_reference(x, k, dilate):
    """a pixel survives erosion when no in-image pixel of its k x k window is < 0.5; dilation: any in-image pixel of
    the window is >= 0.5.  x (..., H, W) -> float32 {0, 1}"""
    x = np.asarray(x, np.float32)
    H, W = x.shape[-2:]
    r = int(k) // 2
    flag = (x >= HALF) if dilate else (x < HALF)
    hit = np.zeros(x.shape, bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y1 > y0 and x1 > x0:
                hit[..., y0:y1, x0:x1] |= flag[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return (hit if dilate else ~hit).astype(np.float32)


def erode_bits_reference(bits, N, passes=1):
    """Erode2D(3) on every bit plane, `passes` times; bits at and above N are set in every input word here or not at
    all, so they are compared too (a plane of zeros stays zeros, a plane of ones stays ones)"""
    p = planes(bits, 32)
    for _ in range(passes):
        p = morph_reference(p, 3, False)
    return words(p)


@functools.lru_cache(maxsize=None)
def morph_input(H, W, lead=(2, 3)):
    """float maps with values on both sides of and exactly at the threshold"""
    rng = np.random.RandomState(100 * H + W)
    x = np.asarray([0.0, BELOW_HALF, 0.5, 0.7, 1.0, 1.0, 1.0, 1.0], np.float32)[rng.randint(0, 8, tuple(lead) + (H, W))]
    _freeze(x)
    return x


# ---------------------------------------------------------------------------------------------------------------
# gates (optimizer.py:404-409)
# ---------------------------------------------------------------------------------------------------------------
GATE_BODIES = (1, 255, 256, 257)
GATE_THRESHOLDS = (0.5, 0.3)
GATE_IMAGE = (20, 30)                                       # H * W = 600, a multiple of 200: min_area = 3 exactly
NKP = 17


def gates_reference(pose2d, area, thr, min_area):
    """at least 2 joints with conf >= thr, and area >= min_area, both comparisons in float32"""
    conf = np.asarray(pose2d, np.float32)[..., 2] >= F(thr)
    return (conf.sum(axis=1) >= 2).astype(np.float32), (np.asarray(area, np.float32) >= F(min_area)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gates_case(B, thr):
    """body b % 8 == 0: exactly 2 joints AT the threshold, the others just below it (valid); 1: exactly 1 at it
    (invalid); 2: 2 joints just below it (invalid); 3: 3 joints above, on the last three joints; the others random.  The
    areas cycle through min_area, min_area - 1 and random counts."""
    rng = np.random.RandomState(B + int(thr * 100))
    t = F(thr)
    below = np.nextafter(t, F(0), dtype=np.float32)
    pose2d = rng.uniform(0, 1, (B, NKP, 3)).astype(np.float32)
    H, W = GATE_IMAGE
    min_area = 0.005 * H * W
    area = rng.randint(0, 8, B).astype(np.float32)
    for b in range(B):
        j = rng.permutation(NKP)
        if b % 8 == 0:
            pose2d[b, :, 2] = below
            pose2d[b, j[:2], 2] = t
            area[b] = F(min_area)
        elif b % 8 == 1:
            pose2d[b, :, 2] = below
            pose2d[b, j[:1], 2] = t
            area[b] = F(min_area) - F(1)
        elif b % 8 == 2:
            pose2d[b, :, 2] = 0
            pose2d[b, j[:2], 2] = below
        elif b % 8 == 3:
            pose2d[b, :, 2] = 0
            pose2d[b, -3:, 2] = 0.9
    _freeze(pose2d, area)
    return pose2d, area, float(thr), float(min_area)


# ---------------------------------------------------------------------------------------------------------------
# silhouette statistics (optimizer.py:450-477)
# ---------------------------------------------------------------------------------------------------------------
SIL_PEOPLE = (1, 4, 5, 8, 9, 16, 17, 31, 32)                # both sides of every hand-over <4> | <8> | <16> | <32>
SIL_PEOPLE_SHAPE = (3, 17, 19)                              # T, H, W: 323 pixels, 8 parts of 40 or 41
SIL_FRAMES = (1, 511, 512, 2047, 2048)                      # parts = 8 | 4 | 1
SIL_FRAMES_SHAPE = (2, 3, 5)                                # N, H, W: 15 pixels in 8 parts, parts of one or two pixels
SIL_ORDERINGS = ('random', 'all_equal', 'pairs', 'zeros', 'inf')

SilRef = namedtuple('SilRef', 'front apply D S')


def sil_reference(seg, z, p2d_valid, mask_valid):
    """the reference's loop: people in a stable argsort of z (ties to the lower index), an accumulated mask acc;
    at rank r with n the person of that rank: front[n] = the earlier people, apply[n] = mask_valid[t, r] *
    pose2d_valid[t, r] (indexed by RANK, optimizer.py:472), D[n] = #(1 - acc), S[n] = #((1 - acc) & seg_n), acc |= seg_n"""
    seg = np.asarray(seg) > 0
    T, N, H, W = seg.shape
    front = np.zeros((T, N), np.uint32)
    apply = np.zeros((T, N), np.float32)
    D = np.zeros((T, N), np.float32)
    S = np.zeros((T, N), np.float32)
    for t in range(T):
        order = np.argsort(z[t], kind='stable')
        acc = np.zeros((H, W), bool)
        earlier = 0
        for r, n in enumerate(order):
            n = int(n)
            front[t, n] = earlier
            apply[t, n] = mask_valid[t, r] * p2d_valid[t, r]
            D[t, n] = np.count_nonzero(~acc)
            S[t, n] = np.count_nonzero(~acc & seg[t, n])
            acc |= seg[t, n]
            earlier |= 1 << n
    return SilRef(front, apply, D, S)


def sil_depths(T, N, kind, rng):
    """z (T, N) float32 of one ordering kind"""
    z = rng.randn(T, N).astype(np.float32) + F(3)
    if kind == 'all_equal':
        z[:] = F(2.5)
    elif kind == 'pairs':                                   # people 2i and 2i + 1 of a shuffled list share a depth
        for t in range(T):
            p = rng.permutation(N)
            z[t, p] = (np.arange(N) // 2).astype(np.float32)
    elif kind == 'zeros':                                   # -0.0 == +0.0: a tie, whatever their bits
        for t in range(T):
            p = rng.permutation(N)
            k = max(1, N // 2)
            z[t, p[:k]] = np.where(np.arange(k) % 2 == 0, F(0.0), F(-0.0))
            z[t, p[k:]] -= F(3)                             # some people in front of the zeros, some behind
    elif kind == 'inf':
        for t in range(T):
            p = rng.permutation(N)
            z[t, p[:min(N, 2)]] = np.inf                    # two people at +inf tie; everybody else is in front
    return z


SilCase = namedtuple('SilCase', 'seg bits z p2d_valid mask_valid')


@functools.lru_cache(maxsize=None)
def sil_case(T, N, H, W, kind):
    rng = np.random.RandomState(T * 131 + N * 17 + SIL_ORDERINGS.index(kind))
    seg = (rng.rand(T, N, H, W) > 0.55).astype(np.float32)
    z = sil_depths(T, N, kind, rng)
    p2d = (rng.rand(T, N) > 0.3).astype(np.float32)
    mv = (rng.rand(T, N) > 0.3).astype(np.float32)
    bits = words(seg)
    _freeze(seg, bits, z, p2d, mv)
    return SilCase(seg, bits, z, p2d, mv)


@functools.lru_cache(maxsize=None)
def sil_case_reference(T, N, H, W, kind):
    c = sil_case(T, N, H, W, kind)
    r = sil_reference(c.seg, c.z, c.p2d_valid, c.mask_valid)
    _freeze(*r)
    return r


def apply_by_person(c):
    """what apply would be with the gate indexed by the person: the tests need cases where this differs"""
    return c.mask_valid * c.p2d_valid


# ---------------------------------------------------------------------------------------------------------------
# priors (optimizer.py:523-532, 535-542)
# ---------------------------------------------------------------------------------------------------------------
PRIOR_SHAPES = ((1, 1), (3, 2), (5, 9), (2, 32))
PRIOR_BATCHES = (1, 3)
PRIOR_XSCALE = ('zero', 'null', 'small', 'large')
NUM_BETAS = 10
LN_1_1 = 0.0953101798043249

PriorCase = namedtuple('PriorCase', 'T N nbatches poses ref valid betas betas_ref xscale cp cs gposes0 gbetas0 gxscale0')
PriorRef = namedtuple('PriorRef', 'body_loss loss3 gposes gbetas gxscale')


@functools.lru_cache(maxsize=None)
def prior_case(T, N, nbatches, xkind, cs=1e-4):
    """valid with zeros; one pose entry in seven and one beta in five bitwise equal to its reference (sign 0), every other
    |difference| in [1e-3, 0.5]; the three gradient leaves pre-filled, because the kernel adds into them"""
    rng = np.random.RandomState(T * 100 + N + 7 * nbatches + 1000 * PRIOR_XSCALE.index(xkind))
    ref = rng.normal(0, 0.4, (T, N, 72)).astype(np.float32)
    delta = (rng.uniform(1e-3, 0.5, ref.shape) * rng.choice([-1.0, 1.0], ref.shape)).astype(np.float32)
    poses = (ref + delta).astype(np.float32)
    same = rng.rand(*ref.shape) < 1.0 / 7
    poses[same] = ref[same]
    valid = (rng.rand(T, N) > 0.3).astype(np.float32)
    if T * N > 1:
        valid.reshape(-1)[0], valid.reshape(-1)[-1] = 0, 1
    betas_ref = rng.normal(0, 0.8, (N, NUM_BETAS)).astype(np.float32)
    dbeta = (rng.uniform(1e-3, 0.5, betas_ref.shape) * rng.choice([-1.0, 1.0], betas_ref.shape)).astype(np.float32)
    betas = (betas_ref + dbeta).astype(np.float32)
    sameb = rng.rand(*betas.shape) < 0.2
    betas[sameb] = betas_ref[sameb]
    xscale = {'zero': np.zeros(N, np.float32), 'null': None,
              'small': rng.uniform(-1e-3, 1e-3, N).astype(np.float32),
              'large': rng.uniform(-4, 4, N).astype(np.float32)}[xkind]
    g0 = rng.randn(T, N, 72).astype(np.float32)
    gb0 = rng.randn(N, NUM_BETAS).astype(np.float32)
    gx0 = rng.randn(N).astype(np.float32)
    _freeze(poses, ref, valid, betas, betas_ref, xscale, g0, gb0, gx0)
    return PriorCase(T, N, nbatches, poses, ref, valid, betas, betas_ref, xscale, 0.002, float(cs), g0, gb0, gx0)


def prior_reference(c):
    """float64 torch on the CPU, gradients from autograd.  The total of a cycle: every batch adds coef_poses * (its
    bodies' pose prior + batch_size * L1(beta, beta_ref)) (optimizer.py:523-526, 538) and coef_scales * mean((s-1)^2) +
    (coef_scales > 0) * (sum(s-1))^2 (:531-532, 539): the shape term T times, the scale terms once per batch.
    -> body_loss (T,N), loss3 = {T * L1(beta), (sum(s-1))^2, mean((s-1)^2)}, and the three leaves AFTER the addition"""
    import torch
    d = torch.float64
    poses = torch.tensor(c.poses, dtype=d, requires_grad=True)
    betas = torch.tensor(c.betas, dtype=d, requires_grad=True)
    x = torch.tensor(c.xscale if c.xscale is not None else np.zeros(c.N, np.float32), dtype=d, requires_grad=True)
    valid = torch.tensor(c.valid, dtype=d)[..., None]
    body = (valid * torch.tensor(c.ref, dtype=d) - valid * poses).abs().sum(-1)                       # :523-525
    lbeta = (betas - torch.tensor(c.betas_ref, dtype=d)).abs().sum()                                 # :526
    s = torch.pow(torch.tensor(1.1, dtype=d), x)
    s_avg = torch.square(torch.sum(s - 1.0))                                                         # :531
    s_per = torch.mean(torch.square(s - 1.0))                                                        # :532
    total = c.cp * (body.sum() + c.T * lbeta) + c.nbatches * (c.cs * s_per + float(c.cs > 0) * s_avg)    # :538-539
    total.backward()
    gx = c.gxscale0.astype(np.float64) + (x.grad.numpy() if c.xscale is not None else 0.0)
    return PriorRef(body.detach().numpy(), np.array([c.T * float(lbeta.detach()), float(s_avg.detach()), float(s_per.detach())]),
                    c.gposes0.astype(np.float64) + poses.grad.numpy(), c.gbetas0.astype(np.float64) + betas.grad.numpy(), gx)


def prior_float32(c):
    """the same formulas evaluated in numpy float32 (products and sums rounded to float32 one by one).  gposes and gbetas
    are products of float32 values added to a float32 leaf: a kernel has to give these bits."""
    cp, cs = F(c.cp), F(c.cs)
    v = c.valid[..., None]
    dd = (v * c.ref).astype(np.float32) - (v * c.poses).astype(np.float32)
    body = np.abs(dd).sum(-1, dtype=np.float32)
    gposes = c.gposes0 + (cp * (-v * np.sign(dd)).astype(np.float32)).astype(np.float32)
    db = c.betas - c.betas_ref
    gbetas = c.gbetas0 + ((cp * F(c.T)).astype(np.float32) * np.sign(db)).astype(np.float32)
    x = c.xscale if c.xscale is not None else np.zeros(c.N, np.float32)
    s = np.power(F(1.1), x).astype(np.float32)
    sm1 = s - F(1)
    ssum = sm1.sum(dtype=np.float32)
    loss3 = np.array([F(c.T) * np.abs(db).sum(dtype=np.float32), ssum * ssum, (sm1 * sm1).sum(dtype=np.float32) / F(c.N)], np.float32)
    gx = c.gxscale0.copy()
    if c.xscale is not None:
        g = cs * F(2) * sm1 / F(c.N) + F(1.0 if c.cs > 0 else 0.0) * F(2) * ssum
        gx = gx + F(c.nbatches) * g * (s * F(LN_1_1))
    return PriorRef(body, loss3, gposes.astype(np.float32), gbetas.astype(np.float32), gx.astype(np.float32))


def prior_errors(c, got, want=None):
    """|got - float64| per output group, each relative to the largest magnitude of that output in the case (at xscale of
    1e-3 an error relative to (s - 1) itself says nothing: s carries an absolute error of one float32 step at 1);
    body_loss relative to itself, a sum of magnitudes -> dict name -> worst figure"""
    want = want or prior_reference(c)
    out = {}
    b = want.body_loss
    e = np.abs(np.asarray(got.body_loss, np.float64) - b)
    out['body_loss'] = float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    assert (e[b == 0] == 0).all()
    for i, name in ((1, 'scale_avg'), (2, 'scale_person')):
        w = want.loss3[i]
        out[name] = float(abs(float(got.loss3[i]) - w) / (abs(w) if w != 0 else 1.0))
    w = want.gxscale
    out['gxscale'] = float(np.abs(np.asarray(got.gxscale, np.float64) - w).max() / max(np.abs(w).max(), 1e-30))
    return out


PRIOR_GROUPS = ('body_loss', 'scale_avg', 'scale_person', 'gxscale')


def prior_cases():
    return [(T, N, nb, xk) for T, N in PRIOR_SHAPES for nb in PRIOR_BATCHES for xk in PRIOR_XSCALE]


@functools.lru_cache(maxsize=None)
def prior_yardstick():
    """the worst error of the float32 numpy evaluation per output group and xscale kind, over all cases: a kernel is allowed
    4 times it (powf, logf and another summation order)"""
    y = {}
    for T, N, nb, xk in prior_cases():
        c = prior_case(T, N, nb, xk)
        for k, v in prior_errors(c, prior_float32(c)).items():
            key = (k, xk) if k != 'body_loss' else (k, None)
            y[key] = max(y.get(key, 0.0), v)
    return y


# ---------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------
SUM_LENGTHS = (0, 1, 255, 256, 257, 65537)


@functools.lru_cache(maxsize=None)
def sum_input(n, seed=0):
    """mixed signs over four decades: the sum is much smaller than the sum of magnitudes"""
    rng = np.random.RandomState(n + 31 * seed)
    x = (rng.randn(n) * 10.0 ** rng.randint(-2, 2, n)).astype(np.float32)
    _freeze(x)
    return x


def sum_reference(x):
    return math.fsum(float(v) for v in x)


def sum_bound(x):
    """one workgroup of 256 threads: a thread adds ceil(n / 256) terms in turn (at most that many roundings on its partial
    sum, each relative to a partial sum of magnitudes), eight levels of the tree add one rounding each, the scale one more:
    |err| <= (ceil(n / 256) + 9) * 2^-24 * sum|x|"""
    n = len(x)
    return (math.ceil(n / 256) + 9) * 2.0 ** -24 * math.fsum(abs(float(v)) for v in x)


# ---------------------------------------------------------------------------------------------------------------
# stand-alone losses (losses.py:19-40)
# ---------------------------------------------------------------------------------------------------------------
LOSS_RTOL, GRAD_RTOL = 2e-5, 2e-4                           # tests/test_losses_gpu.py
DEPTH_PIXELS = ((1, 1), (15, 17), (1, 257))                 # P = 1, 255, 257: below, at and above one workgroup's stride
MSE_COUNTS = (1, 1023, 1025)                                # around the 1024 threads of the one workgroup that sums

DepthRef = namedtuple('DepthRef', 'loss gpred gtrue loss_scale gpred_scale gtrue_scale')
MseRef = namedtuple('MseRef', 'loss g1 g2 g2_scale')


def depth_reference(pred, true, mask, eps=1e-3):
    """oracle.fit_oracle.avg_log_depth_loss in float64 with the gradients of both arguments from autograd, and the
    magnitudes the errors are taken relative to where terms cancel: the row difference d = sum(m * (log p - log t)) / cnt
    has terms of both signs, so the loss sum(d^2) is measured against sum(D^2) with D = sum(|m log p| + |m log t|) / cnt,
    and a gradient 2 d / cnt * m / p against 2 D / cnt * |m / p| (summed over the rows that share a target pixel)."""
    import torch
    from oracle import fit_oracle
    d = torch.float64
    p = torch.tensor(np.asarray(pred), dtype=d, requires_grad=True)
    t = torch.tensor(np.asarray(true), dtype=d, requires_grad=True)
    m = torch.tensor(np.asarray(mask), dtype=d)
    loss = fit_oracle.avg_log_depth_loss(p, t, m, eps=eps)
    loss.backward()
    with torch.no_grad():
        me = m.expand_as(p)
        cnt = me.sum(dim=(2, 3)) + 1
        lp = (me * torch.log(torch.clamp(p, min=eps))).abs().sum(dim=(2, 3))
        lt = (me * torch.log(torch.clamp(t, min=eps))).abs().expand_as(p).sum(dim=(2, 3))
        D = (lp + lt) / cnt
        row = (2 * D / cnt)[..., None, None] * me.abs()
        gp_scale = torch.where(p >= eps, row / p.abs().clamp(min=1e-300), torch.zeros_like(row))
        gt_rows = torch.where(t.expand_as(p) >= eps, row / t.expand_as(p).abs().clamp(min=1e-300), torch.zeros_like(row))
        gt_scale = gt_rows.sum(dim=1, keepdim=True) if t.shape[1] == 1 and p.shape[1] > 1 else gt_rows
    return DepthRef(float(loss.detach()), p.grad.numpy(), t.grad.numpy(), float((D ** 2).sum()), gp_scale.numpy(), gt_scale.numpy())


def depth_float32(pred, true, mask, eps=1e-3):
    """the loss value by the same formula in numpy float32"""
    p, t, m = (np.asarray(a, np.float32) for a in (pred, true, mask))
    m = np.broadcast_to(m, p.shape)
    lp = (m * np.log(np.maximum(p, F(eps)))).sum(axis=(2, 3), dtype=np.float32)
    lt = (m * np.log(np.maximum(np.broadcast_to(t, p.shape), F(eps)))).sum(axis=(2, 3), dtype=np.float32)
    cnt = m.sum(axis=(2, 3), dtype=np.float32) + F(1)
    return ((lp / cnt - lt / cnt) ** 2).sum(dtype=np.float32)


def mse_reference(y1, y2, mask):
    """oracle.fit_oracle.masked_mse_loss in float64, the gradients of BOTH arguments from autograd (the second one's is
    minus the first one's summed over the broadcast dimensions: measured against the sum of the magnitudes)"""
    import torch
    from oracle import fit_oracle
    d = torch.float64
    a = torch.tensor(np.asarray(y1), dtype=d, requires_grad=True)
    b = torch.tensor(np.asarray(y2), dtype=d, requires_grad=True)
    m = torch.tensor(np.asarray(mask), dtype=d)
    loss = fit_oracle.masked_mse_loss(a, b, m)
    loss.backward()
    g2_scale = torch.tensor(np.abs(a.grad.numpy())).sum_to_size(b.shape).numpy()
    return MseRef(float(loss.detach()), a.grad.numpy(), b.grad.numpy(), g2_scale)


def mse_float32(y1, y2, mask):
    a, b, m = (np.asarray(v, np.float32) for v in (y1, y2, mask))
    d = (m * (a - b)).astype(np.float32)
    return (d * d).sum(dtype=np.float32) / (m.sum(dtype=np.float32) + F(1))        # the mask as handed in (losses.py:36)


@functools.lru_cache(maxsize=None)
def depth_rows_case(H, W, group, b=2, N=3):
    """C-ABI form: pred (b,N,H,W), true (b,1 or N,H,W), mask (b,N,H,W) non-binary in the second frame; pixels below, at
    and above eps (and 0, negative) wherever the image has room for them"""
    rng = np.random.RandomState(H * 10 + W + group)
    pred = rng.uniform(0.05, 1.0, (b, N, H, W)).astype(np.float32)
    true = rng.uniform(0.05, 1.0, (b, 1 if group > 1 else N, H, W)).astype(np.float32)
    mask = (rng.rand(b, N, H, W) > 0.4).astype(np.float32)
    mask[1] *= rng.uniform(0.2, 1.0, mask[1].shape).astype(np.float32)
    if H * W >= 8:
        _clamp_edges(pred.reshape(b, N, -1), 0)
        _clamp_edges(true.reshape(b, true.shape[1], -1), 4)
        mask.reshape(b, N, -1)[:, :, :8] = np.maximum(mask.reshape(b, N, -1)[:, :, :8], F(0.5))
    else:
        pred[0, 0], true[0, 0] = F(1e-3), np.nextafter(F(1e-3), F(0), dtype=np.float32)
        mask[0] = 1
        mask[1] = rng.uniform(0.2, 1.0, mask[1].shape).astype(np.float32)
    _freeze(pred, true, mask)
    return pred, true, mask


def _clamp_edges(flat, at):
    """four consecutive pixels of every map: just below eps, exactly float32(eps), zero, negative"""
    e = F(1e-3)
    flat[..., at:at + 4] = np.array([np.nextafter(e, F(0), dtype=np.float32), e, 0.0, -0.25], np.float32)


@functools.lru_cache(maxsize=None)
def mse_flat_case(n):
    rng = np.random.RandomState(n)
    a = rng.uniform(0, 1, n).astype(np.float32)
    b = rng.uniform(0, 1, n).astype(np.float32)
    m = (rng.rand(n) > 0.3).astype(np.float32) * rng.choice([1.0, 0.5], n).astype(np.float32)
    m[0] = 1                                                # n = 1: not an empty mask
    _freeze(a, b, m)
    return a, b, m


@functools.lru_cache(maxsize=None)
def erode_input(T, N, H, W):
    """{0, 1} masks dense enough (95 %) that two erosions leave about a quarter of the pixels"""
    rng = np.random.RandomState(T + 3 * N + 5 * H + 7 * W)
    seg = (rng.rand(T, N, H, W) > 0.05).astype(np.float32)
    _freeze(seg)
    return seg
