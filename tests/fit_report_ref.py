"""numpy reference of the fit report (``mh_fit_report_pixels``, ``mh_fit_report_verts``, ``mhhip.report.fit_report``): no GPU,
no torch.  Also the inputs the GPU tests run the two kernels on, so that the CPU tests can hold those inputs to their caps.

Pixel kernel: nothing is undecided.  Every comparison is one float32 operation on float32 inputs and is done in float32
here; the counts are exact.  The two sums are evaluated in the precision asked for (``dtype``).

Vertex kernel: a vertex is UNDECIDED, and left out of the exact comparison, when in float64
  * u or v lies within 1e-3 px of an integer (the float32 projection at u <= 256 is good to about 1e-4 px),
  * |z - scene_depth - margin| < 1e-5 max(1, z), or
  * |z| < 1e-6.
"""
import numpy as np

DEPTH_OFFSET = 0.2      # optimizer.py:440
MARGIN = 0.05


# ---- pixels ----------------------------------------------------------------------------------------------------------------

def pixels_ref(person, depth, bits, N, disp=None, min_z=None, max_z=None, scene_depth=None, scene_mask=None,
               depth_offset=DEPTH_OFFSET, margin=MARGIN, dtype=np.float64):
    """counts (T,N,4) int64 = rendered, segmented, intersection, behind; dsum (T,N,2) of ``dtype`` = sum d, sum |d| over the
    intersection, the formula AND the sums evaluated in ``dtype``"""
    person = np.asarray(person)
    depth = np.asarray(depth, np.float32)
    bits = np.asarray(bits).astype(np.int64) & 0xffffffff          # the words are unsigned
    T = person.shape[0]
    counts = np.zeros((T, N, 4), np.int64)
    dsum = np.zeros((T, N, 2), dtype)
    behind = None
    if scene_depth is not None:
        surface = (np.asarray(scene_depth, np.float32) + np.float32(margin)).astype(np.float32)      # ONE float32 add
        behind = (np.asarray(scene_mask) != 0)[None] & (depth > surface[None])
    d = None
    if disp is not None:
        f = lambda a: np.asarray(a, np.float32).astype(dtype)
        a = (dtype(1) / f(max_z)).reshape(T, 1, 1)
        b = (dtype(1) / f(min_z)).reshape(T, 1, 1) - a
        d = f(depth) + dtype(np.float32(depth_offset)) - dtype(1) / (f(disp) * b + a)
    for n in range(N):
        ren = person == n
        seg = ((bits >> n) & 1) != 0
        both = ren & seg
        counts[:, n, 0] = ren.sum(axis=(1, 2))
        counts[:, n, 1] = seg.sum(axis=(1, 2))
        counts[:, n, 2] = both.sum(axis=(1, 2))
        if behind is not None:
            counts[:, n, 3] = (ren & behind).sum(axis=(1, 2))
        if d is not None:
            for t in range(T):
                v = d[t][both[t]]
                dsum[t, n, 0] = v.sum(dtype=dtype)
                dsum[t, n, 1] = np.abs(v).sum(dtype=dtype)
    return counts, dsum


PIXEL_SHAPES = [(1, 1, 1, 1), (1, 1, 55, 97), (3, 4, 55, 97), (2, 32, 17, 33), (70, 2, 9, 16), (2, 4, 135, 240)]


def pixel_case(T, N, H, W):
    """random label, depth, mask, disparity and scene maps of one of PIXEL_SHAPES"""
    rng = np.random.RandomState(1000 + 7 * T + 13 * N + H)
    person = np.where(rng.rand(T, H, W) < 0.5, rng.randint(0, N, (T, H, W)), -1).astype(np.int32)
    bits = np.zeros((T, H, W), np.uint32)
    for n in range(N):
        bits |= (rng.rand(T, H, W) < 0.3).astype(np.uint32) << np.uint32(n)
    # half of the rendered pixels carry their own bit: the intersection is not left to chance
    own = (person >= 0) & (rng.rand(T, H, W) < 0.5)
    bits[own] |= np.uint32(1) << person[own].astype(np.uint32)
    if (T, N, H, W) == (1, 1, 1, 1):
        person[...] = 0
        bits[...] = 1
    if N == 32:                                   # every person present in every frame, with its bit
        flat_p, flat_b = person.reshape(T, -1), bits.reshape(T, -1)
        flat_p[:, :N] = np.arange(N)
        flat_b[:, :N] |= np.uint32(1) << np.arange(N).astype(np.uint32)
    if (H, W) == (135, 240):
        person[0] = -1                            # nothing rendered in frame 0
        bits[1] = 0                               # nothing segmented in frame 1
    scene_depth = rng.uniform(1.0, 6.0, (H, W)).astype(np.float32)
    scene_mask = (rng.rand(H, W) < 0.7).astype(np.uint8)
    depth = np.where(person >= 0, rng.uniform(1.0, 6.0, (T, H, W)), -1.0).astype(np.float32)
    # the edge of the float32 comparison: a sixth of the rendered pixels sit exactly ON the surface + margin (not behind), a
    # sixth one float above it (behind)
    surface = (scene_depth + np.float32(MARGIN)).astype(np.float32)
    kind = rng.randint(0, 6, (T, H, W))
    on = (person >= 0) & (kind == 0)
    above = (person >= 0) & (kind == 1)
    depth = np.where(on, surface[None], depth)
    depth = np.where(above, np.nextafter(surface, np.float32(np.inf))[None], depth).astype(np.float32)
    disp = rng.uniform(0.05, 1.0, (T, H, W)).astype(np.float32)
    min_z = rng.uniform(1.0, 2.0, T).astype(np.float32)
    max_z = (min_z + 1.0 + rng.uniform(0.0, 5.0, T)).astype(np.float32)
    return dict(T=T, N=N, H=H, W=W, person=person, depth=depth, bits=bits, disp=disp, min_z=min_z, max_z=max_z,
                scene_depth=scene_depth, scene_mask=scene_mask)


def sum_budget(cases):
    """the largest error of the float32 evaluation of the two sums against float64 over ``cases``, relative to sum |d|"""
    worst = 0.0
    for c in cases:
        kw = dict(disp=c['disp'], min_z=c['min_z'], max_z=c['max_z'])
        _, s32 = pixels_ref(c['person'], c['depth'], c['bits'], c['N'], dtype=np.float32, **kw)
        _, s64 = pixels_ref(c['person'], c['depth'], c['bits'], c['N'], dtype=np.float64, **kw)
        scale = np.maximum(s64[..., 1:2], 1e-300)
        worst = max(worst, float((np.abs(s32.astype(np.float64) - s64) / scale).max()))
    return worst


# ---- vertices --------------------------------------------------------------------------------------------------------------

def verts_ref(verts, K, scene_depth, scene_mask, margin=MARGIN):
    """per vertex, from float64 arithmetic on the float32 inputs: ``inside`` (decided, counted), ``outside`` (decided, inside
    image and mask, not counted), ``undecided``; ``pen`` = float32(z - scene_depth[pixel]) of the float64 pixel; ``extra`` =
    per body the float32 penetrations an undecided vertex may contribute, over every pixel within 1e-3 px of its projection"""
    v32 = np.asarray(verts, np.float32)
    B, V = v32.shape[:2]
    H, W = scene_depth.shape
    K = np.asarray(K, np.float64).reshape(3, 3)
    sd32 = np.asarray(scene_depth, np.float32)
    mask = np.asarray(scene_mask) != 0
    x, y, z = (v32[..., k].astype(np.float64) for k in range(3))
    tiny = np.abs(z) < 1e-6
    zs = np.where(tiny, 1.0, z)
    u = K[0, 0] * x / zs + K[0, 2]
    v = K[1, 1] * y / zs + K[1, 2]
    front = z > 0
    near_edge = (np.abs(u - np.round(u)) < 1e-3) | (np.abs(v - np.round(v)) < 1e-3)
    iu, iv = np.floor(u), np.floor(v)
    inimg = front & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
    px = np.where(inimg, iu, 0).astype(np.int64)
    py = np.where(inimg, iv, 0).astype(np.int64)
    sd = sd32[py, px].astype(np.float64)
    near_margin = inimg & (np.abs(z - sd - margin) < 1e-5 * np.maximum(1.0, z))
    # a vertex that no rounding can bring into the image, or in front of the camera, is decided whatever its u, v
    reach = front & (u > -1e-3) & (u < W + 1e-3) & (v > -1e-3) & (v < H + 1e-3)
    undecided = tiny | (near_edge & reach) | near_margin
    visible = inimg & mask[py, px] & ~undecided
    inside = visible & (z - sd > margin)
    outside = visible & ~inside
    pen = (v32[..., 2] - sd32[py, px]).astype(np.float32)          # the difference of two float32 values, correctly rounded
    extra = []
    for b in range(B):
        vals = []
        for k in np.nonzero(undecided[b] & front[b])[0]:
            for du in (-1e-3, 1e-3):
                for dv in (-1e-3, 1e-3):
                    cu, cv = int(np.floor(u[b, k] + du)), int(np.floor(v[b, k] + dv))
                    if 0 <= cu < W and 0 <= cv < H and mask[cv, cu]:
                        vals.append(np.float32(v32[b, k, 2] - sd32[cv, cu]))
        extra.append(np.asarray(vals, np.float32))
    return dict(inside=inside, outside=outside, undecided=undecided, pen=pen, extra=extra)


def check_verts(ref, pen_count, pen_max, margin=MARGIN):
    """|D| <= pen_count <= |D| + |U| and pen_max bit-equal to the float32 maximum over a set between D and D + U; raises
    AssertionError with the body and the numbers"""
    pen_count, pen_max = np.asarray(pen_count), np.asarray(pen_max, np.float32)
    for b in range(len(pen_count)):
        D, U = int(ref['inside'][b].sum()), int(ref['undecided'][b].sum())
        assert D <= pen_count[b] <= D + U, 'body %d: pen_count %d not in [%d, %d]' % (b, pen_count[b], D, D + U)
        mD = np.float32(ref['pen'][b][ref['inside'][b]].max()) if D else np.float32(0)
        ok = [mD] + [e for e in ref['extra'][b] if e > mD and e > np.float32(margin) - np.float32(1e-4)]
        assert any(pen_max[b].view(np.int32) == np.float32(c).view(np.int32) for c in ok), \
            'body %d: pen_max %r is none of %r' % (b, pen_max[b], ok[:8])
        if pen_count[b] == 0:
            assert pen_max[b] == 0


VERTEX_CASES = ['one', 'five', 'small', 'bodies', 'wide', 'zero_mask', 'none_inside']
STATISTICAL = ['small', 'bodies', 'wide']       # the cases large enough for the caps and the both-kinds minimum


def vertex_case(name):
    """(B,V) = (1,1), (1,5), (3,257), (8,6890) at 97x55 and (2,6890) at 240x135; an all-zero mask; a scene nobody reaches.
    Vertices uniform in a frustum slightly larger than the image (some outside every border), some with z <= 0; the scene
    depth a tilted plane plus noise, the mask random at 70 %."""
    B, V, W, H, seed = dict(one=(1, 1, 97, 55, 1), five=(1, 5, 97, 55, 2), small=(3, 257, 97, 55, 3), bodies=(8, 6890, 97, 55, 4),
                            wide=(2, 6890, 240, 135, 5), zero_mask=(3, 257, 97, 55, 6), none_inside=(3, 257, 97, 55, 7))[name]
    rng = np.random.RandomState(seed)
    f = 0.5 * H / np.tan(np.radians(30.0))
    K = np.float32([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]])
    yy, xx = np.mgrid[0:H, 0:W]
    scene_depth = (3.0 + 0.01 * xx - 0.02 * yy + rng.uniform(-0.05, 0.05, (H, W))).astype(np.float32)
    scene_mask = (rng.rand(H, W) < 0.7).astype(np.uint8)
    z = rng.uniform(1.5, 5.0, (B, V))
    z[rng.rand(B, V) < 0.05] *= -1.0
    z[rng.rand(B, V) < 0.002] = 0.0
    u = rng.uniform(-0.1 * W, 1.1 * W, (B, V))
    v = rng.uniform(-0.1 * H, 1.1 * H, (B, V))
    verts = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], -1).astype(np.float32)
    if name == 'one':                             # one vertex, half a metre inside the scene at a masked pixel
        scene_mask[20, 30] = 1
        zz = scene_depth[20, 30] + 0.5
        verts = np.float32([[[(30.4 - K[0, 2]) / K[0, 0] * zz, (20.6 - K[1, 2]) / K[1, 1] * zz, zz]]])
    if name == 'five':                            # inside, in front, behind the camera, off screen, on a masked-out pixel
        scene_mask[10, 10], scene_mask[11, 11], scene_mask[12, 12] = 1, 1, 0
        pt = lambda px, py, zz: [(px - K[0, 2]) / K[0, 0] * zz, (py - K[1, 2]) / K[1, 1] * zz, zz]
        verts = np.float32([[pt(10.5, 10.5, scene_depth[10, 10] + 0.3), pt(11.5, 11.5, scene_depth[11, 11] - 0.3),
                             pt(10.5, 10.5, -2.0), pt(-40.5, 10.5, 9.0), pt(12.5, 12.5, scene_depth[12, 12] + 0.3)]])
    if name == 'zero_mask':
        scene_mask[...] = 0
    if name == 'none_inside':
        scene_depth += np.float32(10.0)
    return dict(B=B, V=V, H=H, W=W, K=K, verts=verts, scene_depth=scene_depth, scene_mask=scene_mask, margin=MARGIN)


# ---- derived columns ---------------------------------------------------------------------------------------------------------

def project(points, K, Kd=None):
    """camera_projection of the reference (transforms.py:19-54) in float64: (...,3) -> (...,2) pixels"""
    p = np.asarray(points, np.float64)
    K = np.asarray(K, np.float64).reshape(3, 3)
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    if Kd is not None:
        Kd = np.asarray(Kd, np.float64)
        r = x * x + y * y
        radial = 1 + Kd[0] * r + Kd[1] * r * r + Kd[4] * r * r * r
        x, y = (x * radial + 2 * Kd[2] * x * y + Kd[3] * (r + 2 * x * x),
                y * radial + 2 * Kd[3] * y * y + Kd[2] * (r + 2 * y * y))      # (sic)
    return np.stack([K[0, 0] * x + K[0, 1] * y + K[0, 2], K[1, 0] * x + K[1, 1] * y + K[1, 2]], -1)


def reproj_ref(joints, K, Kd, pose2d, thr):
    """joints (...,J,3), pose2d (...,J,3) = x, y, confidence -> (mean px, max px, joints used) over confidence >= thr; a body
    without such a joint: NaN, NaN, 0"""
    uv = project(joints, K, Kd)
    p2 = np.asarray(pose2d, np.float64)
    dist = np.sqrt(((uv - p2[..., :2]) ** 2).sum(-1))
    use = np.asarray(pose2d, np.float32)[..., 2] >= np.float32(thr)
    n = use.sum(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n > 0, (dist * use).sum(-1) / np.maximum(n, 1), np.nan)
        worst = np.where(n > 0, np.where(use, dist, -np.inf).max(-1), np.nan)
    return mean, worst, n.astype(np.int64)


def derived_ref(counts, dsum):
    """mask_iou, depth_bias_m, depth_abs_m from the two outputs of the pixel kernel"""
    c = np.asarray(counts, np.float64)
    union = c[..., 0] + c[..., 1] - c[..., 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = np.where(union > 0, c[..., 2] / np.where(union > 0, union, 1), np.nan)
        bias = np.where(c[..., 2] > 0, np.asarray(dsum, np.float64)[..., 0] / np.where(c[..., 2] > 0, c[..., 2], 1), np.nan)
        absd = np.where(c[..., 2] > 0, np.asarray(dsum, np.float64)[..., 1] / np.where(c[..., 2] > 0, c[..., 2], 1), np.nan)
    return iou, bias, absd


def lowest_ref(verts):
    """argmax over the vertices of y (first index on ties) and that vertex: verts (...,V,3)"""
    idx = np.argmax(np.asarray(verts)[..., 1], axis=-1)
    low = np.take_along_axis(np.asarray(verts), idx[..., None, None], axis=-2)[..., 0, :]
    return idx, low


def contact_ref(verts, cloud, k=32):
    """dy of optimizer.py:487-506: (mean of the k nearest scene points).y - (lowest vertex).y, float64"""
    _, low = lowest_ref(verts)
    low = low.astype(np.float64)
    cloud = np.asarray(cloud, np.float64)
    flat = low.reshape(-1, 3)
    out = np.zeros(len(flat))
    for i, q in enumerate(flat):
        d2 = ((cloud - q) ** 2).sum(-1)
        near = np.argsort(d2, kind='stable')[:k]
        out[i] = cloud[near, 1].mean() - q[1]
    return out.reshape(low.shape[:-1])


def foot_slide_ref(verts, verts_prev):
    """|| v_low(t) - verts(t-1)[low_idx(t)] ||: verts, verts_prev (...,V,3) of frames t and t-1"""
    idx, low = lowest_ref(verts)
    prev = np.take_along_axis(np.asarray(verts_prev), idx[..., None, None], axis=-2)[..., 0, :]
    return np.sqrt(((low.astype(np.float64) - prev.astype(np.float64)) ** 2).sum(-1))
