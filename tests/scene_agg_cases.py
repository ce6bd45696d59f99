"""Inputs and plain numpy checkers for the device scene update (csrc/mh_sceneagg.hip, k_unproject of csrc/mh_scene.hip)
at the edges of its dispatch: the median over time around the 64-frame register slots, the <4> / <8> / <32>
instantiations of the pixel-major form and the LDS limit of the frame-major one; the fill at every window size, on
images smaller than the window, over many sweeps and with more listed pixels than threads; the un-projection with a
skewed K around its workgroup sizes; the post-processing on inputs whose edge decision float32 and float64 share.

Plain module (no pytest, no GPU, nothing from the product tree; the checkers are numpy and oracle/):
tests/test_scene_agg_cases.py proves that every case has the property it is built for,
tests/test_scene_agg_edges_gpu.py runs the kernels on them.
"""
import functools
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------
# median over time
# ---------------------------------------------------------------------------------------------------------------
MEDIAN_SHAPES = ((1, 1), (3, 7), (5, 13))                 # P = 1; 21: a partial group of four, a partial wave; 65: a second wave
T_PIXEL_MAJOR = (1, 2, 63, 64, 65, 255, 256, 257, 320, 511, 512, 513, 1000, 2047, 2048)      # mh_scene_median_t
T_FRAME_MAJOR = (1, 64, 65, 599, 600, 601, 700)                                              # mh_scene_median
T_ALL = tuple(sorted(set(T_PIXEL_MAJOR) | set(T_FRAME_MAJOR)))
T_REGISTER_FORM_MAX = 2048
T_LDS_MAX = 600                                           # T * 64 lanes * 4 B <= 150 KB
MEDIAN_MODES = ('depth', 'raw_int', 'raw_float')

MedianInputs = namedtuple('MedianInputs', 'vals back zmin zmax')


def depth_ranges(zmin, zmax):
    """optimizer.py:683-688 in float32: inv_min = 1 / min_z, inv_max = 1 / max_z"""
    f = np.float32
    min_z = np.log(f(1.0) + np.exp(zmin.astype(f))).astype(f)
    max_z = (min_z + f(1.0) + np.log(f(1.0) + np.exp(zmax.astype(f))).astype(f)).astype(f)
    return (f(1.0) / min_z).astype(f), (f(1.0) / max_z).astype(f)


@functools.lru_cache(maxsize=None)
def median_inputs(T, H, W, mode):
    """as tests/test_scene_agg_gpu.py::test_masked_median_over_time: 60 % of the frames valid, the first two rows
    quantised to quarters (ties), and from 21 pixels on one pixel that no frame sees, one that frame 0 alone sees, one
    that frames 0 and 1 see.  mode 'depth': normalised disparities in [0, 1] with per-frame depth ranges; 'raw_int':
    integer-valued planes 0..255, no ranges; 'raw_float': positive floats over four decades, no ranges."""
    rng = np.random.RandomState(1000 * MEDIAN_MODES.index(mode) + 7 * T + H)
    if mode == 'raw_int':
        vals = rng.randint(0, 256, (T, H, W)).astype(np.float32)
    else:
        vals = rng.uniform(0, 1, (T, H, W)).astype(np.float32)
        vals[:, :2] = np.round(vals[:, :2] * 4) / 4
        if mode == 'raw_float':
            vals = (np.float32(0.25) + vals) * (np.float32(10.0) ** rng.randint(-2, 3, (T, H, W))).astype(np.float32)
    back = (rng.uniform(0, 1, (T, H, W)) > 0.4).astype(np.uint8)
    if H * W >= 3:
        back[:, 0, 0] = 0
        back[1:, 0, 1] = 0
        back[0, 0, 1] = 1
        back[2:, 0, 2] = 0
        back[:2, 0, 2] = 1
    zmin = zmax = None
    if mode == 'depth':
        zmin = rng.uniform(0.5, 1.5, T).astype(np.float32)
        zmax = rng.uniform(4, 9, T).astype(np.float32)
    for a in (vals, back, zmin, zmax):
        if a is not None:
            a.setflags(write=False)
    return MedianInputs(vals, back, zmin, zmax)


@functools.lru_cache(maxsize=None)
def median_reference(T, H, W, mode):
    """(values float64, mask bool): depth mode -> oracle.scene_oracle.aggregate_scene_median on the float32 metric
    depths 1 / disp (values float32 there); raw modes -> np.ma.median of the values in float64"""
    from oracle import scene_oracle
    c = median_inputs(T, H, W, mode)
    if mode == 'depth':
        inv_min, inv_max = depth_ranges(c.zmin, c.zmax)
        disp = (c.vals * (inv_min - inv_max)[:, None, None] + inv_max[:, None, None]).astype(np.float32)
        depths = (np.float32(1.0) / disp).astype(np.float32)
        _, want, mask = scene_oracle.aggregate_scene_median(depths, None, c.back)
        mask = np.broadcast_to(np.asarray(mask, bool), (H, W)).copy()      # a median nothing is masked in has a scalar mask
        want = np.where(mask, want.astype(np.float64), 0.0)
    else:
        md = np.ma.median(np.ma.array(c.vals.astype(np.float64), mask=c.back == 0), axis=0)
        mask = c.back.max(axis=0) > 0
        want = np.where(mask, np.ma.getdata(md), 0.0)
    want.setflags(write=False)
    mask.setflags(write=False)
    return want, mask


GARBAGE = np.float32(7.0e8)           # under every masked frame of the constructed pixels: far above every valid value but 1e30


def _spread(T, n):
    """n distinct frame indices from 0 to T - 1, both ends included"""
    idx = np.unique(np.round(np.linspace(0, T - 1, n)).astype(np.int64))
    assert idx.size == n and idx[0] == 0 and idx[-1] == T - 1
    return idx


def _next(x, steps):
    x = np.float32(x)
    for _ in range(steps):
        x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    return x


def constructed_pixels(T):
    """raw mode, one pixel per pattern that T frames allow -> (names, vals (T, n) float32, back (T, n) uint8, expected
    (n) float32).  Every expected value is written down here; test_scene_agg_cases.py checks it against np.ma.median."""
    f = np.float32
    pix = []

    def add(name, frames, values, expected):
        v = np.full(T, GARBAGE, np.float32)
        b = np.zeros(T, np.uint8)
        v[np.asarray(frames)] = np.asarray(values, np.float32)
        b[np.asarray(frames)] = 1
        pix.append((name, v, b, f(expected)))

    add('first_only', [0], [7.25], 7.25)
    add('last_only', [T - 1], [6.5], 6.5)           # T = 65, 257, 513: alone in its register slot, beside clamped loads
    add('all_equal', np.arange(T), np.full(T, f(0.3)), f(0.3))                                  # vary == 0
    if T >= 2:
        add('two_distinct', [0, T - 1], [1.5, 4.0], 2.75)
    if T >= 3:
        add('last_three', [T - 3, T - 2, T - 1], [2.0, 3.0, 1.0], 2.0)      # the last frame is not the median
        x = f(1.5)
        add('adjacent_floats', _spread(T, 3), [_next(x, 2), x, _next(x, 1)], _next(x, 1))      # they differ in bits 0 and 1 only
    if T >= 4:
        s = _spread(T, 4)
        add('aabb', s, [2.0, 5.0, 5.0, 2.0], 3.5)       # the prefix never narrows to one value; lower middle != upper
        add('abbb', s, [5.0, 2.0, 5.0, 5.0], 5.0)       # even count, the two middles equal through a tie
        add('zero_lower_middle', s, [4.0, 0.0, 6.0, 0.0], 2.0)
    if T >= 5:
        add('wide_exponents', _spread(T, 5), [1e30, 1e-30, 1.0, 1e10, 1e-10], 1.0)
    names = [p[0] for p in pix]
    return names, np.stack([p[1] for p in pix], 1), np.stack([p[2] for p in pix], 1), np.array([p[3] for p in pix], np.float32)


# ---------------------------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------------------------
FILL_KSIZES = tuple(range(2, 12))
FILL_THREADS = {3: 1024, 5: 1024, 7: 1024, 9: 256, 11: 256}        # workgroup size per instantiation (ksize | 1)

FillCase = namedtuple('FillCase', 'name x mask ksize truncate')
FillRef = namedtuple('FillRef', 'x mask sweeps first_sweep')


def fill_reference(x, mask, ksize, truncate=False):
    """oracle.scene_oracle.fillin_values looped until the mask is full or a sweep fills nothing (the rule k_scene_fill
    states: the reference itself would loop for ever).  truncate: a filled value is floored when it is stored, so the
    next sweep reads the floored one.  -> (values, mask, sweeps that filled something, values after the first sweep
    before flooring)"""
    from oracle import scene_oracle
    x, mask = x.copy(), mask.copy()
    sweeps, first = 0, None
    while mask.min() == 0:
        nx, nm = scene_oracle.fillin_values(x, mask, filter_size=ksize)
        new = (nm > 0) & (mask == 0)
        if not new.any():
            break
        if first is None:
            first = nx.copy()
        if truncate:
            nx[new] = np.floor(nx[new])
        x, mask, sweeps = nx, nm, sweeps + 1
    return FillRef(x, mask, sweeps, first)


def _holes(rng, H, W, share, block=None):
    mask = (rng.uniform(0, 1, (H, W)) > share).astype(np.float32)
    if block is not None:
        y0, y1, x0, x1 = block
        mask[y0:y1, x0:x1] = 0
    return mask


def _fill_names():
    names = []
    for k in FILL_KSIZES:
        names += ['random_k%d' % k, 'columns_k%d' % k]
    names += ['row_1x9_k11', 'column_9x1_k11', 'tiny_2x3_k11', 'corner_40x40_k3',
              'dense_33x33_k7', 'dense_33x33_k11', 'sparse_33x33_k5', 'sparse_33x33_k9', 'full_mask_k7',
              'truncate_k6', 'truncate_k7', 'truncate_k11', 'nan_under_mask_k7', 'nan_under_mask_k11']
    return tuple(names)


FILL_NAMES = _fill_names()


def _build_fill(name):
    k = int(name[name.rindex('_k') + 2:])
    f = np.float32
    if name.startswith('random_k'):
        rng = np.random.RandomState(200 + k)
        x = rng.uniform(1, 9, (16, 30)).astype(f)
        mask = _holes(rng, 16, 30, 0.45, (4, 13, 9, 22))            # a 9 x 13 block: several sweeps at every window size
        x[mask == 0] = -100.0
        return x, mask, k, 0
    if name.startswith('columns_k'):
        import test_scene_oracle as tso
        x, mask, _ = tso.column_hole_case()
        return x, mask, k, 0
    if name in ('row_1x9_k11', 'column_9x1_k11', 'tiny_2x3_k11'):
        # the 11 x 11 window is larger than the image in both directions
        H, W = {'row_1x9_k11': (1, 9), 'column_9x1_k11': (9, 1), 'tiny_2x3_k11': (2, 3)}[name]
        x = np.full((H, W), -100.0, f)
        mask = np.zeros((H, W), f)
        valid = {'row_1x9_k11': [(0, 0)], 'column_9x1_k11': [(8, 0)], 'tiny_2x3_k11': [(1, 2), (0, 0)]}[name]
        for i, (r, c) in enumerate(valid):
            x[r, c], mask[r, c] = 2.5 + i, 1
        return x, mask, k, 0
    if name == 'corner_40x40_k3':
        x = np.full((40, 40), -100.0, f)
        mask = np.zeros((40, 40), f)
        x[0, 0], mask[0, 0] = 5.0, 1
        return x, mask, k, 0
    if name.startswith('dense_33x33') or name.startswith('sparse_33x33'):
        rng = np.random.RandomState(300 + k)
        x = rng.uniform(1, 9, (33, 33)).astype(f)
        mask = _holes(rng, 33, 33, 0.6 if name.startswith('dense') else 0.965)
        x[mask == 0] = -100.0
        return x, mask, k, 0
    if name == 'full_mask_k7':
        rng = np.random.RandomState(31)
        return rng.uniform(1, 9, (16, 30)).astype(f), np.ones((16, 30), f), k, 0
    if name.startswith('truncate_k'):
        rng = np.random.RandomState(400 + k)
        x = rng.randint(0, 256, (16, 30)).astype(f)
        mask = _holes(rng, 16, 30, 0.45, (4, 13, 9, 22))
        x[mask == 0] = -100.0
        return x, mask, k, 1
    if name.startswith('nan_under_mask_k'):
        rng = np.random.RandomState(500 + k)
        x = rng.uniform(1, 9, (16, 30)).astype(f)
        mask = _holes(rng, 16, 30, 0.45, (4, 13, 9, 22))
        x[mask == 0] = np.nan
        return x, mask, k, 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fill_case(name):
    x, mask, k, truncate = _build_fill(name)
    assert x.dtype == np.float32 and mask.dtype == np.float32 and x.shape == mask.shape
    assert (x[mask > 0] >= 0).all()
    x.setflags(write=False)
    mask.setflags(write=False)
    return FillCase(name, x, mask, k, truncate)


@functools.lru_cache(maxsize=None)
def fill_case_reference(name):
    c = fill_case(name)
    r = fill_reference(c.x, c.mask, c.ksize, bool(c.truncate))
    for a in r:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------------------------
# un-projection
# ---------------------------------------------------------------------------------------------------------------
POINTS_SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (3, 683))    # P = 1, 63, 64, 65, 1023, 1024, 1025, 2049
UNPROJECT_SHAPES = ((15, 17), (16, 16), (1, 257))                                            # P = 255, 256, 257
POINTS_MASKS = ('random', 'ones', 'zeros')
UNPROJECT_RTOL, UNPROJECT_ATOL = 2e-6, 1e-6       # tests/test_scene_agg_gpu.py::test_points_are_compacted_in_row_major_order


def skewed_K(H, W):
    """focal lengths of about 200, both off-diagonal terms of the 2 x 2 block set, principal point off the centre"""
    return np.array([[201.3, 3.7, 0.3 * W - 0.8], [-1.9, 198.6, 0.7 * H + 0.4], [0.0, 0.0, 1.0]], np.float32)


@functools.lru_cache(maxsize=None)
def unproject_case(H, W):
    """(depth (H, W) float32, K (3, 3) float32, points (H * W, 3) float64 by oracle.fit_oracle.unproject_points on the
    pixel centres (x + 0.5, y + 0.5, depth))"""
    import torch
    from oracle import fit_oracle
    rng = np.random.RandomState(H * 1000 + W)
    depth = rng.uniform(2, 9, (H, W)).astype(np.float32)
    K = skewed_K(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    uvd = np.stack([xs + 0.5, ys + 0.5, depth.astype(np.float64)], -1).reshape(1, H * W, 3)
    want = fit_oracle.unproject_points(torch.tensor(uvd, dtype=torch.float64), torch.tensor(K.astype(np.float64))[None])[0].numpy()
    for a in (depth, K, want):
        a.setflags(write=False)
    return depth, K, want


def unproject_float32(depth, K):
    """the same formula evaluated in float32 numpy, the 2 x 2 inverse formed in float64 and rounded as the entry points do"""
    f = np.float32
    H, W = depth.shape
    a, b, c, d = float(K[0, 0]), float(K[1, 0]), float(K[0, 1]), float(K[1, 1])
    det = a * d - b * c
    i00, i01, i10, i11 = f(d / det), f(-b / det), f(-c / det), f(a / det)
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs.astype(f) + f(0.5) - K[0, 2]).astype(f)
    v = (ys.astype(f) + f(0.5) - K[1, 2]).astype(f)
    x = (depth * ((u * i00).astype(f) + (v * i10).astype(f)).astype(f)).astype(f)
    y = (depth * ((u * i01).astype(f) + (v * i11).astype(f)).astype(f)).astype(f)
    return np.stack([x, y, depth], -1).reshape(H * W, 3)


def points_mask(H, W, kind):
    if kind == 'ones':
        return np.ones((H, W), np.float32)
    if kind == 'zeros':
        return np.zeros((H, W), np.float32)
    return (np.random.RandomState(H + W).uniform(0, 1, (H, W)) > 0.3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# post-processing
# ---------------------------------------------------------------------------------------------------------------
EDGE_MARGIN_MIN = 0.01
# (H, W, bilateral, seed); 5 x 5 is the legal minimum (reflection on both sides of every pixel), 5 x 51 / 16 x 16 / 13 x 20
# are P = 255 / 256 / 260: one and two partial sums of the Sobel kernel.  32 x 33 with the bilateral filter and 5 x 52 come
# within 1 % of the edge threshold at every seed tried and are left out.
POSTPROCESS_CASES = ((5, 5, 0, 1), (5, 5, 1, 1), (5, 51, 0, 1), (5, 51, 1, 1), (16, 16, 0, 1), (16, 16, 1, 1),
                     (9, 13, 0, 1), (9, 13, 1, 1), (13, 20, 0, 1), (13, 20, 1, 1), (45, 37, 0, 1), (45, 37, 1, 1),
                     (32, 33, 0, 1))
POSTPROCESS_VARIANT_SIZES = ((16, 16), (9, 13))          # also run with ma_mask = NULL and with fill windows 3 and 11


@functools.lru_cache(maxsize=None)
def postprocess_input(H, W, seed):
    """the scene of tests/test_scene_agg_gpu.py scaled to small images: a sloped, wavy background, a box 1.2 m in front
    of it, a hole in the middle and one in the corner (depth 0 under the holes), two masked pixels with a plain depth"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = 3.0 + 0.03 * ys + 0.5 * np.sin(xs / 9.0) + 0.01 * rng.randn(H, W)
    depth[H // 3:H // 2 + 1, W // 4:W // 3 + 1] -= 1.2
    mask = np.ones((H, W), np.float32)
    mask[H // 2:H // 2 + 3, W // 2:W // 2 + 2] = 0
    mask[0, 0] = 0
    depth = depth.astype(np.float32)
    depth[mask == 0] = 0.0
    mask[H - 1, 0:2] = 0                  # two masked pixels with their depth left in place: only the mask tells them apart
    depth.setflags(write=False)
    mask.setflags(write=False)
    return depth, mask


def edge_decision(depth, bilateral):
    """the intermediates of oracle.scene_oracle.postprocess_depthmap up to the edge mask, with the statistics (two
    standard deviations, the mean of grad) once in float32 as the checker has them and once in float64
    -> (edges32, edges64, margin = min |grad - thr| / thr over all pixels and both precisions)"""
    from oracle import scene_oracle as so
    depth = np.asarray(depth, np.float32)
    if bilateral:
        disp = so._bilateral(1.0 / np.clip(depth, 0.01, 100), 9, 0.05, 25)
        depth = 1.0 / np.clip(disp, 0.01, 100)
    disp = 1.0 / np.clip(depth, 0.1, 100)
    g_disp = np.abs(so._sobel(disp, 1, 0)) + np.abs(so._sobel(disp, 0, 1))
    g_depth = np.abs(so._sobel(depth, 1, 0)) + np.abs(so._sobel(depth, 0, 1))
    assert g_disp.dtype == np.float32 and g_depth.dtype == np.float32
    out, margin = [], np.inf
    for t in (np.float32, np.float64):
        a, b = g_disp.astype(t), g_depth.astype(t)
        grad = a / a.std() + b / b.std()
        thr = 3 * grad.mean()
        assert grad.dtype == t
        out.append(grad > thr)
        margin = min(margin, float(np.abs(grad.astype(np.float64) - float(thr)).min() / float(thr)))
    return out[0], out[1], margin


@functools.lru_cache(maxsize=None)
def postprocess_reference(H, W, bilateral, seed, with_mask=True, ksize=7):
    from oracle import scene_oracle as so
    depth, mask = postprocess_input(H, W, seed)
    want = so.postprocess_depthmap(depth, mask if with_mask else None, fillin_ksize=ksize, use_bilateral_filter=bool(bilateral))
    want = np.asarray(want, np.float32)
    want.setflags(write=False)
    return want
