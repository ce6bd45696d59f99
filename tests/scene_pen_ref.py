"""Numpy restatement of the scene-penetration term (``mh_scene_pen_term``, include/mhmocap_hip.h) and the cases its tests
run on.

``evaluate(..., dtype=np.float64)`` is the reference: the header's rules on the float32 inputs, in float64.
``evaluate(..., dtype=np.float32)`` is the same code with every operation in float32, in the order the header writes the
formulas (the per-body sum is ``np.sum`` in float32).  Its distance from the float64 result is the yardstick of the GPU
tests: the kernel may be off by 4x the largest such distance over the cases of this file (``budgets``).

A vertex is UNDECIDED -- float32 may take another branch than float64, so nothing is asserted about its GRADIENT -- when
  * ``a`` or ``b`` is within 1e-3 of 0 or 1 (the float32 projection is good to about 1e-4 px: other taps),
  * ``|p|`` or ``|p - band|`` is below 1e-5 (active or not),
  * the spread of the four taps is within 1e-5 of ``edge`` (skipped or not), or
  * ``|z|`` is below 1e-6.
The first rule is applied to vertices in front of the camera, the second and third where the taps exist.
The per-body VALUE is compared as it is, undecided vertices included: on every case of this file the float32 evaluation takes
the float64 branch for every vertex (tests/test_scene_pen_ref.py asserts it), so a value that differs by a vertex's p^2 is a
fault of the kernel and not a rounding matter.

Cases: (B,V) x (H,W) x map kind.  A case is FULL when it has at least 63 vertices and an image of at least 9 x 16: there the
seeds are chosen so that at most 2 % of the vertices are undecided and at least 20 are active (tests/test_scene_pen_ref.py
holds that on the reference alone).  With fewer vertices or a 1 x 1 / 2 x 2 image neither can be asked for: those cases are
there for the edges (one vertex; no tap inside a 1 x 1 image; one cell of taps in a 2 x 2 image).
"""
import numpy as np

COEF, MARGIN, BAND, EDGE = 0.7, 0.05, 0.5, 0.25
SHAPES = [(1, 1), (1, 63), (2, 64), (3, 65), (2, 257)]          # V = 65 and 257: a workgroup of 256 lanes straddles two bodies
IMAGES = [(1, 1), (2, 2), (9, 16), (135, 240)]                  # (H, W)
KINDS = ['floor', 'step', 'holes']
PLANE_N = np.array([0.1, 0.15, -1.0]) / np.linalg.norm([0.1, 0.15, -1.0])
PLANE_D = -3.0 / np.linalg.norm([0.1, 0.15, -1.0])              # n . X = d: depth 3 m on the optical axis


def evaluate(verts, K, zmap, coef=COEF, margin=MARGIN, band=BAND, edge=EDGE, dtype=np.float64, round_verts=True):
    """-> dict(value, body (B), vloss (B,V) each vertex's share of its body's value, grad (B,V,3), active, skipped, undecided
    (B,V), p (B,V)).  round_verts=False: float64 vertices are taken as they are (the
    finite differences of tests/test_scene_pen_ref.py)"""
    f = dtype
    c = lambda s: f(np.float32(s))                               # the kernel's scalars are float32
    v = (np.asarray(verts, np.float32) if round_verts else np.asarray(verts)).astype(f)
    B, V, _ = v.shape
    zm = np.asarray(zmap, np.float32).astype(f)
    H, W = zm.shape
    K = np.asarray(K, np.float32)
    fx, cx, fy, cy = c(K[0, 0]), c(K[0, 2]), c(K[1, 1]), c(K[1, 2])
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    front = z > 0
    with np.errstate(all='ignore'):
        zs = np.where(front, z, f(1))
        u = fx * x / zs + cx
        w = fy * y / zs + cy
        uc, wc = u - f(0.5), w - f(0.5)
        fi, fj = np.floor(uc), np.floor(wc)
        inimg = front & (fi >= 0) & (fi + f(1) <= f(W - 1)) & (fj >= 0) & (fj + f(1) <= f(H - 1))
        a, b = uc - fi, wc - fj
        i0 = np.where(inimg, fi, 0).astype(np.int64)
        j0 = np.where(inimg, fj, 0).astype(np.int64)
        i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
        D00, D10, D01, D11 = zm[j0, i0], zm[j0, i1], zm[j1, i0], zm[j1, i1]
        lo = np.minimum(np.minimum(D00, D10), np.minimum(D01, D11))
        hi = np.maximum(np.maximum(D00, D10), np.maximum(D01, D11))
        spread = hi - lo
        taps = inimg & (D00 > 0) & (D10 > 0) & (D01 > 0) & (D11 > 0)
        ok = taps & (spread <= c(edge))
        a1, b1 = f(1) - a, f(1) - b
        D = b1 * (a1 * D00 + a * D10) + b * (a1 * D01 + a * D11)
        Du = b1 * (D10 - D00) + b * (D11 - D01)
        Dv = a1 * (D01 - D00) + a * (D11 - D10)
        p = z - D - c(margin)
        active = ok & (p > 0) & (p < c(band))
        p2 = np.where(active, p * p, f(0)).astype(f)
        body = (c(coef) * np.sum(p2, axis=1, dtype=f) / f(V)).astype(f)
        g = f(2) * c(coef) * p / f(V)
        gx = -(g * Du * fx / zs)
        gy = -(g * Dv * fy / zs)
        gz = g * (f(1) + (Du * fx * x + Dv * fy * y) / (zs * zs))
        grad = np.where(active[..., None], np.stack([gx, gy, gz], -1), f(0)).astype(f)
        near = lambda t: (np.abs(t) < 1e-3) | (np.abs(t - 1) < 1e-3)
        undecided = (np.abs(z) < 1e-6) | (front & np.isfinite(u) & np.isfinite(w) & (near(a) | near(b)))
        undecided |= taps & (np.abs(spread - c(edge)) < 1e-5)
        undecided |= ok & ((np.abs(p) < 1e-5) | (np.abs(p - c(band)) < 1e-5))
    return dict(value=body.sum(dtype=f), body=body, grad=grad, active=active, skipped=~ok, p=np.where(ok, p, f(0)),
                sum_p2=np.sum(p2, axis=1, dtype=f), vloss=c(coef) * p2 / f(V), undecided=undecided)


def plane_depth(K, H, W, n=PLANE_N, d=PLANE_D):
    """depth of the plane n . X = d along the ray of every pixel centre (float64)"""
    K = np.asarray(K, np.float64)
    jj, ii = np.mgrid[0:H, 0:W]
    rx, ry = (ii + 0.5 - K[0, 2]) / K[0, 0], (jj + 0.5 - K[1, 2]) / K[1, 1]
    return d / (n[0] * rx + n[1] * ry + n[2])


def make_K(H, W):
    fl = 2.0 * max(H, W) + 4.0
    return np.float32([[fl, 0, W / 2.0], [0, fl, H / 2.0], [0, 0, 1]])


def make_map(kind, K, H, W, rng):
    z = plane_depth(K, H, W)
    if kind == 'step':          # the floor and, on the right half, a wall 0.6 m in front of it: a step of more than ``edge``
        z[:, W // 2:] = z.min() - 0.6
    elif kind == 'holes':       # a random scene mask: 0 = no scene
        z = np.where(rng.rand(H, W) < 0.08, 0.0, z)
    return z.astype(np.float32)


# full cases whose first seed leaves more than 2 % of the vertices undecided or fewer than 20 active: the next seed that does
# not (searched with the float64 reference alone)
RESEED = {(1, 63, 9, 16, 'holes'): 1}


def seed_of(B, V, H, W, kind):
    return 1000 * SHAPES.index((B, V)) + 10 * IMAGES.index((H, W)) + KINDS.index(kind) + 100 * RESEED.get((B, V, H, W, kind), 0)


def case(B, V, H, W, kind, seed=None):
    """vertices scattered over (and a little beyond) the image, in depth from 0.15 m in front of the surface + margin to
    0.15 m behind the band; one in thirty behind the camera"""
    rng = np.random.RandomState(seed_of(B, V, H, W, kind) if seed is None else seed)
    K = make_K(H, W)
    zmap = make_map(kind, K, H, W, rng)
    u = rng.uniform(-0.05 * W, 1.05 * W, (B, V))
    v = rng.uniform(-0.05 * H, 1.05 * H, (B, V))
    if H <= 2:                  # one cell of taps at most: most of the vertices aimed at it
        u, v = rng.uniform(0.4, W - 0.4, (B, V)), rng.uniform(0.4, H - 0.4, (B, V))
    surf = np.where(zmap > 0, zmap, plane_depth(K, H, W))[np.clip(np.floor(v).astype(int), 0, H - 1), np.clip(np.floor(u).astype(int), 0, W - 1)]
    z = surf + MARGIN + rng.uniform(-0.15, BAND + 0.15, (B, V))
    z = np.where(rng.rand(B, V) < 1 / 30.0, -z, z)
    verts = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], -1).astype(np.float32)
    return dict(B=B, V=V, H=H, W=W, kind=kind, K=K, zmap=zmap, verts=verts, full=B * V >= 63 and H >= 9)


def body_case(v_template):
    """two bodies of the synthetic model (6890 vertices each; y up -> the camera's y down), standing 0.3 m deep in a
    horizontal floor 0.8 m below the optical axis, 135 x 240"""
    H, W = 135, 240
    fl = 0.5 * H / np.tan(np.pi / 6)
    K = np.float32([[fl, 0, W / 2.0], [0, fl, H / 2.0], [0, 0, 1]])
    vt = np.asarray(v_template, np.float64) * np.array([1.0, -1.0, -1.0])
    feet = vt[:, 1].max()
    verts = np.stack([vt + np.array([-0.45, 0.8 + 0.3 - feet, 3.0]), vt + np.array([0.5, 0.8 + 0.3 - feet, 3.4])]).astype(np.float32)
    jj = np.arange(H)[:, None]
    ry = (jj + 0.5 - K[1, 2]) / K[1, 1]
    zmap = np.tile(np.where(ry > 1e-3, 0.8 / np.maximum(ry, 1e-3), 0.0), (1, W)).astype(np.float32)
    zmap[zmap > 10.0] = 0.0
    return dict(B=2, V=vt.shape[0], H=H, W=W, kind='body', K=K, zmap=zmap, verts=verts, full=True)


def all_cases():
    return {(B, V, H, W, k): case(B, V, H, W, k) for (B, V) in SHAPES for (H, W) in IMAGES for k in KINDS}


def errors(got_body, got_grad, r64):
    """distance of a result from the float64 reference: (value, gradient).  Value: the largest |body value - float64 body
    value|, relative to the value of the whole case (coef sum p^2 / V summed over the bodies; absolute when the case has no
    active vertex) -- every vertex counts, decided or not.  Gradient: decided vertices only, relative to the largest gradient
    entry of the case."""
    got = np.asarray(got_body, np.float64)
    scale = float(np.abs(r64['body']).sum())
    scale = scale if scale > 0 else 1.0
    ev = float(np.abs(got - r64['body']).max() / scale)
    dec = ~r64['undecided']
    if not dec.any():
        return ev, 0.0
    gs = float(np.abs(r64['grad'][dec]).max())
    gs = gs if gs > 0 else 1.0
    return ev, float(np.abs(np.asarray(got_grad, np.float64) - r64['grad'])[dec].max() / gs)


def budgets(cases):
    """the largest distance of the float32 evaluation from the float64 one over ``cases``: (value, gradient)"""
    bv = bg = 0.0
    for c in cases:
        r64 = evaluate(c['verts'], c['K'], c['zmap'])
        r32 = evaluate(c['verts'], c['K'], c['zmap'], dtype=np.float32)
        ev, eg = errors(r32['body'], r32['grad'], r64)
        bv, bg = max(bv, ev), max(bg, eg)
    return bv, bg
