"""Inputs of tests/test_raster_gpu.py that need no GPU: the scene, the instance masks and, for 9 to 32 people per frame, a
built layout with the conditions it has to meet (asserted from the oracle alone by tests/test_raster_cases.py and again, on the
oracle's side, inside the GPU test)."""
import numpy as np
import torch

from mhhip import synthetic
from oracle import fit_oracle as fo
from oracle import lbs_oracle as lo
from oracle import raster_oracle as ro

CROWDS = {                                 # name: the arguments of _run_case
    'n32': dict(T=1, N=32, W=160, H=90, seed=21, layout='rows'),
    'n9': dict(T=2, N=9, W=96, H=54, seed=22, layout='rows'),
    'n17': dict(T=1, N=17, W=96, H=54, seed=23, layout='rows'),
}


def rows_layout(T, N, W, H, fov=60.0):
    """(T,N,3) translations of N people standing in staggered rows on a stand, every row higher and half a place to the side of
    the one before it, which hides its legs.  Every person of a frame is at a depth of its own (the oracle orders by argsort, the
    kernel puts the lower index in front on a tie: they only agree without ties), and the person index does not follow the
    depth: person N - 1 stands nearest, in front of everybody."""
    cols = int(np.ceil(np.sqrt(2.0 * N)))
    tan = np.tan(np.pi * fov / 360.0) * W / min(W, H)          # half width of the view at depth 1
    z0 = 3.4 if min(W, H) >= 90 else 2.8                      # a small image: nearer, so that an eroded mask keeps pixels
    pitch = min(0.74, 1.7 * tan * z0 / cols)                   # shoulder to shoulder, within 85 % of the view at the first row
    pT = np.zeros((T, N, 3), np.float32)
    for n in range(N):
        slot = (5 * (N - 1 - n)) % N                            # 5 is coprime to 9, 17 and 32
        r, c = divmod(slot, cols)
        z = z0 + 0.9 * r + 0.013 * c
        x = (c - 0.5 * (cols - 1) + (0.5 if r % 2 else 0.0)) * pitch * (z / z0) * 0.93
        y = 0.55 - 0.62 * r                                     # y points down: the rows behind stand higher
        for t in range(T):
            pT[t, n] = (x + 0.03 * t, y, z + 0.002 * t * (1 if n % 2 else -1))
    return pT


def _scene(T, N, W, H, seed, zlo, zhi, layout=None, fov=60.0):
    rng = np.random.RandomState(seed)
    sp = synthetic.make_sequence_params(N, T, seed)
    pT = sp['trans_gt'].copy()
    pT[..., 2] = rng.uniform(zlo, zhi, (T, N))
    pT[..., 0] = rng.uniform(-0.25, 0.25, (T, N)) * pT[..., 2]
    pT[..., 1] = rng.uniform(-0.05, 0.1, (T, N))
    if layout == 'rows':
        pT = rows_layout(T, N, W, H, fov)
    elif layout is not None:
        pT = np.asarray(layout, np.float32).reshape(T, N, 3)
    return sp, pT.astype(np.float32), rng


def inputs(smpl_struct, smpl_regs, T, N, W, H, seed, zlo=3.0, zhi=6.0, fov=60.0, layout=None):
    """Everything a case stages, drawn in the order tests/test_raster_gpu.py has always drawn it.  With a layout every mask and
    every 2D pose stays valid; without one person 0 of frame 0 has an empty mask and the last person of frame 1 no 2D pose."""
    K = synthetic.default_cam_K((W, H), fov)
    sp, pT, rng = _scene(T, N, W, H, seed, zlo, zhi, layout, fov)
    omodel = lo.BodyModel(smpl_struct, smpl_regs)
    faces = np.asarray(smpl_struct.f).astype(np.int64)
    betas = sp['betas_gt']
    zmin = rng.uniform(0.5, 1.5, T).astype(np.float32)
    zmax = rng.uniform(4.0, 9.0, T).astype(np.float32)
    xscale = rng.normal(0, 0.5, N).astype(np.float32)
    if layout is not None:
        xscale = (0.2 * xscale).astype(np.float32)             # sizes within a few per cent: the rows stay rows
    # masks: silhouette of a slightly different pose, so that alpha - seg is non-trivial
    with torch.no_grad():
        be = torch.tensor(betas)[None].expand(T, N, 10).reshape(-1, 10)
        out = lo.smpl_forward(omodel, be, torch.tensor(sp['poses_init']).view(-1, 72))
        s = torch.pow(torch.tensor(1.1), torch.tensor(xscale))[None, :, None, None]
        v0 = s * out['verts'].view(T, N, -1, 3) + torch.tensor(pT).view(T, N, 1, 3) + torch.tensor([0.03, -0.02, 0.0])
        _, a0 = ro.render(v0.view(T * N, -1, 3), faces, K, (W, H))
    seg = (a0.view(T, N, H, W) > 0.5).float().numpy()
    pose2d = np.zeros((T, N, 17, 3), np.float32)
    pose2d[..., 2] = 0.9
    if layout is None:
        seg[0, 0] = 0                                              # an empty mask
    depths = rng.uniform(0, 1, (T, H, W)).astype(np.float32)
    if layout is None and T > 1:
        pose2d[1, N - 1, :, 2] = 0.1                               # a body without a valid 2D pose
    return dict(K=K, sp=sp, pT=pT, omodel=omodel, faces=faces, betas=betas, zmin=zmin, zmax=zmax, xscale=xscale, seg=seg,
                depths=depths, pose2d=pose2d)


def oracle_verts(inp):
    """the fitted bodies' vertices as the engine's forward computes them, from the oracle's LBS (float32, CPU)"""
    T, N = inp['pT'].shape[:2]
    with torch.no_grad():
        be = torch.tensor(inp['betas'])[None].expand(T, N, 10).reshape(-1, 10)
        out = lo.smpl_forward(inp['omodel'], be, torch.tensor(inp['sp']['poses_gt']).view(-1, 72))
        s = torch.pow(torch.tensor(1.1), torch.tensor(inp['xscale']))[None, :, None, None]
        return (s * out['verts'].view(T, N, -1, 3) + torch.tensor(inp['pT']).view(T, N, 1, 3)).view(T * N, -1, 3)


def crowd_conditions(seg, pT, pose2d, zbuf, alpha):
    """What a crowd case has to contain, from the masks, the translations and the ORACLE's render (zbuf, alpha: (T,N,H,W)) of
    the fitted bodies -- nothing of the kernel's.  -> a line of figures for pytest -s"""
    T, N, H, W = seg.shape
    seg = np.asarray(seg) > 0.5
    z = np.asarray(pT)[..., 2]
    tseg = torch.tensor(seg, dtype=torch.float32)
    er = fo.erode3x3(fo.erode3x3(tseg)).numpy() > 0.5
    p2d_valid = (np.asarray(pose2d)[..., 2] >= 0.5).sum(-1) >= 2
    zbuf, alpha = np.asarray(zbuf), torch.as_tensor(np.asarray(alpha, np.float32))
    figures = []
    for t in range(T):
        assert len(set(z[t].tolist())) == N, 'two people of a frame at one depth'
        assert (seg[t].sum(axis=(1, 2)) >= 0.005 * H * W).all(), 'a person without a valid mask'
        free, partly = np.zeros(N, int), np.zeros(N, bool)
        for n in range(N):
            cover = np.zeros((H, W), bool)
            for m in range(N):
                if z[t, m] < z[t, n]:
                    cover |= seg[t, m]
            free[n] = int((seg[t, n] & ~cover).sum())
            partly[n] = 0 < free[n] < seg[t, n].sum()
        seen = free >= 20
        must = sorted(set([N - 1] + ([8, 16, 31] if N == 32 else [])))
        assert seen.sum() * 4 >= 3 * N, 'only %d of %d people have 20 mask pixels nobody in front covers' % (seen.sum(), N)
        assert seen[must].all(), 'people %s must be seen: free pixels %s' % (must, free[must].tolist())
        assert partly.sum() * 4 >= N, 'only %d of %d people are partly covered' % (partly.sum(), N)
        # person N - 1: bit 31 of bits / ebits / front at N = 32
        n = N - 1
        acc = torch.tensor(np.any([seg[t, m] for m in range(N) if z[t, m] < z[t, n]] + [np.zeros((H, W), bool)], axis=0), dtype=torch.float32)
        sil = float(fo.masked_mse_loss(alpha[t, n], tseg[t, n], 1 - acc))
        ndepth = int(((zbuf[t, n] > 0) & er[t, n]).sum()) * int(p2d_valid[t, n])
        behind = int((z[t] > z[t, n]).sum())
        assert sil > 0, 'person N - 1 has no silhouette residual'
        assert ndepth > 0, 'person N - 1 has no eroded-mask depth pixel'
        assert behind >= 1, 'person N - 1 is in front of nobody'
        figures.append('frame %d: %d of %d seen (fewest free pixels of %s: %d), %d partly covered, person %d: silhouette %.3g, '
                       '%d depth pixels, in front of %d' % (t, seen.sum(), N, must, free[must].min(), partly.sum(), n, sil, ndepth, behind))
    return '; '.join(figures)
