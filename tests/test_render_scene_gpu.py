"""The scene renderer (``mh_scene_composite`` / ``mhhip.raster.render_scene`` / ``SMPLDepthSequenceOptimizer.render_scene``)
on small synthetic scenes: 240x135, a square 256x256 and an odd 97x55 image (whose pixel count is no multiple of four: the
overlay's byte path), 1, 2 and 4 people, one sequence longer than ``chunk``, bodies at the image border and off screen.

The composite (depth, person, face), visibility and coverage are exact: they are compared bit for bit with a numpy
construction from the per-body images of ``raster.render`` and the keys of ``RasterTerms.selection``.

Normals: the tolerance is not chosen in advance.  The same formula is evaluated in numpy float32 and float64 on the
scenes of this file (from the same float32 vertices and the kernel's own face map); the kernel may be off by 4x the largest
float32 component error (operation order, fused multiply-adds).  Faces whose float64 cross product is shorter than 1e-12 are
left out, at most 0.1 % of the covered pixels.  On the CPU (the oracle's LBS on the poses of these scenes, all 13776 faces
of the synthetic capsule, every body): 0 faces below 1e-12, the shortest cross product is 2.3e-7 -- nothing is excluded.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xffffffffffffffff)
LIGHT = np.asarray([0.3, -0.4, 0.8660254], np.float32)
LIGHT = LIGHT / np.linalg.norm(LIGHT)
AMBIENT, ALPHA = 0.25, 0.7


def scene_params(name):
    """(W, H, T, N, chunk, poses (T,N,72), translations (T,N,3), betas (N,10)) of the scenes of this file"""
    from mhhip import synthetic
    W, H, T, N, chunk, seed = dict(wide=(240, 135, 3, 4, 32, 11), square=(256, 256, 2, 2, 32, 12), odd=(97, 55, 5, 1, 2, 13),
                                   odd4=(97, 55, 2, 4, 32, 14))[name]
    rng = np.random.RandomState(seed)
    sp = synthetic.make_sequence_params(N, T, seed)
    pT = np.zeros((T, N, 3), np.float32)
    pT[..., 2] = rng.uniform(2.6, 5.0, (T, N))
    pT[..., 0] = rng.uniform(-0.25, 0.25, (T, N)) * pT[..., 2]
    pT[..., 1] = rng.uniform(-0.05, 0.1, (T, N))
    poses = sp['poses_gt'].copy()
    if name == 'wide':
        pT[0, 2, 0] = 1.0 * pT[0, 2, 2]            # across the right border: a clipped window
        pT[1, 3, 0] = 5.0 * pT[1, 3, 2]            # off screen: an empty window
        pT[2, 1] = pT[2, 0] + np.float32([0.05, 0.0, 0.4])      # overlapping bodies
    if name == 'square':
        poses[:, 1] = poses[:, 0]                  # two identical bodies ...
        pT[:, 0] = np.float32([0.3, 0.1, 3.0])
        pT[:, 1] = pT[:, 0] + np.float32([0.0, 0.0, 1.0])       # ... the second 1 m further back
    return W, H, T, N, chunk, poses, pT, sp['betas_gt']


def _cross_normals(verts, faces, person, face, dtype):
    """unit normal (v1-v0)x(v2-v0) of the face of every covered pixel, n_z <= 0, in ``dtype``; (pixels (t,y,x), normals,
    length of the cross product)"""
    tt, yy, xx = np.nonzero(person >= 0)
    tri = faces[face[tt, yy, xx]]
    v = verts.astype(dtype)
    nn = person[tt, yy, xx]
    v0, v1, v2 = (v[tt, nn, tri[:, k]] for k in range(3))
    c = np.cross(v1 - v0, v2 - v0)
    ln = np.sqrt((c * c).sum(-1))
    n = c / np.where(ln > 0, ln, 1)[:, None]
    n = np.where(n[:, 2:3] > 0, -n, n)
    return (tt, yy, xx), n, ln


@pytest.fixture(scope='module')
def scenes(smpl_struct, smpl_regs):
    """every scene rendered once: vertices, inputs, all outputs of render_scene, and the numpy composite of the per-body
    images of raster.render with the keys of RasterTerms.selection"""
    import types
    import torch
    from mhhip import engine, raster, synthetic, _lib
    from mhhip._lib import check, ptr
    model = engine.BodyModel(smpl_struct, smpl_regs)
    faces = np.asarray(smpl_struct.f).astype(np.int64)
    dev = model.device
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    out = {}
    for name in ('wide', 'square', 'odd', 'odd4'):
        W, H, T, N, chunk, poses, pT, betas = scene_params(name)
        K = synthetic.default_cam_K((W, H), 60.0)
        verts, _, _, _ = model.lbs_forward(t(betas), t(poses).view(T * N, 72), None, t(pT).view(T * N, 3), want_vposed=False)
        verts = verts.view(T, N, -1, 3).clone()
        if name == 'square':
            # frame 1: the second body becomes a copy of the first at a third of its size, half as far again along the ray
            # through its centre: it projects well inside the first body's silhouette, fully hidden
            c = verts[1, 0].mean(0, keepdim=True)
            verts[1, 1] = 1.5 * c + 0.5 * (verts[1, 0] - c)
        rng = np.random.RandomState(100 + T * N)
        images = rng.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
        palette = rng.uniform(0.1, 1.0, (N, 3)).astype(np.float32)
        got = raster.render_scene(model, verts, K, (W, H), images=images, palette=palette, light=LIGHT, ambient=AMBIENT,
                                  alpha=ALPHA, chunk=chunk)
        black = raster.render_scene(model, verts, K, (W, H), images=None, palette=palette, light=LIGHT, ambient=AMBIENT,
                                    alpha=ALPHA, chunk=chunk, outputs=('overlay',))
        # ---- per-body images and keys of the existing rasteriser -------------------------------------------------------------
        B, V = T * N, verts.shape[2]
        zbuf, _ = raster.render(model, verts.view(B, V, 3), K, (W, H))
        fake = types.SimpleNamespace(dev=dev, m=types.SimpleNamespace(faces=faces), T=B, N=1, V=V, H=H, W=W, B=B,
                                     K=np.asarray(K, np.float32))
        rt = raster.RasterTerms(fake)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        zf = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        bits, depths, tz, ones = zi(B, H, W), zf(B, H, W), zf(B), torch.ones(B, device=dev)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        check(_lib.lib().mh_raster_terms(B, 1, V, faces.shape[0], H, W, Kh.ctypes.data_as(_lib.c_float_p), ptr(verts.view(B, V, 3)),
                                         ptr(rt.faces), ptr(bits), ptr(bits), ptr(depths), ptr(tz), ptr(tz), ptr(ones), ptr(zi(B)),
                                         ptr(tz), ptr(ones), ptr(tz), 0.0, 0.0, 1e-3, None, None, None, ptr(zf(B)), ptr(zf(B)),
                                         ptr(rt.ws), None, None, _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        win, koff, keys = rt.selection(fake)
        zb = zbuf.cpu().numpy()
        kz = np.full((B, H, W), -1.0, np.float32)
        kf = np.full((B, H, W), -1, np.int32)
        for b in range(B):
            x0, y0, ww, wh = (int(v) for v in win[b])
            if ww <= 0 or wh <= 0:
                continue
            k = keys[koff[b]:koff[b + 1], 0].reshape(wh, ww)
            ok = k != EMPTY
            z = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
            f = (k & np.uint64(0xffffffff)).astype(np.int64)
            kz[b, y0:y0 + wh, x0:x0 + ww] = np.where(ok, z, np.float32(-1))
            kf[b, y0:y0 + wh, x0:x0 + ww] = np.where(ok, f, -1)
        assert np.array_equal(kz.view(np.int32), zb.view(np.int32)), 'raster.render and the selection keys disagree'
        zb, kf = zb.reshape(T, N, H, W), kf.reshape(T, N, H, W)
        valid = kf >= 0
        zinf = np.where(valid, zb, np.float32(np.inf))
        who = np.argmin(zinf, axis=1)                         # the first minimum: the lower person index wins a tie
        cov = valid.any(axis=1)
        take = lambda a: np.take_along_axis(a, who[:, None], axis=1)[:, 0]
        want = dict(depth=np.where(cov, take(zb), np.float32(-1)).astype(np.float32),
                    person=np.where(cov, who, -1).astype(np.int32), face=np.where(cov, take(kf), -1).astype(np.int32))
        out[name] = dict(W=W, H=H, T=T, N=N, K=K, model=model, faces=faces, verts=verts, verts_np=verts.cpu().numpy(),
                         images=images, palette=palette, got={k: v.cpu().numpy() for k, v in got.items()},
                         black=black['overlay'].cpu().numpy(), black_keys=sorted(black), want=want, alone=zb)
    return out


NAMES = ['wide', 'square', 'odd', 'odd4']


@pytest.mark.parametrize('name', NAMES)
def test_composite_is_exact(scenes, name):
    """(a) depth, person and face against the numpy composite: a minimum over identical floats, no tolerance"""
    s = scenes[name]
    got, want = s['got'], s['want']
    assert got['depth'].shape == (s['T'], s['H'], s['W']) and got['depth'].dtype == np.float32
    assert got['person'].dtype == np.int32 and got['face'].dtype == np.int32
    covered = int((want['person'] >= 0).sum())
    print('%s: %d of %d pixels covered, people seen: %s' % (name, covered, want['person'].size, np.unique(want['person'])))
    assert covered > 200
    assert np.array_equal(got['person'], want['person'])
    assert np.array_equal(got['face'], want['face'])
    assert np.array_equal(got['depth'].view(np.int32), want['depth'].view(np.int32))
    if name == 'wide':
        assert (s['alone'][1, 3] == -1).all(), 'the off-screen body of this scene must have an empty window'
        assert (s['alone'][0, 2][:, [0, -1]] > 0).any(), 'the body across the border must reach the first or last column'


def test_occlusion_order_and_coverage(scenes):
    """(b) two identical bodies, the second 1 m further back"""
    from mhhip import raster
    s = scenes['square']
    person, cov = s['got']['person'][0], s['got']['coverage'][0]
    near_alone, far_alone = s['alone'][0, 0] > -1, s['alone'][0, 1] > -1
    assert near_alone.sum() > 500 and far_alone.sum() > 300
    assert (person[near_alone] == 0).all()
    alone = raster.render_scene(s['model'], s['verts'][:1, 1:2], s['K'], (s['W'], s['H']), outputs=('coverage',))
    alone = int(alone['coverage'].cpu().numpy()[0, 0])
    print('far body: %d pixels alone, %d behind the near one' % (alone, cov[1]))
    assert alone == int(far_alone.sum()) and 0 <= cov[1] < alone


@pytest.mark.parametrize('name', NAMES)
def test_coverage_is_the_bincount_of_person(scenes, name):
    s = scenes[name]
    person, cov = s['got']['person'], s['got']['coverage']
    assert cov.shape == (s['T'], s['N']) and cov.dtype == np.int32
    for t in range(s['T']):
        assert np.array_equal(cov[t], np.bincount(person[t][person[t] >= 0], minlength=s['N']))


@pytest.fixture(scope='module')
def normal_budget(scenes):
    """the largest component error of the float32 numpy evaluation of the normal formula against float64, over all scenes"""
    worst = 0.0
    for name in NAMES:
        s = scenes[name]
        _, n32, _ = _cross_normals(s['verts_np'], s['faces'], s['got']['person'], s['got']['face'], np.float32)
        _, n64, ln = _cross_normals(s['verts_np'], s['faces'], s['got']['person'], s['got']['face'], np.float64)
        keep = ln >= 1e-12
        worst = max(worst, float(np.abs(n32[keep].astype(np.float64) - n64[keep]).max()))
    return worst


@pytest.mark.parametrize('name', NAMES)
def test_normals(scenes, normal_budget, name):
    """(c) against float64 from the same vertices and the kernel's own face map, within 4x the float32 formula's own error"""
    s = scenes[name]
    got = s['got']['normal'].astype(np.float64)
    person = s['got']['person']
    (tt, yy, xx), n64, ln = _cross_normals(s['verts_np'], s['faces'], person, s['got']['face'], np.float64)
    keep = ln >= 1e-12
    n = got[tt, yy, xx]
    err = float(np.abs(n[keep] - n64[keep]).max())
    print('%s: kernel normal error %.3e, numpy float32 error (all scenes) %.3e, %d of %d covered pixels excluded'
          % (name, err, normal_budget, int((~keep).sum()), keep.size))
    assert (~keep).sum() <= 0.001 * keep.size
    assert err <= 4 * normal_budget
    assert (n[keep][:, 2] <= 0).all()
    assert np.abs(np.sqrt((n[keep] ** 2).sum(-1)) - 1).max() <= 1e-6      # a few float32 roundings of the normalisation
    assert (got[person < 0] == 0).all()


@pytest.mark.parametrize('name', NAMES)
def test_overlay(scenes, name):
    """(d) the blend formula in float64 from the kernel's own person and normal maps"""
    s = scenes[name]
    person, normal = s['got']['person'], s['got']['normal'].astype(np.float64)
    shade = AMBIENT + (1 - AMBIENT) * np.maximum(0.0, -(normal * LIGHT.astype(np.float64)).sum(-1))
    colour = 255.0 * s['palette'].astype(np.float64)[np.maximum(person, 0)] * shade[..., None]
    empty = person < 0
    for img, got in ((s['images'], s['got']['overlay']), (np.zeros_like(s['images']), s['black'])):
        want = np.clip((1 - ALPHA) * img.astype(np.float64) + ALPHA * colour, 0, 255)
        assert got.dtype == np.uint8 and got.shape == img.shape
        diff = np.abs(got.astype(np.float64) - want)[~empty]
        print('%s: overlay off by at most %.3f levels on %d covered pixels' % (name, diff.max(), (~empty).sum()))
        assert diff.max() <= 1.0
        assert np.array_equal(got[empty], img[empty])
    assert (s['black'][empty] == 0).all()
    assert (shade[~empty] > AMBIENT + 0.05).any(), 'the light of this file must shade some pixels'


@pytest.mark.parametrize('name', NAMES)
def test_visibility(scenes, name):
    """(e) the vertices of the faces that own a pixel, exactly"""
    s = scenes[name]
    person, face, vis = s['got']['person'], s['got']['face'], s['got']['visible']
    want = np.zeros_like(vis)
    tt, yy, xx = np.nonzero(person >= 0)
    tri = s['faces'][face[tt, yy, xx]]
    for k in range(3):
        want[tt, person[tt, yy, xx], tri[:, k]] = 1
    assert vis.dtype == np.uint8 and vis.shape == (s['T'], s['N'], s['verts_np'].shape[2])
    assert np.array_equal(vis, want)
    assert vis.sum() > 0
    if name == 'square':
        assert s['got']['coverage'][1, 1] == 0 and vis[1, 1].sum() == 0, 'a fully hidden body has no visible vertex'
        assert vis[1, 0].sum() > 100
    if name == 'wide':
        assert vis[1, 3].sum() == 0            # off screen


def test_outputs_limit_what_is_returned(scenes):
    """(g) outputs=('depth',) allocates and returns only that"""
    from mhhip import raster
    s = scenes['odd']
    assert s['black_keys'] == ['overlay']
    got = raster.render_scene(s['model'], s['verts'], s['K'], (s['W'], s['H']), outputs=('depth',), chunk=2)
    assert sorted(got) == ['depth']
    assert np.array_equal(got['depth'].cpu().numpy().view(np.int32), s['got']['depth'].view(np.int32))
    with pytest.raises(ValueError):
        raster.render_scene(s['model'], s['verts'], s['K'], (s['W'], s['H']), outputs=('colour',))


def test_scene_composite_argument_checks(scenes):
    from mhhip import _lib
    L = _lib.lib()
    assert L.mh_scene_composite(1, 1, 10, 10, 8, 8, *([None] * 5), None, 0.3, 0.6, *([None] * 8)) != 0
    assert b'output' in L.mh_last_error()


# ---- through the optimiser -------------------------------------------------------------------------------------------------

LEAVES = ['poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale']


def _optimiser(smpl_struct, smpl_regs, oracle_model, tmp_path, seed):
    from test_fit_full_gpu import _setup
    T, N, W, H, batch = 4, 2, 96, 54, 2
    opt, dl, _, _, seq = _setup(smpl_struct, smpl_regs, oracle_model, tmp_path, T, N, W, H, batch, seed, False)
    return opt, dl, seq


def test_optimiser_render_scene_reads_only(smpl_struct, smpl_regs, oracle_model, tmp_path):
    """(f), (g): the optimiser's method equals render_scene on the vertices of those frames, leaves untouched"""
    import torch
    from mhhip import raster
    opt, dl, seq = _optimiser(smpl_struct, smpl_regs, oracle_model, tmp_path, 41)
    with pytest.raises(ValueError):
        opt.render_scene(frames=[0, 4])
    with pytest.raises(ValueError):
        opt.render_scene(frames=[-1])
    opt.fit(dl, num_iter=3)
    e = opt.engine
    before = {k: e.leaf(k).clone() for k in LEAVES}
    grads = e.grads.clone()
    got = opt.render_scene(frames=[0, 3], light=LIGHT)
    torch.cuda.synchronize()
    for k in LEAVES:
        assert torch.equal(e.leaf(k), before[k]), k
    assert torch.equal(e.grads, grads)
    assert np.array_equal(got['frames'], [0, 3])
    fr = torch.as_tensor([0, 3], device=e.dev)
    T, N = 4, 2
    verts, _, _, _ = opt.SMPLPY.body_model.lbs_forward(e.leaf('betas'), e.leaf('poses_smpl')[fr].reshape(2 * N, 72), e.leaf('xscale'),
                                                       e.leaf('poses_T')[fr].reshape(2 * N, 3), want_vposed=False)
    want = raster.render_scene(opt.SMPLPY.body_model, verts.view(2, N, -1, 3), opt.cam_K, (96, 54), images=seq['images'][[0, 3]],
                               light=LIGHT)
    assert sorted(got) == sorted(list(want) + ['frames'])
    for k, v in want.items():
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], v.cpu().numpy()), k
    assert (got['person'] >= 0).sum() > 100
    # the staged frames are the background; images=False: black
    empty = got['person'] < 0
    assert np.array_equal(got['overlay'][empty], seq['images'][[0, 3]][empty])
    assert (opt.render_scene(frames=[3], images=False, outputs=('overlay', 'person'))['overlay'][empty[1:]] == 0).all()
    assert sorted(opt.render_scene(outputs=('depth',))) == ['depth', 'frames']
    opt._world = lambda: (2, 0)                 # a frame-sharded run is refused
    with pytest.raises(RuntimeError, match='shard'):
        opt.render_scene()


def _child(out_path, tmp_root):
    """fit(k) -> fit(k) and fit(k) -> render_scene() -> fit(k) on two optimisers with the same start (the process was started
    with MHHIP_DETERMINISTIC=1): log rows and leaves of the second fit of both, for the parent to compare"""
    import pathlib
    import conftest  # noqa: F401  (the suite's import paths)
    import torch
    from mhhip import synthetic
    from oracle import lbs_oracle
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    omodel = lbs_oracle.BodyModel(struct, regs)
    res = {}
    for tag in ('plain', 'render'):
        tmp = pathlib.Path(tmp_root) / tag
        tmp.mkdir()
        opt, dl, _ = _optimiser(struct, regs, omodel, tmp, 43)
        opt.fit(dl, num_iter=3)
        if tag == 'render':
            assert (opt.render_scene()['person'] >= 0).any()
        log = opt.fit(dl, num_iter=3)
        torch.cuda.synchronize()
        keys = sorted(log[0])
        res[tag + '_log'] = np.asarray([[row[k] for k in keys] for row in log], np.float64)
        for k in LEAVES:
            res[tag + '_' + k] = opt.engine.leaf(k).cpu().numpy()
    np.savez(out_path, **res)


def test_fit_is_the_same_with_a_render_in_between(tmp_path):
    """(f) under MHHIP_DETERMINISTIC=1, set for a fresh child process: a render between two fits changes no bit of the second"""
    out = str(tmp_path / 'runs.npz')
    env = dict(os.environ, MHHIP_DETERMINISTIC='1')
    p = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out, str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = np.load(out)
    assert r['plain_log'].shape[0] == 3 and np.isfinite(r['plain_log']).all()
    assert np.array_equal(r['plain_log'], r['render_log']), json.dumps(dict(plain=r['plain_log'].tolist(), render=r['render_log'].tolist()))
    for k in LEAVES:
        assert np.array_equal(r['plain_' + k].view(np.int32), r['render_' + k].view(np.int32)), k


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2])
