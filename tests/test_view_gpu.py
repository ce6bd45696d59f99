"""The free-viewpoint renderer (``mh_view_*`` / ``mhhip.view.render_view`` / ``SMPLDepthSequenceOptimizer.render_view``) on
the device.  Only the projection is float32 (compared with float64 within one fixed-point unit); rasterisation, splatting
and the resolve are integer arithmetic and are compared with the numpy restatement tests/view_ref.py BIT FOR BIT, the
kernels being fed their own snapped coordinates.  No tolerance, no excluded pixels."""
import numpy as np
import pytest

import view_ref as vr

pytestmark = pytest.mark.gpu

NEAR = 0.5
LIGHT = np.asarray([0.3, -0.4, 0.8660254], np.float32)
LIGHT = LIGHT / np.linalg.norm(LIGHT)
AMBIENT = 0.25
BACKGROUND = (250, 240, 230)


def _fp(a):
    from mhhip import _lib
    return a.ctypes.data_as(_lib.c_float_p)


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype))).to('cuda:0')


def gpu_project(xyz, R, t, K, near, per_view):
    """xyz (rows,3) -> int32 (Tv, count, 3) through mh_view_project"""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    R, t = np.ascontiguousarray(R, np.float32).reshape(-1, 3, 3), np.ascontiguousarray(t, np.float32).reshape(-1, 3)
    Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
    Tv = len(R)
    x = _dev(xyz, np.float32).view(-1, 3)
    count = int(x.shape[0]) // Tv if per_view else int(x.shape[0])
    out = torch.full((Tv, count, 3), 7, dtype=torch.int32, device=x.device)
    check(_lib.lib().mh_view_project(count, int(per_view), Tv, ptr(x), _fp(R), _fp(t), _fp(Kh), float(near), ptr(out), _lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gpu_draw(T, N, H, W, vq=None, faces=None, pq=None, size_q=None, fq=6400, max_half=3):
    """clear, then the faces, then the points -> keys (T,H,W) uint64"""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    L = _lib.lib()
    keys = torch.zeros(T, H, W, dtype=torch.int64, device='cuda:0')
    st = _lib.stream_ptr(keys.device)
    check(L.mh_view_clear(T, H, W, ptr(keys), st))
    if vq is not None:
        v, f = _dev(vq, np.int32), _dev(faces, np.int32)
        check(L.mh_view_raster(T, N, int(v.shape[1]), int(f.shape[0]), H, W, ptr(v), ptr(f), ptr(keys), st))
    if pq is not None:
        p = _dev(pq, np.int32)
        s = None if size_q is None else _dev(size_q, np.int32)
        check(L.mh_view_splat(T, int(p.shape[1]), H, W, ptr(p), ptr(s), int(fq), int(max_half), ptr(keys), st))
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


# ---- projection ---------------------------------------------------------------------------------------------------------------
def test_project_against_float64():
    from mhhip import synthetic, view
    rng = np.random.RandomState(7)
    xyz = (rng.uniform(-1, 1, (4096, 3)) * (3.0, 2.0, 3.0) + (0.0, 0.0, 3.0)).astype(np.float32)
    K = synthetic.default_cam_K((64, 48), 60.0)
    views = [view.look_at((0.2, -0.1, -0.5), (0, 0, 3)), view.orbit((0, 0, 3), 3.5, 25.0, 40.0), view.top_down((0, 0.5, 3), 1.5)]
    R = np.stack([v[0] for v in views]).astype(np.float32)
    t = np.stack([v[1] for v in views]).astype(np.float32)
    got = gpu_project(xyz, R, t, K, NEAR, per_view=0)
    assert got.shape == (3, 4096, 3)
    worst, n_valid = 0, 0
    for i in range(3):
        want, valid, dist = vr.project(xyz, R[i], t[i], K, NEAR)
        # the condition on this test's own inputs: no random point within 1e-5 (relative) of a validity boundary
        assert dist.min() > 1e-5, (i, dist.min())
        assert 0.3 * len(xyz) < valid.sum() < len(xyz), 'view %d must see valid and invalid points' % i
        assert np.array_equal(got[i, :, 0] != vr.INVALID, valid)
        assert (got[i][~valid] == (vr.INVALID, 0, 0)).all()
        err = np.abs(got[i][valid].astype(np.int64) - want[valid])
        worst, n_valid = max(worst, int(err.max())), n_valid + int(valid.sum())
    print('projection: %d valid entries, largest difference from float64 %d unit(s)' % (n_valid, worst))
    assert worst <= 1
    # the same entries through the other form: the points repeated once per view
    again = gpu_project(np.tile(xyz, (3, 1)), R, t, K, NEAR, per_view=1)
    assert np.array_equal(again, got)


def test_project_placed_cases():
    """values exact in float32, R = I, t = 0, fx = fy = 64, cx = cy = 0: u 64 = 4096 x / z"""
    K = np.asarray([[64, 0, 0], [0, 64, 0], [0, 0, 1]], np.float32)
    one = np.float32(1.0)
    below, above = np.nextafter(np.float32(NEAR), np.float32(0)), np.nextafter(np.float32(NEAR), one)
    e = np.float32(2.0 ** -12)
    xyz = np.asarray([
        [0, 0, NEAR], [0, 0, below], [0, 0, above],                                            # zc exactly near, just below, just above
        [64, 0, 1], [-64, 0, 1], [0, 64, 1], [0, -64, 1],                                      # ON the guard band: |q| = 2^18
        [64 - e, 0, 1], [-(64 - e), 0, 1], [0, 64 - e, 1], [0, -(64 - e), 1],                  # one unit inside it
        [0, 0, 256], [0, 0, 256 - e],                                                          # zq = 2^20 and 2^20 - 1
        [np.nan, 0, 1], [0, 0, np.inf], [1e30, 0, 1]], np.float32)
    got = gpu_project(xyz, np.eye(3), np.zeros(3), K, NEAR, per_view=0)[0]
    want, valid, _ = vr.project(xyz[:13], np.eye(3), np.zeros(3), K, NEAR)
    assert valid.tolist() == [True, False, True] + [False] * 4 + [True] * 4 + [False, True]
    assert np.array_equal(got[:13], want)
    g = 2 ** 18 - 1
    assert got[0].tolist() == [0, 0, 2048] and got[2].tolist() == [0, 0, 2048]
    assert got[7:11].tolist() == [[g, 0, 4096], [-g, 0, 4096], [0, g, 4096], [0, -g, 4096]] and got[12].tolist() == [0, 0, 2 ** 20 - 1]
    assert (got[13:] == (vr.INVALID, 0, 0)).all()           # NaN, infinity and overflow are invalid, not converted


# ---- rasterisation, exact -----------------------------------------------------------------------------------------------------
def hand_mesh():
    """case (i): W = 37, H = 23, two people with the same 7 faces over 15 vertices (pixel units; z in 2^-12 m)"""
    q = lambda x, y, z: (int(round(x * 64)), int(round(y * 64)), z)
    bad = (vr.INVALID, 0, 0)
    p0 = [q(2.5, 2.5, 8000), q(12.5, 2.5, 8200), q(2.5, 12.5, 8400), q(12.5, 12.5, 8000),      # 0-3: a square, split along 1-2
          q(20.3, 3.7, 9000), q(30.9, 5.2, 9100), q(24.1, 15.8, 9500),                          # 4-6: off the pixel centres
          q(7.5, 7.5, 8100),                                                                    # 7: on the line 0-3
          bad,                                                                                  # 8
          q(50, 5, 7000), q(60, 5, 7000), q(55, 30, 7000),                                      # 9-11: right of the image
          q(-100, -50, 20000), q(300, -50, 21000), q(-100, 250, 22000)]                         # 12-14: over the whole image and beyond
    # person 1: only face 0, two pixels to the right IN THE PLANE of person 0's face 0 (z = 8000 + 20 dx + 40 dy): where both
    # cover a pixel the depths are identical integers
    p1 = [q(4.5, 2.5, 8040), q(14.5, 2.5, 8240), q(4.5, 12.5, 8440)] + [bad] * 12
    faces = [[0, 1, 2], [1, 3, 2],      # a shared edge (through pixel centres)
             [4, 6, 5],                 # the other winding
             [0, 3, 7],                 # zero area
             [4, 5, 8],                 # an invalid vertex
             [9, 10, 11],               # off screen
             [12, 13, 14]]              # the wide path, box clipped to the image
    return np.asarray([p0, p1], np.int64), np.asarray(faces, np.int64)


def test_raster_hand_mesh_is_exact():
    vq, faces = hand_mesh()
    H, W, N, F = 23, 37, 2, len(faces)
    got = gpu_draw(1, N, H, W, vq, faces)
    want = vr.raster(vr.clear(1, H, W), vq, faces, N)
    assert np.array_equal(got, want)
    out = vr.resolve(got, N, F)
    assert (out['label'] >= 0).all(), 'the wide face covers every pixel'
    assert set(np.unique(out['face'][out['label'] == 0]).tolist()) == {0, 1, 2, 6}
    assert out['face'][0, 4, 10] == 0 and out['face'][0, 10, 4] == 0 and out['face'][0, 7, 7] == 0      # the shared edge: lower payload
    # person 1 alone: its face is there; where it and person 0's face 0 both cover a pixel the depth is ONE integer and the
    # pixel is person 0's
    alone = gpu_draw(1, 1, H, W, vq[1:], faces)
    assert np.array_equal(alone, vr.raster(vr.clear(1, H, W), vq[1:], faces, 1))
    first = vr.resolve(vr.raster(vr.clear(1, H, W), vq[:1], faces, 1), 1, F)['face'] == 0
    both = (alone != vr.EMPTY) & first
    assert both.sum() > 20 and (out['label'][both] == 0).all() and (out['face'][both] == 0).all()
    assert np.array_equal(got[both] >> np.uint64(32), alone[both] >> np.uint64(32))
    assert out['coverage'][0, 1] > 0                        # (right of person 0's square it is in front of the wide face only)


@pytest.fixture(scope='module')
def bodies(smpl_struct, smpl_regs):
    """case (ii): the synthetic model's full V and F, T = 3 frames of N = 2 people at 64x48 with a ground cloud; an oblique
    orbit, a top-down view and a view one body straddles the near plane of.  Rendered TWICE through render_view."""
    import torch
    from mhhip import engine, synthetic, view
    model = engine.BodyModel(smpl_struct, smpl_regs)
    T, N, W, H = 3, 2, 64, 48
    sp = synthetic.make_sequence_params(N, T, 21)
    pT = np.zeros((T, N, 3), np.float32)
    pT[:, 0], pT[:, 1] = (-0.5, 0.2, 3.0), (0.6, 0.2, 3.6)
    pT[2, 1] = (0.1, 0.2, 0.55)                            # frame 2: the second body stands IN the near plane of the (identity) view
    t_ = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)
    verts, _, _, _ = model.lbs_forward(t_(sp['betas_gt']), t_(sp['poses_gt']).view(T * N, 72), None, t_(pT).view(T * N, 3), want_vposed=False)
    verts = verts.view(T, N, -1, 3).clone()
    K = synthetic.default_cam_K((W, H), 60.0)
    views = [view.orbit((0, 0.2, 3.3), 3.5, 25.0, 40.0), view.top_down((0, 0.2, 3.3), 4.0), (np.eye(3), np.zeros(3))]
    R = np.stack([v[0] for v in views]).astype(np.float32)
    t = np.stack([v[1] for v in views]).astype(np.float32)
    rng = np.random.RandomState(5)
    gx, gz = np.meshgrid(np.linspace(-2, 2, 40), np.linspace(1, 5, 40))
    cloud = np.stack([gx.ravel(), np.full(gx.size, 1.1), gz.ravel()], 1).astype(np.float32)       # the ground, y = 1.1 m
    rgb = rng.randint(0, 256, (len(cloud), 3)).astype(np.uint8)
    size = rng.uniform(0.02, 0.25, len(cloud)).astype(np.float32)
    palette = rng.uniform(0.1, 1.0, (N, 3)).astype(np.float32)
    kw = dict(cloud=cloud, cloud_rgb=rgb, cloud_size_m=size, palette=palette, light=LIGHT, ambient=AMBIENT, background=BACKGROUND,
              near=NEAR, max_half=3, outputs=view.VIEW_OUTPUTS + ('keys',))
    runs = [{k: v.cpu().numpy() for k, v in view.render_view(model, verts, (R, t), K, (W, H), **kw).items()} for _ in range(2)]
    V = verts.shape[2]
    vq = gpu_project(verts.cpu().numpy().reshape(T * N * V, 3), R, t, K, NEAR, per_view=1).reshape(T * N, V, 3)
    pq = gpu_project(cloud, R, t, K, NEAR, per_view=0)
    return dict(model=model, T=T, N=N, W=W, H=H, V=V, K=K, R=R, t=t, verts=verts, faces=np.asarray(smpl_struct.f).astype(np.int64),
                cloud=cloud, rgb=rgb, size=size, palette=palette, kw=kw, runs=runs, vq=vq, pq=pq,
                size_q=np.rint(size.astype(np.float64) * 4096).astype(np.int64), fq=int(np.rint(float(K[0, 0]) * 64)))


def test_raster_bodies_are_exact(bodies):
    b = bodies
    T, N, H, W, F = b['T'], b['N'], b['H'], b['W'], len(b['faces'])
    got = gpu_draw(T, N, H, W, b['vq'], b['faces'])
    want = vr.raster(vr.clear(T, H, W), b['vq'], b['faces'], N)
    assert np.array_equal(got, want)
    out = vr.resolve(got, N, F)
    print('bodies alone: pixels per frame and person', out['coverage'][:, :N].tolist())
    assert (out['coverage'][:2, :N] > 5).all()
    # the body in the near plane: some of its vertices are invalid, so some of its faces are gone -- the others are drawn
    ok = (b['vq'][2 * N + 1][:, 0] != vr.INVALID)
    whole = ok[b['faces']].all(1)
    print('straddling body: %d of %d vertices valid, %d of %d faces whole' % (ok.sum(), ok.size, whole.sum(), F))
    assert 0 < whole.sum() < F and out['coverage'][2, 1] > 100
    drawn = np.unique(out['face'][2][out['label'][2] == 1])
    assert whole[drawn].all()


def test_pipeline_keys_are_exact(bodies):
    """meshes and cloud through render_view: the z-buffer equals the restatement fed with the kernel's snapped coordinates"""
    b = bodies
    want = vr.raster(vr.clear(b['T'], b['H'], b['W']), b['vq'], b['faces'], b['N'])
    vr.splat(want, b['pq'], b['size_q'], b['fq'], 3)
    assert np.array_equal(b['runs'][0]['keys'].view(np.uint64), want)
    lab = b['runs'][0]['label']
    assert (lab == -2).sum() > 100 and (lab >= 0).sum() > 100 and (lab == -1).sum() > 100


def test_resolve(bodies):
    from mhhip import view
    b = bodies
    got = b['runs'][0]
    T, N, H, W, F = b['T'], b['N'], b['H'], b['W'], len(b['faces'])
    want = vr.resolve(got['keys'].view(np.uint64), N, F)
    for k in ('depth', 'label', 'face', 'coverage'):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
    assert got['coverage'].shape == (T, N + 1) and (got['coverage'][:, N] > 0).all()
    # the image: float64 evaluation of the formula from the kernel's own labels; one rounding of 255 * ... is the only float step
    vv = np.einsum('tij,tnvj->tnvi', b['R'].astype(np.float64), b['verts'].cpu().numpy().astype(np.float64)) + b['t'].astype(np.float64)[:, None, None]
    img = vr.shade_image(got['label'], got['face'], vv, b['faces'], b['palette'], LIGHT, AMBIENT, BACKGROUND, b['rgb'])
    assert got['image'].dtype == np.uint8 and got['image'].shape == (T, H, W, 3)
    diff = np.abs(got['image'].astype(np.float64) - img)
    print('image: off by at most %.3f levels' % diff.max())
    assert diff.max() <= 1.0
    assert np.array_equal(got['image'][got['label'] == -1], np.broadcast_to(np.uint8(BACKGROUND), ((got['label'] == -1).sum(), 3)))
    assert np.array_equal(got['image'][got['label'] == -2], b['rgb'][got['face'][got['label'] == -2]])
    # outputs= restricts what is computed and returned
    kw = dict(b['kw'], outputs=('depth',))
    only = view.render_view(b['model'], b['verts'], (b['R'], b['t']), b['K'], (W, H), **kw)
    assert sorted(only) == ['depth'] and np.array_equal(only['depth'].cpu().numpy(), got['depth'])
    kw = dict(b['kw'], outputs=None, chunk=2)             # the default: the five images, no keys; two chunks
    five = view.render_view(b['model'], b['verts'], (b['R'], b['t']), b['K'], (W, H), **kw)
    assert sorted(five) == sorted(view.VIEW_OUTPUTS)
    for k in view.VIEW_OUTPUTS:
        assert np.array_equal(five[k].cpu().numpy(), got[k]), k


def test_two_launches_give_identical_bytes(bodies):
    a, b = bodies['runs']
    assert sorted(a) == sorted(['image', 'depth', 'label', 'face', 'coverage', 'keys'])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- splatting, exact ---------------------------------------------------------------------------------------------------------
def test_splat_is_exact():
    H, W, fq = 23, 37, 6400
    c = lambda px, py, z, dx=17, dy=40: (64 * px + dx, 64 * py + dy, z)
    flat = np.asarray([[(64 * 4 + 32, 64 * 4 + 32, 5000), (64 * 14 + 32, 64 * 4 + 32, 5000), (64 * 4 + 32, 64 * 14 + 32, 5000)]], np.int64)
    pts = [(c(20, 8, 4096), 41), (c(25, 8, 4096), 100), (c(30, 12, 4096), 4096),           # half 0, 1 and max_half = 3
           (c(0, 0, 6000), 4096), (c(36, 0, 6000), 4096), (c(0, 22, 6000), 4096), (c(36, 22, 6000), 4096),        # the corners: clipped
           (c(15, 18, 7000, 1, 1), 0), (c(15, 18, 7000, 63, 63), 0),                           # two points in one pixel at one depth
           (c(4, 4, 5000), 0), (c(5, 5, 4999), 0), (c(6, 5, 5001), 0),                         # against the face at 5000: loses the tie, wins, loses
           ((vr.INVALID, 0, 0), 4096), (c(-2, 10, 4096), 4096), (c(38, -2, 4096), 4096),       # invalid; outside, the footprint reaches in
           (c(-9, 10, 4096), 4096), (c(18, 10, 8192), -7)]                                     # outside altogether; a negative extent
    pq = np.asarray([[p for p, _ in pts]], np.int64)
    size_q = np.asarray([s for _, s in pts], np.int64)
    assert [vr.point_half(size_q[i], fq, pq[0, i, 2], 3) for i in range(3)] == [0, 1, 3]
    got = gpu_draw(1, 1, H, W, flat, [[0, 1, 2]], pq, size_q, fq, 3)
    want = vr.splat(vr.raster(vr.clear(1, H, W), flat, [[0, 1, 2]], 1), pq, size_q, fq, 3)
    assert np.array_equal(got, want)
    out = vr.resolve(got, 1, 1)
    pt = lambda px, py: (int(out['label'][0, py, px]), int(out['face'][0, py, px]))
    assert pt(15, 18) == (-2, 7)                            # the lower index
    assert pt(4, 4) == (0, 0) and pt(5, 5) == (-2, 10) and pt(6, 5) == (0, 0)
    assert (out['face'][0, :4, :4] == 3).all() and (out['face'][0, -4:, -4:] == 6).all() and out['label'][0, 4, 36] == -1
    assert pt(0, 10) == (-2, 13) and pt(1, 13) == (-2, 13) and pt(2, 10) == (-1, -1)
    assert pt(36, 0) == (-2, 14) and pt(35, 1) == (-2, 14) and pt(34, 1) == (-2, 4) and pt(36, 2) == (-2, 4) and pt(18, 10) == (-2, 16)
    # P = 1, and 300 points (no multiple of the workgroup size, two workgroups), T = 2, without extents and with
    one = gpu_draw(1, 1, H, W, pq=pq[:, 2:3], size_q=size_q[2:3], fq=fq, max_half=8)
    assert np.array_equal(one, vr.splat(vr.clear(1, H, W), pq[:, 2:3], size_q[2:3], fq, 8)) and (one != vr.EMPTY).sum() == 15 * 17
    rng = np.random.RandomState(9)
    many = np.stack([rng.randint(-200, 64 * W + 200, (2, 300)), rng.randint(-200, 64 * H + 200, (2, 300)), rng.randint(2000, 9000, (2, 300))], -1)
    sizes = rng.randint(0, 600, 300)
    for s, mh in ((None, 3), (sizes, 0), (sizes, 2), (sizes, 8)):
        assert np.array_equal(gpu_draw(2, 1, H, W, pq=many, size_q=s, fq=fq, max_half=mh), vr.splat(vr.clear(2, H, W), many, s, fq, mh)), mh


# ---- identity view, end to end ------------------------------------------------------------------------------------------------
def test_identity_view_returns_the_scene_depth(smpl_struct, smpl_regs):
    import torch
    from mhhip import engine, synthetic, view
    model = engine.BodyModel(smpl_struct, smpl_regs)
    W, H = 40, 30
    K = synthetic.default_cam_K((W, H), 60.0)
    rng = np.random.RandomState(17)
    depth = (rng.randint(2 * 4096, 6 * 4096, (H, W)) / 4096.0).astype(np.float32)           # multiples of 2^-12 m
    mask = rng.rand(H, W) < 0.7
    cloud, rgb, extent, pix = view.cloud_from_depth(depth, mask, K, rgb=rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
    assert len(cloud) == mask.sum() and np.array_equal(pix, np.flatnonzero(mask.ravel()))
    verts = torch.zeros(1, 1, model.V, 3, device=model.device)
    verts[..., 2] = -5.0                                   # the body is behind the camera: nothing of it is drawn
    got = view.render_view(model, verts, (np.eye(3), np.zeros(3)), K, (W, H), cloud=cloud, cloud_rgb=rgb, cloud_size_m=extent, max_half=0)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(got['label'][0] == -2, mask) and (got['label'][0][~mask] == -1).all()
    assert np.array_equal(got['depth'][0][mask], depth[mask]) and (got['depth'][0][~mask] == -1).all()
    index = np.cumsum(mask.ravel()).reshape(H, W) - 1
    assert np.array_equal(got['face'][0][mask], index[mask])
    assert got['coverage'].tolist() == [[0, int(mask.sum())]]
    assert np.array_equal(got['image'][0][mask], rgb) and (got['image'][0][~mask] == 255).all()


# ---- through the optimiser ----------------------------------------------------------------------------------------------------
LEAVES = ['poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale']


def test_optimiser_render_view_reads_only(smpl_struct, smpl_regs, oracle_model, tmp_path):
    import torch
    from mhhip import view
    from mhmocap.optimizer import SMPLDepthSequenceOptimizer
    from test_fit_full_gpu import _setup
    T, N, W, H = 4, 2, 96, 54
    opt, dl, _, _, seq = _setup(smpl_struct, smpl_regs, oracle_model, tmp_path, T, N, W, H, 2, 41, True)
    fresh = SMPLDepthSequenceOptimizer(image_size=(W, H), num_frames=T, fov=60, device='cuda:0', smpl_model_parameters_path=str(tmp_path),
                                       smpl_data_struct=smpl_struct, scene_update='none', cam_K=opt.cam_K)
    side = view.orbit((0.0, 0.2, 3.1), 3.0, 20.0, 60.0)
    with pytest.raises(RuntimeError, match='init_optimized_variables'):
        fresh.render_view(side)
    opt.fit(dl, num_iter=3)
    e = opt.engine
    before = {k: e.leaf(k).clone() for k in LEAVES}
    grads = e.grads.clone()
    got = opt.render_view(side)
    torch.cuda.synchronize()
    for k in LEAVES:
        assert torch.equal(e.leaf(k), before[k]), k
    assert torch.equal(e.grads, grads)
    assert sorted(got) == sorted(['image', 'depth', 'label', 'face', 'coverage', 'frames'])
    assert np.array_equal(got['frames'], np.arange(T))
    assert got['image'].shape == (T, H, W, 3) and got['image'].dtype == np.uint8
    assert got['depth'].shape == (T, H, W) and got['label'].shape == (T, H, W) and got['face'].shape == (T, H, W)
    assert got['coverage'].shape == (T, N + 1)
    print('optimiser, side view: coverage', got['coverage'].tolist())
    assert (got['coverage'][:, N] > 0).all() and (got['label'] == -2).any()
    assert (got['coverage'][:, :N].sum(1) > 0).all()
    bare = opt.render_view(side, scene=False)
    assert not (bare['label'] == -2).any() and (bare['coverage'][:, N] == 0).all()
    # a path with one view per frame, other frames, another image size
    path = view.orbit((0.0, 0.2, 3.1), 3.0, np.asarray([10.0, 80.0]), np.asarray([-45.0, 0.0]))
    two = opt.render_view(path, frames=[3, 1], image_size=(64, 48), K=np.asarray([[50, 0, 32], [0, 50, 24], [0, 0, 1]], np.float32),
                          outputs=('label', 'coverage'), chunk=1)
    assert sorted(two) == ['coverage', 'frames', 'label'] and two['label'].shape == (2, 48, 64) and np.array_equal(two['frames'], [3, 1])
    with pytest.raises(ValueError):
        opt.render_view(path)                              # two views for four frames
    with pytest.raises(ValueError):
        opt.render_view(side, frames=[0, 4])
    opt._world = lambda: (2, 0)                            # a frame-sharded run is refused
    with pytest.raises(RuntimeError, match='shard'):
        opt.render_view(side)
