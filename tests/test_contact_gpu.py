"""``mh_scene_nearest`` and ``mh_contact_parts`` against the numpy definition (tests/contact_ref.py), BIT FOR BIT on d2,
near_xyz, counts and min_d2: the definition does not depend on the order the cloud is visited in, so no query is left out.

Clouds: a dense sheet (M = 1500 with duplicates: cells of about 0.04 m), a lone point, 40 coincident points (the minimum
extent and cell), a 9 x 16 lattice on a plane with a spacing that is exact in binary (queries between lattice points tie
exactly), a cloud built with its count on the device and decoys behind the count, and the cloud of a 48 x 32 depth map with
two posed bodies.  Queries: on and around the points, outside the bounding box within and beyond the radius, at
mn + k cell on the cell boundaries of every axis, NaN and inf.  Radii: below one cell, about five cells, and larger than
the whole grid (0.6 m over a cloud 0.4 m wide)."""
import numpy as np
import pytest
import torch

import contact_ref as cr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F = np.float32


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _build(pts, count=None):
    """grid over pts (count: the device-count build over the first ``count`` rows) -> (workspace, M to pass on)"""
    L, check, ptr, st = _api()
    M = pts.shape[0]
    tp = torch.tensor(pts, device=DEV)
    ws = torch.full((L.mh_scene_grid_bytes(M),), 0xA5, dtype=torch.uint8, device=DEV)
    if count is None:
        check(L.mh_scene_grid_build(ptr(tp), M, ptr(ws), st))
    else:
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        check(L.mh_scene_grid_build_dev(ptr(tp), ptr(cnt), M, ptr(ws), st))
    torch.cuda.synchronize()
    return ws, M


def _header(ws):
    """mn (3) float32, cell float32, dim (3) of the grid's device header"""
    raw = ws[:36].cpu().numpy()
    return raw[:12].view(F).copy(), raw[12:16].view(F)[0], raw[16:28].view(np.int32).copy()


def _nearest(ws, M, q, radius, want_d2=True, want_near=True):
    L, check, ptr, st = _api()
    Q = q.shape[0]
    tq = torch.tensor(q, device=DEV)
    sentinel = 0x7fc12345                      # a NaN with a payload: an output that is not written shows
    d2 = torch.full((Q,), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    near = torch.full((Q, 3), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    check(L.mh_scene_nearest(ptr(ws), M, ptr(tq), Q, float(radius), ptr(d2) if want_d2 else None, ptr(near) if want_near else None, st))
    torch.cuda.synchronize()
    return d2.cpu().numpy(), near.cpu().numpy()


def _same(tag, got, ref):
    gd, gn = got
    rd, rn = ref
    bad = np.nonzero((cr.bits(gd) != cr.bits(rd)) | (cr.bits(gn) != cr.bits(rn)).any(1))[0]
    print('%s: %d queries, %d with a candidate, %d differ' % (tag, len(rd), int(np.isfinite(rd).sum()), bad.size))
    assert bad.size == 0, '%s: query %d: got d2 %r near %r, reference d2 %r near %r' % (tag, bad[0], gd[bad[0]], gn[bad[0]], rd[bad[0]], rn[bad[0]])


def _sheet():
    rng = np.random.RandomState(3)
    pts = np.stack([rng.uniform(-0.2, 0.2, 1400), 1.0 + 0.02 * rng.randn(1400).clip(-2, 2), rng.uniform(2.8, 3.2, 1400)], 1).astype(F)
    return np.concatenate([pts, pts[:100]])                  # 100 duplicates


def _queries(pts, hdr, radius, seed):
    """inside the box, around the points, on them, outside the box within and beyond the radius, on every cell boundary, not finite"""
    rng = np.random.RandomState(seed)
    mn, cell, dim = hdr
    lo, hi = pts.min(0), pts.max(0)
    M = pts.shape[0]
    parts = [rng.uniform(lo, hi, (150, 3)),                                                   # inside the bounding box
             pts[rng.randint(0, M, 300)] + rng.uniform(-1, 1, (300, 3)) * radius,            # around the points
             pts[rng.randint(0, M, 40)]]                                                       # on (d2 = 0)
    for axis in range(3):
        for side, edge in ((-1, lo), (1, hi)):
            for off in (0.5, 0.999, 1.001, 2.0, 1000.0):                                      # outside: within, at, beyond, far
                q = rng.uniform(lo, hi, (6, 3))
                q[:, axis] = edge[axis] + side * off * radius
                parts.append(q)
        for k in range(int(dim[axis]) + 1):                                                   # q = mn + k cell
            q = rng.uniform(lo, hi, (2, 3)).astype(F)
            q[:, axis] = mn[axis] + F(k) * cell
            parts.append(q)
    q = np.concatenate(parts).astype(F)
    odd = q[:6].copy()
    odd[0, 0], odd[1, 1], odd[2, 2] = np.nan, np.inf, -np.inf
    odd[3], odd[4, 0], odd[5, 2] = np.nan, 3e38, -3e38
    return np.concatenate([q, odd])


@pytest.fixture(scope='module')
def sheet():
    pts = _sheet()
    ws, M = _build(pts)
    hdr = _header(ws)
    print('sheet: cell %.4f dims %s' % (hdr[1], hdr[2]))
    assert 0.02 < hdr[1] < 0.06
    return pts, ws, M, hdr


@pytest.mark.parametrize('radius', [0.015, 0.2, 0.6])
def test_sheet_radius_below_a_cell_five_cells_and_beyond_the_grid(sheet, radius):
    pts, ws, M, hdr = sheet
    assert radius < hdr[1] or radius > 4 * hdr[1]
    q = _queries(pts, hdr, radius, 11)
    ref = cr.nearest_ref(pts, q, radius)
    if radius == 0.6:                          # the box of a query inside the cloud covers every cell: all points are candidates
        inside = ((q >= pts.min(0)) & (q <= pts.max(0))).all(1)
        assert inside.sum() > 100 and np.isfinite(ref[0][inside]).all()
    got = _nearest(ws, M, q, radius)
    _same('sheet r=%g' % radius, got, ref)
    again = _nearest(ws, M, q, radius)
    assert np.array_equal(cr.bits(got[0]), cr.bits(again[0])) and np.array_equal(cr.bits(got[1]), cr.bits(again[1]))


@pytest.mark.parametrize('Q', [1, 255, 256, 257])
def test_query_counts_around_the_workgroup(sheet, Q):
    pts, ws, M, hdr = sheet
    q = _queries(pts, hdr, 0.1, 12)[:Q]
    _same('Q=%d' % Q, _nearest(ws, M, q, 0.1), cr.nearest_ref(pts, q, 0.1))


def test_either_output_alone(sheet):
    pts, ws, M, hdr = sheet
    q = _queries(pts, hdr, 0.1, 13)
    rd, rn = cr.nearest_ref(pts, q, 0.1)
    d2, near = _nearest(ws, M, q, 0.1, want_near=False)
    assert np.array_equal(cr.bits(d2), cr.bits(rd)) and (cr.bits(near) == 0x7fc12345).all()
    d2, near = _nearest(ws, M, q, 0.1, want_d2=False)
    assert np.array_equal(cr.bits(near), cr.bits(rn)) and (cr.bits(d2) == 0x7fc12345).all()


@pytest.mark.parametrize('point', [(0.0, 0.0, 0.0), (1.0, 2.0, 3.0)])
def test_lone_point_and_the_inclusive_radius(point):
    pts = np.array([point], F)
    ws, M = _build(pts)
    r = F(0.25)                                # 0.25 and the coordinates are short binary fractions: q = p +- r is exact
    q = []
    for axis in range(3):
        for sign in (-1, 1):
            for step in (r, np.nextafter(r, F(1)), np.nextafter(r, F(0))):
                a = pts[0].copy()
                a[axis] += sign * step
                q.append(a)
    q = np.asarray(q + [pts[0], pts[0] + F(0.125), pts[0] - F(5)], F)
    ref = cr.nearest_ref(pts, q, r)
    if point == (0.0, 0.0, 0.0):               # exactly at the radius: in; one float beyond it: out
        assert (ref[0][0:18:3] == r * r).all() and np.isinf(ref[0][1:18:3]).all() and np.isfinite(ref[0][2:18:3]).all()
    _same('lone point %s' % (point,), _nearest(ws, M, q, r), ref)


def test_coincident_points():
    pts = np.tile(np.array([[0.3, 1.1, 2.7]], F), (40, 1))
    ws, M = _build(pts)
    mn, cell, dim = _header(ws)
    assert cell == F(0.02) and dim.tolist() == [1, 1, 1]
    for radius in (0.01, 0.1, 0.64):
        q = _queries(pts, (mn, cell, dim), radius, 14)
        _same('coincident r=%g' % radius, _nearest(ws, M, q, radius), cr.nearest_ref(pts, q, radius))


def test_lattice_on_a_plane_ties():
    s = F(0.0625)
    ix, iz = np.meshgrid(np.arange(9), np.arange(16), indexing='ij')
    pts = np.stack([ix.ravel() * s - F(0.25), np.full(144, 1.0), iz.ravel() * s + F(2.5)], 1).astype(F)
    pts = pts[np.random.RandomState(5).permutation(144)]
    ws, M = _build(pts)
    hdr = _header(ws)
    # between four lattice points (a four-way tie: x decides, then z), between two along x and along z, lifted off the plane
    q = []
    for dx, dz in ((0.5, 0.5), (0.5, 0.0), (0.0, 0.5)):
        a = pts.copy()
        a[:, 0] += F(dx) * s
        a[:, 2] += F(dz) * s
        a[:, 1] += F(0.03125)
        q.append(a)
    q = np.concatenate(q + [_queries(pts, hdr, 0.1, 15)]).astype(F)
    ref = cr.nearest_ref(pts, q, 0.1)
    e = pts[None] - q[:200, None]                            # (the first rows of q are the queries between lattice points)
    tied = (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) == ref[0][:200, None]).sum(1) > 1
    assert tied.sum() > 100                    # the ties are there
    _same('lattice', _nearest(ws, M, q, 0.1), ref)
    _same('lattice r=0.3', _nearest(ws, M, q, 0.3), cr.nearest_ref(pts, q, 0.3))


def test_device_count_build_ignores_rows_behind_the_count():
    pts = _sheet()
    count = 900
    rng = np.random.RandomState(6)
    q = (pts[rng.randint(0, count, 400)] + rng.uniform(-0.05, 0.05, (400, 3))).astype(F)
    buf = pts.copy()
    buf[count:] = q[np.arange(len(buf) - count) % len(q)]     # decoys exactly on the queries: they would win if they were read
    ref = cr.nearest_ref(pts[:count], q, 0.1)
    assert (ref[0] > 0).all() and (cr.nearest_ref(buf, q, 0.1)[0] == 0).all()
    ws, M = _build(buf, count=count)
    _same('build_dev', _nearest(ws, M, q, 0.1), ref)


@pytest.fixture(scope='module')
def bodies(smpl_struct, smpl_regs):
    """2 posed bodies of the synthetic model standing on the floor of a 48 x 32 depth map, and that map's cloud"""
    from mhhip import engine, synthetic
    model = engine.BodyModel(smpl_struct, smpl_regs)
    W, H, N = 48, 32, 2
    K = synthetic.default_cam_K((W, H), 60.0)
    sp = synthetic.make_sequence_params(N, 1, 31, (2.6, 3.6))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=F)).to(DEV)
    verts, _, _, _ = model.lbs_forward(t(sp['betas_gt']), t(sp['poses_gt']).view(N, 72), None, t(sp['trans_gt']).view(N, 3), want_vposed=False)
    verts = verts.view(N, -1, 3).cpu().numpy().astype(F)
    floor = float(verts[..., 1].max(1).min())                 # y down: under the feet of the shallower body
    ys = (np.arange(H, dtype=F) + 0.5 - K[1, 2]) / K[1, 1]
    xs = (np.arange(W, dtype=F) + 0.5 - K[0, 2]) / K[0, 0]
    d = np.where(ys > 1e-3, floor / np.maximum(ys, 1e-3), 10.0).astype(F)
    keep = (ys > 1e-3) & (d <= 10.0)
    depth = np.tile(np.minimum(d, 10.0)[:, None], (1, W))
    cloud = np.stack([depth * xs[None, :], depth * ys[:, None], depth], -1)[keep].reshape(-1, 3).astype(F)
    for n in range(N):                                        # slide every body over the floor until its lowest vertex is 0.036 m
        low = verts[n, verts[n, :, 1].argmax()]               # beside a cloud point: the coarse cloud is in reach of the feet
        near = cloud[((cloud - low) ** 2).sum(1).argmin()]
        verts[n] += np.array([near[0] - low[0] + 0.02, 0.0, near[2] - low[2] + 0.03], F)
    return model, verts, cloud


@pytest.mark.parametrize('radius', [0.1, 0.3])
def test_two_bodies_against_a_depth_map_cloud(bodies, radius):
    model, verts, cloud = bodies
    ws, M = _build(cloud)
    q = verts.reshape(-1, 3)
    ref = cr.nearest_ref(cloud, q, radius)
    assert q.shape[0] == 2 * 6890 and np.isfinite(ref[0][:6890]).any() and np.isinf(ref[0]).any()
    _same('bodies r=%g' % radius, _nearest(ws, M, q, radius), ref)


# ---- per body and part ----------------------------------------------------------------------------------------------------------
def _parts(d2, part, P, thr):
    L, check, ptr, st = _api()
    B, V = d2.shape
    td, tp = torch.tensor(d2, device=DEV), torch.tensor(part, device=DEV)
    outs = []
    for fill in (-7, 123456):                  # whatever the outputs held is overwritten
        counts = torch.full((B, P), fill, dtype=torch.int32, device=DEV)
        mins = torch.full((B, P), float(fill), dtype=torch.float32, device=DEV)
        check(L.mh_contact_parts(B, V, ptr(td), ptr(tp), P, float(thr), ptr(counts), ptr(mins), st))
        torch.cuda.synchronize()
        outs.append((counts.cpu().numpy(), mins.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(cr.bits(outs[0][1]), cr.bits(outs[1][1]))
    return outs[0]


@pytest.mark.parametrize('P', [1, 24])
@pytest.mark.parametrize('V', [1, 257, 6890])
def test_parts_counts_and_minima(P, V):
    rng = np.random.RandomState(100 * P + V % 97)
    B = 3
    d2 = (rng.uniform(0, 0.06, (B, V)) ** 2).astype(F)
    d2[rng.rand(B, V) < 0.3] = np.inf
    d2[2] = np.inf                             # a body out of reach altogether
    part = rng.randint(0, P, V).astype(np.uint8)
    if P > 2:
        part[part == 5] = 6                    # a part without a vertex
    thr = F(0.03)
    d2[0, 0] = thr * thr                       # exactly on the threshold: counted
    if V > 1:
        d2[0, 1] = np.nextafter(thr * thr, F(1))
    want = cr.parts_ref(d2, part, P, thr)
    got = _parts(d2, part, P, thr)
    print('parts P=%d V=%d: %d vertices in contact' % (P, V, int(want[0].sum())))
    assert want[0][0, part[0]] >= 1 and (want[0][2] == 0).all() and np.isinf(want[1][2]).all()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(cr.bits(got[1]), cr.bits(want[1]))


def test_parts_of_the_model_on_the_bodies(bodies):
    from mhhip import contact
    model, verts, cloud = bodies
    part = contact.body_parts(model)
    assert part.shape == (6890,) and part.max() < 24
    d2 = cr.nearest_ref(cloud, verts.reshape(-1, 3), 0.3)[0].reshape(2, 6890)
    want = cr.parts_ref(d2, part, 24, 0.1)
    got = _parts(d2, part, 24, 0.1)
    assert want[0].sum() > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(cr.bits(got[1]), cr.bits(want[1]))
    # and the module's own path end to end
    out = contact.contact_map(model, torch.tensor(verts[None], device=DEV), torch.tensor(cloud, device=DEV), radius=0.3, contact=0.1)
    assert np.array_equal(out['part_verts'].cpu().numpy()[0], want[0])
    dist, root = out['dist_m'].cpu().numpy()[0], np.sqrt(d2)
    assert np.array_equal(np.isinf(dist), np.isinf(root))
    assert (np.abs(dist - root)[np.isfinite(root)] <= 2.0 ** -22 * root[np.isfinite(root)]).all()       # a square root within 2 ulp
    assert np.array_equal(out['contact'].cpu().numpy()[0], d2 <= F(0.1) * F(0.1))
    assert np.array_equal(out['contact_verts'].cpu().numpy()[0], want[0].sum(1))
