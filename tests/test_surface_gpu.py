"""``mh_surface_grid``, ``mh_mesh_closest``, ``mh_person_surface`` and ``mh_surface_pairs`` against the float32 definition
(tests/surface_ref.py), BIT FOR BIT on every output: the distance is defined in float32 in a fixed order and on the SET of
candidate faces, so no query is left out and no tolerance is needed.  Every call is made twice, into outputs and a workspace
filled differently, and must give the same bits both times; and once more with every body forced to walk all faces, which
must give the same bits as the grid -- the test of the ring walk's pruning.

Shapes: the smallest at which the kernels can go wrong -- 1, 63, 64, 65 and 257 queries (around the wave and one above the
workgroup of 256), meshes that walk all faces (4, 12 and 28 faces) and meshes that take the grid (320 and 1280 faces), bodies
of very different size in one call, 642 vertices per person (three workgroups, the last one short)."""
import numpy as np
import pytest
import torch

import inside_ref as ir
import surface_ref as sr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
SENTINEL = 0x5a5a5a5a                          # an output that is not written shows
INF = float('inf')


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _full(shape, fill):
    return torch.full(shape, fill, dtype=torch.int32, device=DEV)


def _grid(L, check, ptr, st, verts, faces, live, fill):
    B, V = verts.shape[:2]
    nbytes = L.mh_surface_grid_bytes(B, int(faces.shape[0]))
    ws = torch.full((nbytes,), fill & 0xff, dtype=torch.uint8, device=DEV)
    status = _full((B,), fill)
    check(L.mh_surface_grid(B, V, int(faces.shape[0]), ptr(verts), ptr(faces), ptr(live), ptr(ws), nbytes, ptr(status), st))
    return ws, status


def _closest(verts, faces, points, radius=INF, live=None, force=False):
    """verts (B,V,3), faces (F,3), points (B,Q,3) -> [d2 (B,Q) f32, face (B,Q) i32, point, weights (B,Q,3) f32, status (B)];
    two launches into differently filled memory"""
    L, check, ptr, st = _api()
    B, V = verts.shape[:2]
    Q = points.shape[1]
    tv, tf, tp = _dev(verts.astype(F32)), _dev(np.asarray(faces, np.int32).reshape(-1, 3)), _dev(points.astype(F32))
    tl = _dev(None if live is None else np.asarray(live, np.uint8))
    runs = []
    was = L.mh_surface_set_all_faces(1 if force else 0)
    try:
        for fill in (SENTINEL, 7):
            ws, status = _grid(L, check, ptr, st, tv, tf, tl, fill)
            res = [_full((B, Q), fill), _full((B, Q), fill), _full((B, Q, 3), fill), _full((B, Q, 3), fill)]
            check(L.mh_mesh_closest(B, V, int(tf.shape[0]), ptr(tf), ptr(ws), Q, ptr(tp), float(radius), *[ptr(r) for r in res], st))
            torch.cuda.synchronize()
            runs.append([r.cpu().numpy() for r in res] + [status.cpu().numpy()])
    finally:
        L.mh_surface_set_all_faces(was)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    d2, face, point, weights, status = runs[0]
    return [d2.view(F32), face, point.view(F32), weights.view(F32), status]


def _closest_want(verts, faces, points, radius=INF, live=None):
    B = verts.shape[0]
    alive = [True if live is None else bool(live[b]) for b in range(B)]
    rows = [sr.closest_ref(verts[b], faces, points[b], radius, live=alive[b]) for b in range(B)]
    status = np.array([sr.grid_ref(verts[b], faces, live=alive[b])[0] for b in range(B)], np.int32)
    return [np.stack([r[k] for r in rows]) for k in range(4)] + [status]


NAMES = ('d2', 'face', 'point', 'weights')


def _check_closest(verts, faces, points, radius=INF, live=None):
    """the natural path (which must be the one ``grid_ref`` expects) and the forced all-faces path against the reference"""
    verts, points = np.asarray(verts, F32), np.asarray(points, F32)
    want = _closest_want(verts, faces, points, radius, live)
    got = _closest(verts, faces, points, radius, live)
    assert np.array_equal(got[4], want[4]), (got[4], want[4])
    for k, name in enumerate(NAMES):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), name
    forced = _closest(verts, faces, points, radius, live, force=True)
    assert np.array_equal(forced[4], np.where(want[4] & sr.NOT_LIVE, want[4], sr.ALL_FACES))
    for k, name in enumerate(NAMES):
        assert np.array_equal(_bits(forced[k]), _bits(want[k])), 'forced ' + name
    return want


def _snap(v, steps=4096.0):
    """onto multiples of 1 / steps: the midpoint of two vertices is a float32, exactly on their edge"""
    return (np.rint(np.asarray(v, np.float64) * steps) / steps).astype(F32)


def _tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32) * F32(0.5) + F32([0.25, -0.5, 2.0])
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def _meshes():
    cube = ir.cube(0.0, 1.0)
    prism = ir.u_prism()
    ico = ir.icosphere(2, 0.5, (0.125, -0.25, 2.0))
    return dict(tetrahedron=_tetrahedron(), cube=(cube[0] + F32([0, 0, 1.5]), cube[1]), u_prism=(_snap(prism[0]), prism[1]),
                icosphere2=(_snap(ico[0]), ico[1]))


def _queries(v, f, rng, n):
    """n queries, in turn: a random point of the grown box (inside or outside the mesh), a vertex (D2 = 0), the midpoint of
    an edge (D2 = 0, a tie between the faces that share it), a point a little off a face's centroid"""
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    k = n // 4 + 1
    box = rng.uniform(lo - 0.3, hi + 0.3, (k, 3))
    fi = rng.randint(0, len(f), k)
    corner = v[f[fi, rng.randint(0, 3, k)]].astype(np.float64)
    mid = (v[f[fi, 0]].astype(np.float64) + v[f[fi, 1]]) / 2
    near = v[f[fi]].astype(np.float64).mean(1) + rng.normal(0, 0.01, (k, 3))
    return np.stack([box, corner, mid, near], 1).reshape(-1, 3)[:n].astype(F32)


@pytest.mark.parametrize('Q', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('name', ['tetrahedron', 'cube', 'u_prism', 'icosphere2'])
def test_closest_equals_the_reference(name, Q):
    v, f = _meshes()[name]
    assert f.shape[0] == dict(tetrahedron=4, cube=12, u_prism=28, icosphere2=320)[name]
    rng = np.random.RandomState(Q)
    q = _queries(v, f, rng, max(Q, 4))
    if Q == 1:
        q = q[2:3]                                          # the edge midpoint
    want = _check_closest(v[None], f, q[None])
    d2, face = want[0][0], want[1][0]
    assert (face >= 0).all() and np.isfinite(d2).all()
    if Q == 1:
        assert d2[0] == 0
    else:
        # on a vertex and over an edge D2 is exactly 0 on every face around it: the smallest of them is the answer
        assert (d2[1::4] == 0).all() and (d2[2::4] == 0).all() and (d2[0::4] > 0).any()
    assert want[4][0] == (0 if name == 'icosphere2' else sr.ALL_FACES)
    # with a radius: what lies beyond it is not found, the rest is unchanged
    near = _check_closest(v[None], f, q[None], radius=0.1)
    assert np.array_equal(near[1][0] >= 0, d2 <= F32(0.1) * F32(0.1))


def test_the_radius_is_inclusive_to_the_last_bit():
    """the cube's z = 1.5 side seen from 3 m under it: D2 = 9 exactly; found at radius 3, not one float32 step below"""
    v, f = _meshes()['cube']
    q = np.array([[0.5, 0.25, -1.5], [0.25, 0.75, -1.5]], F32)
    want = _check_closest(v[None], f, q[None], radius=3.0)
    assert want[0][0].tolist() == [9.0, 9.0] and (want[1][0] >= 0).all() and (v[f[want[1][0]]][..., 2] == 1.5).all()
    below = np.nextafter(F32(3), F32(0))
    want = _check_closest(v[None], f, q[None], radius=below)
    assert np.isinf(want[0][0]).all() and (want[1][0] == -1).all() and not want[2].any() and not want[3].any()
    # the same on a mesh that takes the grid: an icosphere vertex at distance 0.25 along x from the query (D2 = 0.0625)
    v, f = _meshes()['icosphere2']
    top = v[np.argmax(v[:, 0])]
    q = (top + F32([0.25, 0, 0]))[None]
    want = _check_closest(v[None], f, q[None], radius=0.25)
    assert want[0][0, 0] == F32(0.0625) and want[4][0] == 0
    want = _check_closest(v[None], f, q[None], radius=np.nextafter(F32(0.25), F32(0)))
    assert want[1][0, 0] == -1


def test_a_query_a_kilometre_away_and_queries_and_vertices_that_are_not_finite():
    v, f = ir.icosphere(3, 0.45, (0.1, -0.2, 2.0))
    rng = np.random.RandomState(5)
    q = np.concatenate([[[1000.0, 0, 2], [0.1, -1000.0, 2.0], [-600, 700, -800]], _queries(v, f, rng, 60), v[100:101],
                        [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 3e38]]]).astype(F32)
    want = _check_closest(v[None], f, q[None])                                      # radius = +inf: it finishes, and finds
    assert want[4][0] == 0 and (want[1][0, :64] >= 0).all() and (want[1][0, 64:67] == -1).all()
    assert abs(np.sqrt(want[0][0, 0]) - (1000.0 - 0.1 - 0.45)) < 0.01
    # vertices that are not finite: their faces drop out, the others stay
    bad = v.copy()
    bad[[0, 100, 333]] = [[np.nan, 0, 2], [0, np.inf, 2], [0.1, 0.2, -np.inf]]
    want2 = _check_closest(bad[None], f, q[None])
    gone = np.isin(f, [0, 100, 333]).any(1)
    assert not gone[want2[1][0][want2[1][0] >= 0]].any() and (want2[1][0, :64] >= 0).all()
    assert (want2[0][0, :64] >= want[0][0, :64]).all() and want[0][0, 63] == 0 and want2[0][0, 63] > 0     # (query 63: the old vertex 100)
    _check_closest(bad[None], f, q[None], radius=0.3)


def test_bodies_of_very_different_size_in_one_call():
    """twelve faces: a cube of 100 m (walks all faces by itself), every vertex at one point (one cell), a dead body, a cube
    of one millimetre; then 1280 faces: spheres of 5 m and of 1 cm, both on the grid"""
    v, f = ir.cube(0.0, 1.0)
    verts = np.stack([v * F32(100) - F32(50), v * F32(0) + F32([0.5, 0.25, 2.0]), v, v * F32(0.001) + F32([3, 3, 3])])
    rng = np.random.RandomState(11)
    pts = np.stack([rng.uniform(-60, 60, (65, 3)), rng.uniform(-1, 3, (65, 3)), rng.uniform(0, 1, (65, 3)),
                    rng.uniform(2.999, 3.002, (65, 3))]).astype(F32)
    live = [1, 1, 0, 1]
    want = _check_closest(verts, f, pts, live=live)
    assert want[4].tolist() == [sr.ALL_FACES, 0, sr.NOT_LIVE, sr.ALL_FACES]
    assert (want[1][[0, 1, 3]] >= 0).all() and (want[1][2] == -1).all() and np.isinf(want[0][2]).all()
    _check_closest(verts, f, pts, radius=0.5, live=live)
    v, f = ir.icosphere(3)
    verts = np.stack([v * F32(5) + F32([0, 0, 20]), v * F32(0.01) + F32([0.5, 0.5, 2.0])])
    pts = np.stack([_queries(verts[0], f, rng, 129), _queries(verts[1], f, rng, 129)])
    want = _check_closest(verts, f, pts)
    assert want[4].tolist() == [0, 0]
    _check_closest(verts, f, pts, radius=0.2)


def test_module_functions(smpl_struct):
    """``closest_point_on_mesh`` and ``signed_distance``, single and batched, on the body model's rest shape"""
    from mhhip import inside, surface
    faces = np.asarray(smpl_struct.f).astype(np.int64)
    v = (np.asarray(smpl_struct.v_template) + [0.3, -0.2, 3.0]).astype(F32)
    rng = np.random.RandomState(2)
    q = (v[::53] + rng.normal(0, 0.02, v[::53].shape)).astype(F32)
    want = sr.closest_ref(v, faces, q)
    tv, tq = _dev(v), _dev(q)
    got = surface.closest_point_on_mesh(tv, faces, tq)
    assert [tuple(g.shape) for g in got] == [(len(q),), (len(q),), (len(q), 3), (len(q), 3)]
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w)), name
    two = surface.closest_point_on_mesh(torch.stack([tv, tv + 1]), faces, torch.stack([tq, tq + 1]), radius=0.015)
    near = sr.closest_ref(v, faces, q, 0.015)
    assert np.array_equal(_bits(two[0][0].cpu().numpy()), _bits(near[0])) and np.array_equal(two[1][0].cpu().numpy(), near[1])
    assert (near[1] == -1).any() and (near[1] >= 0).any()
    sd = surface.signed_distance(tv, faces, tq).cpu().numpy()
    ins = inside.points_inside_mesh(tv, faces, tq)[1].cpu().numpy()
    assert ins.any() and not ins.all()
    assert np.array_equal(_bits(sd), _bits(np.where(ins, -np.sqrt(want[0]), np.sqrt(want[0]))))     # (the correctly rounded root)
    sd = surface.signed_distance(tv, faces, tq, radius=0.015).cpu().numpy()
    assert np.array_equal(np.isinf(sd), near[1] == -1) and (sd[np.isinf(sd)] > 0).all()


# ---- the clearance map's two calls -----------------------------------------------------------------------------------------------
T, N, P = 2, 3, 6
RADIUS, CONTACT = 0.05, 0.04


@pytest.fixture(scope='module')
def people():
    """three spheres of 642 vertices in two frames: 0 and 1 overlap, 2 stands 2 m away in frame 0 and 3 cm from sphere 0 in
    frame 1, where person 1 is not there"""
    v, f = ir.icosphere(3, 0.45)
    centres = np.array([[[0, 0, 2], [0.3, 0.1, 2.05], [2, 0, 2]], [[0, 0, 2], [-0.2, 0.25, 2.1], [0.93, 0, 2]]], np.float64)
    verts = (v[None, None].astype(np.float64) + centres[:, :, None]).astype(F32)
    live = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    part = (np.arange(v.shape[0]) % 7).astype(np.uint8)     # part 6 >= P: counts in no part
    return verts, f, live, part


def _person(verts, faces, live, part, radius, contact, with_mask=True, force=False):
    """mh_mesh_bins + mh_person_inside for the mask, then the calls under test, twice -> dict of numpy arrays"""
    L, check, ptr, st = _api()
    V, F = verts.shape[2], faces.shape[0]
    tv, tf, tl, tpart = _dev(verts), _dev(np.asarray(faces, np.int32)), _dev(live), _dev(part)
    nb = L.mh_mesh_bins_bytes(T * N, F)
    ws_in = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mask = _full((T, N, V), SENTINEL)
    check(L.mh_mesh_bins(T * N, V, F, ptr(tv), ptr(tf), ptr(tl), ptr(ws_in), nb, None, st))
    check(L.mh_person_inside(T, N, V, F, ptr(tf), ptr(ws_in), ptr(tv), ptr(tpart), P, ptr(mask), None, None, None, None, None, None, st))
    runs = []
    was = L.mh_surface_set_all_faces(1 if force else 0)
    try:
        for fill in (SENTINEL, 7):
            ws, status = _grid(L, check, ptr, st, tv.view(T * N, V, 3), tf, tl.view(-1), fill)
            o = dict(out_d2=_full((T, N, V), fill), out_idx=_full((T, N, V), fill), in_d2=_full((T, N, V), fill), in_idx=_full((T, N, V), fill),
                     out_pt=_full((T, N, V, 3), fill), in_pt=_full((T, N, V, 3), fill), stats=_full((T, N, V, 2), fill))
            check(L.mh_person_surface(T, N, V, F, ptr(tf), ptr(ws), ptr(tv), ptr(mask) if with_mask else None, radius,
                                      *[ptr(o[k]) for k in ('out_d2', 'out_idx', 'in_d2', 'in_idx', 'out_pt', 'in_pt', 'stats')], st))
            tab = dict(pair_depth_d2=_full((T, N, N), fill), pair_min_d2=_full((T, N, N), fill), pair_contact=_full((T, N, N), fill),
                       part_depth_d2=_full((T, N, P), fill), part_min_d2=_full((T, N, P), fill), part_contact=_full((T, N, P), fill))
            check(L.mh_surface_pairs(T, N, V, F, ptr(o['out_d2']), ptr(o['out_idx']), ptr(o['in_d2']), ptr(o['in_idx']), ptr(tpart), P, contact,
                                     *[ptr(tab[k]) for k in ('pair_depth_d2', 'pair_min_d2', 'pair_contact', 'part_depth_d2', 'part_min_d2',
                                                             'part_contact')], st))
            torch.cuda.synchronize()
            o.update(tab)
            o['status'] = status.view(T, N)
            runs.append({k: x.cpu().numpy() for k, x in o.items()})
    finally:
        L.mh_surface_set_all_faces(was)
    for k in runs[0]:
        if k != 'stats':                                    # (a measurement, not a result)
            assert np.array_equal(runs[0][k], runs[1][k]), k
    got = runs[0]
    for k in ('out_d2', 'in_d2', 'out_pt', 'in_pt', 'pair_depth_d2', 'pair_min_d2', 'part_depth_d2', 'part_min_d2'):
        got[k] = got[k].view(F32)
    got['mask'] = mask.cpu().numpy()
    return got


@pytest.fixture(scope='module')
def people_want(people):
    verts, f, live, part = people
    got = _person(verts, f, live, part, RADIUS, CONTACT)
    want = sr.person_surface_ref(verts, f, got['mask'], RADIUS, live)
    return got, want


def test_person_surface_equals_the_reference(people, people_want):
    verts, f, live, part = people
    got, want = people_want
    V, F = verts.shape[2], f.shape[0]
    assert V == 642 and V % 256 != 0 and (got['status'] == np.where(live, 0, 1)).all()
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    mask = got['mask'].view(np.uint32)
    ins = mask != 0
    # the two overlapping spheres are inside each other in places, the third is inside nobody; the dead person has nothing
    assert ins[0, 0].any() and ins[0, 1].any() and ins[1, 0].sum() == 0 and not ins[:, 2].any() and not ins[1, 1].any()
    assert np.array_equal(got['in_idx'] >= 0, ins) and np.array_equal(np.isfinite(got['in_d2']), ins)
    assert (got['out_idx'][1, 1] == -1).all() and np.isinf(got['out_d2'][1, 1]).all()
    # a vertex deeper than the radius still gets its depth: sphere 0's vertex nearest sphere 1's centre is 0.3 m deep
    r2 = F32(RADIUS) * F32(RADIUS)
    assert (got['in_d2'][ins] > r2).any() and got['in_d2'][ins].max() > F32(0.25) ** 2
    # outside, nothing beyond the radius: frame 0's third sphere is 2 m away, frame 1's 3 cm from sphere 0
    assert (got['out_d2'][np.isfinite(got['out_d2'])] <= r2).all()
    assert (got['out_idx'][0, 2] == -1).all() and (got['out_idx'][1, 2] >= 0).any() and (got['out_idx'][1, 2][got['out_idx'][1, 2] >= 0] // F == 0).all()
    # the box test dropped the far sphere for everybody, and the walk looked at a fraction of the 1280 faces
    st = got['stats']
    assert (st[0, 2, :, 0] == 0).all() and (st[1, 1] == 0).all() and (st[0, 0, :, 0] <= 1).all() and (st[0, 0, :, 0][ins[0, 0]] == 1).all()
    assert (st[0, 0, :, 0] == 0).any()                      # sphere 0's far side is more than the radius from sphere 1's box
    outside = (st[0, 0, :, 0] == 1) & ~ins[0, 0]
    assert outside.any() and st[0, 0, :, 1].max() <= 16 * F and st[0, 0, :, 1][outside].mean() < F / 2


def test_forced_all_faces_and_no_mask(people, people_want):
    verts, f, live, part = people
    got, want = people_want
    forced = _person(verts, f, live, part, RADIUS, CONTACT, force=True)
    assert (forced['status'] == np.where(live, sr.ALL_FACES, 1)).all()
    for k in got:
        if k not in ('stats', 'status'):
            assert np.array_equal(_bits(forced[k]), _bits(got[k])), k
    F = f.shape[0]
    searched = forced['stats'][..., 0]
    assert np.array_equal(forced['stats'][..., 1], searched * F)                     # every face of every body that was searched
    # without a mask nobody is inside anybody: every body is searched with the radius
    plain = _person(verts, f, live, part, RADIUS, CONTACT, with_mask=False)
    ref = sr.person_surface_ref(verts, f, None, RADIUS, live)
    for k in ref:
        assert np.array_equal(_bits(plain[k]), _bits(ref[k])), k
    assert (plain['in_idx'] == -1).all() and (plain['pair_depth_d2'] == -1).all()


def test_tables_equal_the_reference(people, people_want):
    verts, f, live, part = people
    got, want = people_want
    tab = sr.pairs_ref(want['out_d2'], want['out_idx'], want['in_d2'], want['in_idx'], part, P, CONTACT, f.shape[0])
    for k in tab:
        assert np.array_equal(_bits(got[k]), _bits(tab[k])), k
    assert tab['pair_depth_d2'][0, 0, 1] > 0 and tab['pair_depth_d2'][0, 1, 0] > 0 and (tab['pair_depth_d2'][:, :, 2] == -1).all()
    assert tab['pair_contact'][1, 2, 0] > 0 and tab['pair_contact'][1, 0, 2] > 0 and np.isfinite(tab['pair_min_d2'][1, 0, 2])
    assert (tab['pair_contact'].sum(-1) > tab['part_contact'].sum(-1)).any()         # part 6 counts in no part
    # a larger threshold than any distance known counts every vertex that found a surface
    L, check, ptr, st = _api()
    V = verts.shape[2]
    ins = [_dev(want[k]) for k in ('out_d2', 'out_idx', 'in_d2', 'in_idx')]
    cnt = _full((T, N, N), SENTINEL)
    check(L.mh_surface_pairs(T, N, V, f.shape[0], *[ptr(i) for i in ins], ptr(_dev(part)), P, 1.0, None, None, ptr(cnt), None, None, None, st))
    assert np.array_equal(cnt.cpu().numpy().sum(-1), (want['out_idx'] >= 0).sum(-1))
