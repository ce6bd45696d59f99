"""``mh_mesh_bins``, ``mh_mesh_winding`` and ``mh_person_inside`` against the int64 definition (tests/inside_ref.py), BIT FOR BIT
on every output: the test is defined in integers and on the SET of faces, so no query is left out and no tolerance is needed.
Every call is made twice, into outputs and a workspace filled differently, and must give the same bits both times.

Shapes: the smallest at which the kernels can go wrong -- one vertex, 257 vertices (one above the workgroup of 256), a mesh
that takes the grid path (an icosphere of 1280 faces) and one that walks all faces (a cube of 12), 1 and 32 people, several
frames, and a last chunk that is short."""
import numpy as np
import pytest
import torch

import inside_ref as ir

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
U = 2.0 ** -16
SENTINEL = 0x5a5a5a5a                          # an output that is not written shows


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def _bins(L, check, ptr, st, verts, faces, live, fill):
    B, V = verts.shape[:2]
    nbytes = L.mh_mesh_bins_bytes(B, int(faces.shape[0]))
    ws = torch.full((nbytes,), fill & 0xff, dtype=torch.uint8, device=DEV)
    status = torch.full((B,), fill, dtype=torch.int32, device=DEV)
    check(L.mh_mesh_bins(B, V, int(faces.shape[0]), ptr(verts), ptr(faces), ptr(live), ptr(ws), nbytes, ptr(status), st))
    return ws, status


def _winding(verts, faces, points, live=None, outs=(1, 1, 1), force=False):
    """verts (B,V,3), faces (F,3), points (B,Q,3) -> (winding, up, down (B,Q) int32 or None, status (B)); two launches"""
    L, check, ptr, st = _api()
    B, V = verts.shape[:2]
    Q = points.shape[1]
    tv, tf, tp = _dev(verts.astype(F32)), _dev(np.asarray(faces, np.int32).reshape(-1, 3)), _dev(points.astype(F32))
    tl = _dev(None if live is None else np.asarray(live, np.uint8))
    runs = []
    was = L.mh_mesh_set_all_faces(1 if force else 0)
    try:
        for fill in (SENTINEL, 7):
            ws, status = _bins(L, check, ptr, st, tv, tf, tl, fill)
            res = [torch.full((B, Q), fill, dtype=torch.int32, device=DEV) if o else None for o in outs]
            check(L.mh_mesh_winding(B, V, int(tf.shape[0]), ptr(tf), ptr(ws), Q, ptr(tp), *[ptr(r) for r in res], st))
            torch.cuda.synchronize()
            runs.append([None if r is None else r.cpu().numpy() for r in res] + [status.cpu().numpy()])
    finally:
        L.mh_mesh_set_all_faces(was)
    for a, b in zip(*runs):
        assert (a is None and b is None) or np.array_equal(a, b)
    return runs[0]


def _winding_want(verts, faces, points, live=None):
    B = verts.shape[0]
    rows = [ir.winding_ref(verts[b], faces, points[b], live=True if live is None else bool(live[b])) for b in range(B)]
    return [np.stack([r[k] for r in rows]) for k in range(3)] + [np.array([r[3] for r in rows], np.int32)]


def _check_winding(verts, faces, points, live=None, path=None):
    """both paths where ``path`` is None, else the natural one, which must be ``path`` (0: grid, 4: all faces) for every
    testable body"""
    want = _winding_want(verts, faces, points, live)
    got = _winding(verts, faces, points, live)
    testable = want[3] == 0
    assert np.array_equal(got[3] & 3, want[3])
    if path is not None:
        assert ((got[3][testable] & ir.ALL_FACES) == path).all(), got[3]
    for k, name in enumerate(('winding', 'up', 'down')):
        assert np.array_equal(got[k], want[k]), name
    forced = _winding(verts, faces, points, live, force=True)
    assert ((forced[3][testable] & ir.ALL_FACES) == ir.ALL_FACES).all() and np.array_equal(forced[3] & 3, want[3])
    for k, name in enumerate(('winding', 'up', 'down')):
        assert np.array_equal(forced[k], want[k]), 'forced ' + name
    return want


def _even_lattice(v):
    """onto even lattice coordinates: the midpoint of two vertices is a lattice point, exactly on their edge"""
    return (2.0 * np.rint(np.asarray(v, np.float64) * 32768.0) / 65536.0).astype(F32)


def _sphere_queries(v, f, rng, n_random=600):
    """random points of the (slightly grown) box, and points planted exactly over vertices and edge midpoints -- under, ON
    (Nn = 0) and over the surface --, on the box's faces and corners, and some that are not finite"""
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    pts = [rng.uniform(lo - 0.02, hi + 0.02, (n_random, 3))]
    mids = (v[f[:60, 0]].astype(np.float64) + v[f[:60, 1]]) / 2
    for base in (v[:60].astype(np.float64), mids):
        for dz in (-0.07, 0.0, 0.07, -2 * U, 2 * U):
            pts.append(base + [0.0, 0.0, dz])
    onbox = rng.uniform(lo, hi, (120, 3))
    for a in range(3):
        onbox[a * 40:a * 40 + 20, a] = lo[a]
        onbox[a * 40 + 20:a * 40 + 40, a] = hi[a]
    pts.append(onbox)
    pts.append(np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0] + U, lo[1], lo[2]], [lo[0] - U, lo[1], lo[2]]]))
    pts = np.concatenate(pts).astype(F32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, 9000.0, 0], [8192.0, 0, 0]], F32)
    return np.concatenate([pts, bad + pts[:6] * F32(0)])


@pytest.fixture(scope='module')
def sphere():
    v, f = ir.icosphere(3, 0.45, (0.1, -0.2, 2.0))
    return _even_lattice(v), f


def test_icosphere_takes_the_grid_path(sphere):
    v, f = sphere
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    pts = _sphere_queries(v, f, np.random.default_rng(11))
    want = _check_winding(v[None], f, pts[None], path=0)
    w, up, down = want[0][0], want[1][0], want[2][0]
    assert (w == 1).sum() > 150 and (w == 0).sum() > 150 and set(np.unique(w)) == {0, 1}
    assert ((up == -1) & (down == -1) & (w == 0)).any() and ((up >= 0) & (down >= 0) & (w == 1)).any()


def test_icosphere_scales_and_places(sphere):
    """the grid's shift follows the box: millimetres to metres across, near the origin and near the range's end"""
    v, f = sphere
    c = np.array([0.1, -0.2, 2.0])
    rng = np.random.default_rng(12)
    bodies, points = [], []
    for scale, shift in ((0.004, (0, 0, 0)), (1.0, (-3.0, 2.0, 0.5)), (8.8, (0, 0, 0)), (1.0, (8100.0, -8100.0, 8100.0)), (0.05, (0, 0, 40.0))):
        b = _even_lattice((v.astype(np.float64) - c) * scale + c + shift)
        bodies.append(b)
        points.append(_sphere_queries(b, f, rng, 300))
    _check_winding(np.stack(bodies), f, np.stack(points), path=0)


def test_cube_walks_all_faces():
    v, f = ir.cube(0.0, 8 * U)
    g = np.arange(-2, 11)
    q = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * U).astype(F32)
    want = _check_winding(v[None], f, q[None], path=ir.ALL_FACES)
    assert (want[0] == 1).sum() == 512
    # a cube of a metre, and the same with its faces reversed
    v, f = ir.cube(-0.25, 0.75)
    pts = np.random.default_rng(13).uniform(-0.3, 0.8, (500, 3)).astype(F32)
    want = _check_winding(np.stack([v, v]), f, np.stack([pts, pts]), path=ir.ALL_FACES)
    assert (want[0][0] == 1).sum() > 100
    want = _check_winding(v[None], f[:, ::-1], pts[None], path=ir.ALL_FACES)
    assert (want[0] == -1).sum() > 100


def test_special_bodies_in_one_call(sphere):
    """a plain body, one of zero extent, one with vertices that are not finite, one over 8 m, one at 9000 m, a dead one"""
    v, f = sphere
    rng = np.random.default_rng(14)
    c = np.array([0.1, -0.2, 2.0], F32)
    zero = np.broadcast_to(c, v.shape).copy()
    holes = v.copy()
    lost = [int(np.argmax(v[:, 2])), int(np.argmin(v[:, 2])), int(np.argmax((v - c).sum(1)))]       # top, bottom, towards (1,1,1)
    holes[lost] = [[np.nan, 0, 0], [0.1, np.inf, 2.0], [np.nan, np.nan, np.nan]]
    wide = ((v - c) * F32(9.5) + c).astype(F32)             # 8.55 m across
    far = (v + F32(9000.0)).astype(F32)
    one_far = v.copy()
    one_far[7, 1] = 8192.0                                   # one coordinate at the range's end is enough
    bodies = np.stack([v, zero, holes, wide, far, v, one_far])
    live = np.array([1, 1, 1, 1, 1, 0, 1], np.uint8)
    base = _sphere_queries(v, f, rng, 300)
    base[:3] = v[lost]                                       # on the axis through the vertices that body 2 loses, at mid height
    base[:3, 2] = c[2]
    points = np.stack([base, np.concatenate([c[None], base[1:]]), base, base, (base + F32(9000.0)).astype(F32), base, base])
    want = _check_winding(bodies, f, points, live=live)
    assert want[3].tolist() == [0, 0, 0, 2, 2, 1, 2]
    assert (want[0][0] != 0).any() and not want[0][1].any() and (want[0][2] != 0).any() and not want[0][3:].any()
    # the skipped faces open the mesh, and it shows: under a hole nothing is above, over one nothing below
    assert all((want[0][2][i] == 0 and want[1][2][i] == -1) or want[2][2][i] == -1 for i in range(3))
    assert (want[0][0][:3] == 1).all() and (want[1][0][:3] >= 0).all() and (want[2][0][:3] >= 0).all()


def test_null_subsets_of_the_winding_outputs(sphere):
    v, f = sphere
    pts = _sphere_queries(v, f, np.random.default_rng(15), 100)
    full = _winding(v[None], f, pts[None])
    for outs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
        got = _winding(v[None], f, pts[None], outs=outs)
        for k in range(3):
            assert (got[k] is None) if not outs[k] else np.array_equal(got[k], full[k]), (outs, k)


def test_points_inside_mesh_module_form(sphere):
    from mhhip import inside
    v, f = sphere
    pts = _sphere_queries(v, f, np.random.default_rng(16), 200)
    w, up, down, status = ir.winding_ref(v, f, pts)
    got = inside.points_inside_mesh(_dev(v), f, _dev(pts))
    assert [tuple(g.shape) for g in got] == [(len(pts),)] * 4
    assert np.array_equal(got[0].cpu().numpy(), w) and np.array_equal(got[1].cpu().numpy(), w != 0)
    for g, lat in ((got[2], up), (got[3], down)):
        m = np.where(lat < 0, np.inf, lat.astype(np.float64) * U).astype(F32)
        assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), m)
    batched = inside.points_inside_mesh(_dev(np.stack([v, v])), f, _dev(np.stack([pts, pts])))
    assert all(np.array_equal(b[1].cpu().numpy(), g.cpu().numpy()) for b, g in zip(batched, got))


# ---- the penetration map ---------------------------------------------------------------------------------------------------------
NAMES = ('mask', 'depth', 'other', 'pair_verts', 'pair_depth', 'part_verts', 'part_depth')


def _inside(verts, faces, part, P, live=None, outs=(1,) * 7, force=False):
    L, check, ptr, st = _api()
    T, N, V = verts.shape[:3]
    tv, tf, tp = _dev(verts.astype(F32)), _dev(np.asarray(faces, np.int32).reshape(-1, 3)), _dev(np.asarray(part, np.uint8))
    tl = _dev(None if live is None else np.asarray(live, np.uint8).reshape(T * N))
    shapes = [(T, N, V)] * 3 + [(T, N, N)] * 2 + [(T, N, P)] * 2
    runs = []
    was = L.mh_mesh_set_all_faces(1 if force else 0)
    try:
        for fill in (SENTINEL, 7):
            ws, status = _bins(L, check, ptr, st, tv.view(T * N, V, 3), tf, tl, fill)
            res = [torch.full(s, fill, dtype=torch.int32, device=DEV) if o else None for s, o in zip(shapes, outs)]
            check(L.mh_person_inside(T, N, V, int(tf.shape[0]), ptr(tf), ptr(ws), ptr(tv), ptr(tp), P, *[ptr(r) for r in res], st))
            torch.cuda.synchronize()
            got = {k: None if r is None else r.cpu().numpy() for k, r in zip(NAMES, res)}
            got['status'] = status.cpu().numpy().reshape(T, N)
            if got['mask'] is not None:
                got['mask'] = got['mask'].view(np.uint32)
            runs.append(got)
    finally:
        L.mh_mesh_set_all_faces(was)
    for k in runs[0]:
        assert (runs[0][k] is None and runs[1][k] is None) or np.array_equal(runs[0][k], runs[1][k]), k
    return runs[0]


def _check_inside(verts, faces, part, P, live=None, path=None):
    want = ir.person_inside_ref(verts, faces, part, P, live)
    got = _inside(verts, faces, part, P, live)
    testable = want['status'] == 0
    assert np.array_equal(got['status'] & 3, want['status'])
    if path is not None:
        assert ((got['status'][testable] & ir.ALL_FACES) == path).all()
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    forced = _inside(verts, faces, part, P, live, force=True)
    assert ((forced['status'][testable] & ir.ALL_FACES) == ir.ALL_FACES).all()
    for k in NAMES:
        assert np.array_equal(forced[k], want[k]), 'forced ' + k
    return want


def _with_probes(base, probes):
    """a body: the mesh's vertices, then vertices that are in no face -- queries put where the test wants them (they widen
    the body's box, nothing else)"""
    return np.concatenate([base, probes]).astype(F32)


def test_one_vertex_and_one_person():
    f = np.array([[0, 0, 0]], np.int32)
    verts = np.random.default_rng(20).uniform(-1, 1, (2, 3, 1, 3)).astype(F32)
    verts[1, 2] = verts[1, 0]                               # two bodies in one point
    want = _check_inside(verts, f, np.array([3], np.uint8), 24)
    assert not want['mask'].any() and (want['depth'] == -1).all() and not want['status'].any()
    # one person per frame: nobody to be inside of
    v, f = ir.cube(0.0, 1.0)
    want = _check_inside(np.stack([v, v + F32(0.5)])[:, None], f, np.arange(8, dtype=np.uint8), 24, path=ir.ALL_FACES)
    assert not want['mask'].any() and (want['pair_depth'] == -1).all() and want['pair_verts'].shape == (2, 1, 1)


def test_cubes_with_257_vertices_dead_people_and_foreign_parts():
    """three overlapping cubes per frame, 249 probe vertices each: V = 257, one above the workgroup"""
    rng = np.random.default_rng(21)
    T, N, K = 3, 3, 249
    cubes = [ir.cube(0.0, 1.0), ir.cube(0.5, 1.5), ir.cube(0.25, 0.75)]
    f = cubes[0][1]
    verts = np.empty((T, N, 8 + K, 3), F32)
    for t in range(T):
        for n in range(N):
            probes = rng.uniform(-0.2, 1.7, (K, 3))
            probes[:20] = np.rint(probes[:20] * 4) / 4      # on the cubes' faces, edges and corners, exactly
            probes[20] = [0.6, 0.6, 0.6]                    # inside all three
            verts[t, n] = _with_probes(cubes[n][0] + F32(0.01 * t), probes)
    verts[1, 2, 30] = [np.nan, 0.6, 0.6]                    # a query that is not finite (and a vertex that is in no face)
    part = rng.integers(0, 31, 8 + K).astype(np.uint8)      # 24 .. 30: in no part
    live = np.ones((T, N), np.uint8)
    live[2, 0] = 0
    want = _check_inside(verts, f, part, 24, live)          # (the probes widen the boxes: the small cube fits the lists)
    two =np.array([bin(int(m)).count('1') for m in want['mask'].reshape(-1)]).reshape(want['mask'].shape)
    assert (two == 2).any() and (two == 1).any() and (two == 0).any()      # a vertex inside two bodies
    assert (want['mask'][:2, 0, 28] == 0b110).all() and (want['mask'][2, 1, 28] == 0b100)
    assert not want['mask'][2, 0].any() and not (want['mask'][2] & 1).any()                  # dead: as query and as container
    assert want['status'].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert (part >= 24).any() and want['part_verts'].sum() < (want['mask'] != 0).sum()
    assert want['mask'][1, 2, 30] == 0
    # without the live array everybody is there
    want = _check_inside(verts, f, part, 24, None)
    assert want['mask'][2, 0].any() and (want['mask'][2] & 1).any()


def test_spheres_take_the_grid_path_in_the_map(sphere):
    v, f = sphere
    rng = np.random.default_rng(22)
    T, N, K = 2, 3, 58                                      # V = 700: three workgroups, the last one short
    c = np.array([0.1, -0.2, 2.0])
    verts = np.empty((T, N, 642 + K, 3), F32)
    for t in range(T):
        for n, off in enumerate(([0, 0, 0], [0.5, 0.1, -0.1], [0.2, -0.45, 0.3])):
            probes = c + rng.uniform(-0.5, 1.0, (K, 3))
            verts[t, n] = _with_probes(_even_lattice(v + np.asarray(off) + 0.003 * t), probes)
    part = rng.integers(0, 24, 642 + K).astype(np.uint8)
    want = _check_inside(verts, f, part, 24, None, path=0)
    two = np.array([bin(int(m)).count('1') for m in want['mask'].reshape(-1)])
    assert (two == 2).any() and (two == 1).sum() > 100
    assert (want['pair_verts'] > 0).sum() >= 6 and (want['part_verts'] > 0).any()
    # P below the parts in use: the parts at or above it count nowhere
    small = _check_inside(verts[:1], f, part, 5, None, path=0)
    assert small['part_verts'].shape == (1, N, 5) and np.array_equal(small['part_verts'], want['part_verts'][:1, :, :5])


def test_32_people_the_top_bit_and_the_tie():
    """bodies 5 and 31 are the same cube, so a probe inside them is equally deep in both: ``other`` is the smaller, the mask
    has both bits"""
    N, K = 32, 2
    v, f = ir.cube(0.0, 1.0)
    verts = np.empty((1, N, 8 + K, 3), F32)
    for n in range(N):
        small = v * F32(0.125) + np.asarray([1.25 + 0.1875 * n, 0, 0], F32)      # the others: small cubes in a row, apart
        verts[0, n] = _with_probes(v if n in (5, 31) else small, small[:1] + F32(0.0625) + np.zeros((K, 3), F32))
    verts[0, 0, 8] = [0.5, 0.5, 0.25]                       # in bodies 5 and 31, 0.25 m from the bottom
    verts[0, 3, 9] = [0.25, 0.75, 0.875]                    # the same, 0.125 m from the top
    verts[0, 31, 8] = [1.25 + 0.1875 * 7 + 0.0625, 0.0625, 0.03125]             # body 31's probe inside body 7
    want = _check_inside(verts, f, np.zeros(8 + K, np.uint8), 1, None)
    top = np.uint32((1 << 31) | (1 << 5))
    assert want['mask'][0, 0, 8] == top and want['other'][0, 0, 8] == 5 and want['depth'][0, 0, 8] == 16384
    assert want['mask'][0, 3, 9] == top and want['other'][0, 3, 9] == 5 and want['depth'][0, 3, 9] == 8192
    assert want['mask'][0, 31, 8] == 1 << 7 and want['other'][0, 31, 8] == 7
    assert want['pair_verts'][0, 0, 31] == 1 and want['pair_verts'][0, 0, 5] == 1 and want['pair_depth'][0, 3, 31] == 8192
    assert want['mask'].view(np.int32)[0, 0, 8] < 0          # the top bit, read as the int32 it is stored in


def test_null_subsets_of_the_map_outputs(sphere):
    v, f = sphere
    verts = np.stack([v, _even_lattice(v + [0.3, 0.1, 0.0])])[None]
    part = (np.arange(642) % 24).astype(np.uint8)
    full = _inside(verts, f, part, 24)
    assert full['mask'].any()
    for outs in ((1, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1, 0, 0), (0, 0, 1, 0, 0, 1, 0), (0, 1, 0, 1, 0, 0, 1)):
        got = _inside(verts, f, part, 24, outs=outs)
        for k, o in zip(NAMES, outs):
            assert (got[k] is None) if not o else np.array_equal(got[k], full[k]), (outs, k)


def test_module_form_with_a_short_last_chunk(sphere):
    from mhhip import inside
    v, f = sphere

    class Model:
        pass
    rng = np.random.default_rng(23)
    model = Model()
    model.faces = f
    model.lbs_weights = rng.uniform(0, 1, (642, 24)).astype(F32)
    part = inside.body_parts(model)
    T, N = 3, 2
    verts = np.stack([np.stack([_even_lattice(v + [0.002 * t, 0, 0]), _even_lattice(v + [0.3, 0.1 * t, 0.05])]) for t in range(T)])
    live = np.array([[1, 1], [1, 0], [1, 1]])
    want = ir.person_inside_ref(verts, f, part, 24, live)
    metres = lambda a: np.where(a < 0, np.inf, a.astype(np.float64) * U).astype(F32)
    for chunk in (2, 8, 1):                                 # 2: the last chunk holds one frame
        got = {k: t.cpu().numpy() for k, t in inside.penetration_map(model, _dev(verts), live=live, chunk=chunk).items()}
        assert sorted(got) == ['depth_z_m', 'inside', 'inside_verts', 'mask', 'other', 'pair_depth_z_m', 'pair_verts', 'part_depth_z_m',
                               'part_verts', 'status']
        assert np.array_equal(got['mask'].view(np.uint32), want['mask']) and np.array_equal(got['inside'], want['mask'] != 0)
        assert np.array_equal(got['other'], want['other']) and np.array_equal(got['depth_z_m'], metres(want['depth']))
        assert np.array_equal(got['pair_verts'], want['pair_verts']) and np.array_equal(got['pair_depth_z_m'], metres(want['pair_depth']))
        assert np.array_equal(got['part_verts'], want['part_verts']) and np.array_equal(got['part_depth_z_m'], metres(want['part_depth']))
        assert np.array_equal(got['inside_verts'], (want['mask'] != 0).sum(-1)) and got['inside_verts'].dtype == np.int32
        assert np.array_equal(got['status'] & 3, want['status']) and not (got['status'] & 4).any()
    assert want['mask'][0].any() and not want['mask'][1].any() and want['status'][1, 1] == 1
