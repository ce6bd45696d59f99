"""``mh_vertex_normals``, ``mh_person_nearest`` and ``mh_person_pairs`` against the numpy definition (tests/proximity_ref.py),
BIT FOR BIT on every output (floats compared as int32 views): the definitions do not depend on the order anything is
visited in, so no vertex is left out.  Every call is made twice, into outputs and a workspace filled differently, and must
give the same bits both times.

Shapes: the smallest at which the kernels can go wrong -- one vertex, vertex counts around the workgroup of 256, 32 people,
several frames, and two SMPL bodies of 6890 vertices."""
import numpy as np
import pytest
import torch

import proximity_ref as pr
from test_proximity_ref import radius_edge_pair

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F = np.float32
SENTINEL = 0x7fc12345                          # a NaN with a payload: an output that is not written shows


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


# ---- normals ------------------------------------------------------------------------------------------------------------------
def _normals(verts, faces, adj_start, adj_face):
    L, check, ptr, st = _api()
    B, V = verts.shape[:2]
    tv, tf, ts = _dev(verts.astype(F)), _dev(np.asarray(faces, np.int32).reshape(-1, 3)), _dev(np.asarray(adj_start, np.int32))
    ta = _dev(np.asarray(adj_face, np.int32)) if len(adj_face) else None
    outs = []
    for fill in (SENTINEL, 7):
        out = torch.full((B, V, 3), fill, dtype=torch.int32, device=DEV).view(torch.float32)
        check(L.mh_vertex_normals(B, V, int(tf.shape[0]), ptr(tv), ptr(tf), ptr(ts), ptr(ta), len(adj_face), ptr(out), st))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(pr.bits(outs[0]), pr.bits(outs[1]))
    return outs[0]


def _csr(lists):
    start = np.zeros(len(lists) + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in lists])
    return start, np.asarray([f for l in lists for f in l], np.int32).reshape(-1)


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('V', [1, 255, 256, 257])
def test_normals_around_the_workgroup(V, B):
    rng = np.random.RandomState(10 * V + B)
    verts = rng.uniform(-1, 1, (B, V, 3)).astype(F)
    nf = 2 * V + 3
    faces = rng.randint(min(1, V - 1), V, (nf, 3))                            # vertex 0 is in no face (V > 1)
    faces[0] = [V - 1, V - 1, V - 1]                                          # zero-area faces
    faces[1] = [faces[1, 0], faces[1, 0], faces[1, 2]]
    faces[2] = [V - 1, V, V - 1]                                              # names vertices outside [0, V): skipped
    faces[3] = [-1, V - 1, V - 1]
    start, adj = pr.vertex_faces_ref(faces, V)
    lists = [adj[start[v]:start[v + 1]].tolist() for v in range(V)]
    assert V == 1 or not lists[0]                                             # the vertex without faces
    assert 2 in lists[V - 1] and 3 in lists[V - 1]                            # the faces with bad corners are in the table
    lists[V - 1] = [-1] + lists[V - 1] + [nf, nf + 100]                       # face indices outside [0, F): skipped, no fault
    start, adj = _csr(lists)
    want = pr.normals_ref(verts, faces, start, adj)
    got = _normals(verts, faces, start, adj)
    assert V == 1 or (want != 0).any()
    assert (pr.bits(got[:, 0]) == 0).all() if V > 1 else True
    assert np.array_equal(pr.bits(got), pr.bits(want))


def test_normals_of_the_smpl_faces_over_random_vertices(smpl_struct):
    from mhhip import proximity
    faces = np.asarray(smpl_struct['f'] if isinstance(smpl_struct, dict) else smpl_struct.f).astype(np.int64)
    V = 6890
    assert faces.max() == V - 1 and faces.shape == (13776, 3)
    verts = np.random.RandomState(3).uniform(-1, 1, (1, V, 3)).astype(F)
    start, adj = proximity.vertex_faces(faces, V)
    rs, ra = pr.vertex_faces_ref(faces, V)
    assert np.array_equal(start, rs) and np.array_equal(adj, ra)
    want = pr.normals_ref(verts, faces, start, adj)
    assert np.array_equal(pr.bits(_normals(verts, faces, start, adj)), pr.bits(want))
    # and through the module: the faces themselves stand in for a model
    got = proximity.vertex_normals(faces, torch.tensor(verts[0], device=DEV))
    assert np.array_equal(pr.bits(got.cpu().numpy()), pr.bits(want[0]))


# ---- nearest ------------------------------------------------------------------------------------------------------------------
def _nearest(verts, radius, live=None, want_d2=True, want_idx=True):
    L, check, ptr, st = _api()
    T, N, V = verts.shape[:3]
    tv = _dev(verts.astype(F))
    tl = None if live is None else _dev(np.asarray(live, np.uint8).reshape(T, N))
    nbytes = L.mh_person_nearest_bytes(T, N, V)
    outs = []
    for fill in (0xA5, 0x00):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        d2 = torch.full((T, N, V), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        idx = torch.full((T, N, V), SENTINEL, dtype=torch.int32, device=DEV)
        check(L.mh_person_nearest(T, N, V, ptr(tv), ptr(tl), float(radius), ptr(ws), nbytes, ptr(d2) if want_d2 else None,
                                  ptr(idx) if want_idx else None, st))
        torch.cuda.synchronize()
        outs.append((d2.cpu().numpy(), idx.cpu().numpy()))
    assert np.array_equal(pr.bits(outs[0][0]), pr.bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _same(tag, got, ref):
    bad = np.argwhere((pr.bits(got[0]) != pr.bits(ref[0])) | (got[1] != ref[1]))
    print('%s: %d vertices, %d with a candidate, %d differ' % (tag, ref[1].size, int((ref[1] >= 0).sum()), len(bad)))
    if len(bad):
        t, n, v = bad[0]
        raise AssertionError('%s: (t,n,v)=%s: got d2 %r idx %d, reference d2 %r idx %d'
                             % (tag, (t, n, v), got[0][t, n, v], got[1][t, n, v], ref[0][t, n, v], ref[1][t, n, v]))


def _boxes(rng, N, V, side=0.3, spread=0.2, at=(0.0, 1.0, 3.0)):
    """N random boxes of ``side`` whose centres lie within ``spread`` of each other: they overlap"""
    c = np.asarray(at) + rng.uniform(-spread, spread, (N, 1, 3))
    return (c + rng.uniform(-side / 2, side / 2, (N, V, 3))).astype(F)


def _lattice(rng, N, V):
    """points of an integer lattice scaled by 2^-6: every difference and square is exact, equal distances abound"""
    return (rng.randint(0, 8, (N, V, 3)) * F(2.0 ** -6) + np.array([0.5, 1.0, 2.0], F)).astype(F)


@pytest.mark.parametrize('shape', [(1, 2, 1), (3, 3, 257), (2, 32, 5)])
def test_nearest_shapes_on_overlapping_boxes(shape):
    T, N, V = shape
    rng = np.random.RandomState(sum(shape))
    side, spread = {1: (0.05, 0.03), 5: (0.3, 0.1), 257: (0.3, 0.25)}[V]
    verts = np.stack([_boxes(rng, N, V, side=side, spread=spread) for _ in range(T)])
    ref = pr.nearest_ref(verts, 0.1)
    assert (ref[1] >= 0).any() and (V < 100 or (ref[1] < 0).any())
    _same('boxes %s' % (shape,), _nearest(verts, 0.1), ref)


def test_nearest_either_output_alone():
    rng = np.random.RandomState(4)
    verts = np.stack([_boxes(rng, 3, 70) for _ in range(2)])
    ref = pr.nearest_ref(verts, 0.1)
    d2, idx = _nearest(verts, 0.1, want_idx=False)
    assert np.array_equal(pr.bits(d2), pr.bits(ref[0])) and (idx == SENTINEL).all()
    d2, idx = _nearest(verts, 0.1, want_d2=False)
    assert np.array_equal(idx, ref[1]) and (pr.bits(d2) == SENTINEL).all()


def test_nearest_lattice_ties_and_duplicates_across_persons():
    rng = np.random.RandomState(5)
    T, N, V = 2, 3, 257
    verts = np.stack([_lattice(rng, N, V) for _ in range(T)])
    verts[1, 2, :100] = verts[1, 0, 50:150]                # person 2 repeats points of person 0 (and of 1: the lattice is small)
    for radius in (0.05, 0.02):
        ref = pr.nearest_ref(verts, radius)
        # the tie rule decides: count the vertices whose smallest d2 is attained by more than one candidate
        tied = 0
        for t in range(T):
            pts = verts[t].reshape(-1, 3)
            for n in range(N):
                e = pts[None] - verts[t, n][:, None]
                d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                d2[:, n * V:(n + 1) * V] = np.inf
                tied += int(((d2 == ref[0][t, n][:, None]).sum(1) > 1)[ref[1][t, n] >= 0].sum())
        assert tied > 500, tied
        assert (ref[0] == 0).sum() > 100                   # duplicates across persons: distance 0
        _same('lattice r=%g' % radius, _nearest(verts, radius), ref)


def test_nearest_ignores_the_own_body():
    rng = np.random.RandomState(6)
    V = 300
    own = (np.array([0.0, 1.0, 3.0]) + rng.uniform(-1e-3, 1e-3, (V, 3))).astype(F)        # a cluster 2 mm wide
    other = (np.array([0.05, 1.0, 3.0]) + rng.uniform(-0.02, 0.02, (V, 3))).astype(F)     # 3 to 7 cm away
    verts = np.stack([own, other])[None]
    ref = pr.nearest_ref(verts, 0.1)
    assert (ref[1][0, 0] >= V).all() and (ref[0][0, 0] > 0.02 ** 2).all()                 # never one of its own
    _same('own body', _nearest(verts, 0.1), ref)


def test_nearest_people_far_apart_find_nobody():
    rng = np.random.RandomState(7)
    verts = np.stack([_boxes(rng, 3, 257, spread=0.0) for _ in range(2)])
    verts[:, 1, :, 0] += F(5.0)
    verts[:, 2, :, 2] += F(5.0)
    for radius in (0.1, 0.64):
        d2, idx = _nearest(verts, radius)
        assert np.isinf(d2).all() and (d2 > 0).all() and (idx == -1).all()
    _same('far apart', (d2, idx), pr.nearest_ref(verts, 0.64))


def test_nearest_body_inside_anothers_box_and_a_coincident_body():
    rng = np.random.RandomState(8)
    V = 257
    big = _boxes(rng, 1, V, side=0.5, spread=0.0)[0]
    small = _boxes(rng, 1, V, side=0.05, spread=0.0)[0]                                   # wholly inside big's box
    point = np.tile(np.array([[0.1, 1.05, 3.1]], F), (V, 1))                             # a body of zero extent
    verts = np.stack([np.stack([big, small, point]), np.stack([point, point + F(0.03125), big])])
    for radius in (0.05, 0.3):
        ref = pr.nearest_ref(verts, radius)
        assert (ref[1][0, 1] >= 0).any() and (ref[1][1, 0] >= 0).any()
        _same('inside / coincident r=%g' % radius, _nearest(verts, radius), ref)


def test_nearest_around_z_50_metres():
    rng = np.random.RandomState(9)
    verts = np.stack([_boxes(rng, 3, 257, at=(2.0, -1.0, 50.0)) for _ in range(2)])       # ulp 4e-6 m: coarse differences
    verts[1] = _lattice(rng, 3, 257) + np.array([0, 0, 48.0], F)
    ref = pr.nearest_ref(verts, 0.1)
    assert (ref[1] >= 0).sum() > 500
    _same('z = 50', _nearest(verts, 0.1), ref)


def test_nearest_dead_persons_as_queries_and_targets():
    rng = np.random.RandomState(10)
    T, N, V = 3, 3, 100
    verts = np.stack([_boxes(rng, N, V, spread=0.05) for _ in range(T)])
    live = np.array([[1, 0, 1], [0, 0, 1], [2, 255, 0]], np.uint8)                       # any value but 0 is live
    ref = pr.nearest_ref(verts, 0.2, live)
    assert (ref[1][0, 1] == -1).all() and (ref[1][1] == -1).all()                         # dead, and alone among the dead
    assert (ref[1][0, 0] // V == 2).all() and (ref[1][2, 0] // V == 1).all()
    _same('live mask', _nearest(verts, 0.2, live), ref)
    _same('all live', _nearest(verts, 0.2, np.ones((T, N))), pr.nearest_ref(verts, 0.2))


def test_nearest_survives_vertices_that_are_not_finite():
    rng = np.random.RandomState(11)
    T, N, V = 2, 3, 257
    verts = np.stack([_boxes(rng, N, V, spread=0.05) for _ in range(T)])
    ref_clean = pr.nearest_ref(verts, 0.15)
    bad = rng.rand(T, N, V) < 0.1
    bad[1, 2] = True                                       # a body without one untouched vertex
    vals = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F)          # (+-3e38 is finite: such vertices stay in, and make
    broken = verts.copy()                                               # a box whose extent overflows float32)
    which = np.argwhere(bad)
    broken[which[:, 0], which[:, 1], which[:, 2], rng.randint(0, 3, len(which))] = vals[rng.randint(0, 5, len(which))]
    broken[0, 1, :, :][bad[0, 1]] = np.nan                 # (and a body whose bad vertices are all NaN)
    ref = pr.nearest_ref(broken, 0.15)
    fin = np.isfinite(broken).all(-1)
    assert (~fin).sum() > 100 and (ref[1][~fin] == -1).all()
    found = np.argwhere(ref[1] >= 0)
    assert fin.reshape(T, N * V)[found[:, 0], ref[1][ref[1] >= 0]].all()                  # no target that is not finite
    assert (ref[1] != ref_clean[1]).sum() > (~fin).sum()   # they are missed as targets too
    _same('not finite', _nearest(broken, 0.15), ref)


def test_nearest_radius_edge_pair():
    verts, r = radius_edge_pair()
    ref = pr.nearest_ref(verts, r)
    assert ref[1].reshape(-1).tolist() == [2, -1, 0, -1]
    _same('radius edge', _nearest(verts, r), ref)


@pytest.mark.parametrize('radius', [0.64, 1e-4])
def test_nearest_largest_and_a_tiny_radius(radius):
    rng = np.random.RandomState(12)
    verts = np.stack([_boxes(rng, 3, 257, spread=0.3) for _ in range(2)])
    verts[1, 1, :50] = verts[1, 0, :50] + (rng.uniform(-1, 1, (50, 3)) * 1e-4).astype(F)  # within about the tiny radius
    ref = pr.nearest_ref(verts, radius)
    found = ref[1][1, 1, :50] >= 0
    assert found.any() and (radius > 0.1 or not found.all())
    _same('r=%g' % radius, _nearest(verts, radius), ref)


@pytest.fixture(scope='module')
def bodies(smpl_struct, smpl_regs):
    """2 posed bodies of the synthetic model, the second moved until the centres are 0.3 m apart: arms and flanks in reach"""
    from mhhip import engine, synthetic
    model = engine.BodyModel(smpl_struct, smpl_regs)
    N = 2
    sp = synthetic.make_sequence_params(N, 1, 31, (2.6, 3.6))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=F)).to(DEV)
    verts, _, _, _ = model.lbs_forward(t(sp['betas_gt']), t(sp['poses_gt']).view(N, 72), None, t(sp['trans_gt']).view(N, 3), want_vposed=False)
    verts = verts.view(N, -1, 3).cpu().numpy().astype(F)
    verts[1] += (verts[0].mean(0) - verts[1].mean(0) + np.array([0.3, 0.0, 0.0])).astype(F)
    return model, verts[None]


@pytest.fixture(scope='module')
def bodies_ref(bodies):
    """the reference over the two bodies at radius 0.1, computed once"""
    model, verts = bodies
    return pr.nearest_ref(verts, 0.1)


def test_nearest_two_smpl_bodies(bodies, bodies_ref):
    model, verts = bodies
    assert verts.shape == (1, 2, 6890, 3)
    assert (bodies_ref[1] >= 0).sum() > 200 and (bodies_ref[1] < 0).sum() > 200
    _same('two bodies', _nearest(verts, 0.1), bodies_ref)


# ---- pairs --------------------------------------------------------------------------------------------------------------------
KEYS = ['behind', 'pair_verts', 'pair_min_d2', 'pair_behind', 'part_verts', 'part_min_key']


def _pairs(verts, normals, d2, idx, part, P, thr):
    L, check, ptr, st = _api()
    T, N, V = verts.shape[:3]
    tv, tn, td, ti, tp = _dev(verts.astype(F)), _dev(normals), _dev(d2.astype(F)), _dev(idx.astype(np.int32)), _dev(part.astype(np.uint8))
    outs = []
    for fill in (-7, 123456):                              # whatever the outputs held is overwritten
        o = dict(behind=torch.full((T, N, V), fill & 0xff, dtype=torch.uint8, device=DEV),
                 pair_verts=torch.full((T, N, N), fill, dtype=torch.int32, device=DEV),
                 pair_min_d2=torch.full((T, N, N), float(fill), dtype=torch.float32, device=DEV),
                 pair_behind=torch.full((T, N, N), fill, dtype=torch.int32, device=DEV),
                 part_verts=torch.full((T, N, P), fill, dtype=torch.int32, device=DEV),
                 part_min_key=torch.full((T, N, P), fill, dtype=torch.int64, device=DEV))
        check(L.mh_person_pairs(T, N, V, ptr(tv), ptr(tn), ptr(td), ptr(ti), ptr(tp), P, float(thr), *[ptr(o[k]) for k in KEYS], st))
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in o.items()}
        o['part_min_key'] = o['part_min_key'].view(np.uint64)
        outs.append(o)
    for k in KEYS:
        assert np.array_equal(_raw(outs[0][k]), _raw(outs[1][k])), k
    return outs[0]


def _raw(a):
    return pr.bits(a) if a.dtype == np.float32 else a


def _same_pairs(tag, got, want):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k)
        assert np.array_equal(_raw(got[k]), _raw(want[k])), (tag, k)


@pytest.mark.parametrize('V', [1, 257, 600])
def test_pairs_with_vertex_counts_straddling_the_workgroup(V):
    rng = np.random.RandomState(V)
    T, N, P = 2, 3, 24
    verts = np.stack([_boxes(rng, N, V, spread=0.05) for _ in range(T)])
    normals = rng.randn(T, N, V, 3).astype(F)
    part = rng.randint(0, P + 6, V).astype(np.uint8)       # values >= P count nowhere
    part[part == 5] = 6                                    # a part without a vertex
    d2, idx = pr.nearest_ref(verts, 0.2)
    want = pr.pairs_ref(verts, normals, d2, idx, part, P, 0.08)
    assert want['pair_verts'].sum() > 0 and (V == 1 or 0 < want['behind'].sum() < idx.size)
    assert V == 1 or (part >= P).any() and want['part_verts'].sum() < want['pair_verts'].sum()
    _same_pairs('V=%d' % V, _pairs(verts, normals, d2, idx, part, P, 0.08), want)


def test_pairs_third_person_nearest_no_normals_and_zero_threshold():
    rng = np.random.RandomState(21)
    V, P = 300, 4
    a = _boxes(rng, 1, V, side=0.2, spread=0.0)[0]
    verts = np.stack([a, a + np.array([0.25, 0, 0], F), a + np.array([0.0625, 0, 0], F)])[None]       # 2 lies between 0 and 1
    verts[0, 1, 7] = verts[0, 0, 9]                        # one exact coincidence: d2 = 0
    part = rng.randint(0, P, V).astype(np.uint8)
    d2, idx = pr.nearest_ref(verts, 0.1)
    other = idx[0, 0][idx[0, 0] >= 0] // V
    assert (other == 2).sum() > (other == 1).sum() >= 1
    want = pr.pairs_ref(verts, None, d2, idx, part, P, 0.05)
    assert want['pair_verts'][0, 0, 2] > 0 and not want['behind'].any() and not want['pair_behind'].any()
    _same_pairs('no normals', _pairs(verts, None, d2, idx, part, P, 0.05), want)
    # thr = 0: only the coincident pair is in contact; the minima do not move
    zero = pr.pairs_ref(verts, None, d2, idx, part, P, 0.0)
    assert zero['pair_verts'][0, 0, 1] == 1 and zero['pair_verts'][0, 1, 0] == 1 and zero['pair_verts'].sum() == 2
    assert np.array_equal(zero['part_min_key'], want['part_min_key'])
    _same_pairs('thr=0', _pairs(verts, None, d2, idx, part, P, 0.0), zero)


def test_pair_minimum_is_symmetric_between_two_people(bodies, bodies_ref):
    from mhhip import contact, proximity
    model, verts = bodies
    d2, idx = bodies_ref
    part = contact.body_parts(model)
    start, adj = proximity.vertex_faces(model.faces, 6890)
    normals = pr.normals_ref(verts[0], model.faces, start, adj)[None]
    want = pr.pairs_ref(verts, normals, d2, idx, part, 24, 0.05)
    got = _pairs(verts, normals, d2, idx, part, 24, 0.05)
    _same_pairs('two bodies', got, want)
    assert np.isfinite(got['pair_min_d2'][0, 0, 1])
    assert pr.bits(got['pair_min_d2'])[0, 0, 1] == pr.bits(got['pair_min_d2'])[0, 1, 0]
    assert np.isinf(got['pair_min_d2'][0, 0, 0]) and got['pair_verts'][0, 0, 0] == 0


# ---- the module -----------------------------------------------------------------------------------------------------------------
def test_module_equals_the_reference_and_does_not_depend_on_the_chunk():
    from mhhip import proximity
    rng = np.random.RandomState(31)
    T, N, V, P = 5, 3, 257, 24
    verts = np.stack([_boxes(rng, N, V, spread=0.05) for _ in range(T)])
    live = rng.rand(T, N) < 0.8
    live[0] = True
    faces = rng.randint(0, V, (2 * V, 3))
    weights = np.zeros((V, 24), F)
    weights[np.arange(V), rng.randint(0, 24, V)] = 1.0

    class Model:                                           # what the module reads of a body model
        pass
    model = Model()
    model.faces, model.lbs_weights = faces, weights
    tv = torch.tensor(verts, device=DEV)
    full = proximity.proximity_map(model, tv, live=live, radius=0.2, contact=0.08, nearest=True, chunk=T)
    for chunk in (1, 2):
        other = proximity.proximity_map(model, tv, live=live, radius=0.2, contact=0.08, nearest=True, chunk=chunk)
        assert sorted(other) == sorted(full)
        for k in full:
            a, b = full[k].cpu().numpy(), other[k].cpu().numpy()
            assert np.array_equal(_raw(a), _raw(b)), (chunk, k)
    again = proximity.proximity_map(model, tv, live=live, radius=0.2, contact=0.08, nearest=True, chunk=T)
    for k in full:
        assert np.array_equal(_raw(full[k].cpu().numpy()), _raw(again[k].cpu().numpy())), k
    assert 'nearest' not in proximity.proximity_map(model, tv) and 'other_vert' not in proximity.proximity_map(model, tv)
    # against the definition
    got = {k: v.cpu().numpy() for k, v in full.items()}
    d2, idx = pr.nearest_ref(verts, 0.2, live)
    nd2, nidx = proximity.person_nearest(tv, 0.2, live)
    assert np.array_equal(pr.bits(nd2.cpu().numpy()), pr.bits(d2)) and np.array_equal(nidx.cpu().numpy(), idx)
    part = np.argmax(weights, 1).astype(np.uint8)
    start, adj = pr.vertex_faces_ref(faces, V)
    normals = pr.normals_ref(verts.reshape(T * N, V, 3), faces, start, adj).reshape(T, N, V, 3)
    want = pr.pairs_ref(verts, normals, d2, idx, part, P, 0.08)
    has = idx >= 0
    assert has.any() and want['behind'].any() and want['pair_verts'].sum() > 0
    assert np.array_equal(got['contact'], has & (d2 <= F(0.08) * F(0.08))) and got['contact'].dtype == np.bool_
    assert np.array_equal(got['behind'], want['behind'] != 0) and np.array_equal(got['other'], np.where(has, idx // V, -1))
    assert np.array_equal(got['other_vert'], np.where(has, idx % V, -1))
    for k in ('pair_verts', 'pair_behind', 'part_verts'):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == np.int32, k
    assert np.array_equal(got['contact_verts'], got['contact'].sum(-1)) and np.array_equal(got['behind_verts'], got['behind'].sum(-1))
    kd, ki = pr.decode_key(want['part_min_key'])
    assert np.array_equal(got['part_other'], np.where(ki >= 0, ki // V, -1))
    assert np.array_equal(got['part_other_part'], np.where(ki >= 0, part.astype(np.int32)[np.maximum(ki, 0) % V], -1))
    near = np.where(has[..., None], verts.reshape(T, N * V, 3)[np.arange(T)[:, None, None], np.maximum(idx, 0)], 0)
    assert np.array_equal(pr.bits(got['nearest']), pr.bits(near.astype(F)))
    for name, sq in (('dist_m', d2), ('pair_min_m', want['pair_min_d2']), ('part_min_m', kd)):      # a square root within 2 ulp
        root, fin = np.sqrt(sq.astype(np.float64)), np.isfinite(sq)
        assert np.array_equal(np.isinf(got[name]), ~fin), name
        assert (np.abs(got[name][fin] - root[fin]) <= 2.0 ** -22 * root[fin]).all(), name
    # one person per frame is not an error
    alone = proximity.proximity_map(model, tv[:, :1])
    assert torch.isinf(alone['dist_m']).all() and (alone['other'] == -1).all() and (alone['part_other'] == -1).all()
    assert not alone['contact'].any() and not alone['behind'].any() and (alone['pair_verts'] == 0).all()
    assert torch.isinf(alone['pair_min_m']).all() and torch.isinf(alone['part_min_m']).all() and (alone['contact_verts'] == 0).all()
