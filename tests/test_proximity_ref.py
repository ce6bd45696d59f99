"""The numpy restatement of the person-to-person contact map (tests/proximity_ref.py) on cases small enough to check by
hand: it is the yardstick of the device tests, so its own reading of the definitions is pinned here."""
import numpy as np

import proximity_ref as pr

F = np.float32

TET = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
TET_FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])          # outward
CUBE = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)          # vertex = x + 2 y + 4 z
CUBE_FACES = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4],
                       [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]])  # outward


def test_two_tetrahedra():
    a = TET * F(0.1)
    b = a + np.array([0.125, 0, 0], F)                    # b's vertex 0 is 0.025 beyond a's vertex 1
    d2, idx = pr.nearest_ref(np.stack([a, b])[None], 0.05)
    assert d2.shape == (1, 2, 4) and idx.dtype == np.int32
    # a's vertex 1 (0.1,0,0) and b's vertex 0 (0.125,0,0) see each other; idx = m V + u
    assert idx[0, 0, 1] == 1 * 4 + 0 and idx[0, 1, 0] == 0 * 4 + 1
    gap = b[0, 0] - a[1, 0]                               # (0.1 is no binary fraction: the gap as float32 gives it)
    assert d2[0, 0, 1] == gap * gap == d2[0, 1, 0] and abs(gap - 0.025) < 1e-8
    # a's vertex 0 is 0.125 from b's vertex 0: out of reach, like everything else
    assert idx[0, 0, 0] == -1 and np.isinf(d2[0, 0, 0])
    assert (idx >= 0).sum() == 2


def test_two_cubes_and_the_pair_tables():
    a = CUBE * F(0.25)
    b = a + np.array([0.25 + 0.0625, 0, 0], F)            # a gap of 1/16 between a's x = 0.25 face and b's x = 0 face
    verts = np.stack([a, b])[None]
    d2, idx = pr.nearest_ref(verts, 0.1)
    right, left = [1, 3, 5, 7], [0, 2, 4, 6]
    assert (idx[0, 0, right] == 4 * 0 + 8 + np.array(left)).all() and (idx[0, 1, left] == np.array(right)).all()
    assert (d2[0, 0, right] == F(0.0625) ** 2).all() and np.isinf(d2[0, 0, left]).all()
    start, adj = pr.vertex_faces_ref(CUBE_FACES, 8)
    normals = pr.normals_ref(verts[0], CUBE_FACES, start, adj)[None]
    part = np.array([0, 1, 0, 1, 2, 3, 2, 3], np.uint8)   # by x and z
    out = pr.pairs_ref(verts, normals, d2, idx, part, 4, 0.0625)
    assert out['pair_verts'].tolist() == [[[0, 4], [4, 0]]] and out['pair_behind'].tolist() == [[[0, 0], [0, 0]]]
    assert not out['behind'].any()                        # each is outside the other
    assert out['pair_min_d2'][0, 0, 1] == out['pair_min_d2'][0, 1, 0] == F(0.0625) ** 2
    assert np.isinf(out['pair_min_d2'][0, 0, 0]) and np.isinf(out['pair_min_d2'][0, 1, 1])
    assert out['part_verts'].tolist() == [[[0, 2, 0, 2], [2, 0, 2, 0]]]
    kd, ki = pr.decode_key(out['part_min_key'])
    assert kd[0, 0, 1] == F(0.0625) ** 2 and ki[0, 0, 1] == 8 + 0          # part 1 of a = vertices 1, 3: the smaller idx of a tie
    assert np.isinf(kd[0, 0, 0]) and ki[0, 0, 0] == -1
    # below the gap nothing is in contact, the minima stay
    none = pr.pairs_ref(verts, normals, d2, idx, part, 4, 0.06)
    assert not none['pair_verts'].any() and not none['part_verts'].any()
    assert np.array_equal(none['pair_min_d2'], out['pair_min_d2']) and np.array_equal(none['part_min_key'], out['part_min_key'])
    # b pushed INTO a by 1/16: its left face lies behind a's right face, and the other way round
    b2 = a + np.array([0.25 - 0.0625, 0, 0], F)
    v2 = np.stack([a, b2])[None]
    d2b, idxb = pr.nearest_ref(v2, 0.1)
    n2 = pr.normals_ref(v2[0], CUBE_FACES, start, adj)[None]
    inn = pr.pairs_ref(v2, n2, d2b, idxb, part, 4, 0.0625)
    assert inn['behind'][0, 1, left].all() and inn['behind'][0, 0, right].all()
    assert inn['pair_behind'].tolist() == [[[0, 4], [4, 0]]]
    # without normals nothing is behind
    flat = pr.pairs_ref(v2, None, d2b, idxb, part, 4, 0.0625)
    assert not flat['behind'].any() and not flat['pair_behind'].any() and np.array_equal(flat['pair_verts'], inn['pair_verts'])


def test_tie_rule_smaller_person_then_smaller_vertex():
    q = np.zeros((2, 3), F)
    q[1] = [5, 5, 5]
    one = np.array([[0.0625, 0, 0], [0, 0.0625, 0]], F)   # both at the same distance from q[0]
    two = np.array([[0, 0, 0.0625], [-0.0625, 0, 0]], F)
    d2, idx = pr.nearest_ref(np.stack([q, one, two])[None], 0.1)
    assert idx[0, 0, 0] == 1 * 2 + 0 and d2[0, 0, 0] == F(0.0625) ** 2
    d2, idx = pr.nearest_ref(np.stack([q, one[::-1], two])[None], 0.1)
    assert idx[0, 0, 0] == 1 * 2 + 0                      # still the smaller vertex of the smaller person
    d2, idx = pr.nearest_ref(np.stack([one, two, q])[None], 0.1)
    assert idx[0, 2, 0] == 0                              # person 0, vertex 0


def test_live_mask():
    a = TET * F(0.1)
    verts = np.stack([a, a + F(0.01), a + F(0.02)])[None]
    d2, idx = pr.nearest_ref(verts, 0.1, live=[[1, 0, 1]])
    assert (idx[0, 1] == -1).all() and np.isinf(d2[0, 1]).all()              # dead as a query
    assert (idx[0, 0] // 4 == 2).all() and (idx[0, 2] // 4 == 0).all()       # and as a target: 0 and 2 see each other only
    d2, idx = pr.nearest_ref(verts, 0.1)
    assert (idx[0, 0] // 4 == 1).all()
    # frames do not see each other
    two = np.concatenate([verts, verts + F(3)])[:, :1]
    assert (pr.nearest_ref(two, 0.64)[1] == -1).all()


def test_third_person_nearer_than_the_second():
    q = np.zeros((1, 3), F)
    verts = np.stack([q, q + F(0.05), q + F(0.02)])[None]
    d2, idx = pr.nearest_ref(verts, 0.2)
    assert idx[0, 0, 0] == 2 and idx[0, 1, 0] == 2 and idx[0, 2, 0] == 0
    out = pr.pairs_ref(verts, None, d2, idx, np.zeros(1, np.uint8), 1, 0.2)
    assert out['pair_verts'][0].tolist() == [[0, 0, 1], [0, 0, 1], [1, 0, 0]]


def test_radius_edge_pair():
    verts, r = radius_edge_pair()
    d2, idx = pr.nearest_ref(verts, r)
    r2 = F(r) * F(r)
    assert d2[0, 0, 0] == r2 and idx[0, 0, 0] == 1 * 2 + 0                   # exactly at the radius: in
    assert np.isinf(d2[0, 0, 1]) and idx[0, 0, 1] == -1                      # one float beyond: out
    assert d2[0, 1, 0] == r2 and idx[0, 1, 0] == 0 and idx[0, 1, 1] == -1


def radius_edge_pair():
    """(verts (1,2,2,3), radius): vertex 0 of either person has d2 == fl(r r) exactly, vertex 1 the next float above it"""
    r = F(0.25)
    verts = np.zeros((1, 2, 2, 3), F)
    verts[0, :, 1] = [[8, 0, 0], [8, 0, 0]]
    verts[0, 1, 0, 0] = r
    verts[0, 1, 1, 1] = np.nextafter(r, F(1))             # 8 and 0.25 (1 + 2^-23) are exact; d2 = fl(r'^2) > r^2
    e = verts[0, 1, 1] - verts[0, 0, 1]
    assert (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > r * r
    return verts, r


def test_vertex_faces_on_a_cube():
    from mhhip import proximity
    start, adj = proximity.vertex_faces(CUBE_FACES, 8)
    rs, ra = pr.vertex_faces_ref(CUBE_FACES, 8)
    assert start.dtype == np.int32 and adj.dtype == np.int32
    assert np.array_equal(start, rs) and np.array_equal(adj, ra)
    assert start[0] == 0 and start[-1] == 36 == len(adj)
    for v in range(8):
        mine = adj[start[v]:start[v + 1]]
        assert (np.diff(mine) > 0).all() and all(v in CUBE_FACES[f] for f in mine)        # ascending face index
        assert len(mine) == (CUBE_FACES == v).sum()
    # a degenerate face is listed once per corner that names the vertex; a corner outside [0, V) is left out
    faces = np.array([[0, 1, 2], [3, 3, 1], [2, 2, 2], [0, 9, -1]])
    start, adj = proximity.vertex_faces(faces, 4)
    assert [adj[start[v]:start[v + 1]].tolist() for v in range(4)] == [[0, 3], [0, 1], [0, 2, 2, 2], [1, 1]]
    rs, ra = pr.vertex_faces_ref(faces, 4)
    assert np.array_equal(start, rs) and np.array_equal(adj, ra)


def test_unnormalised_normals_of_a_closed_cube_point_outward():
    start, adj = pr.vertex_faces_ref(CUBE_FACES, 8)
    verts = (CUBE * F(0.5) + np.array([1, 2, 3], F))[None]
    n = pr.normals_ref(verts, CUBE_FACES, start, adj)[0]
    centre = verts[0].mean(0)
    assert ((n * (verts[0] - centre)).sum(1) > 0).all()
    assert (np.sign(n) == np.sign(verts[0] - centre)).all()                  # every component, by symmetry of the corner
    assert not np.allclose(np.linalg.norm(n, axis=1), 1.0)                   # area-weighted, not unit length
    # a vertex without faces, and faces that are skipped
    faces = np.array([[0, 1, 2], [0, 1, 7], [0, 2, 1]])
    s4, a4 = pr.vertex_faces_ref(faces, 4)
    n = pr.normals_ref(TET[None], faces, s4, a4)[0]
    assert (n[3] == 0).all() and (n[0] == 0).all()                           # face 1 names vertex 7: nothing; 0 and 2 cancel
    tet = pr.normals_ref(TET[None], TET_FACES, *pr.vertex_faces_ref(TET_FACES, 4))[0]
    assert ((tet * (TET - TET.mean(0))).sum(1) > 0).all()


def test_key_decoding():
    d2 = np.array([0.0, 1e-6, 0.25, 1e-6], F)
    idx = np.array([5, 70000, 2 ** 31 - 1, 3], np.int32)
    key = pr.make_key(d2, idx)
    assert key.dtype == np.uint64 and key[0] == 5 and key[3] < key[1] < key[2]           # d2 first, then idx
    kd, ki = pr.decode_key(np.concatenate([key, [pr.ALL_ONES]]))
    assert np.array_equal(pr.bits(kd[:4]), pr.bits(d2)) and np.array_equal(ki[:4], idx)
    assert np.isinf(kd[4]) and ki[4] == -1
    # the module's decoder reads the same bits (as int64, the all-ones key is -1)
    import torch
    from mhhip import proximity
    part = torch.arange(8, dtype=torch.uint8)
    keys = torch.tensor(np.array([pr.make_key(np.array([0.04], F), np.array([2 * 8 + 3]))[0], pr.ALL_ONES]).view(np.int64))
    got = proximity.decode_keys(keys, 8, part)
    assert got[0][0].item() == float(F(0.04)) and got[1].tolist() == [2, -1] and got[2].tolist() == [3, -1]
    assert torch.isinf(got[0][1])
