"""The contact term's neighbour searches (k_contact_knn, the bucket grid and k_contact_knn_grid) against the float64
reference of tests/knn_cases.py at their edges: k below 32, clouds around k / the 64-point chunk / the four-wave split,
clamped extents and cells, one cell with thousands of points, the 2^20-cell cap, queries on points, on the bounding box
and outside it; the device-count build with stale rows behind the count, rebuilt in place from a large cloud to a small
one; the two-grid form against two different clouds; the key form on bodies whose lowest vertex is tied.

Tolerance on dy: atol 2e-5, rtol 1e-5 as in test_scene_knn_gpu.py (all |y| <= 4).  A query is compared unless float32
cannot tell its k-th from its (k+1)-th neighbour (knn_cases: the decided rule); tests/test_scene_knn_cases.py bounds
how many those are, without a GPU.

Measured on an MI355X (worst |dy - dy_ref| over the checked queries; the tolerance is >= 2e-5): every case and every
form between 0 and 2.4e-7 -- the k sweeps 0 .. 1.6e-7 (k = 1: 0 and 7.5e-9), M = 1 .. 257 1.5e-8 .. 8.9e-8, planes
5.4e-8 .. 7.5e-8, line_y 2.4e-7 (2 of 128 queries skipped, the only skips anywhere), identical 5.2e-8, speck 1.3e-7,
beam 1.3e-7, outlier_span 1.6e-7, two_clusters 8.9e-8, cell_cap 1.5e-7, query_positions 1.8e-7, brute force and grid
within 5e-8 of each other; device-count builds and rebuilds 6.0e-8 .. 1.4e-7, two-grid form 1.1e-7, key form 1.0e-7.
Each test prints its own figure (-s)."""
import numpy as np
import pytest
import torch

import knn_cases as kc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _api():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr(torch.device(DEV))


def _workspace(L, M):
    # 0xA5 everywhere: a build must not rely on anything a workspace held before
    return torch.full((L.mh_scene_grid_bytes(M),), 0xA5, dtype=torch.uint8, device=DEV)


def _brute(pts, q, k):
    L, check, ptr, st = _api()
    tp, tq = torch.tensor(pts, device=DEV), torch.tensor(q, device=DEV)
    dy = torch.full((q.shape[0],), float('nan'), device=DEV)
    check(L.mh_contact_knn(ptr(tp), pts.shape[0], ptr(tq), q.shape[0], k, ptr(dy), st))
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def _grid(pts, q, k):
    L, check, ptr, st = _api()
    M = pts.shape[0]
    tp, tq = torch.tensor(pts, device=DEV), torch.tensor(q, device=DEV)
    ws = _workspace(L, M)
    check(L.mh_scene_grid_build(ptr(tp), M, ptr(ws), st))
    dy = torch.full((q.shape[0],), float('nan'), device=DEV)
    check(L.mh_contact_knn_grid(ptr(ws), M, ptr(tq), q.shape[0], k, ptr(dy), st))
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def _compare(tag, got, ref):
    """every output finite, every checked query within the tolerance; prints the worst error and the skipped count"""
    err = np.abs(got.astype(np.float64) - ref.dy)
    over = err - kc.tolerance(ref.dy)
    worst = float(err[ref.checked].max())
    print('%s: worst |dy - dy_ref| %.3e over %d checked queries, %d skipped' % (tag, worst, int(ref.checked.sum()), int((~ref.checked).sum())))
    assert np.isfinite(got).all(), tag
    bad = np.nonzero(ref.checked & (over > 0))[0]
    assert bad.size == 0, '%s: %d queries off, first %d: got %.7g, reference %.7g (swap %.7g)' % (
        tag, bad.size, bad[0], got[bad[0]], ref.dy[bad[0]], ref.swap[bad[0]])


@pytest.mark.parametrize('kernel', ['brute', 'grid'])
@pytest.mark.parametrize('name', kc.NAMES)
def test_neighbour_search_at_its_edges(name, kernel):
    c, ref = kc.case(name), kc.case_reference(name)
    got = (_brute if kernel == 'brute' else _grid)(c.pts, c.q, c.k)
    _compare('%s/%s' % (name, kernel), got, ref)


# ---------------------------------------------------------------------------------------------------------------
# device-count build: rows behind the count are not part of the cloud
# ---------------------------------------------------------------------------------------------------------------
M_CAP = 4000


def _counted_cloud():
    rng = np.random.RandomState(41)
    base = np.stack([rng.uniform(-2, 2, M_CAP), 1.0 + 0.3 * rng.randn(M_CAP).clip(-3, 3), rng.uniform(2, 6, M_CAP)], 1).astype(np.float32)
    q = (base[rng.randint(0, M_CAP, 96)] + 0.3 * rng.randn(96, 3)).astype(np.float32)
    return base, q


def _counted_build_and_query(ws, base, q, m_dev):
    """rows [m_dev, M_CAP) are decoys exactly on the queries: they would win every search if they were read"""
    L, check, ptr, st = _api()
    buf = base.copy()
    n = M_CAP - m_dev
    buf[m_dev:] = q[np.arange(n) % q.shape[0]]
    tp, tq = torch.tensor(buf, device=DEV), torch.tensor(q, device=DEV)
    cnt = torch.tensor([m_dev], dtype=torch.int32, device=DEV)
    check(L.mh_scene_grid_build_dev(ptr(tp), ptr(cnt), M_CAP, ptr(ws), st))
    dy = torch.full((q.shape[0],), float('nan'), device=DEV)
    check(L.mh_contact_knn_grid(ptr(ws), M_CAP, ptr(tq), q.shape[0], 32, ptr(dy), st))
    torch.cuda.synchronize()
    return dy.cpu().numpy()


@pytest.fixture(scope='module')
def counted():
    base, q = _counted_cloud()
    refs = {m: kc.reference(base[:m], q, 32) for m in (1, 31, 2000, 4000)}
    for m, r in refs.items():
        assert (~r.checked).sum() <= 0.02 * q.shape[0]
        # the decoys matter: with them the answer would be another one
        if m < M_CAP:
            buf = base.copy()
            buf[m:] = q[np.arange(M_CAP - m) % q.shape[0]]
            with_decoys = kc.reference(buf, q, 32).dy
            assert (np.abs(with_decoys - r.dy) > 4 * kc.tolerance(r.dy)).mean() > 0.9
    return base, q, refs


@pytest.mark.parametrize('m_dev', [1, 31, 2000, 4000])
def test_device_count_build_ignores_rows_behind_the_count(counted, m_dev):
    base, q, refs = counted
    L = _api()[0]
    got = _counted_build_and_query(_workspace(L, M_CAP), base, q, m_dev)
    _compare('build_dev/M_dev=%d' % m_dev, got, refs[m_dev])


def test_device_count_rebuild_large_to_small_in_one_workspace(counted):
    base, q, refs = counted
    L = _api()[0]
    ws = _workspace(L, M_CAP)
    for m_dev in (4000, 31, 2000):        # stale cell counts, cursors and sorted rows must not survive a rebuild
        got = _counted_build_and_query(ws, base, q, m_dev)
        _compare('rebuild/M_dev=%d' % m_dev, got, refs[m_dev])


# ---------------------------------------------------------------------------------------------------------------
# two grids over two different clouds, chosen by device words; queries given as low_xyz (lowkey = NULL)
# ---------------------------------------------------------------------------------------------------------------
def test_two_grid_form_reads_the_selected_cloud():
    L, check, ptr, st = _api()
    rng = np.random.RandomState(42)
    M, B = 3000, 64
    clouds = [kc._sheet(rng, M), (kc._sheet(rng, M) * np.array([1.0, 0.5, 1.0], np.float32) - np.array([0.0, 1.1, 0.0], np.float32))]
    q = (clouds[0][rng.randint(0, M, B)] + rng.randn(B, 3) * np.array([0.3, 0.2, 0.3])).astype(np.float32)
    refs = [kc.reference(p, q, 32) for p in clouds]
    assert (np.abs(refs[0].dy - refs[1].dy) > 0.5).all()          # the reference answers differ for every query
    grids = []
    for p in clouds:
        ws = _workspace(L, M)
        check(L.mh_scene_grid_build(ptr(torch.tensor(p, device=DEV)), M, ptr(ws), st))
        grids.append(ws)
    tq = torch.tensor(q, device=DEV)
    sentinel = np.int32(0x7fc12345)                               # a NaN with a payload: only the bits can be compared
    dy = torch.full((B,), int(sentinel), dtype=torch.int32, device=DEV).view(torch.float32)
    sel = torch.zeros(2, dtype=torch.int32, device=DEV)
    call = lambda: check(L.mh_contact_knn_grid_sel(ptr(grids[0]), ptr(grids[1]), M, ptr(sel), None, 0, None, B, 32, None, ptr(tq),
                                                   ptr(dy), st))
    for second in (0, 1):                                         # sel = (0, .): no scene yet, dy is not touched
        sel.copy_(torch.tensor([0, second], dtype=torch.int32))
        call()
        torch.cuda.synchronize()
        assert (dy.view(torch.int32).cpu().numpy() == sentinel).all()
    for which in (0, 1):
        sel.copy_(torch.tensor([1, which], dtype=torch.int32))
        call()
        torch.cuda.synchronize()
        _compare('grid_sel/(1,%d)' % which, dy.cpu().numpy(), refs[which])
    assert torch.equal(tq.cpu(), torch.tensor(q))                 # low_xyz is an input in this form


# ---------------------------------------------------------------------------------------------------------------
# key form: the query is the body's lowest vertex (largest y, first index on ties), found from a zero key
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def key_scene():
    rng = np.random.RandomState(43)
    pts = kc._sheet(rng, 3000)
    L, check, ptr, st = _api()
    ws = _workspace(L, pts.shape[0])
    check(L.mh_scene_grid_build(ptr(torch.tensor(pts, device=DEV)), pts.shape[0], ptr(ws), st))
    torch.cuda.synchronize()
    return pts, ws


@pytest.mark.parametrize('V', [1, 63, 64, 65, 200])
def test_key_form_on_small_bodies_with_a_tied_lowest_vertex(key_scene, V):
    L, check, ptr, st = _api()
    pts, ws = key_scene
    M, B = pts.shape[0], 5
    rng = np.random.RandomState(50 + V)
    verts = np.stack([rng.uniform(-2, 2, (B, V)), rng.uniform(0.2, 0.9, (B, V)), rng.uniform(3, 7, (B, V))], 2).astype(np.float32)
    first = np.zeros(B, np.int64)
    if V > 1:
        # two vertices share the largest y; the pairs include the two ends, neighbours, and (V = 65, 200) two vertices
        # that the same lane of the scan reads
        pairs = [(0, V - 1), (V // 2, V // 2 + 1), (V - 2, V - 1), (0, 64 if V > 64 else 1), tuple(sorted(rng.choice(V, 2, replace=False)))]
        for b, (i, j) in enumerate(pairs):
            verts[b, i, 1] = verts[b, j, 1] = np.float32(1.05 + 0.01 * b)
            first[b] = i
    low = verts[np.arange(B), first]
    ref = kc.reference(pts, low, 32)
    tv = torch.tensor(verts, device=DEV)
    key = torch.zeros(B, dtype=torch.int64, device=DEV)           # 0 = nobody reported: the kernel scans the body
    outs = []
    for _ in range(2):                                            # the second call starts from the keys the first wrote
        low_idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        low_xyz = torch.full((B, 3), float('nan'), device=DEV)
        dy = torch.full((B,), float('nan'), device=DEV)
        check(L.mh_contact_knn_grid_key(ptr(ws), M, ptr(tv), V, ptr(key), B, 32, ptr(low_idx), ptr(low_xyz), ptr(dy), st))
        torch.cuda.synchronize()
        outs.append((low_idx.cpu().numpy(), low_xyz.cpu().numpy(), dy.cpu().numpy(), key.cpu().numpy().copy()))
    idx, xyz, dy, keys = outs[0]
    assert (idx == first).all(), (idx, first)
    assert (xyz == low).all()
    _compare('grid_key/V=%d' % V, dy, ref)
    assert (keys != 0).all()
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
