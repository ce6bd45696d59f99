"""tests/scene_terms_ref.py against torch autograd (float64) of the contact / foot-sliding formulas of oracle/fit_oracle.py
(:352-358, reference optimizer.py:502-518), and the conditions the GPU test's inputs are built to meet.  No GPU."""
import numpy as np
import pytest
import torch

import scene_terms_ref as sr


def _oracle_batch(pT, gv, low_idx, dy, cc, cf):
    """one batch the way fit_oracle.SequenceOracle.batch_loss writes it: pT (b,N,1,3), gv (b,N,V,3) leaves, low_idx (b,N), dy (b,N,1,1)"""
    b, N = low_idx.shape
    gi = low_idx[..., None, None].expand(b, N, 1, 3)
    low = torch.gather(gv, 2, gi)
    tgt = pT.detach().clone()
    tgt[..., 1:2] = tgt[..., 1:2] + (dy + sr.C_OFFSET).detach()
    contact = (pT - tgt).abs().sum()
    gate = (dy > sr.C_GATE)[1:].double()
    low_t = low[1:]
    low_tm1 = torch.gather(gv[:-1], 2, gi[1:])
    foot = (gate * low_t - gate * low_tm1).abs().sum() / torch.clamp(gate.sum(), min=1)
    return contact, foot


def _oracle(case, cc, cf):
    T, N, V = case['T'], case['N'], case['V']
    rng = np.random.RandomState(3)
    pT = torch.tensor(rng.uniform(-2, 2, (T, N, 1, 3)), dtype=torch.float64, requires_grad=True)
    gv = torch.tensor(case['verts'].reshape(T, N, V, 3).astype(np.float64), requires_grad=True)
    low_idx = torch.tensor(case['low_idx'].reshape(T, N).astype(np.int64))
    dy = torch.tensor(case['dy'].reshape(T, N, 1, 1).astype(np.float64))
    bc, bf, total = [], [], 0.0
    for row in sr.batch_table(T, case['batch'], case['table']):
        fr = torch.tensor([int(t) for t in row if 0 <= t < T])
        c, f = _oracle_batch(pT[fr], gv[fr], low_idx[fr], dy[fr], cc, cf)
        bc.append(float(c.detach()))
        bf.append(float(f.detach()))
        total = total + float(np.float32(cc)) * c + float(np.float32(cf)) * f
    total.backward()
    return pT.grad.numpy().reshape(T * N, 3), gv.grad.numpy().reshape(T * N, V, 3), np.array(bc), np.array(bf)


CONTIGUOUS = [k for k, v in sr.SHAPES.items() if v[3] is None]


@pytest.mark.parametrize('name', CONTIGUOUS + sorted(sr.SHUFFLED_FOR_ORACLE))
def test_reference_equals_autograd_of_the_oracle_formulas(name):
    shapes = sr.SHAPES if name in CONTIGUOUS else sr.SHUFFLED_FOR_ORACLE
    case = sr.make_case(name, shapes=shapes)
    assert np.array_equal(case['low_xyz'], case['verts'][np.arange(case['T'] * case['N']), case['low_idx']])
    cc, cf = 0.1, 0.2
    gpT, gverts, bc, bf = sr.reference(case, cc, cf)
    wpT, wverts, wbc, wbf = _oracle(case, cc, cf)
    # pT - (pT + c) is c to a rounding of pT (|pT| <= 2) in the oracle's float64; everything else is the same arithmetic
    np.testing.assert_allclose(bc, wbc, rtol=0, atol=case['batch'] * case['N'] * 3 * 4.5e-16)
    np.testing.assert_allclose(bf, wbf, rtol=1e-13, atol=0)
    np.testing.assert_allclose(gpT, wpT, rtol=1e-14, atol=0)
    np.testing.assert_allclose(gverts, wverts, rtol=1e-13, atol=0)
    assert np.abs(gpT).max() > 0 and (name in ('single',) or np.abs(gverts).max() > 0)


def test_float32_sums_are_the_same_terms():
    case = sr.make_case('items320')
    _, _, bc, bf = sr.reference(case, 0.1, 0.2)
    _, _, bc32, bf32 = sr.reference(case, 0.1, 0.2, dtype=np.float32)
    assert 0 < np.abs(bc32 - bc).max() <= 1e-5 * bc.max() and np.abs(bf32 - bf).max() <= 1e-5 * bf.max()


def test_lowest_vertex_reference():
    v = np.zeros((5, 4, 3), np.float32)
    v[0, :, 1] = [1, 3, 3, 2]                          # a tie: the first index
    v[1, :, 1] = [-0.0, 0.0, -1, -2]                   # -0.0 before +0.0: equal, the earlier one
    v[2, :, 1] = np.nan
    v[3, :, 1] = -np.inf
    v[4, :, 1] = [np.nan, -5, np.nan, -3]              # the largest y negative, NaN never wins
    idx, xyz = sr.lowest_vertex(v)
    assert idx.tolist() == [1, 0, 0, 0, 3] and idx.dtype == np.int32
    assert np.array_equal(xyz.view(np.uint32), v[np.arange(5), idx].view(np.uint32))
    key = sr.lowest_key(v, idx)
    assert int(key[0]) == ((0x40400000 ^ 0x80000000) << 32) | (~1 & 0xffffffff)         # 3.0f
    assert int(key[1]) == (0x80000000 << 32) | 0xffffffff                               # -0.0 + 0.0f = +0.0: one key for both zeros
    assert int(key[4]) == ((0xc0400000 ^ 0xffffffff) << 32) | (~3 & 0xffffffff)         # -3.0f
    assert key[4] < key[1] < key[0]                    # the high word keeps the order of y


def _in_stride(case, i):
    """the kernel visits item j = k * N + person at thread j % 256: j >= 256 is the second trip of the stride loops"""
    T, N = case['T'], case['N']
    for row in sr.batch_table(T, case['batch'], case['table'])[:1]:
        for k, t in enumerate(row):
            if int(t) == i // N:
                return k * N + i % N >= 256
    return False


@pytest.mark.parametrize('name', sorted(sr.SHAPES))
def test_cases_hold_what_they_promise(name):
    case = sr.make_case(name)
    T, N, V, batch, dy = case['T'], case['N'], case['V'], case['batch'], case['dy']
    pl = case['planted']
    rows = sr.batch_table(T, batch, case['table'])
    live = [int(t) for t in rows.ravel() if 0 <= t < T]
    assert sorted(live) == list(range(T)), 'every frame sits at exactly one position'
    pairs = sr.pairs_of(T, N, batch, case['table'])
    cur = set(p[3] for p in pairs)
    gpT, gverts, bc, bf = sr.reference(case, 0.1, 0.2)
    if name == 'single':
        assert not pairs and bf[0] == 0 and not gverts.any() and bc[0] > 0
    if name == 'items256':
        assert batch * N == 256
    if name in ('items260', 'items260_full'):
        assert batch * N == 260 and (len(pairs) == 9 * N) == (name == 'items260_full')
    if name in ('items320', 'positions320'):
        assert batch * N == 320
    if name == 'positions320':
        assert case['nb'] == 1 and len(pairs) == 2 * N
    if name == 'hole':
        assert all(-1 in row[1:-1] for row in case['table'])
    if name == 'past_T':
        assert T in case['table'] and (case['table'] > T).any() and (case['table'] < -1).any()
    if name in ('items256', 'items260', 'items260_full', 'items320', 'positions320', 'permuted', 'hole', 'past_T'):
        assert pl['at_gate'] and pl['above_gate'] and pl['zero_sign'] and pl['zero_d']
    if name in ('items260_full', 'items320'):      # the planted values sit on both sides of the stride
        for key in ('at_gate', 'above_gate', 'zero_sign'):
            assert sorted(_in_stride(case, i) for i in pl[key]) == [False, True]
        assert sorted(_in_stride(case, p[0]) for p in pl['zero_d']) == [False, True]
    if name in ('ragged', 'items320', 'permuted', 'hole', 'past_T'):
        assert pl['closed'] == 1
    # the planted values are what they are said to be, where they matter
    g = dy.astype(np.float64)
    for i in pl['at_gate']:
        assert i in cur and dy[i] == np.float32(-0.20) and not g[i] > sr.C_GATE
    for i in pl['above_gate']:
        assert i in cur and dy[i] > np.float32(-0.20) and np.nextafter(dy[i], np.float32(-1)) == np.float32(-0.20) and g[i] > sr.C_GATE
    for i in pl['zero_sign']:
        assert dy[i] + np.float32(0.02) == 0 and gpT[i, 1] == 0 and g[i] > sr.C_GATE
    others = np.setdiff1d(np.arange(T * N), pl['zero_sign'])
    assert (np.abs(gpT[others, 1]) == float(np.float32(0.1))).all() and not gpT[:, [0, 2]].any()
    for i, ip, c in pl['zero_d']:
        vi = case['low_idx'][i]
        assert (i, ip) in set((p[3], p[4]) for p in pairs) and g[i] > sr.C_GATE
        assert case['low_xyz'][i, c] == case['verts'][ip, vi, c] and (case['low_xyz'][i] != case['verts'][ip, vi]).sum() == 2
    if pl['closed'] is not None:
        bt = pl['closed']
        its = [p for p in pairs if p[0] == bt]
        assert its and not any(g[p[3]] > sr.C_GATE for p in its) and any(dy[p[3]] == np.float32(-0.20) for p in its)
        assert bf[bt] == 0 and bc[bt] > 0
        for p in its:
            assert not gverts[p[3]].any() and not gverts[p[4]].any()
    # dy + 0.02f is exact in float32 wherever its sign could be in doubt: float64 and float32 agree on every sign
    s32 = np.sign(-(dy + np.float32(0.02)))
    assert np.array_equal(s32, np.sign(-(g + sr.C_OFFSET)))
    if name in ('items256', 'items260', 'items260_full', 'items320', 'permuted'):
        # person 0 keeps its lowest vertex: an element of a frame between two others is written in both sweeps
        li = case['low_idx'].reshape(T, N)
        assert (li[:, 0] == 3).all()
        mids = [(a, b) for a in pairs for b in pairs if a[2] == 0 and b[2] == 0 and a[3] == b[4] and g[a[3]] > sr.C_GATE and g[b[3]] > sr.C_GATE]
        assert mids, 'no frame of person 0 is current in one open pair and previous in the next'
        # the last person's changes with every position
        assert all(li[p[3] // N, N - 1] != li[p[4] // N, N - 1] for p in pairs if p[2] == N - 1)
