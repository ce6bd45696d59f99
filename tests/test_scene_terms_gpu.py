"""k_lowest_vertex, k_lowest_resolve and k_contact_foot (csrc/mh_scene.hip) alone through the C ABI, against the float64
references of tests/scene_terms_ref.py (pinned to the oracle's formulas by tests/test_scene_terms_ref.py, which also asserts
what the inputs here are built to contain).

Every output is a slice of a larger device tensor between canaries (Guard of tests/test_cycle_kernels_gpu.py), compared after
every call.

Lowest vertex: index equal to the reference, xyz bit-equal to verts[index], V = 1 ... 6890 (one to 27 trips of the 256 threads),
B = 1 and 3; the largest y shared by two vertices of one thread (v, v + 256), of two lanes of a wave, of two waves and at 0 and
V - 1; -0.0 before +0.0; every y negative; a body of NaN and a body of -inf between finite ones (index 0: the guard; before it
thread 0 read verts[0x7fffffff * 3]).  mh_lowest_resolve: the same bits from zero keys, the key it writes back equal to the
documented encoding, a key that names no vertex scanned and rewritten, a valid key trusted, the key of a NaN body left alone.

Contact and foot sliding: the shapes of scene_terms_ref.SHAPES, (T, N, batch) from (1, 1, 1) over exactly 256 items to 320 items
in two trips of the stride loops, contiguous, permuted, with empty positions in the middle of a batch and entries >= T; dy exactly
at the gate and one ulp above, dy + 0.02f == 0, a foot that did not move in one coordinate, a batch with every gate closed, a
lowest vertex that stays and one that changes.  All three entry points, the switch at 0, either gradient NULL, two launches from
one start.  Gradients start from random values (the kernel adds), sums from NaN (it overwrites).

Gates, none from the kernel.  Gradients: 4 ulp of the largest expected entry (an element receives at most two adds of
cf * sign / count, cc * sign is exact).  Sums: gate_of -- twice the deviation from float64 of the same terms summed one after the
other in float32, floor rtol 1e-5 (tests/test_lbs_gpu.py::test_temporal_terms).

Measured on the MI355X, largest error as a fraction of its gate (every test prints its own with pytest -s):
  lowest vertex       index, xyz and key exact in every case (equalities, no gate)
  contact / foot      contact sum 0.01, foot sum 0.01, gpT 0.07, gverts 0.12 over the shapes of SHAPES; 384 items per batch with one
                      lowest vertex per person: gverts 0.21, thirteen launches the same bits; the entry points, the NULL forms and
                      a second launch equal the first bit for bit everywhere
"""
import numpy as np
import pytest
import torch

import scene_terms_ref as sr
from test_cycle_kernels_gpu import EPS32, Guard, dev, gate_of, lib, ptr, report, within

pytestmark = pytest.mark.gpu

CC, CF = 0.1, 0.2
SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 6890]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# =====================================================================================================================
# lowest vertex
# =====================================================================================================================
def _lowest(verts, G):
    L, check, st = lib()
    B, V = verts.shape[:2]
    dv = dev(verts)
    idx, xyz = G(B, dtype=torch.int32, init=-7), G((B, 3), init=9.0)
    check(L.mh_lowest_vertex(ptr(dv), B, V, ptr(idx), ptr(xyz), st))
    G.check()
    return idx, xyz


def _resolve(verts, keys, G):
    """keys (B,) uint64 -> (low_idx, low_xyz, keys afterwards as uint64)"""
    L, check, st = lib()
    B, V = verts.shape[:2]
    dv = dev(verts)
    dk = G(B, dtype=torch.int64, init=np.asarray(keys, np.uint64).view(np.int64))
    idx, xyz = G(B, dtype=torch.int32, init=-7), G((B, 3), init=9.0)
    check(L.mh_lowest_resolve(ptr(dv), B, V, ptr(dk), ptr(idx), ptr(xyz), st))
    G.check()
    return idx, xyz, dk.cpu().numpy().view(np.uint64)


def _expect_lowest(verts, idx, xyz, what):
    widx, wxyz = sr.lowest_vertex(verts)
    assert np.array_equal(idx.cpu().numpy(), widx), '%s: index %s, reference %s' % (what, idx.tolist(), widx.tolist())
    assert np.array_equal(_bits(xyz), wxyz.view(np.int32)), '%s: xyz is not verts[index] bit for bit' % what
    return widx


def _bodies(B, V, seed):
    return np.random.RandomState(seed).uniform(-1, 1, (B, V, 3)).astype(np.float32)


def _ties(V):
    """pairs of vertices to share the largest y, by where the kernel meets them"""
    out = [(0, V - 1)] if V > 1 else []
    if V > 256:
        out += [(0, 256), (V - 257, V - 1)]                    # one thread, two trips
    if V > 40:
        out += [(3, 40), (40, 3)]                              # two lanes of a wave
    if V > 130:
        out += [(10, 130), (70, 200 % V)]                      # two waves
    if V > 300:
        out += [(250, 260)]                                    # wave 3 of the first trip, wave 0 of the second
    return out


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('V', SIZES)
def test_lowest_vertex_and_resolve_against_the_reference(V, B):
    verts = _bodies(B, V, 10 * V + B)
    G = Guard()
    idx, xyz = _lowest(verts, G)
    widx = _expect_lowest(verts, idx, xyz, 'mh_lowest_vertex')
    ridx, rxyz, keys = _resolve(verts, np.zeros(B, np.uint64), G)
    assert torch.equal(ridx, idx) and np.array_equal(_bits(rxyz), _bits(xyz)), 'mh_lowest_resolve from zero keys'
    assert np.array_equal(keys, sr.lowest_key(verts, widx)), 'the key written back is not (ordered bits of y) << 32 | ~index'


@pytest.mark.parametrize('V', SIZES)
def test_lowest_vertex_ties_zeros_and_negative_maxima(V):
    pairs = _ties(V)
    B = len(pairs) + 3
    verts = _bodies(B, V, 7 * V)
    for b, (i, j) in enumerate(pairs):
        verts[b, [i, j], 1] = 2.0
    nb = len(pairs)
    verts[nb, :, 1] = -np.abs(verts[nb, :, 1]) - 1.0           # every y negative
    verts[nb + 1, :, 1] = -np.abs(verts[nb + 1, :, 1]) - 1.0   # -0.0 at an earlier index than +0.0: equal, the earlier one
    verts[nb + 2, :, 1] = -np.abs(verts[nb + 2, :, 1]) - 1.0   # ... and the other way round
    if V > 1:
        a, z = V // 3, V - 1
        verts[nb + 1, a, 1], verts[nb + 1, z, 1] = -0.0, 0.0
        verts[nb + 2, a, 1], verts[nb + 2, z, 1] = 0.0, -0.0
    G = Guard()
    idx, xyz = _lowest(verts, G)
    widx = _expect_lowest(verts, idx, xyz, 'mh_lowest_vertex')
    assert widx[:nb].tolist() == [min(p) for p in pairs]
    if V > 1:
        assert widx[nb + 1] == V // 3 and widx[nb + 2] == V // 3
        assert np.signbit(xyz[nb + 1, 1].item()) and not np.signbit(xyz[nb + 2, 1].item())
    ridx, rxyz, keys = _resolve(verts, np.zeros(B, np.uint64), G)
    assert torch.equal(ridx, idx) and np.array_equal(_bits(rxyz), _bits(xyz))
    assert np.array_equal(keys, sr.lowest_key(verts, widx))
    if V > 1:
        assert keys[nb + 1] == keys[nb + 2]                    # y + 0.0f: one key for both zeros


@pytest.mark.parametrize('V', [1, 65, 257, 6890])
def test_body_without_a_finite_y_gives_vertex_0_and_leaves_its_neighbours_alone(V):
    """every y NaN (a diverged fit) or -inf: nothing compares greater than the start value.  mh_lowest_from_key has always
    answered vertex 0; k_lowest_vertex does since this test exists (it is not run against a build without that line)"""
    verts = _bodies(4, V, 3 * V)
    verts[1, :, 1] = np.nan
    verts[2, :, 1] = -np.inf
    G = Guard()
    idx, xyz = _lowest(verts, G)
    widx = _expect_lowest(verts, idx, xyz, 'mh_lowest_vertex')
    assert widx[1] == 0 and widx[2] == 0
    assert np.array_equal(widx[[0, 3]], np.argmax(verts[[0, 3], :, 1], axis=1))
    before = np.array([0, 0x1234567800000000 | (~(V + 5) & 0xffffffff), 0, 0], np.uint64)      # body 1: a key that names no vertex
    ridx, rxyz, keys = _resolve(verts, before, G)
    assert torch.equal(ridx, idx) and np.array_equal(_bits(rxyz), _bits(xyz))
    want = sr.lowest_key(verts, widx)
    assert keys[0] == want[0] and keys[3] == want[3]
    assert keys[1] == before[1] and keys[2] == 0, 'the key of a body without a finite y is left as it was'


@pytest.mark.parametrize('V', [1, 64, 257, 6890])
def test_resolve_trusts_a_valid_key_and_scans_for_one_that_names_no_vertex(V):
    B = 6
    verts = _bodies(B, V, 5 * V + 1)
    widx, _ = sr.lowest_vertex(verts)
    named = np.array([(widx[b] + 1 + b) % V for b in range(B)], np.uint32)                 # a vertex that is not the lowest (V > 1)
    HI = 0x7f00000000000000
    low = lambda i: ~int(i) & 0xffffffff
    keys = np.array([HI | low(named[0]),                       # valid: trusted
                     (1 << 32) | low(named[1]),                # valid, any high word: trusted
                     HI | low(V),                              # index == V: no key
                     HI,                                       # low word 0: index 0xffffffff, no key
                     HI | low(V + 1000000),                    # far past V: no key
                     0], np.uint64)                            # nobody reported
    G = Guard()
    idx, xyz, after = _resolve(verts, keys, G)
    want_idx = widx.copy()
    want_idx[:2] = named[:2]
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(_bits(xyz), verts[np.arange(B), want_idx].view(np.int32))
    full = sr.lowest_key(verts, widx)
    assert np.array_equal(after[:2], keys[:2]), 'a trusted key is not rewritten'
    assert np.array_equal(after[2:], full[2:]), 'a body scanned for want of a key gets its key written'


# =====================================================================================================================
# contact + foot sliding
# =====================================================================================================================
def _start(case, seed=11):
    B, V = case['T'] * case['N'], case['V']
    rng = np.random.RandomState(seed)
    g = lambda *s: (rng.uniform(0.25, 1.0, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32)      # non-zero everywhere
    return g(B, 3), g(B, V, 3)


def _call(case, entry, d, gpT, gv, bc, bfo, live=None):
    L, check, st = lib()
    c = case
    head = (c['T'], c['N'], c['V'], c['batch'])
    body = (ptr(d['verts']), ptr(d['low_idx']), ptr(d['low_xyz']), ptr(d['dy']), CC, CF, ptr(gpT), ptr(gv), ptr(bc), ptr(bfo))
    if entry == 'plain':
        assert c['table'] is None
        check(L.mh_contact_foot_terms(*head, *body, st))
    elif entry == 'idx':
        check(L.mh_contact_foot_terms_idx(*head, c['nb'], ptr(d['table']), *body, st))
    else:
        check(L.mh_contact_foot_terms_gated(*head, c['nb'], ptr(d['table']) if c['table'] is not None else None, *body, ptr(live), st))


def _device(case):
    c = case
    table = c['table'] if c['table'] is not None else sr.batch_table(c['T'], c['batch'])
    return dict(verts=dev(c['verts']), low_idx=dev(c['low_idx'], np.int32), low_xyz=dev(c['low_xyz']), dy=dev(c['dy']),
                table=dev(table, np.int32))


def _launch(case, entry, d, p0, v0, live=None, no_gpT=False, no_gv=False):
    """one call from the start values p0 / v0 -> (gpT, gverts, batch_contact, batch_foot), canaries checked"""
    B, V, nb = case['T'] * case['N'], case['V'], case['nb']
    G = Guard()
    gpT, gv = G((B, 3), init=p0), G((B, V, 3), init=v0)
    bc, bfo = G(nb, init=float('nan')), G(nb, init=float('nan'))
    _call(case, entry, d, None if no_gpT else gpT, None if no_gv else gv, bc, bfo, live)
    G.check()
    return gpT, gv, bc, bfo


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('name', list(sr.SHAPES))
def test_contact_foot_against_float64(name):
    case = sr.make_case(name)
    d = _device(case)
    p0, v0 = _start(case)
    ref = sr.reference(case, CC, CF) + sr.reference(case, CC, CF, dtype=np.float32)[2:]
    one, zero = dev([1], np.int32), dev([0], np.int32)
    tag = 'cf'
    outs = {}
    for entry in (('plain',) if case['table'] is None else ()) + ('idx', 'gated'):
        outs[entry] = _launch(case, entry, d, p0, v0, live=one)
        _check(case, outs[entry], p0, v0, tag, ref)
    assert all(_same(outs['idx'], o) for o in outs.values()), 'the entry points differ'
    again = _launch(case, 'idx', d, p0, v0)
    assert _same(again, outs['idx']), 'two launches from the same start differ'
    # the switch at 0: both sums 0, both gradients untouched
    gpT, gv, bc, bfo = _launch(case, 'gated', d, p0, v0, live=zero)
    assert np.array_equal(_bits(gpT), p0.view(np.int32)) and np.array_equal(_bits(gv), v0.view(np.int32))
    assert not bool(bc.any()) and not bool(bfo.any()) and not bool(torch.isnan(bc).any()) and not bool(torch.isnan(bfo).any())
    # either gradient absent: the sums and the other gradient as before
    o = _launch(case, 'idx', d, p0, v0, no_gpT=True)
    _check(case, o, p0, v0, tag, ref, no_gpT=True)
    assert _same(o[1:], outs['idx'][1:])
    o = _launch(case, 'idx', d, p0, v0, no_gv=True)
    _check(case, o, p0, v0, tag, ref, no_gv=True)
    assert _same((o[0],) + o[2:], (outs['idx'][0],) + outs['idx'][2:])
    # what the case was built for, on the kernel's side
    pl = case['planted']
    got_p = outs['idx'][0].cpu().numpy()
    for i in pl['zero_sign']:
        assert got_p[i, 1] == p0[i, 1]
    if pl['closed'] is not None:
        assert float(outs['idx'][3][pl['closed']]) == 0.0
    if name == 'single':
        assert float(outs['idx'][3][0]) == 0.0 and np.array_equal(_bits(outs['idx'][1]), v0.view(np.int32))
    report(tag)


def _check(case, out, p0, v0, tag, ref, no_gpT=False, no_gv=False):
    gpT64, gv64, bc64, bf64, bc32, bf32 = ref
    gpT, gv, bc, bfo = out
    wp = p0.astype(np.float64) + (0 if no_gpT else gpT64)
    wv = v0.astype(np.float64) + (0 if no_gv else gv64)
    within(tag + ' gpT', gpT, wp, 4 * EPS32 * float(np.abs(wp).max()))
    within(tag + ' gverts', gv, wv, 4 * EPS32 * float(np.abs(wv).max()))
    for b in range(case['nb']):                                 # every batch is a sum of its own: a gate each
        within(tag + ' contact', bc[b], bc64[b], gate_of(bc32[b], bc64[b], rtol=1e-5))
        within(tag + ' foot', bfo[b], bf64[b], gate_of(bf32[b], bf64[b], rtol=1e-5))
    if no_gpT:
        assert np.array_equal(_bits(gpT), p0.view(np.int32)), 'gpT == NULL and yet written'
    if no_gv:
        assert np.array_equal(_bits(gv), v0.view(np.int32)), 'gverts == NULL and yet written'


def _two_trip_case(nbatches=16):
    """(12 * nbatches, 32, 12): 384 items per batch, so waves 0 and 1 make two trips through each sweep and waves 2 and 3 one.
    Everybody keeps one lowest vertex, so the element of an item is written again by the item 32 further on, in the other
    sweep; positions 3 and 4 -- the first trip of wave 1 -- have their gates closed, so that wave 1 is through its first sweep
    early.  The kernel's claim -- plain read-modify-writes, the same bits in every launch -- rests on the barrier between the
    sweeps for exactly such items: thread 32 + t adds to an element in its second trip of sweep 0 that thread 64 + t
    (another wave) subtracts from in its second trip of sweep 1."""
    shapes = {'two_trips': (12 * nbatches, 32, 12, None)}
    case = sr.make_case('two_trips', shapes=shapes)
    T, N = case['T'], case['N']
    case['low_idx'][:] = 3
    dy = np.random.RandomState(5).uniform(-0.19, 0.1, (T, N)).astype(np.float32)
    for t in range(T):
        if t % 12 in (3, 4):
            dy[t] = -0.3
    case['dy'] = dy.reshape(-1)
    case['low_xyz'] = case['verts'][np.arange(T * N), 3].copy()
    return case


def test_contact_foot_is_reproducible_bit_for_bit_where_both_sweeps_write_an_element():
    case = _two_trip_case()
    d = _device(case)
    p0, v0 = _start(case, seed=12)
    ref = sr.reference(case, CC, CF) + sr.reference(case, CC, CF, dtype=np.float32)[2:]
    first = _launch(case, 'plain', d, p0, v0)
    _check(case, first, p0, v0, 'cf two trips', ref)
    for _ in range(12):
        assert _same(_launch(case, 'plain', d, p0, v0), first), 'two launches from the same start differ'
    report('cf two trips')
