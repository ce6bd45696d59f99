"""The kernels of csrc/mh_optim.hip, each alone through the C ABI, against the float64 references of tests/cycle_ref.py at
their path and grid edges.

Every output buffer and workspace is a slice of a larger device tensor at a 256-byte offset with 256 canary bytes on either
side; the canaries are compared after every call, so a write past a buffer is an assertion here and not a fault.

Gates.  None is taken from the kernel under test.  Element-wise outputs: twice the largest deviation from float64 of the
project's float32 oracle on the same inputs (fit_oracle on torch-CPU, or the same formula in NumPy float32), computed in
the test, with a floor of 4 ulp of the output's largest magnitude.  Summed losses: the same, the oracle summing in float32,
or rtol 1e-5 (tests/test_lbs_gpu.py::test_temporal_terms) where that is looser.  One-euro: four times the oracle's deviation;
a scan split into shards equals the whole bit for bit.

Which case enters which path:
  k_filtered_verts<float4, *>   E = 4, 452 and the large E = 4 * (1024 * 256 + 300), whose columns exceed the 1024-workgroup cap:
                                the float4 grid-stride loop
  k_filtered_verts<float, *>    E = 450, 451; E = 452 with verts or gverts one float off 16 bytes (the fallback of aligned());
                                E = 1024 * 256 + 3: the scalar grid-stride loop
  add / overwrite / gated       mh_filtered_verts_term, _init, _init_gated with the switch at 1 and at 0 (the C ABI has no gated
                                add form)
  window of FV_TB = 8 frames    T = 7 (short window), 8 (one full window), 9, 16, 17 (a window that starts on the row before it);
                                T = 1, 2: the pair at the halos only
  k_one_euro                    T = 1, 2 (tail loop only), 8 (tail: 7 frames), 9 (one prefetch block), 10, 16, 17, 40 (blocks and
                                tail); E = 1, 63, 257 (two workgroups), 4096 * 256 + 5 (the grid-stride loop); a shard starts at
                                local frame 0, so cuts 7, 8 and 16 of T = 17 send global frames through the tail loop that the
                                whole scan sends through the prefetch block, and cut 1 the other way round
  updates                       n = 1, 255, 256, 257 and 2048 * 256 + 77 (the grid-stride loop) for every entry point
  k_velocity                    T * N * 3 = 3, 255, 258, 771 (one to four strides of the 256 threads)
  k_project_loss                both modes; confidences exactly at the threshold; the warm-up form with and without scales
  k_project_points / unproject  B * M = 1, 255, 256, 257 with a different K per batch entry

Measured on the MI355X, largest error as a fraction of its gate (every test prints its own with pytest -s):
  filtered vertices   gradient 0.30, loss 0.02, add form 0.30, add form against gverts + the overwriting form's output 0.72 of
                      one ulp; the unaligned (scalar) call equals the aligned (float4) one bit for bit
  one-euro            0.25 everywhere, i.e. the kernel equals fit_oracle.one_euro_sequence bit for bit (printed per test), and
                      every split equals the whole.  Before this test existed it did not: the tail loop of k_one_euro, spelled
                      with __f*_rn, was contracted into FMAs, the prefetch block was not -- inside the gate against float64, but not
                      bit-equal to the oracle, and the cut at 7 of T = 17 differed from the whole scan.  Fixed in mh_optim.hip
                      (one_euro_step, one body for both loops)
  RMSprop / Adam      parameters 0.28 / 0.30, second moment 0.16 / 0.11, momentum 0.38 / 0.09; log row, poke words and the
                      device-resident learning rate exact
  velocity            gradient 0.39, loss 0.01
  projection loss     uv 0.21, loss 0.02, gradient 0.46; warm-up form: gradient 0.37, loss 0.01
  points              uv 0.21, unprojection 0.24, round trip 0.33
"""
import numpy as np
import pytest
import torch

import cycle_ref as cr
import golden_inputs as gi
from oracle import fit_oracle as fo

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS32 = float(np.finfo(np.float32).eps)            # one ulp of a float32 in [1, 2), relative
CANARY = 0xA5
WORST = {}


def dev(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(np.asarray(a, dtype)), device=DEV)


class Guard(object):
    """Buffers cut out of larger tensors: [256 canary bytes (+ off)] [payload] [256 canary bytes]"""

    def __init__(self):
        self.items = []

    def __call__(self, shape, dtype=torch.float32, init=None, off=0):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        lo = 256 + off
        base = torch.full((lo + n + 256,), CANARY, dtype=torch.uint8, device=DEV)
        assert base.data_ptr() % 256 == 0
        t = base[lo:lo + n].view(dtype).view(shape)
        if init is None:
            t.zero_()
        elif np.isscalar(init):
            t.fill_(init)
        else:
            t.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(dtype).view(shape))
        self.items.append((base, lo, n))
        return t

    def check(self):
        torch.cuda.synchronize()
        for base, lo, n in self.items:
            assert bool((base[:lo] == CANARY).all()) and bool((base[lo + n:] == CANARY).all()), 'a kernel wrote outside its buffer'


def lib():
    from mhhip import _lib
    return _lib.lib(), _lib.check, _lib.stream_ptr(torch.device(DEV))


def ptr(t):
    if t is None:
        return None
    assert t.is_contiguous()
    return t.data_ptr()


def gate_of(o32, r64, factor=2.0, floor_ulp=4.0, rtol=0.0):
    """factor x the float32 oracle's largest deviation from float64; floor: floor_ulp ulp (or rtol) of the largest magnitude"""
    r64 = np.asarray(r64, np.float64)
    mag = float(np.abs(r64).max()) if r64.size else 0.0
    return max(factor * float(np.abs(np.asarray(o32, np.float64) - r64).max()), floor_ulp * EPS32 * mag, rtol * mag)


def within(name, got, r64, gate):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    err = float(np.abs(got.reshape(np.shape(r64)) - r64).max())
    if gate > 0:
        WORST[name] = max(WORST.get(name, 0.0), err / gate)
    assert err <= gate, '%s: error %.3e over its gate %.3e' % (name, err, gate)
    return err


def report(prefix):
    print(' '.join('%s %.2f' % (k, v) for k, v in sorted(WORST.items()) if k.startswith(prefix)), '(largest error / gate)')


# =====================================================================================================================
# filtered vertices
# =====================================================================================================================
HALOS = ('none', 'prev', 'next', 'both')


def _fv_inputs(T, E, halo, seed):
    rng = np.random.RandomState(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    v, vf = u(T, E), u(T, E)
    prev = (u(E), u(E)) if halo in ('prev', 'both') else None
    nxt = (u(E), u(E)) if halo in ('next', 'both') else None
    return v, vf, prev, nxt


def _fv_call(entry, T, E, v, vf, prev, nxt, coef, gv, loss, ws, live=None):
    L, check, st = lib()
    pv, pvf = (ptr(prev[0]), ptr(prev[1])) if prev is not None else (None, None)
    nv, nvf = (ptr(nxt[0]), ptr(nxt[1])) if nxt is not None else (None, None)
    head = (T, E, ptr(v), ptr(vf), pv, pvf, nv, nvf, coef, ptr(gv), ptr(loss))
    if entry == 'add':
        check(L.mh_filtered_verts_term(*head, ptr(ws), st))
    elif entry == 'init':
        check(L.mh_filtered_verts_term_init(*head, ptr(ws), st))
    else:
        check(L.mh_filtered_verts_term_init_gated(*head, ptr(live), ptr(ws), st))


def _fv_case(T, E, halo, seed, entries=('init', 'gated', 'add'), off_v=0, off_g=0, want=None):
    """-> (init gradient, init loss) on the device; ``want``: the aligned call's to agree with"""
    L, _, _ = lib()
    coef = 0.3
    v, vf, prev, nxt = _fv_inputs(T, E, halo, seed)
    l64, g64 = cr.filtered64(v, vf, coef, prev, nxt)
    l32, g32 = cr.filtered64(v, vf, coef, prev, nxt, dtype=np.float32)
    gg, gl = gate_of(g32, g64), gate_of(l32, l64, rtol=1e-5)
    G = Guard()
    dv = G((T, E), init=v, off=off_v)
    dvf = dev(vf)
    dprev = None if prev is None else (dev(prev[0]), dev(prev[1]))
    dnxt = None if nxt is None else (dev(nxt[0]), dev(nxt[1]))
    ws = G(L.mh_filtered_verts_workspace_bytes(T, E), dtype=torch.uint8, init=0)
    one, zero = dev([1], np.int32), dev([0], np.int32)
    tag = 'fv E%d' % E
    out = {}
    for entry in entries:
        gv, loss = G((T, E), init=7.0, off=off_g), G(1, init=-1.0)
        if entry == 'add':
            g0 = np.random.RandomState(seed + 1).uniform(-1, 1, (T, E)).astype(np.float32)
            gv.copy_(dev(g0))
        _fv_call(entry, T, E, dv, dvf, dprev, dnxt, coef, gv, loss, ws, live=one)
        G.check()
        out[entry] = (gv, loss)
        within(tag + ' loss', loss, l64, gl)
        if entry == 'add':
            r = g0.astype(np.float64) + g64
            within(tag + ' add', gv, r, gg + 0.5 * EPS32 * float(np.abs(r).max()))      # + the rounding of the sum
            if 'init' in out:                      # gverts + the overwriting form's output: one rounding, fused or not
                r = g0.astype(np.float64) + out['init'][0].cpu().numpy().astype(np.float64)
                within(tag + ' add-init', gv, r, EPS32 * float(np.abs(r).max()))
            if T == 1 and halo == 'none':
                assert torch.equal(gv, dev(g0)), 'the add form of a term without pairs changed the buffer'
        else:
            within(tag + ' grad', gv, g64, gg)
        if T == 1 and halo == 'none':
            assert float(loss) == 0.0 and (entry == 'add' or not bool(gv.any()))
    if 'gated' in out:
        assert torch.equal(out['gated'][0], out['init'][0]) and torch.equal(out['gated'][1], out['init'][1])
        gv, loss = G((T, E), init=7.0), G(1, init=-1.0)
        _fv_call('gated', T, E, dv, dvf, dprev, dnxt, coef, gv, loss, ws, live=zero)          # the term does not exist yet
        G.check()
        assert float(loss) == 0.0 and not bool(gv.any()), 'gated off: the overwriting form clears exactly its rows, the sum is 0'
    if want is not None:
        r = want[0].cpu().numpy().astype(np.float64)
        within(tag + ' unaligned', out['init'][0], r, EPS32 * float(np.abs(r).max()))
    return out['init']


@pytest.mark.parametrize('E', [4, 452, 450, 451])
def test_filtered_verts_against_float64(E):
    for T in (1, 2, 7, 8, 9, 16, 17):
        for h, halo in enumerate(HALOS):
            _fv_case(T, E, halo, 1000 * E + 10 * T + h)
    report('fv E%d' % E)


@pytest.mark.parametrize('which', ['verts', 'gverts'])
def test_filtered_verts_unaligned_buffer_takes_the_scalar_form(which):
    T, E = 9, 452
    want = _fv_case(T, E, 'both', 77, entries=('init',))
    _fv_case(T, E, 'both', 77, entries=('init', 'add'), off_v=4 if which == 'verts' else 0, off_g=4 if which == 'gverts' else 0,
             want=want)
    report('fv E452 unaligned')


@pytest.mark.parametrize('E', [4 * (1024 * 256) + 4 * 300, 1024 * 256 + 3])
def test_filtered_verts_grid_stride_loop(E):
    _fv_case(2, E, 'both', 5, entries=('init', 'add'))
    _fv_case(2, E, 'none', 6, entries=('init',))
    report('fv E%d' % E)


# =====================================================================================================================
# one-euro
# =====================================================================================================================
PAIRS = [(0.01, 0.02), (0.001, 0.5)]           # the two filters of a fit (the one_euro_a / one_euro_b fixtures)


def _walk(T, E, seed):
    rng = np.random.RandomState(seed)
    w = np.cumsum(rng.normal(0, 0.02, (T, E)), axis=0) + rng.normal(0, 0.005, (T, E))
    return (0.5 * w / max(0.5, float(np.abs(w).max()))).astype(np.float32)


def _scan(x, c, b, G):
    L, check, st = lib()
    T, E = x.shape
    y, dx = G((T, E), init=9.0), dev(x)
    check(L.mh_one_euro_scan(ptr(dx), ptr(y), T, E, c, b, 25.0, st))
    G.check()
    return y


def _shard(x, c, b, first, state, G):
    from mhhip import engine
    L, check, st = lib()
    T, E = x.shape
    y, dxo, dx = G((T, E), init=9.0), G(E, init=9.0), dev(x)
    xp, dxp = (None, None) if state is None else state
    check(L.mh_one_euro_scan_shard(ptr(dx), ptr(y), T, E, c, b, 25.0, first, engine.one_euro_time_before(first, 25.0),
                                   ptr(xp), ptr(dxp), ptr(dxo), st))
    G.check()
    return y, (y[-1].clone(), dxo)


@pytest.mark.parametrize('E', [1, 63, 257])
def test_one_euro_against_float64(E):
    bits = True
    for T in (1, 2, 8, 9, 10, 16, 17, 40):
        for k, (c, b) in enumerate(PAIRS):
            x = _walk(T, E, 100 * T + E + k)
            G = Guard()
            y = _scan(x, c, b, G)
            y64, _ = cr.one_euro64(x, c, b)
            y32 = fo.one_euro_sequence(x, c, b)
            within('oe E%d' % E, y, y64, gate_of(y32, y64, factor=4.0, floor_ulp=0.0))
            bits = bits and np.array_equal(y.cpu().numpy(), y32)
    print('equals fit_oracle.one_euro_sequence bit for bit: %s' % bits)
    report('oe E%d' % E)


def test_one_euro_fixture_inputs_and_grid_stride_loop(golden):
    x = gi.one_euro_inputs().reshape(40, 15)
    for (c, b), key in zip(PAIRS, ('one_euro_a', 'one_euro_b')):
        G = Guard()
        y64, _ = cr.one_euro64(x, c, b)
        within('oe fixture', _scan(x, c, b, G), y64, gate_of(fo.one_euro_sequence(x, c, b), y64, factor=4.0, floor_ulp=0.0))
    T, E = 2, 4096 * 256 + 5
    x = _walk(T, E, 3)
    G = Guard()
    y = _scan(x, 0.01, 0.02, G)
    y64, _ = cr.one_euro64(x, 0.01, 0.02)
    y32 = fo.one_euro_sequence(x, 0.01, 0.02)
    within('oe large', y, y64, gate_of(y32, y64, factor=4.0, floor_ulp=0.0))
    print('large E equals the oracle bit for bit: %s' % np.array_equal(y.cpu().numpy(), y32))
    report('oe ')


@pytest.mark.parametrize('c,b', PAIRS)
def test_one_euro_shards_equal_the_whole_scan_bit_for_bit(c, b):
    T, E = 17, 257
    x = _walk(T, E, 41)
    G = Guard()
    whole = _scan(x, c, b, G)
    y64, dx64 = cr.one_euro64(x, c, b)
    _, dx32 = cr.one_euro64(x, c, b, dtype=np.float32)                       # the float32 oracle with its outgoing state
    for cuts in ([1], [7], [8], [9], [16], [5, 11], [8, 16]):
        bounds = [0] + cuts + [T]
        ys, state = [], None
        for s, e in zip(bounds[:-1], bounds[1:]):
            y, state = _shard(x[s:e], c, b, s, state, G)
            ys.append(y)
        assert torch.equal(torch.cat(ys), whole), 'cuts %s: the sharded scan differs from the whole' % (cuts,)
        within('oe dx', state[1], dx64, gate_of(dx32, dx64, factor=4.0, floor_ulp=0.0))
    # a shard that starts the sequence and hands nothing in is the whole scan, its state included
    y, state = _shard(x, c, b, 0, None, G)
    assert torch.equal(y, whole)
    within('oe dx', state[1], dx64, gate_of(dx32, dx64, factor=4.0, floor_ulp=0.0))
    report('oe dx')


# =====================================================================================================================
# optimiser updates
# =====================================================================================================================
SIZES = [1, 255, 256, 257, 2048 * 256 + 77]


def _steps(n, seed):
    rng = np.random.RandomState(seed)
    p = rng.normal(0, 1, n).astype(np.float32)
    gs = [rng.normal(0, 1, n).astype(np.float32) * np.float32(it != 3) for it in range(5)]      # step 4: all-zero gradient
    return p, gs


def _compare_update(tag, got, ref64, ref32):
    for name, g, r, o in zip(('p', 'a', 'b'), got, ref64, ref32):
        within('%s %s' % (tag, name), g, r, gate_of(o.numpy(), r))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('entry', ['step', 'log', 'log_row', 'poke1', 'poke2', 'dev'])
def test_rmsprop_entry_points_against_float64(entry, n):
    L, check, st = lib()
    p0, gs = _steps(n, 9 + n % 1000)
    G = Guard()
    dp, dsq, dbuf = G(n, init=p0), G(n), G(n)
    p64, sq64, buf64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    tp, tsq, tbuf = torch.tensor(p0), torch.zeros(n), torch.zeros(n)
    lr, gamma = np.float32(0.01), np.float32(0.99)
    lr_dev = G(1, init=np.array([lr]))
    nlog = 13
    log_dst, poke = G(nlog, init=5.0), G(2, dtype=torch.int32, init=np.array([-7, -8], np.int32))
    for it, g in enumerate(gs):
        dg = dev(g)
        src = dev(np.random.RandomState(it).normal(0, 1, nlog))
        tail = (float(lr), 0.5, 0.9, 1e-8)
        if entry == 'step':
            check(L.mh_rmsprop_step(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), n, *tail, st))
        elif entry == 'log':
            check(L.mh_rmsprop_step_log(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), n, *tail, None, None, 0, st))
        elif entry == 'log_row':
            check(L.mh_rmsprop_step_log(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), n, *tail, ptr(src), ptr(log_dst), nlog, st))
        elif entry in ('poke1', 'poke2'):
            check(L.mh_rmsprop_step_log_poke(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), n, *tail, ptr(src), ptr(log_dst), nlog,
                                             ptr(poke), int(entry[-1]), 100 + it, 200 + it, st))
        else:
            check(L.mh_rmsprop_step_dev(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), n, ptr(lr_dev), float(gamma), 0.5, 0.9, 1e-8, st))
        G.check()
        cr.rmsprop64(p64, g.astype(np.float64), sq64, buf64, float(lr))
        fo.rmsprop_step(tp, torch.tensor(g), tsq, tbuf, float(lr))
        lr = np.float32(lr * gamma)
        if entry in ('log_row', 'poke1', 'poke2'):
            assert torch.equal(log_dst, src), 'the log row is a copy'
        if entry == 'poke1':
            assert poke.tolist() == [100 + it, -8]
        if entry == 'poke2':
            assert poke.tolist() == [100 + it, 200 + it]
        if entry == 'dev':                          # the step used the value from before; one float32 product per call
            assert float(lr_dev) == float(lr)
    _compare_update('rms', (dp, dsq, dbuf), (p64, sq64, buf64), (tp, tsq, tbuf))
    if entry == 'log_row':                          # n = 0 with a log row: the copy alone
        src = dev(np.arange(nlog) + 0.5)
        before = dp.clone()
        dg = dev(gs[0])
        check(L.mh_rmsprop_step_log(ptr(dp), ptr(dg), ptr(dsq), ptr(dbuf), 0, 0.01, 0.5, 0.9, 1e-8, ptr(src), ptr(log_dst),
                                    nlog, st))
        G.check()
        assert torch.equal(log_dst, src) and torch.equal(dp, before)
    report('rms')


@pytest.mark.parametrize('n', SIZES)
def test_adam_against_float64(n):
    L, check, st = lib()
    p0, gs = _steps(n, 29 + n % 1000)
    G = Guard()
    dp, dm, dv = G(n, init=p0), G(n), G(n)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    tp, tm, tv = torch.tensor(p0), torch.zeros(n), torch.zeros(n)
    lr = 0.5
    for it, g in enumerate(gs):
        dg = dev(g)
        check(L.mh_adam_step(ptr(dp), ptr(dg), ptr(dm), ptr(dv), n, it + 1, float(np.float32(lr)), 0.5, 0.5, 1e-6, st))
        G.check()
        cr.adam64(p64, g.astype(np.float64), m64, v64, it + 1, float(np.float32(lr)))
        fo.adam_step(tp, torch.tensor(g), tm, tv, it + 1, float(np.float32(lr)))
        lr *= 0.95
    _compare_update('adam', (dp, dm, dv), (p64, m64, v64), (tp, tm, tv))
    report('adam')


# =====================================================================================================================
# velocity
# =====================================================================================================================
@pytest.mark.parametrize('T,N', [(1, 1), (5, 17), (2, 43), (257, 1), (1, 257)])
def test_velocity_against_float64(T, N):
    L, check, st = lib()
    coef = 0.05
    for h, halo in enumerate(HALOS):
        rng = np.random.RandomState(10 * T + N + h)
        u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
        pT, g0 = u(T, N, 3), u(T, N, 3)
        prev = u(N, 3) if halo in ('prev', 'both') else None
        nxt = u(N, 3) if halo in ('next', 'both') else None
        l64, g64 = cr.velocity64(pT, coef, prev, nxt)
        l32, g32 = cr.velocity64(pT, coef, prev, nxt, dtype=np.float32)
        G = Guard()
        gp, loss = G((T, N, 3), init=g0), G(1, init=-1.0)
        dpT, dprev, dnxt = dev(pT), None if prev is None else dev(prev), None if nxt is None else dev(nxt)
        check(L.mh_velocity_term(T, N, ptr(dpT), ptr(dprev), ptr(dnxt), coef, ptr(gp), ptr(loss), st))
        G.check()
        within('vel loss', loss, l64, gate_of(l32, l64, rtol=1e-5))
        r = g0.astype(np.float64) + g64                                       # the gradient accumulates
        within('vel grad', gp, r, gate_of(g32, g64) + 0.5 * EPS32 * float(np.abs(r).max()))
        if T == 1 and halo in ('none', 'next'):
            assert float(loss) == 0.0                                         # the pair (t-1, t) belongs to the owner of t
    report('vel')


# =====================================================================================================================
# projection + 2D residual
# =====================================================================================================================
W_IMG, H_IMG = 240.0, 135.0
JW = (np.linspace(0.5, 1.5, 17) / np.linspace(0.5, 1.5, 17).mean()).astype(np.float32)


def _proj_inputs(B, thr, seed):
    rng = np.random.RandomState(seed)
    Z = rng.uniform(1.0, 6.0, (B, 17, 1))
    j = np.concatenate([rng.uniform(-0.9, 0.9, (B, 17, 2)) * Z, Z], -1).astype(np.float32)      # Z >= 1, |X / Z| <= 1
    p2d = np.concatenate([rng.uniform(0, W_IMG, (B, 17, 1)), rng.uniform(0, H_IMG, (B, 17, 1)), rng.uniform(0, 1, (B, 17, 1))],
                         -1).astype(np.float32)
    p2d[:, 2::5, 2] = np.float32(thr)              # exactly at the threshold: counts in mode 0 (>=), not in mode 1 (>)
    p2d[:, 4, 2] = np.float32(thr) / 2
    _, K, Kd = gi.projection_inputs()
    return j, p2d, K[0], Kd


def _fp(a):
    from mhhip import _lib
    return None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(_lib.c_float_p)


@pytest.mark.parametrize('B', [1, 5, 64])
@pytest.mark.parametrize('mode,thr', [(0, 0.5), (1, 0.15)])
def test_project_loss_against_float64(B, mode, thr):
    L, check, st = lib()
    j, p2d, K, Kd = _proj_inputs(B, thr, 50 + B + mode)
    at_thr = p2d[..., 2] == np.float32(thr)
    assert at_thr.sum() == 3 * B
    for kd in (None, Kd):
        for jw in (None, JW):
            uv64, l64, g64 = cr.project_loss64(j, K, kd, p2d, thr, mode, W_IMG, H_IMG, 0.7, jw)
            uv32, l32, g32 = cr.project_loss64(j, K, kd, p2d, thr, mode, W_IMG, H_IMG, 0.7, jw, dtype=torch.float32)
            # the joints at the threshold carry gradient in mode 0 and none in mode 1
            assert bool(np.abs(g64[at_thr]).max() > 0) == (mode == 0) and not np.abs(g64[:, 4]).any()
            Kh, kdh, jwh = np.ascontiguousarray(K.reshape(9), np.float32), None if kd is None else np.asarray(kd, np.float32), jw
            G = Guard()
            uv, gj, loss = G((B, 17, 2), init=9.0), G((B, 17, 3), init=9.0), G(B, init=9.0)
            dj, dp = dev(j), dev(p2d)
            if jw is None:
                check(L.mh_project_joints_loss(B, ptr(dj), _fp(Kh), _fp(kdh), ptr(dp), thr, mode, W_IMG, H_IMG, 0.7, ptr(uv), ptr(gj),
                                               ptr(loss), st))
            else:
                check(L.mh_project_joints_loss_w(B, ptr(dj), _fp(Kh), _fp(kdh), _fp(jwh), ptr(dp), thr, mode, W_IMG, H_IMG, 0.7, ptr(uv),
                                                 ptr(gj), ptr(loss), st))
            G.check()
            within('proj uv', uv, uv64, gate_of(uv32, uv64))
            within('proj loss', loss, l64, gate_of(l32, l64, rtol=1e-5))
            within('proj grad', gj, g64, gate_of(g32, g64))
            gj2, loss2 = G((B, 17, 3), init=9.0), G(B, init=9.0)                     # want_uv off: the same bits
            check(L.mh_project_joints_loss_w(B, ptr(dj), _fp(Kh), _fp(kdh), _fp(jwh), ptr(dp), thr, mode, W_IMG, H_IMG, 0.7, None,
                                             ptr(gj2), ptr(loss2), st))
            G.check()
            assert torch.equal(gj2, gj) and torch.equal(loss2, loss)
    report('proj')


@pytest.mark.parametrize('B,NB', [(1, 1), (6, 3), (35, 5)])
def test_warmup_form_against_float64(B, NB):
    L, check, st = lib()
    thr = 0.15
    rng = np.random.RandomState(70 + B)
    _, p2d, K, Kd = _proj_inputs(B, thr, 80 + B)
    local = rng.uniform(-0.8, 0.8, (B, 17, 3)).astype(np.float32)
    tr = np.concatenate([rng.uniform(-1, 1, (B, 2)), rng.uniform(3, 8, (B, 1))], -1).astype(np.float32)
    xs = rng.uniform(-1.5, 2.0, NB).astype(np.float32)
    Kh = np.ascontiguousarray(K.reshape(9), np.float32)
    dlocal, dtr, dp2d = dev(local), dev(tr), dev(p2d)
    for x in (xs, None):
        dxs = None if x is None else dev(x)
        for kd, jw in ((None, None), (Kd, JW)):
            l64, g64 = cr.warmup64(local, x, tr, NB, K, kd, p2d, thr, 0.7, jw)
            l32, g32 = cr.warmup64(local, x, tr, NB, K, kd, p2d, thr, 0.7, jw, dtype=torch.float32)
            G = Guard()
            gt, loss = G((B, 3), init=9.0), G(B, init=9.0)
            check(L.mh_warmup_project_w(B, NB, ptr(dlocal), ptr(dxs), ptr(dtr), _fp(Kh),
                                        _fp(None if kd is None else np.asarray(kd, np.float32)), _fp(jw), ptr(dp2d), thr, 0.7,
                                        ptr(gt), ptr(loss), st))
            G.check()
            within('warm loss', loss, l64, gate_of(l32, l64, rtol=1e-5))
            within('warm grad', gt, g64, gate_of(g32, g64))
    report('warm')


# =====================================================================================================================
# generic projection / unprojection
# =====================================================================================================================
@pytest.mark.parametrize('B,M', [(1, 1), (5, 51), (4, 64), (257, 1)])
def test_project_and_unproject_points_against_float64(B, M):
    L, check, st = lib()
    rng = np.random.RandomState(B * 1000 + M)
    Z = rng.uniform(1.0, 6.0, (B, M, 1))
    pts = np.concatenate([rng.uniform(-0.9, 0.9, (B, M, 2)) * Z, Z], -1).astype(np.float32)
    K = np.tile(np.array([[117.0, 0.3, 120.0], [0.1, 118.5, 67.5], [0, 0, 1]], np.float32), (B, 1, 1))
    K[:, :2] += rng.uniform(-3, 3, (B, 2, 3)).astype(np.float32)               # a different K, skew included, per batch entry
    _, _, Kd = gi.projection_inputs()
    dK, dp = dev(K), dev(pts)
    t64, t32 = (lambda a: torch.tensor(a, dtype=torch.float64)), (lambda a: torch.tensor(a, dtype=torch.float32))
    for kd in (None, Kd):
        kdl = None if kd is None else [float(c) for c in kd]
        uv64, uv32 = fo.project_points(t64(pts), t64(K), kdl).numpy(), fo.project_points(t32(pts), t32(K), kdl).numpy()
        for with_depth in (0, 1):
            G = Guard()
            out = G((B, M, 3 if with_depth else 2), init=9.0)
            check(L.mh_project_points(B, M, ptr(dp), ptr(dK), _fp(kd), with_depth, ptr(out), st))
            G.check()
            within('pts uv', out[..., :2], uv64, gate_of(uv32, uv64))
            if with_depth:
                assert torch.equal(out[..., 2], dp[..., 2])
        if kd is None:                             # out is the (u, v, Z) of the last call: back to the points
            G = Guard()
            back = G((B, M, 3), init=9.0)
            uvd = out.clone()
            check(L.mh_unproject_points(B, M, ptr(uvd), ptr(dK), ptr(back), st))
            G.check()
            h = uvd.cpu().numpy()
            b64, b32 = fo.unproject_points(t64(h), t64(K)).numpy(), fo.unproject_points(t32(h), t32(K)).numpy()
            within('pts unproject', back, b64, gate_of(b32, b64))
            trip32 = fo.unproject_points(torch.cat([t32(uv32), t32(pts[..., 2:])], -1), t32(K)).numpy()
            within('pts round trip', back, pts.astype(np.float64), gate_of(trip32, pts.astype(np.float64)))
    report('pts')
