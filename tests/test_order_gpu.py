"""The depth-ordering kernel (``mh_order_term_keys`` / ``mh_order_term``) against tests/order_ref.py.  The definition fixes
every rounding and the sums are integers, so every comparison is BIT EQUALITY: counts, pairs, ``body_loss`` and the
gradient added into ``gtransl``.

Hand-made tables at the smallest sizes where the kernel can go wrong: 5 x 7 pixels (a row is no multiple of anything, one
partial workgroup), windows inside, at the edge of, outside the image and of width 0, keys that are empty, point past the
face table, hold a NaN, a negative or an infinite depth, exact depth ties, a gated-out body; 32 people (person 31 is bit 31);
527 pixels in three workgroups and three frames; one person.  Then a real rasteriser workspace.
"""
import numpy as np
import pytest

import order_ref

pytestmark = pytest.mark.gpu

MARGIN, DELTA, COEF = 0.25, 0.5, 3.0


def _random_keys(rng, records, F):
    """depths from a small set (exact ties) and from a continuous range, faces in [0, F); then the keys that must not count"""
    z = np.where(rng.rand(records) < 0.5, rng.choice(np.float32([1.0, 1.5, 2.0, 2.5]), records),
                 rng.uniform(0.8, 3.0, records).astype(np.float32)).astype(np.float32)
    keys = np.full((records, 5), order_ref.EMPTY, np.uint64)
    keys[:, 0] = order_ref.pack_keys(z, rng.randint(0, F, records).astype(np.uint64))
    keys[:, 1:] = rng.randint(0, 2 ** 62, (records, 4)).astype(np.uint64)       # the other slots must not be read
    return keys


def _spoil(rng, keys, F, each):
    """``each`` records of every kind that counts as empty"""
    idx = rng.permutation(len(keys))[:5 * each].reshape(5, each)
    keys[idx[0], 0] = order_ref.EMPTY
    keys[idx[1], 0] = order_ref.pack_keys(np.float32(1.5), np.uint64(F))
    keys[idx[2], 0] = order_ref.pack_keys(np.float32(np.nan), np.uint64(0))
    keys[idx[3], 0] = order_ref.pack_keys(np.float32(-1.5), np.uint64(0))
    keys[idx[4], 0] = order_ref.pack_keys(np.float32(np.inf), np.uint64(0))


def _words(rng, T, H, W, N, dense=False):
    """raw words with stray bits above N, eroded words a random subset of them (dense: all of them) plus a few bits the raw
    word lacks"""
    hi = 2 ** min(32, N + 2)
    bits = rng.randint(0, hi, (T, H, W), dtype=np.uint64).astype(np.uint32)
    keep = np.uint32(0xffffffff) if dense else rng.randint(0, hi, (T, H, W), dtype=np.uint64).astype(np.uint32)
    ebits = (bits & keep) | \
        (rng.randint(0, hi, (T, H, W), dtype=np.uint64).astype(np.uint32) * (rng.rand(T, H, W) < 0.1)).astype(np.uint32)
    return bits, ebits


def base_case(gate_out=False):
    T, N, F, H, W = 2, 3, 10, 5, 7
    rng = np.random.RandomState(7)
    win = np.asarray([[1, 1, 5, 3],        # inside the image
                      [2, 1, 5, 4],        # touching the right and the bottom edge
                      [2, 2, 0, 3],        # width 0
                      [0, 0, 7, 5],        # frame 1: the whole image
                      [5, 0, 4, 2],        # sticking out on the right: skipped whole
                      [0, 0, 7, 5]], np.int32)
    koff = np.asarray([0, 15, 35, 40, 80, 100], np.int64)
    keys = _random_keys(rng, T * N * H * W, F)
    _spoil(rng, keys, F, 6)
    bits, ebits = _words(rng, T, H, W, N, dense=True)
    gate = None
    if gate_out:
        gate = np.asarray([1, 1, 1, 0.5, 1, 0], np.float32)           # the last body of frame 1 takes part in nothing
    return dict(T=T, N=N, F=F, H=H, W=W, win=win, koff=koff, keys=keys, bits=bits, ebits=ebits, gate=gate)


def full_case(T, N, H, W, seed, F=10, spoil=0):
    rng = np.random.RandomState(seed)
    win = np.tile(np.asarray([0, 0, W, H], np.int32), (T * N, 1))
    koff = np.arange(T * N, dtype=np.int64) * (H * W)
    keys = _random_keys(rng, T * N * H * W, F)
    if spoil:
        _spoil(rng, keys, F, spoil)
    bits, ebits = _words(rng, T, H, W, N)
    return dict(T=T, N=N, F=F, H=H, W=W, win=win, koff=koff, keys=keys, bits=bits, ebits=ebits, gate=None)


def people32_case():
    c = full_case(1, 32, 8, 8, 8)
    P = 64
    z = lambda v: order_ref.pack_keys(np.float32(v), np.uint64(1))
    c['keys'][0 * P + 0, 0], c['keys'][31 * P + 0, 0] = z(2.0), z(1.0)      # pixel 0: person 0 owns it, person 31 in front
    c['ebits'][0, 0, 0], c['bits'][0, 0, 0] = 1, 1
    c['keys'][0 * P + 1, 0], c['keys'][31 * P + 1, 0] = z(1.0), z(2.0)      # pixel 1: person 31 owns it, person 0 in front
    c['ebits'][0, 0, 1], c['bits'][0, 0, 1] = 1 << 31, 1 << 31
    return c


def run_kernel(c, gtransl, acc='own', margin=MARGIN, delta=DELTA, coef=COEF):
    """-> dict of numpy arrays: gtransl after the call, body_loss, count, pairs"""
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    dev = torch.device('cuda:0')
    T, N, B = c['T'], c['N'], c['T'] * c['N']
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    win, koff = d(c['win']), d(c['koff'])
    keys = d(c['keys'].view(np.int64))
    bits, ebits = d(c['bits'].view(np.int32)), d(c['ebits'].view(np.int32))
    gate = None if c['gate'] is None else d(c['gate'])
    g = d(gtransl)
    body = torch.full((B,), 7.0, device=dev)
    count = torch.full((B,), 7, dtype=torch.int32, device=dev)
    pairs = torch.full((T, N, N), 7, dtype=torch.int32, device=dev)
    accb = torch.full((B, 3), 7, dtype=torch.int64, device=dev) if acc == 'own' else None     # (cleared by the call)
    check(_lib.lib().mh_order_term_keys(T, N, c['F'], c['H'], c['W'], ptr(win), ptr(koff), ptr(keys), ptr(bits), ptr(ebits), ptr(gate),
                                        coef, margin, delta, ptr(g), ptr(body), ptr(count), ptr(pairs), ptr(accb),
                                        _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    return dict(gtransl=g.cpu().numpy(), body_loss=body.cpu().numpy(), count=count.cpu().numpy(), pairs=pairs.cpu().numpy())


def reference(c, gtransl, margin=MARGIN, delta=DELTA, coef=COEF):
    return order_ref.order_ref(c['T'], c['N'], c['F'], c['H'], c['W'], c['win'], c['koff'], c['keys'], c['bits'], c['ebits'], c['gate'],
                               coef, margin, delta, gtransl=gtransl)


def same_bits(got, want):
    for k in ('count', 'pairs'):
        assert np.array_equal(got[k], want[k]), k
    for k in ('body_loss', 'gtransl'):
        assert got[k].dtype == np.float32 and want[k].dtype == np.float32
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (k, got[k], want[k])


def _prefill(c, seed=3):
    return np.random.RandomState(seed).uniform(-1, 1, (c['T'] * c['N'], 3)).astype(np.float32)


CASES = {'base': lambda: base_case(), 'base_gated': lambda: base_case(True), 'people32': people32_case,
         'three_workgroups': lambda: full_case(3, 2, 17, 31, 9, spoil=40)}


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_matches_the_reference_bit_for_bit(name):
    """``gtransl`` is pre-filled: the call adds into its z and leaves x and y alone"""
    c = CASES[name]()
    g0 = _prefill(c)
    want = reference(c, g0)
    got = run_kernel(c, g0)
    print('%s: active triples per body %s, G %s' % (name, want['count'].tolist(), want['G']))
    same_bits(got, want)
    assert np.array_equal(got['gtransl'][:, :2].view(np.int32), g0[:, :2].view(np.int32))
    # not vacuous: something is active in every frame (but the one whose second body is gated out), and the cases hold what
    # they are there for
    per_frame = want['count'].reshape(c['T'], c['N']).sum(1)
    assert (per_frame > 0).all() if name != 'base_gated' else (per_frame[0] > 0 and per_frame[1] == 0)
    assert not np.array_equal(got['gtransl'][:, 2], g0[:, 2])
    for t in range(c['T']):
        assert sum(want['G'][t * c['N']:(t + 1) * c['N']]) == 0
    if name == 'base':
        assert want['count'][2] == 0 and want['count'][4] == 0 and not want['pairs'][0, :, 2].any() and not want['pairs'][1, :, 1].any()
        assert want['count'][5] > 0
    if name == 'base_gated':
        assert want['count'][5] == 0 and not want['pairs'][1, :, 2].any() and want['count'][3] == 0
    if name == 'people32':
        assert want['pairs'][0, 0, 31] >= 1 and want['pairs'][0, 31, 0] >= 1
    if name == 'three_workgroups':
        assert (want['count'] > 0).all()


def test_exact_ties_are_active_by_the_margin_and_inactive_without():
    c = full_case(1, 2, 5, 7, 10)
    c['keys'][:, 0] = order_ref.pack_keys(np.float32(2.0), np.uint64(0))
    g0 = _prefill(c)
    for margin in (0.0, 0.25):
        want = reference(c, g0, margin=margin)
        same_bits(run_kernel(c, g0, margin=margin), want)
        assert (want['count'].sum() > 0) == (margin > 0)


def test_one_person_touches_nothing():
    c = full_case(2, 1, 5, 7, 11)
    g0 = _prefill(c)
    g0[0, 2] = -0.0
    got = run_kernel(c, g0)
    assert np.array_equal(got['gtransl'].view(np.int32), g0.view(np.int32))
    assert not got['count'].any() and not got['pairs'].any() and not got['body_loss'].view(np.int32).any()
    same_bits(got, reference(c, g0))


def test_same_bits_twice_and_with_pooled_accumulators():
    c = CASES['three_workgroups']()
    g0 = _prefill(c)
    a, b, pooled = run_kernel(c, g0), run_kernel(c, g0), run_kernel(c, g0, acc=None)
    same_bits(b, a)
    same_bits(pooled, a)


def test_each_output_alone():
    import torch
    from mhhip import _lib
    from mhhip._lib import check, ptr
    c = CASES['base']()
    g0 = _prefill(c)
    want = run_kernel(c, g0)
    dev = torch.device('cuda:0')
    T, N, B = c['T'], c['N'], c['T'] * c['N']
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    tabs = (d(c['win']), d(c['koff']), d(c['keys'].view(np.int64)), d(c['bits'].view(np.int32)), d(c['ebits'].view(np.int32)))
    outs = dict(gtransl=d(g0), body_loss=torch.zeros(B, device=dev), count=torch.zeros(B, dtype=torch.int32, device=dev),
                pairs=torch.zeros(T, N, N, dtype=torch.int32, device=dev))
    for k in outs:
        args = [ptr(outs[j]) if j == k else None for j in ('gtransl', 'body_loss', 'count', 'pairs')]
        check(_lib.lib().mh_order_term_keys(T, N, c['F'], c['H'], c['W'], *(ptr(x) for x in tabs), None, COEF, MARGIN, DELTA, *args, None,
                                            _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    same_bits({k: v.cpu().numpy() for k, v in outs.items()}, want)


def test_pooled_accumulators_are_refused_on_a_capturing_stream():
    """``acc`` NULL asks for the stream's memory pool: on a stream that is being captured the call answers -1 with a message,
    before any launch (the captured graph holds the one fill below and is never replayed)"""
    import torch
    from mhhip import _lib
    from mhhip._lib import ptr
    c = CASES['base']()
    dev = torch.device('cuda:0')
    T, N, B = c['T'], c['N'], c['T'] * c['N']
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    tabs = (d(c['win']), d(c['koff']), d(c['keys'].view(np.int64)), d(c['bits'].view(np.int32)), d(c['ebits'].view(np.int32)))
    g0 = _prefill(c)
    g, body, other = d(g0), torch.full((B,), 7.0, device=dev), torch.zeros(4, device=dev)
    L = _lib.lib()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        other.fill_(1.0)
        rc = L.mh_order_term_keys(T, N, c['F'], c['H'], c['W'], *(ptr(x) for x in tabs), None, COEF, MARGIN, DELTA, ptr(g), ptr(body),
                                  None, None, None, _lib.stream_ptr(dev))
        msg = L.mh_last_error()
    torch.cuda.synchronize()
    assert rc == -1 and b'capturing' in msg and b'acc' in msg, (rc, msg)
    assert np.array_equal(g.cpu().numpy().view(np.int32), g0.view(np.int32)) and (body == 7.0).all()


def test_real_workspace(smpl_struct, smpl_regs):
    """``mh_order_term`` on the workspace of a selection pass, T=3, N=3, 48 x 32: persons 0 and 1 one behind the other, person
    2 apart.  The masks are packed from the ``person`` labels ``render_scene`` gives for ANOTHER depth order (0 and 1 swapped
    along their rays); the result is compared with the reference fed by ``RasterTerms.selection``'s tables."""
    import types
    import torch
    from mhhip import engine, raster, synthetic, _lib
    from mhhip._lib import check, ptr
    T, N, W, H = 3, 3, 48, 32
    model = engine.BodyModel(smpl_struct, smpl_regs)
    dev = model.device
    K = synthetic.default_cam_K((W, H), 60.0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    sp = synthetic.make_sequence_params(N, T, 21)

    def bodies(z0, z1):
        pT = np.zeros((T, N, 3), np.float32)
        pT[:, 0] = np.float32([0.02, 0.05, 1.0]) * z0          # on nearly the same ray
        pT[:, 1] = np.float32([-0.02, 0.05, 1.0]) * z1
        pT[:, 2] = np.float32([0.45, 0.05, 1.0]) * 2.0         # apart
        pT[:, :, 2] += 0.02 * np.arange(T, dtype=np.float32)[:, None]
        v, _, _, _ = model.lbs_forward(t(sp['betas_gt']), t(sp['poses_gt']).view(T * N, 72), None, t(pT).view(T * N, 3), want_vposed=False)
        return v.view(T, N, -1, 3).contiguous()

    seen = raster.render_scene(model, bodies(2.2, 1.6), K, (W, H), outputs=('person',))['person']      # the images: person 1 in front
    seg = torch.stack([(seen == n).float() for n in range(N)], 1).contiguous()                          # (T,N,H,W)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    bits = torch.zeros(T, H, W, dtype=torch.int32, device=dev)
    tmp, ebits, area = torch.zeros_like(bits), torch.zeros_like(bits), torch.zeros(T * N, device=dev)
    check(L.mh_pack_masks(ptr(seg), T, N, H, W, ptr(bits), ptr(area), st))
    check(L.mh_erode_bits(ptr(bits), ptr(tmp), T, H, W, st))
    check(L.mh_erode_bits(ptr(tmp), ptr(ebits), T, H, W, st))
    verts = bodies(1.6, 2.2)                                                                            # the fit: person 0 in front
    faces = torch.as_tensor(np.ascontiguousarray(np.asarray(model.faces).astype(np.int32))).to(dev)
    F, V = int(faces.shape[0]), int(verts.shape[2])
    dims = (T, N, V, F, H, W)
    ws = torch.empty(L.mh_raster_workspace_bytes(*dims), dtype=torch.uint8, device=dev)
    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    zf = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    raster.selection_pass(dims, np.ascontiguousarray(K.reshape(9)), verts, faces, ws, st)
    g0 = _prefill(dict(T=T, N=N))
    g = t(g0)
    body, count, pairs = zf(T * N), zi(T * N), zi(T, N, N)
    check(L.mh_order_term(*dims, ptr(ws), ptr(bits), ptr(ebits), None, COEF, 0.05, DELTA, ptr(g), ptr(body), ptr(count), ptr(pairs), None, st))
    torch.cuda.synchronize()
    got = dict(gtransl=g.cpu().numpy(), body_loss=body.cpu().numpy(), count=count.cpu().numpy(), pairs=pairs.cpu().numpy())
    # the reference on the tables of the same workspace: selection() gathers the keys into body order
    stand_in = types.SimpleNamespace(B=T * N, H=H, W=W)
    sel = types.SimpleNamespace(ws=ws, dims=dims)
    win, koff, keys = raster.RasterTerms.selection(sel, stand_in)
    full = np.full((T * N * H * W, 5), order_ref.EMPTY, np.uint64)
    full[:len(keys)] = keys
    want = order_ref.order_ref(T, N, F, H, W, win, koff[:-1], full, bits.cpu().numpy(), ebits.cpu().numpy(), None, COEF, 0.05, DELTA,
                               gtransl=g0)
    print('active triples per body %s' % want['count'].reshape(T, N).tolist())
    same_bits(got, want)
    assert (want['count'].reshape(T, N)[:, 1] > 0).all(), 'person 1 is seen in front but fitted behind: it owns violated pixels'
    assert want['pairs'][:, 1, 0].sum() == want['count'].reshape(T, N)[:, 1].sum() and not want['pairs'][:, 2].any()
