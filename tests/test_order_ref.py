"""The numpy reference of the depth-ordering term (tests/order_ref.py) against cases computed by hand.  Every number here
is a dyadic rational, so the expected fixed-point sums are exact integers."""
import numpy as np

import order_ref
from order_ref import FIX


def _run(z, bits, ebits, margin, delta, coef=1.0, gate=None, gtransl=None, empty=None, face=None, F=4):
    z = np.asarray(z, np.float32)
    T, N, H, W = z.shape
    win, koff, keys = order_ref.full_tables(z, face=face, empty=empty)
    return order_ref.order_ref(T, N, F, H, W, win, koff, keys, np.asarray(bits, np.uint32).reshape(T, H, W),
                               np.asarray(ebits, np.uint32).reshape(T, H, W), gate, coef, margin, delta, gtransl=gtransl)


def test_two_bodies_three_pixels():
    """pixel 0: person 0 owns it, person 1 is 0.5 m in FRONT: d = 0.5 + 0.25 = 0.75 > delta: m = 0.5, r = 0.5 (1.5 - 0.5) = 0.5;
    pixel 1: person 0 owns it, person 1 is 0.5 m behind: d = -0.25, inactive;
    pixel 2: person 1 owns it, person 0 at the same depth: d = 0.25, m = 0.25, r = 0.25 (0.5 - 0.25) = 0.0625"""
    z = [[[[2.0, 2.0, 3.0]], [[1.5, 2.5, 3.0]]]]
    g0 = np.asarray([[1, 2, 3], [4, 5, -6]], np.float32)
    r = _run(z, bits=[1, 1, 2], ebits=[1, 1, 2], margin=0.25, delta=0.5, coef=3.0, gtransl=g0)
    assert r['G'] == [FIX // 2 - FIX // 4, FIX // 4 - FIX // 2]
    assert r['R'] == [FIX // 2, FIX // 16]
    assert r['C'] == [1, 1]
    assert r['pairs'].tolist() == [[[0, 1], [1, 0]]]
    # cl = 3 / 3 = 1, cg = 2 * 3 / 3 = 2
    assert r['body_loss'].tolist() == [0.5, 0.0625] and r['body_loss'].dtype == np.float32
    assert r['count'].tolist() == [1, 1]
    assert r['gtransl'].tolist() == [[1, 2, 3.5], [4, 5, -6.5]]


def test_raw_bit_set_means_no_occluder_and_unowned_pixels_count_nothing():
    z = [[[[2.0, 2.0]], [[1.0, 1.0]]]]
    r = _run(z, bits=[3, 1], ebits=[1, 0], margin=0.0, delta=0.5)      # pixel 0: person 1 may be there; pixel 1: nobody is sure
    assert r['C'] == [0, 0] and r['G'] == [0, 0] and r['R'] == [0, 0]


def test_d_exactly_zero_is_inactive():
    z = [[[[2.0]], [[2.0]]]]
    r = _run(z, bits=[1], ebits=[1], margin=0.0, delta=0.5)
    assert r['C'] == [0, 0] and r['G'] == [0, 0] and r['R'] == [0, 0] and not r['pairs'].any()
    r = _run(z, bits=[1], ebits=[1], margin=2.0 ** -20, delta=0.5)     # the smallest step above: active
    assert r['C'] == [1, 0] and r['G'] == [16, -16]


def test_d_equal_delta_joins_the_two_branches():
    z = [[[[2.5]], [[2.0]]]]
    r = _run(z, bits=[1], ebits=[1], margin=0.0, delta=0.5)            # d = delta: m = delta, r = delta (2 delta - delta) = delta^2
    assert r['G'] == [FIX // 2, -(FIX // 2)] and r['R'] == [FIX // 4, 0]


def test_linear_branch_far_beyond_delta():
    z = [[[[12.0]], [[2.0]]]]
    r = _run(z, bits=[1], ebits=[1], margin=0.0, delta=0.5)            # d = 10: m = 0.5, r = 0.5 (20 - 0.5) = 9.75 = 2 delta d - delta^2
    assert r['G'] == [FIX // 2, -(FIX // 2)] and r['R'] == [39 * FIX // 4, 0]
    assert r['body_loss'].tolist() == [9.75, 0.0]


def test_r_is_clamped():
    z = [[[[3002.0]], [[2.0]]]]
    r = _run(z, bits=[1], ebits=[1], margin=0.0, delta=1024.0)         # d = 3000: m = 1024, r = 1024 (6000 - 1024) -> 1024
    assert r['G'] == [1024 * FIX, -1024 * FIX] and r['R'] == [1024 * FIX, 0]
    z = [[[[3e38]], [[2.0]]]]
    r = _run(z, bits=[1], ebits=[1], margin=0.0, delta=0.5)            # d + d overflows to infinity: still the clamp
    assert r['R'] == [1024 * FIX, 0] and r['G'][0] == FIX // 2


def test_undefined_depths_and_the_gate():
    """an empty key, a face index >= F, a NaN, a negative and an infinite z count as empty -- for an owner and for an occluder"""
    z = np.asarray([[[[2.0, 2.0, 2.0, 2.0, 2.0, 2.0]], [[1.0, 1.0, np.nan, -1.0, np.inf, 1.0]]]], np.float32)
    empty = np.zeros(z.shape, bool)
    empty[0, 1, 0, 0] = True
    face = np.zeros(z.shape, np.uint64)
    face[0, 1, 0, 1] = 4
    r = _run(z, bits=[1] * 6, ebits=[1] * 6, margin=0.0, delta=0.5, empty=empty, face=face, F=4)
    assert r['C'] == [1, 0] and r['pairs'][0, 0, 1] == 1               # only the last pixel
    r = _run(z, bits=[2] * 6, ebits=[2] * 6, margin=5.0, delta=0.5, empty=empty, face=face, F=4)
    assert r['C'] == [0, 1]                                            # person 1 as the owner: its bad depths own nothing
    for gate in ([1, 0], [0, 1]):
        r = _run(z, bits=[1] * 6, ebits=[1] * 6, margin=0.0, delta=0.5, gate=np.asarray(gate, np.float32))
        assert r['C'] == [0, 0] and r['G'] == [0, 0]


def test_person_31_is_bit_31_and_g_sums_to_zero_per_frame():
    rng = np.random.RandomState(0)
    T, N, H, W = 2, 32, 3, 4
    z = rng.choice(np.float32([1.0, 1.5, 2.0, 2.7, 3.1]), (T, N, H, W))
    bits = rng.randint(0, 2 ** 32, (T, H, W), dtype=np.uint64).astype(np.uint32)
    ebits = bits & rng.randint(0, 2 ** 32, (T, H, W), dtype=np.uint64).astype(np.uint32)
    z[0, 31, 0, 0], z[0, 0, 0, 0] = 3.0, 1.0
    ebits[0, 0, 0], bits[0, 0, 0] = 1 << 31, 1 << 31                   # person 31 owns the pixel, everybody else is absent
    win, koff, keys = order_ref.full_tables(z)
    r = order_ref.order_ref(T, N, 4, H, W, win, koff, keys, bits, ebits, None, 1.0, 0.05, 0.5, gtransl=np.zeros((T * N, 3), np.float32))
    assert r['pairs'][0, 31, 0] >= 1 and sum(r['C']) > 100
    for t in range(T):
        assert sum(r['G'][t * N:(t + 1) * N]) == 0
    assert any(v != 0 for v in r['G'])
    assert sum(r['C']) == int(r['pairs'].sum()) and (r['pairs'].sum(2).reshape(-1) == r['count']).all()


def test_one_person_touches_nothing():
    z = np.full((2, 1, 2, 2), 2.0, np.float32)
    g0 = np.asarray([[1, 2, -0.0], [3, 4, 5]], np.float32)
    r = _run(z, bits=[1] * 8, ebits=[1] * 8, margin=1.0, delta=0.5, gtransl=g0)
    assert r['C'] == [0, 0] and r['body_loss'].tolist() == [0.0, 0.0]
    assert np.array_equal(r['gtransl'].view(np.int32), g0.view(np.int32))


def test_windows():
    """a window inside the image, one whose keys would leave the key array, one sticking out and one of width 0"""
    T, N, F, H, W = 1, 2, 4, 3, 4
    keys = np.full((T * N * H * W, 5), order_ref.EMPTY, np.uint64)
    keys[:, 0] = order_ref.pack_keys(np.float32(1.0), 0)
    keys[0:2, 0] = order_ref.pack_keys(np.float32(2.0), 0)             # body 0: window (1,1) 2 x 1 at key 0
    bits, ebits = np.full((T, H, W), 1, np.uint32), np.full((T, H, W), 1, np.uint32)
    base = np.asarray([[1, 1, 2, 1], [0, 0, 4, 3]], np.int32)
    r = order_ref.order_ref(T, N, F, H, W, base, np.asarray([0, 12]), keys, bits, ebits, None, 1.0, 0.0, 0.5)
    assert r['C'] == [2, 0]                                            # the two pixels of body 0's window, person 1 1 m in front
    for win1, ko1 in (([0, 0, 4, 3], 13), ([1, 0, 4, 3], 12), ([0, 1, 4, 3], 12), ([0, 0, 0, 3], 12), ([-1, 0, 4, 3], 12), ([0, 0, 4, 3], -1)):
        w = base.copy()
        w[1] = win1
        r = order_ref.order_ref(T, N, F, H, W, w, np.asarray([0, ko1]), keys, bits, ebits, None, 1.0, 0.0, 0.5)
        assert r['C'] == [0, 0], (win1, ko1)
