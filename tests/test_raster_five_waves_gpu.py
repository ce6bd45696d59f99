"""The selection kernel (csrc/mh_raster.hip, k_raster_strip) was put on a register diet and built with tile workgroups of
ten waves (five per SIMD, RSB = 640) as well as the eight it keeps: a tile's rounds of 64 candidate faces are dealt to the
waves with a stride of RSB faces, so with another wave count another wave meets a face, and the keys reach a pixel in
another order.  Whatever RSB the library is built with, the 40 bytes per pixel must be the same:

* against two independent forms of the same launch the tree already has -- every round through the even split
  (mh_raster_set_path), and a fresh sort without the winners' list (mh_raster_set_winners) -- on meshes whose candidate
  counts straddle the strides of eight and of ten waves (fewer rounds than waves, exactly one per wave, one more), bit for
  bit;
* against keys recorded with the build of the commit before the change (tests/golden/make_five_waves.py), bit for bit;
* a three-cycle deterministic fit twice (same bits) and against the leaves recorded with that build: with ten waves the
  depth term's tile sums add ten partial sums instead of eight, in wave order, so this one is held to the cycle tests'
  tolerance (tests/test_cycle_fuzz_gpu.py: every entry within 1e-4 of the leaf's largest, 1e-3 for the scale leaf) through
  tests/parity_gates.py."""
import numpy as np
import pytest

import make_five_waves as mk
from parity_gates import two_precision_gate

pytestmark = pytest.mark.gpu

_R_CAP = 704          # pixels of a tile (csrc/mh_raster.hip)


def _subset(faces, F, seed, verts, W, H, fov):
    """F faces of the body model: faces that own a pixel of the whole mesh first (so that a mesh of one face is on screen),
    then random ones"""
    if F is None:
        return faces
    _, k = mk.Selection(verts, faces, W, H, fov).launch()
    rng = np.random.RandomState(seed)
    own = np.unique((k[:, 0][k[:, 0] != mk.EMPTY] & np.uint64(0xffffffff)).astype(np.int64))
    rest = np.setdiff1d(np.arange(len(faces)), own)
    order = np.concatenate([rng.permutation(own), rng.permutation(rest)])[:F]
    return np.ascontiguousarray(faces[rng.permutation(order)])


def _mesh_cases():
    cases = []
    for i, F in enumerate([1, 63, 64, 65, 639, 640, 641, 1279, 1281, 511, 512, 513, 1025]):
        W, H = ((48, 27), (27, 48))[i % 2]
        # far enough for a window of one tile (every face is a candidate of it); every other pair nearer: the faces are split
        # between two tiles
        cases.append(('F%d' % F, dict(F=F, W=W, H=H, N=1 + i % 2, seed=900 + i, zlo=(2.6, 0.8)[i // 2 % 2], zhi=(3.0, 0.95)[i // 2 % 2])))
    cases.append(('smpl_sized', dict(F=None, W=27, H=48, N=2, seed=920, zlo=0.9, zhi=1.1)))
    cases.append(('single_row_window', dict(F=None, W=27, H=48, N=8, seed=921, zlo=1.2, zhi=1.3, single_row=True)))
    cases.append(('column_tiles', dict(F=None, W=1000, H=40, N=1, seed=9, zlo=0.85, zhi=1.0, fov=1.6, wide=True)))
    cases.append(('behind_camera', dict(F=1281, W=48, H=27, N=2, seed=923, zlo=2.0, zhi=2.4, behind=True)))
    return cases


@pytest.mark.parametrize('name,c', _mesh_cases(), ids=[n for n, _ in _mesh_cases()])
def test_keys_do_not_depend_on_the_path_or_the_sort(smpl_struct, smpl_regs, name, c):
    from mhhip import _lib
    from mhhip.raster import set_sort_margin, set_winners
    W, H, N = c['W'], c['H'], c['N']
    fov = c.get('fov', 60.0)
    verts = mk.posed_bodies(smpl_struct, smpl_regs, 1, N, W, H, c['seed'], c['zlo'], c['zhi'])
    if c.get('behind'):
        verts[0, 0, :, 2] -= 6.0
    if c.get('single_row'):
        # windows are the vertices' pixel box +- 2 pixels, clipped to the image: bodies 1.. are copies of body 1 whose lowest
        # vertex ends 1.5 to 3 rows above the image in quarter-row steps -- the window of some of them is row 0 alone
        f = 0.5 * min(W, H) / np.tan(np.pi * fov / 360.0)
        for n in range(1, N):
            v = verts[0, 1].copy()
            row = f * v[:, 1] / v[:, 2] + 0.5 * H
            v[:, 1] -= (row.max() + 1.5 + 0.25 * (n - 1)) * v[:, 2] / f
            verts[0, n] = v
    faces = _subset(np.asarray(smpl_struct.f).astype(np.int32), c['F'], c['seed'], verts, W, H, fov)
    s = mk.Selection(verts, faces, W, H, fov)
    L = _lib.lib()
    old_margin, old_winners = set_sort_margin(0), set_winners(True)        # margin 0: every launch sorts its faces
    try:
        win, k_first = s.launch()                  # fresh workspace: no keys of a launch before, so no winners yet
        _, k_winners = s.launch()                  # the sort puts the first launch's winners in front
        try:
            L.mh_raster_set_path(1)                # every round through the even split
            _, k_even = s.launch()
        finally:
            L.mh_raster_set_path(0)
        set_winners(False)
        _, k_plain = s.launch()                    # fresh sort, winners' list off
    finally:
        set_sort_margin(old_margin)
        set_winners(old_winners)
    live = int((k_first[:, 0] != mk.EMPTY).sum())
    print('%s: windows %s, %d live pixels' % (name, win.tolist(), live))
    assert live >= (1 if c['F'] else 100), 'the bodies are not on screen'
    if c.get('behind'):
        assert win[0, 2] <= 0 or win[0, 3] <= 0 or (k_first[:int(win[0, 2]) * int(win[0, 3]), 0] == mk.EMPTY).all()
    if c.get('single_row'):
        assert (win[1:, 3] == 1).any(), win.tolist()
    if c.get('wide'):
        assert win[0, 2] > _R_CAP, win.tolist()
    for what, k in (('winners first', k_winners), ('all even split', k_even), ('fresh sort without winners', k_plain)):
        assert k.shape == k_first.shape
        diff = (k != k_first).any(axis=1)
        assert not diff.any(), '%s, %s: %d of %d window pixels differ' % (name, what, int(diff.sum()), len(diff))


@pytest.mark.parametrize('scene', mk.KEY_SCENES, ids=[s[0] for s in mk.KEY_SCENES])
def test_keys_are_those_of_the_build_before_the_register_diet(smpl_struct, scene):
    fx = np.load(mk.FIXTURE, allow_pickle=False)
    name, W, H = scene[0], scene[1], scene[2]
    faces = np.asarray(smpl_struct.f).astype(np.int32)
    assert mk.faces_digest(faces) == str(fx['faces_sha1']), 'the synthetic body model is not the one the fixture was written with'
    win, keys = mk.Selection(fx[name + '_verts'], faces, W, H).launch()
    assert (win == fx[name + '_win']).all(), (win.tolist(), fx[name + '_win'].tolist())
    want = fx[name + '_keys']
    assert int((want[:, 0] != mk.EMPTY).sum()) > 100
    assert keys.shape == want.shape
    diff = (keys != want).any(axis=1)
    assert not diff.any(), '%s: %d of %d window pixels differ from the recorded keys' % (name, int(diff.sum()), len(diff))


def test_three_cycle_fit_repeats_and_matches_the_build_before_the_register_diet(smpl_struct, smpl_regs, oracle_model, tmp_path):
    fx = np.load(mk.FIXTURE, allow_pickle=False)
    runs = []
    for r in range(2):
        sub = tmp_path / ('run%d' % r)
        sub.mkdir()
        runs.append(mk.fit_leaves(smpl_struct, smpl_regs, oracle_model, sub))
    for n, v in runs[0].items():
        assert np.array_equal(v, runs[1][n]), '%s differs between two runs of the same build' % n
        want = fx['fit_' + n].reshape(v.shape)
        scale = max(float(np.abs(want).max()), 1e-8)
        print('%s: largest difference from the recorded leaves %.3e of the largest entry' % (n, float(np.abs(v - want).max()) / scale))
    for n, v in runs[0].items():
        want = fx['fit_' + n].reshape(v.shape)
        two_precision_gate(v, want, want, 1e-3 if n == 'xscale' else 1e-4, 'leaf %s after %d cycles' % (n, mk.FIT['cycles']))
