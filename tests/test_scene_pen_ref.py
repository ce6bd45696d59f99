"""The float64 restatement of the scene-penetration term (tests/scene_pen_ref.py) against itself: its analytic gradient
against central differences, the direction of the gradient on a plane, cases computed by hand, and the conditions the
generated cases must meet before anything on the device is compared with them.  No GPU."""
import numpy as np
import pytest

import scene_pen_ref as sp

CASES = [(B, V, H, W, k) for (B, V) in sp.SHAPES for (H, W) in sp.IMAGES for k in sp.KINDS]


@pytest.fixture(scope='module')
def body_case(smpl_struct):
    return sp.body_case(smpl_struct.v_template)


@pytest.mark.parametrize('key', [k for k in CASES if k[0] * k[1] >= 63 and k[2] >= 2])
def test_gradient_equals_central_difference(key):
    """every vertex contributes on its own, so one pair of evaluations per axis differentiates all of them.  Step 1e-6 m: a
    decided vertex (1e-3 px and 1e-5 m away from every branch) keeps its branch; the truncation error h^2 f''' / 6 and the
    rounding error 1e-16 |value| / h are both below 1e-7 of the largest gradient entry"""
    c = sp.case(*key)
    v = c['verts'].astype(np.float64)
    r = sp.evaluate(v, c['K'], c['zmap'], round_verts=False)
    dec = ~r['undecided']
    h = 1e-6
    for ax in range(3):
        d = np.zeros(3)
        d[ax] = h
        up = sp.evaluate(v + d, c['K'], c['zmap'], round_verts=False)['vloss']
        dn = sp.evaluate(v - d, c['K'], c['zmap'], round_verts=False)['vloss']
        fd = (up - dn) / (2 * h)
        scale = max(np.abs(r['grad']).max(), 1e-30)
        assert np.abs(fd - r['grad'][..., ax])[dec].max() <= 1e-7 * scale, (key, ax)
    if c['full']:
        assert (np.abs(r['grad'][dec & r['active']]).sum(-1) > 0).all()


@pytest.mark.parametrize('size', [(9, 16), (135, 240)])
def test_gradient_on_a_plane_is_parallel_to_its_normal(size):
    """The map is the depth of the plane n . X = d at the pixel centres, D(ray) = d / (n . ray).  With the header's formulas
    the gradient of p at a vertex at depth z on that ray is, exactly,

        grad p = s n + (1 - D / z) e_z,      s = D / (z n . ray),      1 - D / z = (p + margin) / z:

    parallel to n ON the surface and tilted towards the optical axis by (p + margin) / z behind it -- at most
    (band + margin) / z, a few degrees at room distances.  Both halves are asserted: (a) what is left after taking
    (p + margin) / z e_z away is parallel to n, and (b) the gradient itself is within that tilt of n.
    Discretisation: depth along a row is not linear, the slope of a bilinear cell is off by at most half a pixel of the second
    derivative 2 D n_x^2 / f^2 per pixel^2 -- in the units of grad p 2.8e-4 per axis at 9 x 16 (f = 36, D = 3), less at
    135 x 240: an angle of a few 1e-4 rad, 1 - cos of order 1e-7.  Asserted: 1 - cos <= 1e-6 for (a) and the same angle,
    sqrt(2e-6) = 1.5e-3 rad, as slack for (b)."""
    H, W = size
    c = sp.case(2, 257, H, W, 'floor')
    r = sp.evaluate(c['verts'], c['K'], c['zmap'])
    act = r['active']
    assert act.sum() >= 20
    z, p = c['verts'][..., 2].astype(np.float64)[act], r['p'][act]
    gp = r['grad'][act] / (2 * np.float64(np.float32(sp.COEF)) * p / c['V'])[:, None]       # grad p
    tilt = (p + np.float64(np.float32(sp.MARGIN))) / z
    rest = gp - tilt[:, None] * np.array([0, 0, 1.0])
    cos = (rest @ sp.PLANE_N) / np.linalg.norm(rest, axis=1)
    print('%dx%d: %d active vertices, on-surface part 1 - |cos| at most %.2e, tilt at most %.3f rad' % (H, W, act.sum(), (1 - np.abs(cos)).max(),
                                                                                                         tilt.max()))
    assert (1 - np.abs(cos)).max() <= 1e-6
    assert (cos < 0).all()          # n points away from the camera's side of the plane (n_z < 0): the push is against it, out of the scene
    sin = np.linalg.norm(np.cross(gp, sp.PLANE_N), axis=1) / np.linalg.norm(gp, axis=1)
    bound = tilt * np.linalg.norm(np.cross([0, 0, 1.0], sp.PLANE_N)) / np.linalg.norm(gp, axis=1)
    assert (sin <= bound + 1.5e-3).all()


K4 = np.float32([[10, 0, 2], [0, 10, 2], [0, 0, 1]])       # 4 x 4 image; the vertex (0, 0, z) projects to u = v = 2: taps 1, 2


def _one(z, zmap, x=0.0, y=0.0, **kw):
    kw = dict(dict(coef=0.5, margin=0.0625, band=0.5, edge=0.25), **kw)
    return sp.evaluate(np.float32([[[x, y, z]]]), K4, np.asarray(zmap, np.float32), **kw)


def test_hand_computed_cases():
    flat = np.full((4, 4), 2.0)
    # over a constant map: D = 2, p = 2.3625 - 2 - 0.0625 = 0.3, value 0.5 * 0.09, gradient (0, 0, 2 * 0.5 * 0.3)
    r = _one(2.3625, flat)
    assert r['active'].all() and abs(r['body'][0] - 0.045) < 1e-7 and abs(r['p'][0, 0] - 0.3) < 1e-7
    assert np.allclose(r['grad'][0, 0], [0, 0, 0.3], atol=1e-7) and r['grad'][0, 0, 0] == 0 and r['grad'][0, 0, 1] == 0
    # a map that rises 0.1 m per column: a = 0.5 between columns 1 and 2, D = 2.15, Du = 0.1, p = 2.5 - 2.15 - 0.0625
    ramp = 2.0 + 0.1 * np.tile(np.arange(4.0), (4, 1))
    r = _one(2.5, ramp)
    g = 2 * 0.5 * 0.2875
    assert abs(r['p'][0, 0] - 0.2875) < 1e-7
    assert np.allclose(r['grad'][0, 0], [-g * 0.1 * 10 / 2.5, 0, g], atol=1e-7)
    # p = band exactly (all three numbers are binary fractions): not active, 0 < p < band is strict on both sides
    r = _one(2.5625, flat)
    assert r['p'][0, 0] == 0.5 and not r['active'].any() and r['body'][0] == 0 and (r['grad'] == 0).all()
    r = _one(2.0625, flat)
    assert r['p'][0, 0] == 0.0 and not r['active'].any() and r['body'][0] == 0
    # behind a discontinuity: columns 0-1 at 2 m, columns 2-3 at 3 m, the taps straddle the step
    step = np.where(np.arange(4)[None] < 2, 2.0, 3.0) * np.ones((4, 1))
    r = _one(3.3, step)
    assert r['skipped'].all() and r['body'][0] == 0 and (r['grad'] == 0).all()
    assert _one(2.3, step, x=-0.23).get('active').all()          # u = 1.0: taps 0 and 1, no step between them
    # a tap outside the image: u = 0.25 -> i0 = -1; u = 3.75 -> i0 + 1 = 4
    for x in (-0.35 * 2.3, 0.35 * 2.3):
        r = _one(2.3, flat, x=x / 2.0)
        assert r['skipped'].all() and r['body'][0] == 0, x
    # a zero tap (no scene there)
    hole = flat.copy()
    hole[2, 2] = 0.0
    r = _one(2.3, hole)
    assert r['skipped'].all() and r['body'][0] == 0 and (r['grad'] == 0).all()
    # behind the camera
    r = _one(-2.3, flat)
    assert r['skipped'].all() and r['body'][0] == 0


@pytest.mark.parametrize('key', CASES)
def test_generated_cases_meet_their_conditions(key):
    c = sp.case(*key)
    r = sp.evaluate(c['verts'], c['K'], c['zmap'])
    n = c['B'] * c['V']
    if c['full']:
        assert r['undecided'].sum() <= 0.02 * n and r['active'].sum() >= 20, (int(r['undecided'].sum()), int(r['active'].sum()))
    if (c['H'], c['W']) == (1, 1):
        assert r['skipped'].all() and r['value'] == 0
    if key[4] == 'step' and c['full']:
        assert (r['skipped'] & ~r['undecided']).sum() > 0
    again = sp.case(*key)
    assert np.array_equal(again['verts'], c['verts']) and np.array_equal(again['zmap'], c['zmap'])


def test_body_case_meets_its_conditions(body_case):
    c = body_case
    r = sp.evaluate(c['verts'], c['K'], c['zmap'])
    assert c['V'] == 6890 and r['undecided'].sum() <= 0.02 * c['B'] * c['V'] and r['active'].sum() >= 20
    assert r['active'][0].any() and r['active'][1].any()


def test_float32_evaluation_is_close(body_case):
    """the yardstick itself: p = z - D - margin loses z / p of the 2^-24 of its inputs, so the float32 evaluation is good to
    about 1e-6 of the value and of the largest gradient entry -- if it were 1e-4 the budget would check nothing"""
    cases = [sp.case(*k) for k in CASES] + [body_case]
    for c in cases:             # no vertex of any case changes its branch in float32: the values are compared without a window
        r64, r32 = sp.evaluate(c['verts'], c['K'], c['zmap']), sp.evaluate(c['verts'], c['K'], c['zmap'], dtype=np.float32)
        assert np.array_equal(r32['active'], r64['active']) and np.array_equal(r32['skipped'], r64['skipped'])
    bv, bg = sp.budgets(cases)
    print('float32 evaluation against float64 over %d cases: value %.3e, gradient %.3e' % (len(cases), bv, bg))
    assert 0 < bv < 1e-5 and 0 < bg < 1e-5
