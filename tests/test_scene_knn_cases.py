"""The neighbour-search edge cases of tests/knn_cases.py against their float64 reference alone (no GPU): the GPU tests
skip a query whose k-th and (k+1)-th neighbour float32 cannot tell apart, and check dy only -- so here every case has
to leave (almost) nothing to that skip rule, and has to be a case in which one wrong neighbour out of k moves dy by
well more than the tolerance."""
import numpy as np
import pytest

import knn_cases as kc


@pytest.mark.parametrize('name', kc.NAMES)
def test_case_is_decided_and_sensitive(name):
    c, r = kc.case(name), kc.case_reference(name)
    B, M = c.q.shape[0], c.pts.shape[0]
    assert r.dy.shape == r.swap.shape == (B,) and r.d2.shape == (B, min(c.k, M) + 1)
    assert np.isfinite(r.dy).all() and np.isfinite(r.swap).all()
    assert (np.diff(r.d2, axis=1) >= 0).all()
    skipped = int((~r.checked).sum())
    sens = np.abs(r.swap - r.dy)[r.checked] > 4.0 * kc.tolerance(r.dy[r.checked])
    print('%s: M %d, B %d, k %d: skipped %d (%.1f %%), undecided but checked %d, sensitive %.1f %% of the checked'
          % (name, M, B, c.k, skipped, 100.0 * skipped / B, int((r.checked & ~r.decided).sum()), 100.0 * sens.mean()))
    assert skipped <= 0.02 * B
    if name.startswith('m_edges_') or name == 'identical' or M <= c.k:
        assert skipped == 0
    if M <= c.k:
        assert r.decided.all()
    if name == 'identical':
        assert not r.decided.any() and r.checked.all()      # all ties, all with the same y
    else:
        assert sens.mean() >= 0.5


def test_reference_matches_a_plain_argsort():
    c, r = kc.case('k_sweep_volume_k7'), kc.case_reference('k_sweep_volume_k7')
    d = ((c.q[:, None, :].astype(np.float64) - c.pts[None].astype(np.float64)) ** 2).sum(-1)
    idx = np.argsort(d, axis=1, kind='stable')
    np.testing.assert_allclose(r.dy, c.pts[idx[:, :7], 1].astype(np.float64).mean(1) - c.q[:, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r.d2, np.take_along_axis(d, idx[:, :8], 1), rtol=1e-14, atol=0)
    want = (c.pts[idx[:, :6], 1].astype(np.float64).sum(1) + c.pts[idx[:, 7], 1]) / 7 - c.q[:, 1]
    np.testing.assert_allclose(r.swap, want, rtol=0, atol=1e-12)


def test_grid_premises():
    """each degenerate cloud reaches the branch of k_grid_setup's sizing rule it is meant for"""
    g = kc.grid_sizing(kc.case('cell_cap').pts)
    assert g['ncells0'] > kc.GRID_MAX_CELLS and g['loops'] >= 1 and np.prod(g['dims']) <= kc.GRID_MAX_CELLS
    for name, axis in (('plane_x', 0), ('plane_z', 2)):
        g = kc.grid_sizing(kc.case(name).pts)
        assert g['ext'][axis] == np.float32(1e-3) and g['dims'][axis] == 1 and min(np.delete(g['dims'], axis)) > 1
    g = kc.grid_sizing(kc.case('line_y').pts)
    assert g['ext'][0] == g['ext'][2] == np.float32(1e-3) and g['cell0'] == np.float32(0.02) and g['dims'][1] > 64
    g = kc.grid_sizing(kc.case('speck').pts)
    assert g['cell0'] == np.float32(0.02) and g['dims'] == [1, 1, 1]
    g = kc.grid_sizing(kc.case('identical').pts)
    assert (g['ext'] == np.float32(1e-3)).all() and g['dims'] == [1, 1, 1]
    g = kc.grid_sizing(kc.case('outlier_span').pts)
    assert g['cell0'] == 4.0 and g['loops'] == 0
    g = kc.grid_sizing(kc.case('beam').pts)
    assert g['dims'][1] == g['dims'][2] == 1 and g['dims'][0] > 256
    g = kc.grid_sizing(kc.case('two_clusters').pts)
    assert g['dims'][0] > 16


def test_query_positions_groups():
    c, r = kc.case('query_positions'), kc.case_reference('query_positions')
    assert (r.d2[:40, 0] == 0).all()                      # exactly on cloud points
    mn, mx = c.pts.min(0), c.pts.max(0)
    corners = c.q[40:48]
    assert ((corners == mn) | (corners == mx)).all() and len({tuple(x) for x in corners}) == 8
    outside = ((c.q < mn) | (c.q > mx)).sum(1)
    assert (outside[54:90] == 1).all() and (outside[90:] == 3).all()    # one axis only; all three
