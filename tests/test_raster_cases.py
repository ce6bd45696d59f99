"""The crowd cases of tests/test_raster_gpu.py (9, 17 and 32 people per frame) contain what they are built for, from the oracle
alone: its LBS for the vertices, its render for z-buffer and silhouette.  No GPU."""
import pytest

import raster_cases as rc
from oracle import raster_oracle as ro


@pytest.mark.parametrize('name', sorted(rc.CROWDS))
def test_crowd_layout_meets_its_conditions(smpl_struct, smpl_regs, name):
    kw = rc.CROWDS[name]
    T, N, W, H = kw['T'], kw['N'], kw['W'], kw['H']
    inp = rc.inputs(smpl_struct, smpl_regs, **kw)
    zbuf, alpha = ro.render(rc.oracle_verts(inp), inp['faces'], inp['K'], (W, H))
    print(name, rc.crowd_conditions(inp['seg'], inp['pT'], inp['pose2d'], zbuf.view(T, N, H, W).numpy(), alpha.view(T, N, H, W).numpy()))


def test_cases_without_a_layout_are_drawn_as_before(smpl_struct, smpl_regs):
    """the random scenes keep their empty mask, their body without a 2D pose and their numbers"""
    inp = rc.inputs(smpl_struct, smpl_regs, T=3, N=2, W=60, H=34, seed=5)
    assert not inp['seg'][0, 0].any() and inp['seg'][1, 0].any() and (inp['pose2d'][1, 1, :, 2] < 0.5).all()
    sp, pT, rng = rc._scene(3, 2, 60, 34, 5, 3.0, 6.0)
    assert (pT == inp['pT']).all() and (rng.uniform(0.5, 1.5, 3).astype('float32') == inp['zmin']).all()
