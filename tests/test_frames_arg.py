"""The ``frames`` argument of the optimiser's diagnostics (render_scene ... clearance_map), on the host."""
import numpy as np
import pytest

from mhmocap.optimizer import frames_arg

T = 5


def test_none_is_every_frame():
    idx = frames_arg(None, T)
    assert idx.dtype == np.int64 and np.array_equal(idx, np.arange(T))


def test_order_and_duplicates_are_kept():
    idx = frames_arg([2, 0, 2], T)
    assert idx.dtype == np.int64 and idx.tolist() == [2, 0, 2]
    assert frames_arg(np.int32(T - 1), T).tolist() == [T - 1]          # a scalar is one frame


@pytest.mark.parametrize('frames', [[], [0.5], [-1], [T]], ids=['empty', 'float', 'negative', 'T'])
def test_refused(frames):
    with pytest.raises(ValueError, match=r'frames must be indices in \[0, %d\)' % T):
        frames_arg(frames, T)
