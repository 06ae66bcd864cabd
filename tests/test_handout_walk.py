"""The CPU half of the hand-out tests (tests/handout.py): the camera walk hides nothing.  Every plane that
tests/test_gpu_handout.py leaves to the library is shown frames of the walk of which no 16 x 4 unit keeps both the colour and the
depth bits of the frame before -- from the oracle's frames alone, no GPU."""
import numpy as np
import pytest

import handout as H


def test_hidden_units_counts_whole_units_only():
    h, w = 9, 40                      # 3 x 3 units, the last of each row and the last row partial
    a = (np.arange(h * w, dtype=np.uint32).reshape(h, w), np.ones((h, w), np.float32))
    assert H.hidden_units(a, a) == 9
    b = (a[0].copy(), a[1].copy())
    b[0][8, 39] += 1                  # one pixel of the corner unit: colour
    assert H.hidden_units(a, b) == 8
    b[1][0, 0] = np.float32(2.0)      # ... and one of the first unit: depth
    assert H.hidden_units(a, b) == 7
    c = (a[0] + 1, a[1])
    assert H.hidden_units(a, c) == 0
    # depth as bits: -0.0 is not 0.0
    d = (a[0], -np.zeros((h, w), np.float32))
    assert H.hidden_units((a[0], np.zeros((h, w), np.float32)), d) == 0


@pytest.mark.parametrize("test", sorted(H.library_planes()))
def test_no_unit_of_the_walk_keeps_colour_and_depth(test):
    for level, w, h, ks in H.library_planes()[test]:
        frames = H.assert_walk_hides_nothing(level, w, h, ks)
        assert len(frames) == len(ks)


@pytest.mark.parametrize("level", sorted(H.LEVELS))
@pytest.mark.parametrize("w,h", [(32, 4), (4, 64), (56, 64), (64, 512), (2080, 36), (1000, 260)])
def test_consecutive_steps_of_the_walk_on_every_level(level, w, h):
    H.assert_walk_hides_nothing(level, w, h, range(H.FRAMES))
