"""The invariant behind K3q's bisection bracket (csrc/mmidx_scan_q.h, selection), restated in numpy.

Lane l of a block's 256 sees the list positions p = l (mod 256) and keeps the six smallest sums it has seen, ascending.  The selection
looks for the smallest A with at least K1 kept values <= A and starts from lo = the smallest, hi = the largest of the lanes' first
slots.  That is sound when at least K1 lanes hold a value: K1 lane minima are <= hi, and no value lies under lo."""
import numpy as np
import pytest


def _kept(a):
    """per lane: its six smallest values, ascending, 0xFFFF where it has fewer (the kernel's empty slot)"""
    n = len(a)
    pad = np.full(((n + 255) // 256) * 256, 0xFFFF, np.int64)
    pad[:n] = a
    per_lane = np.sort(pad.reshape(-1, 256).T, axis=1)  # [256][steps]
    out = np.full((256, 6), 0xFFFF, np.int64)
    out[:, :min(6, per_lane.shape[1])] = per_lane[:, :6]
    return out


@pytest.mark.parametrize("n", [152, 153, 255, 256, 257, 1000, 12207])
@pytest.mark.parametrize("K1", [2, 101, 152])
@pytest.mark.parametrize("spread", [1, 40, 65520])
def test_k1th_smallest_lies_between_the_lane_minima(n, K1, spread):
    rng = np.random.default_rng(n + K1 + spread)
    a = rng.integers(0, spread, n) + (65520 - spread) * int(rng.integers(0, 2))  # sums are at most 16 x 4095
    kept = _kept(a)
    valid = kept[kept != 0xFFFF]
    assert len(valid) >= K1  # (with fewer the kernel does not bisect; every n here is at least the largest K1)
    mins = kept[:, 0][kept[:, 0] != 0xFFFF]
    assert len(mins) >= K1  # n >= K1 codes fill min(n, 256) >= K1 lanes (K1 <= 152)
    lo, hi = mins.min(), mins.max()
    astar = np.sort(valid)[K1 - 1]
    assert lo <= astar <= hi
    assert (valid <= hi).sum() >= K1 and (valid < lo).sum() == 0
    # the bisection from the bracket ends where the one from [0, 0xFFFE] ends
    for lo_a, hi_a in ((int(lo), int(hi)), (0, 0xFFFE)):
        while lo_a < hi_a:
            mid = lo_a + ((hi_a - lo_a) >> 1)
            if (valid <= mid).sum() >= K1:
                hi_a = mid
            else:
                lo_a = mid + 1
        assert lo_a == astar
