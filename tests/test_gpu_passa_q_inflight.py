"""GPU parity of K3q's scan with a code's sixteen table reads in flight (csrc/mmidx_scan_q.h): the sums wait with counted lgkmcnt for
the reads they consume, and a round is 4 x 256 codes from three code buffers that change roles, three rounds per trip.  What can go
wrong is a sum read before its data arrived, or a wrong count where the rounds' structure changed; either shows as lost or wrong
neighbours.

Construction and reference: those of test_gpu_passa_q_groups.py (lists and nearest cells chosen, the probe-0 loop of
computeKnnIVFADC, IVFPQ.java:414-447): ids, distance bits and counts must be the oracle's, the same handle with passa_q = 0 must give
the same answer, and mmidx_get_dispatch must name K3q.

List lengths: R - 1, R, R + 1, 2R - 1, 2R, 2R + 1, 3R + 1 for the round of R = 1024 codes and for the earlier R = 2048, the lengths
around a whole trip (3 x 1024) and around a trip followed by two single rounds (5 x 1024), two trips (6 x 1024), and 1, 255, 256,
257.  Every list is read by a group of two pairs (the 4-byte table) and by a group of four (the packed table); one more call
brings groups of 1, 2, 3 and 4 pairs together, so that every body runs in one launch."""
import numpy as np
import pytest

from test_gpu_parity import mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture)
from test_gpu_passa_q_groups import M, _around, _check, _index, _world

pytestmark = pytest.mark.gpu

R_NEW, R_OLD = 4 * 256, 8 * 256
SIZES = sorted({1, 255, 256, 257}
               | {R - 1 for R in (R_NEW, R_OLD)} | {R for R in (R_NEW, R_OLD)} | {R + 1 for R in (R_NEW, R_OLD)}
               | {2 * R - 1 for R in (R_NEW, R_OLD)} | {2 * R for R in (R_NEW, R_OLD)} | {2 * R + 1 for R in (R_NEW, R_OLD)}
               | {3 * R + 1 for R in (R_NEW, R_OLD)}
               | {3 * R_NEW - 1, 3 * R_NEW, 5 * R_NEW - 1, 5 * R_NEW, 5 * R_NEW + 1, 6 * R_NEW - 1, 6 * R_NEW})


@pytest.mark.parametrize("D", [128, 64])
def test_list_lengths_at_the_rounds_edges(mi, oracle, D):
    rng = np.random.default_rng(D + 5)
    C = len(SIZES)
    mu, pq = _world(rng, D, C)
    base = _around(rng, mu, np.repeat(np.arange(C), SIZES))
    ix, ref = _index(mi, oracle, mu, pq, base, SIZES)
    for per in (2, 4):
        cells = np.repeat(np.arange(C), per)[rng.permutation(C * per)]
        Q = _around(rng, mu, cells)
        for k in (1, 100):
            _check(ix, ref, Q, cells, k)
    # groups of 1, 2, 3 and 4 pairs in one call: list c receives 1 + c % 4 queries
    per = 1 + np.arange(C) % 4
    cells = np.repeat(np.arange(C), per)[rng.permutation(int(per.sum()))]
    Q = _around(rng, mu, cells)
    for k in (1, 100):
        _check(ix, ref, Q, cells, k)
    ix.close()


def test_thread_per_candidate_instantiation(mi, oracle):
    """D = 256 (dsub 16): the instantiation whose exact sums load their own rows.  Lists of R + 1, 3R + 1 and 5R codes, groups of two
    and of four pairs."""
    D = 256
    rng = np.random.default_rng(261)
    sizes = [R_NEW + 1, 3 * R_NEW + 1, 5 * R_NEW]
    C = len(sizes)
    mu, pq = _world(rng, D, C)
    base = _around(rng, mu, np.repeat(np.arange(C), sizes))
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    for per in (2, 4):
        cells = np.repeat(np.arange(C), per)
        Q = _around(rng, mu, cells)
        for k in (1, 100):
            _check(ix, ref, Q, cells, k)
    ix.close()


def test_rescue_walk_group_of_four(mi, oracle):
    """The construction of test_rescue_a_lane_with_more_candidates_than_slots, read by a group of FOUR pairs: the 40 codes nearest to
    the queries sit at positions 7, 263, 519, ... of their list, all of them lane 7's, which keeps six; the block builds the packed
    table again and the lane walks its codes once more -- through the same lookup as the scan."""
    D, C, k = 128, 8, 20
    rng = np.random.default_rng(613)
    mu, pq = _world(rng, D, C)
    n0 = 10400
    V = _around(rng, mu, np.zeros(n0, np.int64))
    q0 = _around(rng, mu, [0])[0]
    tmp = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D, M, 256, C, 3)
    tmp.add_vectors(V)
    near = tmp.search_batch(q0[None, :], 40)[0][0]
    slots = 7 + 256 * np.arange(40)
    order = np.empty(n0, np.int64)
    order[slots] = near
    order[np.setdiff1d(np.arange(n0), slots)] = np.setdiff1d(np.arange(n0), near)
    sizes = [n0] + [300] * (C - 1)
    base = np.concatenate([V[order], _around(rng, mu, np.repeat(np.arange(1, C), 300))])
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    Q = q0 + 0.002 * rng.standard_normal((4, D))
    got = _check(ix, ref, Q, [0] * 4, k)
    assert np.all(np.isin(got[0][:, :12], slots))  # the construction holds: the best sit on lane 7's positions
    got = _check(ix, ref, Q[:2], [0] * 2, k)  # and by a group of two: the 4-byte table
    assert np.all(np.isin(got[0][:, :12], slots))
    ix.close()
