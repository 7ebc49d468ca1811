"""GPU parity of K3q's bodies by group size (csrc/mmidx_scan_q.h): a group of one pair runs the u16 table with one insertion per code,
a group of two the 4-byte table, a group of three the packed table with three insertions, a group of four the packed table with four;
k_q_scan_groups hands the groups out largest first; the selection's bisection starts from the lanes' minima.

Reference loop: the probe-0 iteration of computeKnnIVFADC, IVFPQ.java:414-447, as in test_gpu_passa_q.py.  Here the index is built so
that BOTH the list lengths and every query's nearest cell are chosen: centroids far apart (40 sigma per dimension), vectors and queries
0.3 sigma around them.  Each test asserts the list lengths from the exported index and the queries' cells from the index's own coarse
quantizer before it searches; then ids and distance bits must be the oracle's, the same handle with K3q off must give the same
answer, and mmidx_get_dispatch must name K3q."""
import numpy as np
import pytest

import synth
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture)

pytestmark = pytest.mark.gpu

M = 16


def _world(rng, D, C):
    mu = 40.0 * rng.standard_normal((C, D))
    res = 0.3 * rng.standard_normal((3000, D))
    ds = D // M
    pq = np.stack([synth.kmeans(res[:, s * ds:(s + 1) * ds], 256, iters=2, seed=s) for s in range(M)])
    return mu, pq


def _around(rng, mu, cells, sigma=0.3):
    cells = np.asarray(cells, np.int64)
    return mu[cells] + sigma * rng.standard_normal((len(cells), mu.shape[1]))


def _index(mi, oracle, mu, pq, base, sizes, w=3, tr=0):
    """`base` holds the lists one after the other, sizes[c] vectors of cell c; positions within a list follow the insertion order."""
    C, D = mu.shape
    n = len(base)
    ix = mi.IVFPQ(D, n, False, "", M, 256, tr, C, 512)
    ix.loadCoarseQuantizer(mu)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ref = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D, M, 256, C, w, tr=tr, perm=oracle.random_permutation(1, D) if tr == 2 else None)
    ix.indexVectors([str(i) for i in range(n)], base)
    ref.add_vectors(base)
    ix.set_option("passa_q", 1)
    off, _, _ = ix.export()
    assert np.array_equal(np.diff(off), np.asarray(sizes))  # the lists are what the test means them to be
    return ix, ref


def _check(ix, ref, Q, cells, k):
    """One call: the queries' nearest cells are `cells`, the answer is the oracle's and that of the same handle without K3q."""
    assert np.array_equal(ix.encode(Q)[0], np.asarray(cells, np.int32))
    want = ref.search_batch(Q, k)
    got = ix.search_batch(k, Q)
    assert ix.get_dispatch()["pass_a"] == "K3q"
    assert_same(got, want)
    ix.set_option("passa_q", 0)
    off = ix.search_batch(k, Q)
    assert ix.get_dispatch()["pass_a"] != "K3q"
    ix.set_option("passa_q", 1)
    assert_same(off, want)
    return got


@pytest.mark.parametrize("D", [128, 64])
def test_group_sizes(mi, oracle, D):
    """Cells 0 .. 7 receive 1, 2, 3, 4, 5, 6, 7 and 9 queries: groups of 1, 2, 3, 4, 4 + 1, 4 + 2, 4 + 3 and 4 + 4 + 1 pairs, every
    body and every class of the size order in one call, in a shuffled batch.  Cell 8's list is empty and receives two queries (a group
    that leaves at once), cell 9 has a list and no query."""
    rng = np.random.default_rng(D + 1)
    C = 10
    mu, pq = _world(rng, D, C)
    sizes = [3000] * 8 + [0, 3000]
    base = _around(rng, mu, np.repeat(np.arange(C), sizes))
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    cells = np.repeat(np.arange(9), [1, 2, 3, 4, 5, 6, 7, 9, 2])
    cells = cells[rng.permutation(len(cells))]
    Q = _around(rng, mu, cells)
    for k in (1, 100, 151):
        _check(ix, ref, Q, cells, k)
    ix.close()


@pytest.mark.parametrize("D", [128, 64])
def test_list_lengths_at_the_scan_loops_edges(mi, oracle, D):
    """The scan takes two rounds of 8 x 256 codes per trip, one single round, then up to seven steps of 256 with the last one partly
    past the end: lists of 1, 100 (fewer than K1 = 101 codes: no evidence), 255, 256, 257, 2047, 2048, 2049, 4095, 4096 and 4097 codes,
    each read by a group of one pair and, in a second call, by a group of three."""
    rng = np.random.default_rng(D + 2)
    sizes = [1, 100, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]
    C = len(sizes)
    mu, pq = _world(rng, D, C)
    base = _around(rng, mu, np.repeat(np.arange(C), sizes))
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    for per in (1, 3):
        cells = np.repeat(np.arange(C), per)[rng.permutation(C * per)]
        _check(ix, ref, _around(rng, mu, cells), cells, 100)
    ix.close()


def test_rescue_a_lane_with_more_candidates_than_slots(mi, oracle):
    """The construction of test_pass_a_integer_kernel_lane_with_more_candidates_than_slots: the 40 codes nearest to the queries sit at
    positions 7, 263, 519, ... of their list, all of them lane 7's, which keeps six: its sixth key lies within the cut, the block builds
    its table again -- the u16 table through the scalar arithmetic for one query, the packed one for three -- and the lane walks its
    codes once more."""
    D, C, k = 128, 8, 20
    rng = np.random.default_rng(607)
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
    Q = q0 + 0.002 * rng.standard_normal((3, D))
    for nq in (1, 3):
        got = _check(ix, ref, Q[:nq], [0] * nq, k)
        assert np.all(np.isin(got[0][:, :12], slots))  # the construction holds: the best sit on lane 7's positions
    ix.close()


def test_hand_back_more_candidates_than_the_block_takes(mi, oracle):
    """Every vector of list 0 two hundred times: the K1-th smallest integer sum is shared by at least 200 codes, more than the 192
    candidates a block takes per query, so the one-query body and the three-query body hand their queries to the exact kernel.  List 1
    is 3000 copies of ONE vector: every lane minimum is the same value, the bisection's bracket is a single point."""
    D, C, k = 128, 8, 100
    rng = np.random.default_rng(23)
    mu, pq = _world(rng, D, C)
    sizes = [3000, 3000] + [500] * (C - 2)
    l0 = np.repeat(_around(rng, mu, [0] * 15), 200, axis=0)[rng.permutation(3000)]
    l1 = np.repeat(_around(rng, mu, [1]), 3000, axis=0)
    base = np.concatenate([l0, l1, _around(rng, mu, np.repeat(np.arange(2, C), 500))])
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    off, _, codes = ix.export()
    assert np.unique(codes[off[0]:off[1]], axis=0, return_counts=True)[1].min() >= 200  # > MMIDX_Q_HKQ = 192 codes share every sum
    assert len(np.unique(codes[off[1]:off[2]], axis=0)) == 1
    for cells in ([0], [0, 0, 0], [1], [1, 1, 1], [0, 1]):
        _check(ix, ref, _around(rng, mu, cells), cells, k)
    ix.close()


@pytest.mark.parametrize("offset,fits", [(100.0, True), (1e5, False)])
def test_fp32_table_guard_one_query(mi, oracle, offset, fits):
    """test_pass_a_integer_kernel_fp32_table_guard's data through the one-query body: a codebook far from the origin with a small
    spread.  The block's guard, 2 u sqrt(4128 x 4000 / qr) (||r|| + pmax) <= 0.25 with u = 2^-24, is restated here from the exported
    quantizers: offset 100 passes it (the scalar table decides), offset 1e5 fails it (the exact kernel); the oracle's answers both ways."""
    D, C, w, k, n = 128, 8, 3, 30, 9000
    rng = np.random.default_rng(int(offset) + 11)
    coarse = rng.standard_normal((C, D))
    pq = offset + rng.standard_normal((M, 256, D // M))
    base = -offset + 1.5 * rng.standard_normal((n, D))  # residuals c - v = offset + noise: the codebook's neighbourhood
    ix = mi.IVFPQ(D, n, False, "", M, 256, 0, C, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ix.set_option("passa_q", 1)
    ref = oracle_ivfpq(oracle, {"coarse": coarse, "pq": pq}, D, M, 256, C, w)
    ix.indexVectors([str(i) for i in range(n)], base)
    ref.add_vectors(base)
    Q = base[rng.choice(n, 4, replace=False)] + 0.05 * rng.standard_normal((4, D))
    cells = ix.encode(Q)[0]
    pmax = np.sqrt((pq * pq).sum(2).max(1).sum())
    mean_row, mean_sq = pq.mean(1).reshape(-1), (pq * pq).sum(2).mean(1).sum()
    for i in range(4):  # one call per query: a group of one pair
        r = coarse[cells[i]] - Q[i]
        qr = (r * r - 2.0 * r * mean_row).sum() + mean_sq
        assert (2.0 * 2.0 ** -24 * np.sqrt(4128.0 * 4000.0 / qr) * (np.linalg.norm(r) + pmax) <= 0.25) == fits
        _check(ix, ref, Q[i:i + 1], cells[i:i + 1], k)
    ix.close()


def test_bisection_bracket(mi, oracle):
    """The selection starts its bisection from [smallest, largest] of the lanes' minima.  List 0 has 60 codes: at k = 100 fewer than
    K1 = 101 values in all (no bisection, everything is a candidate), at k = 50 sixty lanes with one code each (lane minima = all the
    values).  List 1 has 101 codes, one per lane: at k = 100 the K1-th smallest sum IS the largest lane minimum, the bracket's upper
    end.  List 2 has 400 codes: lanes with two codes and lanes with one.  Groups of one and of three pairs."""
    D, C = 128, 8
    rng = np.random.default_rng(31)
    mu, pq = _world(rng, D, C)
    sizes = [60, 101, 400] + [1000] * (C - 3)
    base = _around(rng, mu, np.repeat(np.arange(C), sizes))
    ix, ref = _index(mi, oracle, mu, pq, base, sizes)
    for per in (1, 3):
        cells = np.repeat(np.arange(4), per)
        Q = _around(rng, mu, cells)
        for k in (100, 50):
            _check(ix, ref, Q, cells, k)
    ix.close()


def test_permutation_one_query_groups(mi, oracle):
    """RandomPermutation: the one-query body permutes its residual like the others.  One query per cell."""
    D, C, k = 128, 8, 100
    rng = np.random.default_rng(41)
    mu, pq = _world(rng, D, C)
    sizes = [2500] * C
    base = _around(rng, mu, np.repeat(np.arange(C), sizes))
    ix, ref = _index(mi, oracle, mu, pq, base, sizes, tr=2)
    cells = rng.permutation(C)
    _check(ix, ref, _around(rng, mu, cells), cells, k)
    ix.close()
