"""The one-probe certificate of the coarse stage (tests/coarse_near_model.py restates k_coarse_front_sel's test) against the exact
twin (tests/np_twin.py), on random and adversarial data: clusters whose separation is swept across the boundary, codebooks scaled
so that Rmax crosses it, and a codebook with one row at 1000 (what an empty k-means cluster leaves).

Wherever the certificate holds:
  * c0 is the exact nearest centroid, alone, and every other centroid lies at L or farther;
  * pair_keep's bound at L exceeds U, and no code of list c0 lies above U;
  * every code of every other cell has an ADC distance strictly above the K1-th smallest of list c0.
Conditions (1) and (3) are then dropped one at a time and a case is shown where the conclusion fails.  Condition (2), r > Rmax, is
what lets pair_keep prune at all (it prunes only on a positive gap), but it adds nothing to (3): for r <= Rmax,
(r - Rmax)^2 <= Rmax^2 <= (sqrt(d0) + Rmax)^2, so (3) fails whenever (2) does -- no case can separate them, and the test asserts
exactly that (the same certified set with and without it, and the inequality on a grid)."""
import numpy as np
import pytest

import coarse_near_model as cm
import np_twin as nt

D, M, KS, C = 16, 4, 16, 40
DSUB = D // M
K = 5
K1 = K + 1


def make_case(seed, sep, pscale, big_row=False, n_per=12):
    rng = np.random.default_rng(seed)
    coarse = sep * rng.standard_normal((C, D)) / np.sqrt(D)
    pq = pscale * rng.standard_normal((M, KS, DSUB))
    if big_row:
        pq[1, 3] = 1000.0
    lists = []
    for c in range(C):
        codes = rng.integers(0, KS, (n_per + int(rng.integers(0, 4)), M))
        codes[codes[:, 1] == 3, 1] = 4  # (the row of an empty cluster is never assigned)
        lists.append(codes)
    lists[7] = lists[7][:K1 - 1]  # a list one code short of K1
    near = rng.integers(0, C, 24)
    Q = np.concatenate([coarse[near] + 0.3 * pscale * rng.standard_normal((24, D)),
                        0.5 * (coarse[near[:8]] + coarse[(near[:8] + 1) % C]) + 0.01 * rng.standard_normal((8, D)),
                        coarse[[7, 7]] + 0.01 * rng.standard_normal((2, D))])
    return coarse, pq, lists, Q


def check_conclusions(coarse, pq, lists, q, cert, rmax):
    exact = nt.sq_dists_rows(coarse, q)
    c0 = cert["c0"]
    others = np.delete(np.arange(C), c0)
    assert int(exact.argmin()) == c0 and np.all(exact[others] > exact[c0])
    assert np.all(exact[others] >= cert["L"])
    assert cert["lb"] > cert["U"]
    gap, lb = cm.pair_keep_bound(exact[others], rmax)
    assert np.all(gap > 0.0) and np.all(lb >= cert["lb"]) and np.all(lb > cert["U"])  # k_pair_hist prunes every one of them
    d_near = np.sort(nt.adc_dists(nt.lookup_adc(pq, coarse[c0] - q), lists[c0]))
    assert len(d_near) >= K1 and d_near[-1] <= cert["U"]
    for c in others:
        d_far = nt.adc_dists(nt.lookup_adc(pq, coarse[c] - q), lists[c])
        assert np.all(d_far > d_near[K1 - 1])
        assert np.all(d_far > cert["U"])


SWEEP = [(sep, ps, False) for sep in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0) for ps in (0.25,)]
SWEEP += [(8.0, ps, False) for ps in (0.05, 0.5, 1.0, 2.0, 4.0)]
SWEEP += [(8.0, 0.25, True), (1e4, 0.25, True)]


@pytest.fixture(scope="module")
def sweep():
    """(case, per query: strict certificate, certificate without (2)) -- computed once, left unchanged"""
    out = []
    for i, (sep, ps, big) in enumerate(SWEEP):
        coarse, pq, lists, Q = make_case(100 + i, sep, ps, big)
        rmax = cm.rmax_of(pq)
        lens = np.array([len(x) for x in lists])
        certs = [(cm.certificate(coarse, q, lens, K1, rmax), cm.certificate(coarse, q, lens, K1, rmax, weaken=2)) for q in Q]
        out.append(((sep, ps, big), coarse, pq, lists, Q, rmax, certs))
    return out


def test_stand_in_distances_respect_eps16(sweep):
    for _, coarse, pq, lists, Q, rmax, certs in sweep:
        for q, (cert, _) in zip(Q, certs):
            assert np.all(np.abs(cm.approx_dists(coarse, q).astype(np.float64) - nt.sq_dists_rows(coarse, q)) <= cert["eps16"])


def test_certified_queries_need_only_their_nearest_list(sweep):
    counts = {}
    for key, coarse, pq, lists, Q, rmax, certs in sweep:
        n_ok = 0
        for q, (cert, _) in zip(Q, certs):
            if cert["ok"]:
                n_ok += 1
                check_conclusions(coarse, pq, lists, q, cert, rmax)
                assert cert["c0"] != 7  # (its list is one code short)
        counts[key] = n_ok
    print(counts)
    # the sweep crosses the boundary both ways: nothing at small separations or large codebooks, most queries at large / small ones
    assert counts[(0.5, 0.25, False)] == 0 and counts[(1.0, 0.25, False)] == 0
    assert counts[(16.0, 0.25, False)] >= 20 and counts[(64.0, 0.25, False)] >= 20
    assert counts[(8.0, 0.05, False)] >= 20 and counts[(8.0, 4.0, False)] == 0
    assert 0 < counts[(4.0, 0.25, False)] < 24  # (the 24 queries beside a centroid: some on either side of the boundary)
    # Rmax of about 1000: nothing at ordinary separations; centroids 10^4 apart are certified again, correctly
    assert counts[(8.0, 0.25, True)] == 0 and counts[(1e4, 0.25, True)] >= 20


def test_condition_2_is_implied_by_condition_3(sweep):
    for _, coarse, pq, lists, Q, rmax, certs in sweep:
        for strict, without2 in certs:
            assert strict["ok"] == without2["ok"]
    rng = np.random.default_rng(5)
    rmax = 10.0 ** rng.uniform(-3, 3, 4000)
    L = (rmax * rng.uniform(0.0, 1.0, 4000)) ** 2  # r <= Rmax
    d0 = 10.0 ** rng.uniform(-8, 3, 4000) * rng.integers(0, 2, 4000)
    gap, lb = cm.pair_keep_bound(L, rmax)
    assert np.all(gap <= 0.0) and np.all(lb <= (np.sqrt(d0) + rmax) ** 2 * (1.0 + 1e-9))


def test_without_condition_1_a_short_list_is_certified_and_the_answer_needs_far_cells(sweep):
    key, coarse, pq, lists, Q, rmax, certs = sweep[SWEEP.index((64.0, 0.25, False))]
    lens = np.array([len(x) for x in lists])
    q = Q[-1]  # beside centroid 7, whose list holds K1 - 1 codes; with K1 = that + 3 the list cannot fill the answer
    k = lens[7] + 2
    assert not cm.certificate(coarse, q, lens, k + 1, rmax)["ok"]
    weak = cm.certificate(coarse, q, lens, k + 1, rmax, weaken=1)
    assert weak["ok"] and weak["c0"] == 7
    ids, _ = nt.ivfpq_search(coarse, pq, [(1000 * c + np.arange(len(x)), x) for c, x in enumerate(lists)], q, k, 4)
    assert len(ids) == k and np.sum(ids // 1000 != 7) == 2  # two of the k nearest come from other cells


def test_without_condition_3_a_far_code_beats_the_nearest_list():
    """c0 = 0 and c1 = (4, 0, ..): the unique nearest cell by a wide margin (L > d0), and sqrt(L) > Rmax = 3 as (2) asks; but the
    codebook holds (3, 0, 0, 0) and (-3, 0, 0, 0): list 1's codes lie 1 away from c1 - q, list 0's codes 3 away from c0 - q."""
    rng = np.random.default_rng(9)
    s = 4.0
    coarse = 20.0 * rng.standard_normal((C, D))
    coarse[0] = 0.0
    coarse[1] = 0.0
    coarse[1, 0] = s
    pq = 0.01 * rng.standard_normal((M, KS, DSUB))
    pq[0, 0] = (3.0, 0, 0, 0)
    pq[0, 1] = (-3.0, 0, 0, 0)
    lists = [rng.integers(2, KS, (K1 + 2, M)) for _ in range(C)]
    lists[0][:, 0] = 1
    lists[1][:, 0] = 0
    lens = np.array([len(x) for x in lists])
    q = 0.01 * rng.standard_normal(D)
    rmax = cm.rmax_of(pq)
    strict = cm.certificate(coarse, q, lens, K1, rmax)
    weak = cm.certificate(coarse, q, lens, K1, rmax, weaken=3)
    assert not strict["ok"] and weak["ok"] and weak["c0"] == 0 and weak["L"] > weak["d0"]
    d_near = np.sort(nt.adc_dists(nt.lookup_adc(pq, coarse[0] - q), lists[0]))
    d_far = nt.adc_dists(nt.lookup_adc(pq, coarse[1] - q), lists[1])
    assert d_far.min() < d_near[0]  # every answer of this query comes from the far cell


def test_ties_nan_and_negative_values_certify_nothing():
    coarse, pq, lists, Q, = make_case(3, 64.0, 0.25)
    rmax = cm.rmax_of(pq)
    lens = np.array([len(x) for x in lists])
    q = coarse[3] + 0.01
    assert cm.certificate(coarse, q, lens, K1, rmax)["ok"]
    dup = coarse.copy()
    dup[3 + 16] = dup[3]  # the same group of 8 (centroids 3, 19, 35, ..): the runner-up equals the minimum
    assert not cm.certificate(dup, q, lens, K1, rmax)["ok"]
    dup = coarse.copy()
    dup[4] = dup[3]  # another group
    assert not cm.certificate(dup, q, lens, K1, rmax)["ok"]
    dt = cm.approx_dists(coarse, q)
    for bad in (np.float32(np.nan), np.float32(-1.0), np.float32(-np.inf)):
        d2 = dt.copy()
        d2[19] = bad  # the runner-up of c0's group
        assert not cm.certificate(coarse, q, lens, K1, rmax, dt=d2)["ok"]
    assert not cm.certificate(coarse, q, lens, K1, float("nan"))["ok"] and not cm.certificate(coarse, q, lens, K1, float("inf"))["ok"]
