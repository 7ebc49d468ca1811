"""The head-only screen of the one-probe certificate (tests/coarse_screen_model.py restates K1s and its certificate kernel)
against the exact twin (tests/np_twin.py).

  * eps1 term for term, and |d~ - d| <= eps1 at D = 128 for scales from 1e-18 to 1e18 and for an adversarial family -- every
    component 128.498 x 2^e, just under a bf16 rounding midpoint, all of one sign, so that the 256 element errors of a pair add
    up.  On that family the observed |d~ - d| is 0.55 of eps1 with the exponents e drawn from -3 .. 3 (the bound takes every centroid
    for the longest one) and 0.98 with one exponent throughout; on N(0, 1) data about 0.09 (all printed by the tests): the bound is
    not padded.  What is asserted of the slack is that eps1 stays within 1 % of its first term at ordinary magnitudes.
  * conclusions 1 to 4 of DESIGN.md 5.1 for every query the screen certifies, on tests/test_coarse_near_cpu.py's sweep across the
    boundary, with the records merged over 1, 2 and 3 splits;
  * the two mutations of the model: eps1 without the cross term breaks the bound, b without the other splits' a certifies a query
    whose nearest centroid is not alone;
  * the offset vectors of tests/test_gpu_coarse_screen.py: eps1 above every b, eps16 far below;
  * the auto rule as a pure function."""
import numpy as np
import pytest

import coarse_near_model as cm
import coarse_screen_model as sm
import np_twin as nt
from test_coarse_near_cpu import K1, SWEEP, check_conclusions, make_case

D = 128


def test_eps1_term_for_term():
    xnorm, cmax = 3.0, 5.0
    got = sm.eps_head16(128, xnorm, 9.0, cmax, 25.0)
    want = (2 * 2.01 / 256 * 15.0 + 2 * 1.01 * 144 * 2.0 ** -22 * 15.0 + 1e-12 * 34.0 + (2.0 ** -21 + 2.0 ** -20) * 64.0 +
            (4 * 128 + 16 + 6 * np.sqrt(128.0) * 8.0) * 2.0 ** -126) * (1 + 1e-9)
    assert got == pytest.approx(want, rel=1e-15)
    # at ordinary magnitudes the head's rounding is all of it, and it is 54 times the split's bound
    assert got < 1.01 * (2 * 2.01 / 256 * 15.0)
    assert 40 < got / cm.eps_split16(128, xnorm, 9.0, cmax, 25.0) < 70


def observed_over_bound(coarse, Q, cross=True):
    worst = 0.0
    for q in Q:
        qnorm, qn, cnorm_max, cn_max = sm.norms_of(coarse, q)
        assert cm.norms_usable(cnorm_max + qnorm)
        eps1 = sm.eps_head16(D, qnorm, qn, cnorm_max, cn_max, cross=cross)
        err = np.abs(sm.head_dists(coarse, q).astype(np.float64) - nt.sq_dists_rows(coarse, q))
        worst = max(worst, float((err / eps1).max()))
    return worst


@pytest.mark.parametrize("scale", [1e-18, 1e-9, 1.0, 1e9, 1e18])
def test_head_only_distances_respect_eps1(scale):
    rng = np.random.default_rng(11)
    coarse = scale / np.sqrt(D) * rng.standard_normal((64, D))
    Q = np.concatenate([coarse[:8] + 0.15 * scale / np.sqrt(D) * rng.standard_normal((8, D)), scale / np.sqrt(D) * rng.standard_normal((8, D))])
    r = observed_over_bound(coarse, Q)
    print("scale", scale, "observed / eps1", r)
    assert 0.0 < r <= 1.0


def adversarial(rng, n):
    e = rng.integers(-3, 4, (n, D))
    return 128.498 * 2.0 ** e


def test_adversarial_family_respects_eps1_and_needs_the_cross_term():
    rng = np.random.default_rng(12)
    coarse, Q = adversarial(rng, 64), adversarial(rng, 16)
    r = observed_over_bound(coarse, Q)
    print("adversarial: observed / eps1", r)
    assert 0.0 < r <= 1.0
    assert observed_over_bound(coarse, Q, cross=False) > 1.0  # (mutation: eps1 without the cross term is no bound)
    same_e = 128.498 * np.ones((1, D))
    print("all components alike: observed / eps1", observed_over_bound(same_e, same_e))


@pytest.fixture(scope="module")
def sweep():
    out = []
    for i, (sep, ps, big) in enumerate(SWEEP):
        coarse, pq, lists, Q = make_case(100 + i, sep, ps, big)
        out.append(((sep, ps, big), coarse, pq, lists, Q, cm.rmax_of(pq), np.array([len(x) for x in lists])))
    return out


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_screen_certified_queries_need_only_their_nearest_list(sweep, splits):
    counts, split_only = {}, 0
    for key, coarse, pq, lists, Q, rmax, lens in sweep:
        n_ok = 0
        for q in Q:
            cert = sm.certificate(coarse, q, lens, K1, rmax, splits=splits)
            if cert["ok"]:
                n_ok += 1
                check_conclusions(coarse, pq, lists, q, cert, rmax)
            elif cm.certificate(coarse, q, lens, K1, rmax)["ok"]:
                split_only += 1
        counts[key] = n_ok
    print(counts, "certified by the split alone:", split_only)
    assert counts[(0.5, 0.25, False)] == 0 and counts[(1.0, 0.25, False)] == 0
    assert counts[(16.0, 0.25, False)] >= 20 and counts[(64.0, 0.25, False)] >= 20
    assert counts[(8.0, 4.0, False)] == 0 and counts[(1e4, 0.25, True)] >= 20
    assert split_only > 0  # (the boundary region where the screen hands on what the split then serves)


def test_b_without_the_other_splits_best_certifies_a_tie():
    """two equal nearest centroids in different splits: b must be a.  Mutation: with the other split's best left out of b the
    query is certified although its nearest centroid is not alone"""
    coarse, pq, lists, Q = make_case(3, 64.0, 0.25)
    rmax, lens = cm.rmax_of(pq), np.array([len(x) for x in lists])
    dup = coarse.copy()
    dup[30] = dup[3]
    q = dup[3] + 0.01
    assert sm.certificate(coarse, q, lens, K1, rmax, splits=2)["ok"]
    for splits in (1, 2, 3):
        c = sm.certificate(dup, q, lens, K1, rmax, splits=splits)
        assert not c["ok"] and c["a"] == c["b"]
    assert sm.certificate(dup, q, lens, K1, rmax, splits=2, other_a=False)["ok"]


def test_offset_vectors_eps1_above_b_eps16_far_below():
    """the `offset` index of tests/test_gpu_coarse_screen.py: component deviation 0.884, residuals 0.0442, every component + 12.4"""
    rng = np.random.default_rng(13)
    coarse = 0.884 * rng.standard_normal((256, D)) + 12.4
    for c in (0, 100, 255):
        q = coarse[c] + 0.0442 * rng.standard_normal(D)
        qnorm, qn, cnorm_max, cn_max = sm.norms_of(coarse, q)
        assert 1.8e4 < qnorm * cnorm_max < 2.3e4
        eps1, eps16 = sm.eps_head16(D, qnorm, qn, cnorm_max, cn_max), cm.eps_split16(D, qnorm, qn, cnorm_max, cn_max)
        b = np.sort(nt.sq_dists_rows(coarse, q))[1]
        print("b", b, "eps1", eps1, "eps16", eps16)
        assert 100 < b < eps1 - 50 and eps16 < b / 10
        assert not sm.certificate(coarse, q, np.full(256, 100), 12, 0.6)["ok"]
        assert cm.certificate(coarse, q, np.full(256, 100), 12, 0.6)["ok"]


def test_auto_rule():
    n = 100
    assert sm.run_auto([0] * 12, n) == [True] * 12
    assert sm.run_auto([25] * 4, n) == [True] * 4  # a quarter exactly: stays
    # a call that hands on more than a quarter: the next seven go without, the eighth probes again
    assert sm.run_auto([100] + [0] * 9, n) == [True] + [False] * 7 + [True, True]
    assert sm.run_auto([26] * 17, n) == ([True] + [False] * 7) * 2 + [True]
    # the word is judged once: a probe that comes back clean stays on
    assert sm.run_auto([100] + [0] * 7 + [0, 100, 0], n) == [True] + [False] * 7 + [True, True, False]
    # the batch size the word is compared with is the screened call's
    s = sm.ScreenAuto()
    assert s.step(0, 1000) and not s.step(300, 10) and s.skip == 6
    s = sm.ScreenAuto()
    assert s.step(0, 1000) and s.step(250, 10)
