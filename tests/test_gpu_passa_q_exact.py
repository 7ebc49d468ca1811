"""GPU parity of K3q's exact-sum phase (csrc/mmidx_scan_q.h, between the hand-back block and the publish loops): the candidates'
fp64 codebook rows are loaded several lanes to a row and handed to the candidate's lane through a per-wave LDS tile, 256 candidates
per pass, sub-quantizer by sub-quantizer.

Reference: the distance of IVFPQ.java:531-534 inside :435-438 (t ascending from 0.0, then s ascending) -- ids and distance BITS must
equal the oracle's.  The shapes move a block's candidate count over every boundary of that loop: fewer candidates than lanes per row
(k = 1: two candidates per query; lists of 3 codes), partial waves, one / two / three passes of 256 (k = 151 with four queries: about
700 candidates), lists with no evidence whose candidates are the whole list (3, 20, 49 ... 52 codes), candidate lists around
the 192 a block takes per query (ties), and the three sub-quantizer widths (DSUB = 4, 8: two and four lanes per row;
DSUB = 16 keeps a thread per candidate).  The instance is forced and mmidx_get_dispatch proves it ran."""
import numpy as np
import pytest

import synth
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture)
from test_gpu_passa_q import _build, _problem

pytestmark = pytest.mark.gpu

M = 16


def _queries(rng, mu, base, nq):
    """Midpoints between vectors, independent Gaussians, self-perturbed vectors, two centroids (as test_passa_q_forced)."""
    D = base.shape[1]
    nself = nq - 24 - 8 - 2
    return np.concatenate([0.5 * (base[:24] + base[100:124]), rng.standard_normal((8, D)), base[200:200 + nself] + 0.01 * rng.standard_normal((nself, D)), mu[:2]])


def _check(ix, ref, Q, k, slices=()):
    want = ref.search_batch(Q, k)
    got = ix.search_batch(k, Q)
    assert ix.get_dispatch()["pass_a"] == "K3q"
    assert_same(got, want)
    for sl in slices:
        assert_same(ix.search_batch(k, Q[sl]), tuple(a[sl] for a in want))
        assert ix.get_dispatch()["pass_a"] == "K3q"


@pytest.fixture(scope="module")
def sweep_index(mi, oracle):
    """One index per width, built on first use: C = 4 lists of ~6000 codes, every list probed (w = 4), 64 queries = 16 per list."""
    made = {}

    def get(D):
        if D not in made:
            rng = np.random.default_rng(7 * D)
            mu, base, pq = _problem(rng, D, M, 4, 24000)
            ix, ref = _build(mi, oracle, mu, base, pq, D, M, 4, 4)
            made[D] = (ix, ref, _queries(rng, mu, base, 64))
        return made[D]

    yield get
    for ix, _, _ in made.values():
        ix.close()


@pytest.mark.parametrize("k", [1, 2, 13, 50, 100, 151])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_exact_sums_k_sweep(sweep_index, D, k):
    """k + 1 evidence codes per query: a block of four queries goes from 2 x 4 candidates to about 700 (one, two and three passes of
    256); the slices are groups of one, two and three queries (from 2 candidates in the block: fewer than the lanes of one row)."""
    ix, ref, Q = sweep_index(D)
    _check(ix, ref, Q, k, (slice(0, 1), slice(5, 7), slice(30, 33)))


@pytest.mark.parametrize("k", [50, 100])
def test_exact_sums_ties(mi, oracle, k):
    """Every vector three times: equal sums inside the candidate range and candidate lists three times as long as the same data gives
    without copies (k = 100: around the 192 a block takes per query).  Whether a query stays in the block or goes to the exact kernel
    is not observable from the host, so nothing here depends on it: test_passa_q_more_candidates_than_the_block_takes forces that path."""
    D = 128
    rng = np.random.default_rng(31 + k)
    mu, base, pq = _problem(rng, D, M, 5, 24000, dup=3)
    ix, ref = _build(mi, oracle, mu, base, pq, D, M, 5, 5)
    _check(ix, ref, _queries(rng, mu, base, 120), k)
    ix.close()


def test_exact_sums_short_lists(mi, oracle):
    """The uneven lists of test_passa_q_short_and_empty_lists, k = 50: the lists of 3, 20, 49, 50, 51 and 52 codes have no (or just
    the) k + 1 evidence codes, so a query's candidates are the whole list -- counts below the lanes of a row and no multiple of them."""
    D, C, w, k = 128, 40, 6, 50
    rng = np.random.default_rng(5)
    mu = 3.0 * rng.standard_normal((C, D))
    sizes = np.array([0, 0, 3, 20, 49, 50, 51, 52, 100, 400] * 4)
    sizes[-8:] = 3000
    lab = np.repeat(np.arange(C), sizes)
    base = mu[lab] + 0.4 * rng.standard_normal((len(lab), D))
    perm = rng.permutation(len(lab))
    base, lab = base[perm], lab[perm]
    ds = D // M
    pq = np.stack([synth.kmeans((mu[lab[:3000]] - base[:3000])[:, s * ds:(s + 1) * ds], 256, iters=2, seed=s) for s in range(M)])
    ix, ref = _build(mi, oracle, mu, base, pq, D, M, C, w)
    Q = np.concatenate([mu + 0.05 * rng.standard_normal((C, D)), mu + 0.05 * rng.standard_normal((C, D)), base[:150] + 0.01 * rng.standard_normal((150, D))])
    _check(ix, ref, Q, k, (slice(2, 3), slice(3, 5)))
    ix.close()


@pytest.mark.parametrize("tr", [1, 2])
def test_exact_sums_transforms(mi, oracle, tr):
    """RandomRotation (an orthogonal matrix: the block rotates its residuals itself) and RandomPermutation: the residuals the sums
    read are the transformed ones.  D = 128, k = 100, groups of four."""
    D, k = 128, 100
    rng = np.random.default_rng(50 + tr)
    mu, base, pq = _problem(rng, D, M, 4, 24000)
    rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if tr == 1 else None
    ix, ref = _build(mi, oracle, mu, base, pq, D, M, 4, 4, tr, rot)
    _check(ix, ref, _queries(rng, mu, base, 64), k)
    ix.close()
