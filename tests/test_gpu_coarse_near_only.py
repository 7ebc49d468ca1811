"""The coarse stage's one-probe certificate on the GPU (k_coarse_front_sel, option "coarse_near").

A certified query gets its nearest cell, w - 1 filler cells and a lower bound for their distances instead of the exact far
ranking; k_pair_hist then prunes the fillers as it would have pruned the real cells, so nothing a caller can see may change.
Every case compares ids, distances as bits and counts with the CPU oracle AND with the same handle at coarse_near = 0, and reads
`near_only` (mmidx_get_dispatch: the queries of the last sub-batch the certificate served) against what the case must give.

Shapes: the smallest for which coarse= reads K1e'+K1f(front_sel) -- D = 64 and 128, C = 256 (w <= 7: Cp / 8 >= 4 (w + 1)) and 384
(w = 8), w = 2 .. 8 -- with eight populated cells of 130 vectors (k + 2 at k = 100, so that pass A publishes a threshold from one
chunk of the list) and m = 16 x 256, which K3q, K3h and K3 all take.  Centroids are 6 sqrt(2 D) apart and the residuals 0.3 sqrt(D)
long: a query beside a centroid is certified by a wide margin, a query midway between two centroids fails by a wide margin, so the
expected counts do not depend on the last bits of the approximate distances."""
import importlib

import numpy as np
import pytest

from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture; torch initialises first)

pytestmark = pytest.mark.gpu

M, KS = 16, 256
FRONT_SEL = "K1e'+K1f(front_sel)"
PASSA_DEFAULTS = {"passa_q": -1, "passa_hist": -1, "passa_mfma": -1}


def same_bits(a, b):
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(np.ascontiguousarray(a[1]).view(np.uint64), np.ascontiguousarray(b[1]).view(np.uint64))


class Case:
    """an index of eight populated cells on the GPU and in the oracle; queries beside those cells (`near`, 4 per cell) and midway
    between two of them (`mid`)"""

    def __init__(self, mi, oracle, D, C, w, tr=0, per=130, short=None, big_row=False, dup=False, copies=1, devices=None, seed=0):
        rng = np.random.default_rng(1000 * D + C + seed)
        self.D, self.C, self.w = D, C, w
        coarse = 6.0 * rng.standard_normal((C, D))
        self.hot = hot = np.array([0, 17, 100, 129, 200, 255, C - 2, C - 1])
        if dup:
            coarse[18] = coarse[17]  # an empty twin of a populated cell
        sizes = [per] * len(hot)
        if short is not None:
            sizes[0] = short
        cell = np.repeat(hot, sizes)
        base = coarse[cell] + 0.3 * rng.standard_normal((len(cell), D))
        resid = coarse[cell] - base
        ds = D // M
        pq = np.stack([resid[rng.choice(len(resid), KS, replace=False), s * ds:(s + 1) * ds] for s in range(M)])
        if big_row:
            pq[1, 3] = 1000.0  # what an empty k-means cluster leaves: never assigned, but Rmax counts it
        base = np.concatenate([base] * copies)[rng.permutation(len(base) * copies)]
        self.near = np.concatenate([coarse[c] + 0.3 * rng.standard_normal((4, D)) for c in hot])  # [32]: four per cell, cell order
        self.mid = np.stack([0.5 * (coarse[hot[i]] + coarse[hot[(i + 1) % 8]]) for i in range(8) for _ in range(4)]) + 0.01 * rng.standard_normal((32, D))
        rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if tr == 1 else None
        self.ix = mi.IVFPQ(D, len(base), False, "", M, KS, tr, C, 512, rot=rot, devices=devices)
        self.ix.loadCoarseQuantizer(coarse)
        self.ix.loadProductQuantizer(pq)
        self.ix.setW(w)
        self.ix.indexVectors([str(i) for i in range(len(base))], base)
        self.ref = oracle_ivfpq(oracle, {"coarse": coarse, "pq": pq}, D, M, KS, C, w, tr=tr, rot=rot)
        self.ref.add_vectors(base)
        self.coarse = coarse

    def both(self, k, Q, want_near, coarse=FRONT_SEL):
        """the call with the certificate on and off: both the oracle's answer, bit for bit each other's; -> (dispatch on, answer)"""
        want = self.ref.search_batch(Q, k)
        self.ix.set_option("coarse_near", -1)
        got = self.ix.search_batch(k, Q)
        d1 = self.ix.get_dispatch()
        self.ix.set_option("coarse_near", 0)
        got0 = self.ix.search_batch(k, Q)
        d0 = self.ix.get_dispatch()
        self.ix.set_option("coarse_near", -1)
        assert_same(got, want)
        assert_same(got0, want)
        same_bits(got, got0)
        assert d1["coarse"] == coarse and d0["coarse"] == coarse, (d1, d0)
        assert int(d0["near_only"]) == 0, d0
        # (pre= and pass_b= follow the pair count of the call before, by design: not compared)
        assert all(d1[f] == d0[f] for f in ("pass_a", "coarse_mm", "assign", "encode", "flagged")), (d1, d0)
        assert list(d1)[-1] == "near_only" and list(d1)[:8] == ["coarse", "pass_a", "pre", "pass_b", "coarse_mm", "assign", "encode", "flagged"]
        if want_near is not None:
            assert int(d1["near_only"]) == want_near, (d1, want_near)
        return d1, got

    def close(self):
        self.ix.close()


@pytest.mark.parametrize("D,C,w", [(64, 256, 2), (64, 256, 7), (128, 256, 3), (128, 384, 8)])
def test_separated_clusters_every_k(mi, oracle, D, C, w):
    """every query beside a centroid: all certified, at k = 1, 10 and 100 (lists of 130 >= k + 2); queries midway between two
    centroids: none; half and half: half"""
    c = Case(mi, oracle, D, C, w)
    try:
        for k in (1, 10, 100):
            c.both(k, c.near, 32)
        c.both(10, c.mid, 0)
        Q = np.concatenate([c.near[:16], c.mid[:16]])[np.random.default_rng(1).permutation(32)]
        d, _ = c.both(10, Q, 16)
        assert 0 < int(d["near_only"]) < len(Q)
        c.both(10, c.near[:1], 1)
    finally:
        c.close()


def test_nearest_list_shorter_than_k_plus_1(mi, oracle):
    """cell 0 holds 50 vectors: at k = 100 its four queries need other cells and are not certified; at k = 10 they are.  A list of
    exactly k + 1 codes is left to the exact ranking as well (the kernel asks for k + 2: a chunk that overfills pass A's buffer)"""
    c = Case(mi, oracle, 64, 256, 4, short=50)
    try:
        c.both(100, c.near, 28)
        c.both(10, c.near, 32)
        c.both(49, c.near, 28)
        c.both(48, c.near, 32)
    finally:
        c.close()


def test_rmax_inflated_by_one_far_codebook_row(mi, oracle):
    c = Case(mi, oracle, 64, 256, 4, big_row=True)
    try:
        c.both(10, c.near, 0)
    finally:
        c.close()


def test_two_identical_centroids(mi, oracle):
    """centroid 18 equals centroid 17: the four queries beside them have a = b and are not certified"""
    c = Case(mi, oracle, 128, 256, 5, dup=True)
    try:
        c.both(10, c.near, 28)
        c.both(10, c.near[4:8], 0)
    finally:
        c.close()


@pytest.mark.parametrize("tr,want", [(2, 32), (1, 0)])
def test_permutation_is_certified_rotation_is_not(mi, oracle, tr, want):
    c = Case(mi, oracle, 64, 256, 4, tr=tr)
    try:
        c.both(10, c.near, want)
    finally:
        c.close()


def test_duplicates_straddling_k_on_certified_queries(mi, oracle):
    """every vector three times: ties straddle k = 10 and k = 100, the flagged replay runs (its count is read with profiling on,
    which itself switches the certificate off) and the certified call gives the oracle's order"""
    c = Case(mi, oracle, 64, 256, 4, per=60, copies=3)
    try:
        for k in (10, 100):
            c.both(k, c.near, 32)
        c.ix.set_profiling(True)
        c.ix.search_batch(10, c.near)
        st, d = c.ix.get_stats(), c.ix.get_dispatch()
        c.ix.set_profiling(False)
        assert st["tie_fallbacks"] > 0, "the fixture did not reach the tie replay"
        assert int(d["near_only"]) == 0
    finally:
        c.close()


def test_sub_batches_certified_and_not(mi, oracle):
    """near_only describes the LAST sub-batch: 16 certified queries then 16 midpoints at sub_batch = 16 read 0, the other order
    reads 16; the unsplit call reads 16 either way"""
    c = Case(mi, oracle, 128, 256, 6)
    try:
        for order, last in (((c.near[:16], c.mid[:16]), 0), ((c.mid[:16], c.near[:16]), 16)):
            Q = np.concatenate(order)
            c.ix.set_option("sub_batch", 0)
            _, whole = c.both(10, Q, 16)
            c.ix.set_option("sub_batch", 16)
            _, split = c.both(10, Q, last)
            same_bits(split, whole)
            c.ix.set_option("sub_batch", 5)  # 5 + 5 + 5 + 1 certified among them
            _, split = c.both(10, Q, None)
            same_bits(split, whole)
        c.ix.set_option("sub_batch", 0)
    finally:
        c.close()


@pytest.mark.parametrize("opts,pass_a", [({"passa_q": 1}, "K3q"), ({"passa_q": 0, "passa_hist": 1}, "K3h"), ({"passa_q": 0, "passa_hist": 0}, "K3"),
                                         ({}, None), ({"passa_mfma": 1}, None)])
def test_pass_a_kernels(mi, oracle, opts, pass_a):
    """K3q, K3h and K3 publish the distance of a code of the nearest list: certified under each.  K3ma is not covered by the
    argument: where forcing it takes effect, nothing is certified"""
    c = Case(mi, oracle, 128, 256, 4)
    try:
        for o, v in dict(PASSA_DEFAULTS, **opts).items():
            c.ix.set_option(o, v)
        Q = np.concatenate([c.near, c.mid[:8]])
        d, _ = c.both(100, Q, None)
        if pass_a is not None:
            assert d["pass_a"] == pass_a, d
        assert int(d["near_only"]) == (0 if d["pass_a"] == "K3ma" else 32), d
    finally:
        c.close()


def test_profiling_keeps_the_exact_ranking_and_its_counters(mi, oracle):
    c = Case(mi, oracle, 64, 256, 4)
    try:
        codes = []
        for v in (-1, 0):
            c.ix.set_option("coarse_near", v)
            c.ix.set_profiling(True)
            got = c.ix.search_batch(10, c.near)
            st, d = c.ix.get_stats(), c.ix.get_dispatch()
            c.ix.set_profiling(False)
            assert_same(got, c.ref.search_batch(c.near, 10))
            assert int(d["near_only"]) == 0 and d["coarse"] == FRONT_SEL
            codes.append(st["scan_codes"])
        c.ix.set_option("coarse_near", -1)
        assert codes[0] == codes[1] and codes[0] > 0
        c.both(10, c.near, 32)  # (and with profiling off again the certificate is back)
    finally:
        c.close()


def test_coarse_device_keeps_the_exact_ranking(mi, oracle):
    """mmidx_coarse_device on a handle whose searches are certified: the oracle's w nearest cells and their exact distances, before
    and after a certified search"""
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    c = Case(mi, oracle, 128, 384, 8)
    try:
        Q = np.concatenate([c.near, c.mid[:8]])
        exp = np.stack([c.ref.nearest_coarse(q, c.w) for q in Q])
        dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")

        def cells_now():
            cells = torch.full((len(Q), c.w), -1, dtype=torch.int32, device="cuda")
            cd = torch.full((len(Q), c.w), -1.0, dtype=torch.float64, device="cuda")
            nat.check(mi.lib().mmidx_coarse_device(c.ix._h, len(Q), dQ.data_ptr(), cells.data_ptr(), cd.data_ptr(), None))
            torch.cuda.synchronize()
            return cells.cpu().numpy(), cd.cpu().numpy()

        c0, d0 = cells_now()
        assert np.array_equal(c0, exp)
        c.both(10, Q, 32)
        c1, d1 = cells_now()
        assert np.array_equal(c1, exp) and np.array_equal(d1.view(np.uint64), d0.view(np.uint64))
        diff = c.coarse[exp] - Q[:, None, :]
        assert np.allclose(d1, (diff * diff).sum(2), rtol=1e-12)
    finally:
        c.close()


def test_two_virtual_shards_equal_the_plain_handle(mi, oracle):
    c = Case(mi, oracle, 64, 256, 4)
    s = Case(mi, oracle, 64, 256, 4, devices=[0, 0])
    try:
        Q = np.concatenate([c.near, c.mid[:8]])
        for k in (10, 100):
            _, plain = c.both(k, Q, 32)
            s.ix.set_option("coarse_near", -1)
            got = s.ix.search_batch(k, Q)
            d = s.ix.get_dispatch()
            s.ix.set_option("coarse_near", 0)
            got0 = s.ix.search_batch(k, Q)
            same_bits(got, plain)
            same_bits(got0, plain)
            assert int(d["near_only"]) == 0, d  # (a shard's phases rank every probe)
    finally:
        s.close()
        c.close()
