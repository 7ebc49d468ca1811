"""The head-only screen in front of the one-probe certificate (K1s = k_coarse_screen16 + k_coarse_near_cert, option "coarse_screen",
DESIGN.md section 5.1 "The screen") on the GPU.

Every case is answered three ways on one handle -- coarse_screen = 1, coarse_screen = 0 and coarse_near = 0 -- and each answer is the
CPU oracle's: ids, distance bits and counts.  `screened` (mmidx_get_dispatch: the queries of the last sub-batch the screen's
certificate served, "-" where the screen did not run) and `near_only` are asserted for every call.

Shapes: D = 128, w = 4; C = 256 (two tiles: two splits of one tile each) and C = 300 (padded to 384: padding columns in the last
tile); nq = 1, 37 and 300 (a partial wave, a partial block, two blocks of K1s and five of the certificate).  The fixture is
tests/test_gpu_coarse_near_only.py's -- centroids 6 sqrt(2 D) apart, residuals 0.3 sqrt(D) long, so every expectation holds by a
wide margin -- with the query kinds
  near    beside a populated cell: screened and certified;
  mid     midway between two cells: neither;
  dup     beside cell 17, whose twin 18 is the same centroid in the same tile, or beside cell 100, whose twin 228 lies in another
          tile and so in another split's record: a = b, neither;
  short   beside cell 0, whose list is shorter than near_min at the case's k: neither;
  huge    a query of norm 1e19: beyond the 1e37 guard, neither;
and, on an index of its own (every centroid and query shifted by one common vector, |q||c| = 2e4 with distances of about 200),
  offset  eps1 (about 310) exceeds b, the screen certifies nothing; the split (eps16 about 6) certifies all of them."""
import importlib

import numpy as np
import pytest

from test_gpu_coarse_near_only import FRONT_SEL, same_bits
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture; torch initialises first)

pytestmark = pytest.mark.gpu

D, W, M, KS = 128, 4, 16, 256
KEYS = ["coarse", "pass_a", "pre", "pass_b", "coarse_mm", "assign", "encode", "flagged", "screened", "near_only"]
NEAR, MID, DUP, SHORT, HUGE = range(5)
KIND_OF = [NEAR, NEAR, NEAR, NEAR, MID, DUP, SHORT, HUGE]  # kind of query i before the permutation: i % 8


class Fix:
    """eight populated cells; cs / rs: standard deviation of a centroid's and a residual's component; shift: added to every
    component of every centroid, vector and query; cell 0 holds `short` vectors, the others 130"""

    def __init__(self, mi, oracle, C, cs=6.0, rs=0.3, shift=0.0, short=11, tr=0, seed=0):
        rng = np.random.default_rng(7000 + C + seed)
        self.C, self.rng, self.cs, self.rs = C, rng, cs, rs
        coarse = cs * rng.standard_normal((C, D)) + shift
        self.hot = hot = np.array([0, 17, 100, 129, 200, 255, C - 2, C - 1])
        coarse[18] = coarse[17]  # an empty twin of a populated cell, in its tile
        coarse[228] = coarse[100]  # ... and one in another tile: the certificate kernel meets it when it merges the splits' records
        cell = np.repeat(hot, [short] + [130] * 7)
        base = coarse[cell] + rs * rng.standard_normal((len(cell), D))
        resid = coarse[cell] - base
        ds = D // M
        pq = np.stack([resid[rng.choice(len(resid), KS, replace=False), s * ds:(s + 1) * ds] for s in range(M)])
        base = base[rng.permutation(len(base))]
        rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if tr == 1 else None
        self.ix = mi.IVFPQ(D, len(base), False, "", M, KS, tr, C, 512, rot=rot)
        self.ix.loadCoarseQuantizer(coarse)
        self.ix.loadProductQuantizer(pq)
        self.ix.setW(W)
        self.ix.indexVectors([str(i) for i in range(len(base))], base)
        self.ref = oracle_ivfpq(oracle, {"coarse": coarse, "pq": pq}, D, M, KS, C, W, tr=tr, rot=rot)
        self.ref.add_vectors(base)
        self.coarse = coarse

    def query(self, kind, i):
        c, hot, rng = self.coarse, self.hot, self.rng
        if kind == NEAR:
            return c[hot[3 + i % 5]] + self.rs * rng.standard_normal(D)
        if kind == MID:
            return 0.5 * (c[hot[3 + i % 5]] + c[hot[3 + (i + 1) % 5]]) + self.rs / 30 * rng.standard_normal(D)
        if kind == DUP:
            return c[(17, 100)[(i >> 3) & 1]] + self.rs * rng.standard_normal(D)
        if kind == SHORT:
            return c[0] + self.rs * rng.standard_normal(D)
        return 1e19 / np.sqrt(D) * rng.standard_normal(D)

    def batch(self, n, kinds=None, seed=5):
        """n queries, kind i % 8 of KIND_OF in a fixed permutation -> (Q, kinds)"""
        kinds = np.array([KIND_OF[i % 8] for i in range(n)] if kinds is None else kinds)
        kinds = kinds[np.random.default_rng(seed).permutation(n)]
        return np.stack([self.query(k, i) for i, k in enumerate(kinds)]), kinds

    def three(self, k, Q, screened, near_only):
        """screen on, screen off, certificate off: the oracle's answer each, the same bits; -> the screened call's dispatch"""
        want = self.ref.search_batch(Q, k)
        out = []
        for opts, scr, near in (({"coarse_screen": 1, "coarse_near": -1}, str(screened), near_only),
                                ({"coarse_screen": 0, "coarse_near": -1}, "-", near_only), ({"coarse_screen": 1, "coarse_near": 0}, "-", 0)):
            for o, v in opts.items():
                self.ix.set_option(o, v)
            got = self.ix.search_batch(k, Q)
            d = self.ix.get_dispatch()
            assert list(d) == KEYS, d
            assert d["coarse"] == FRONT_SEL and d["coarse_mm"] == "groups", d
            assert d["screened"] == scr and int(d["near_only"]) == near, (opts, d, scr, near)
            assert_same(got, want)
            out.append((got, d))
        self.ix.set_option("coarse_near", -1)
        same_bits(out[0][0], out[1][0])
        same_bits(out[0][0], out[2][0])
        return out[0][1]

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module", params=[256, 300])
def fix(request, mi, oracle):
    f = Fix(mi, oracle, request.param)
    yield f
    f.close()


@pytest.mark.parametrize("n", [1, 37, 300])
def test_all_kinds_in_one_batch(fix, n):
    Q, kinds = fix.batch(n)
    near = int((kinds == NEAR).sum())
    fix.three(10, Q, near, near)


def test_each_kind_alone(fix):
    for kind, want in ((NEAR, 37), (MID, 0), (DUP, 0), (SHORT, 0), (HUGE, 0)):
        Q, _ = fix.batch(37, kinds=[kind] * 37)
        fix.three(10, Q, want, want)


def test_sub_batches_of_16(fix):
    """37 queries as 16 + 16 + 5: the answers are the whole call's, the dispatch describes the last five"""
    Q, kinds = fix.batch(37)
    fix.ix.set_option("coarse_screen", 1)
    whole = fix.ix.search_batch(10, Q)
    fix.ix.set_option("sub_batch", 16)
    try:
        last = int((kinds[32:] == NEAR).sum())
        fix.three(10, Q, last, last)
        fix.ix.set_option("coarse_screen", 1)
        same_bits(fix.ix.search_batch(10, Q), whole)
    finally:
        fix.ix.set_option("sub_batch", 0)


def test_k_at_the_edge_of_near_min(mi, oracle):
    """cell 0 holds 50 vectors and near_min = k + 2: its queries are served at k = 48 and handed on, then ranked, at k = 49"""
    f = Fix(mi, oracle, 256, short=50, seed=1)
    try:
        Q, kinds = f.batch(37, kinds=[NEAR] * 20 + [SHORT] * 17)
        f.three(48, Q, 37, 37)
        f.three(49, Q, 20, 20)
    finally:
        f.close()


def test_offset_screen_hands_on_what_the_split_certifies(mi, oracle):
    """a common offset: |q||c| = 2e4 against distances of about 200 between centroids.  eps1 = 4.02 * 2^-8 |q||c| + .. is above every
    b, eps16 = 2.9e-4 |q||c| far below (tests/test_coarse_screen_cpu.py computes both for vectors built this way): the screen serves
    no query and the split serves every `near` one"""
    f = Fix(mi, oracle, 256, cs=0.884, rs=0.0442, shift=12.4)
    try:
        assert 1.9e4 < (f.coarse[f.hot] ** 2).sum(1).max() < 2.2e4
        for n in (37, 300):
            Q, kinds = f.batch(n, kinds=[KIND_OF[i % 5] for i in range(n)])  # near x 4, mid
            f.three(10, Q, 0, int((kinds == NEAR).sum()))
    finally:
        f.close()


def test_rotation_profiling_and_k3ma_leave_the_screen_out(fix, mi, oracle):
    Q, kinds = fix.batch(37, kinds=[NEAR] * 37)
    want = fix.ref.search_batch(Q, 10)
    fix.ix.set_option("coarse_screen", 1)
    fix.ix.set_profiling(True)
    try:
        assert_same(fix.ix.search_batch(10, Q), want)
        d = fix.ix.get_dispatch()
        assert d["screened"] == "-" and int(d["near_only"]) == 0, d
    finally:
        fix.ix.set_profiling(False)
    fix.ix.set_option("passa_mfma", 1)
    try:
        assert_same(fix.ix.search_batch(100, Q), fix.ref.search_batch(Q, 100))
        d = fix.ix.get_dispatch()
        assert (d["screened"] == "-") == (d["pass_a"] == "K3ma"), d
    finally:
        fix.ix.set_option("passa_mfma", -1)
    r = Fix(mi, oracle, 256, tr=1, seed=2)
    try:
        r.ix.set_option("coarse_screen", 1)
        Qr, _ = r.batch(37, kinds=[NEAR] * 37)
        assert_same(r.ix.search_batch(10, Qr), r.ref.search_batch(Qr, 10))
        d = r.ix.get_dispatch()
        assert d["screened"] == "-" and int(d["near_only"]) == 0, d
    finally:
        r.close()


def test_auto_rests_seven_calls_after_a_call_that_handed_everything_on(mi, oracle):
    """coarse_screen = -1 on a fresh handle: a midpoint-only call is screened and hands on all 37; the next seven near-only calls
    go without the screen, the eighth is screened again; every answer is the oracle's and near_only is 37 throughout"""
    f = Fix(mi, oracle, 256, seed=3)
    try:
        Qm, _ = f.batch(37, kinds=[MID] * 37)
        Qn, _ = f.batch(37, kinds=[NEAR] * 37)
        wm, wn = f.ref.search_batch(Qm, 10), f.ref.search_batch(Qn, 10)
        assert_same(f.ix.search_batch(10, Qm), wm)
        d = f.ix.get_dispatch()
        assert d["screened"] == "0" and int(d["near_only"]) == 0, d
        seen = []
        for _ in range(8):
            assert_same(f.ix.search_batch(10, Qn), wn)
            d = f.ix.get_dispatch()
            assert int(d["near_only"]) == 37, d
            seen.append(d["screened"])
        assert seen == ["-"] * 7 + ["37"], seen
    finally:
        f.close()


def test_coarse_device_keeps_the_exact_ranking(fix, mi):
    """mmidx_coarse_device after a screened search on the same handle: the oracle's w nearest cells"""
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    Q, kinds = fix.batch(37, kinds=[KIND_OF[i % 5] for i in range(37)])
    near = int((kinds == NEAR).sum())
    fix.three(10, Q, near, near)
    exp = np.stack([fix.ref.nearest_coarse(q, W) for q in Q])
    dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")
    cells = torch.full((len(Q), W), -1, dtype=torch.int32, device="cuda")
    cd = torch.full((len(Q), W), -1.0, dtype=torch.float64, device="cuda")
    nat.check(mi.lib().mmidx_coarse_device(fix.ix._h, len(Q), dQ.data_ptr(), cells.data_ptr(), cd.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(cells.cpu().numpy(), exp)
