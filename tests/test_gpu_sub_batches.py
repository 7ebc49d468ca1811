"""GPU parity of search calls that `search_common` serves in several sub-batches, on every entry point that reaches it.

A call of more than `pl.qb` queries (make_plan, csrc/mmidx_api.hip; tests/plan_model.py restates it) runs as a loop of sub-batches.
From the second one on every pointer of the caller carries an offset of its own -- queries, probe cells, ids, distances, counts, the
partial lists at q0 (k + 1), the SDC term tables -- every gate of the step (search_batch_device: pass_a_rung, stage_coarse, k3s_decide) sees the sub-batch's size, and no host
synchronisation separates two sub-batches, so the pinned hint words a stage steers by may describe the stage two back.  The caps that
decide `qb` are memory caps (gibibytes): the option "sub_batch" lowers `qb` so that calls of a few dozen queries are split, and three
cases at the end reach the caps themselves with the option at 0.

Every comparison is ids, distances as bits and counts against the CPU oracle (assert_same), and the split call is compared with the
same call at sub_batch = 0 on the same handle, bit for bit, on every query of the call (3g(iii) consults the oracle for 512 of its
16418 queries and says why).  That a call WAS split is read from the library, never assumed from the option: with profiling on,
`passa_launches` counts one pass A per sub-batch, and mmidx_get_dispatch describes the last sub-batch."""
import importlib

import numpy as np
import pytest

import decode_twin as dt
import plan_model as pm
import refine_twin as rt
import sdc_cases as sc
import synth
from test_gpu_call_sequence import DEFAULTS, KS, NC, STATES, D, M, W, classify, data  # noqa: F401  (data: the module fixture)
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture; torch initialises first)

pytestmark = pytest.mark.gpu

NONEMPTY = NC - 1  # the sixth cell of the `data` fixture stays empty here
ONE_LAUNCH = "K3f(one looping launch"


def same_bits(a, b):
    """two answers of the library (ids, distances, counts): equal bit for bit"""
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(np.ascontiguousarray(a[1]).view(np.uint64), np.ascontiguousarray(b[1]).view(np.uint64))


def parts(nq, sub):
    return [nb for _, nb in pm.sub_batches(nq, min(nq, sub) if sub > 0 else nq)]


def whole_and_split(ix, sub, run):
    """run() at sub_batch = 0 and at `sub`, profiling on: (answer, stats, dispatch) of each"""
    out = []
    for s in (0, sub):
        ix.set_option("sub_batch", s)
        ix.set_profiling(True)
        got = run()
        out.append((got, ix.get_stats(), ix.get_dispatch()))
    ix.set_option("sub_batch", 0)
    ix.set_profiling(False)
    return out


def device_outputs(B, k, guard=0):
    """the output tensors of a device call of B queries, `guard` rows in front and behind, filled with -7 / NaN / -7 on torch's
    current stream: the caller synchronises before a launch on another stream reads or writes them"""
    import torch

    return (torch.full((B + 2 * guard, k), -7, dtype=torch.int32, device="cuda"), torch.full((B + 2 * guard, k), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((B + 2 * guard,), -7, dtype=torch.int32, device="cuda"))


def device_launch(mi, ix, k, dQ, out, stream, guard=0):
    """mmidx_search_device on `stream` into `out` (device_outputs), behind its guard rows: enqueues, waits for nothing"""
    nat = importlib.import_module("multimedia-indexing_amd._native")
    iid, dd, cc = out
    nat.check(mi.lib().mmidx_search_device(ix._h, k, dQ.shape[0], dQ.data_ptr(), iid[guard:].data_ptr(), dd[guard:].data_ptr(), cc[guard:].data_ptr(),
                                           stream.cuda_stream if stream is not None else None))


def device_search(mi, ix, k, dQ, stream):
    """one mmidx_search_device on `stream` into fresh sentinel-filled tensors: waits for the fills (torch's current stream) before
    the launch and for nothing after it.  -> the three tensors"""
    import torch

    out = device_outputs(dQ.shape[0], k)
    torch.cuda.synchronize()
    device_launch(mi, ix, k, dQ, out, stream)
    return out


def host(t3, guard=0):
    iid, dd, cc = (t.cpu().numpy() for t in t3)
    n = len(cc) - guard
    return iid[guard:n], dd[guard:n], cc[guard:n]


class Seq:
    """the `data` fixture's index (D = 128, 16 x 256, five cells of 4500 codes and an empty one) on the GPU and in the oracle"""

    def __init__(self, mi, oracle, data, devices=None):
        n0 = len(data["base"])
        self.data = data
        self.ix = mi.IVFPQ(D, n0, False, "", M, KS, 0, NC, 512, devices=devices)
        self.ix.loadCoarseQuantizer(data["mu"])
        self.ix.loadProductQuantizer(data["pq"])
        self.ix.setW(W)
        self.ix.indexVectors([str(i) for i in range(n0)], data["base"])
        self.ref = oracle_ivfpq(oracle, {"coarse": data["mu"], "pq": data["pq"]}, D, M, KS, NC, W)
        self.ref.add_vectors(data["base"])
        self._want = {}

    def want(self, key, Q, k, w):
        """the oracle's answer, computed once per (key, k, w) and left unchanged"""
        if (key, k, w) not in self._want:
            self.ref.set_w(w)
            res = self.ref.search_batch(Q, k, nthreads=8)
            for a in res:
                a.setflags(write=False)
            self._want[(key, k, w)] = res
        return self._want[(key, k, w)]

    def options(self, opts, w):
        for o, v in dict(DEFAULTS, **opts).items():
            self.ix.set_option(o, v)
        self.ix.setW(w)


@pytest.fixture(scope="module")
def seq(mi, oracle, data):
    s = Seq(mi, oracle, data)
    yield s
    s.ix.close()


# ---- 3a -------------------------------------------------------------------------------------------------------------------------
SIZES_A = (17, 8, 1, 39, 40, 41)  # of 40 queries: 17 + 17 + 6, 5 x 8, 40 x 1, 39 + 1, and unsplit at 40 and 41
CASES_A = [(name, s) for name in ("q_gate", "k3h", "k3", "w1", "empty_b") for s in SIZES_A]
CASES_A += [("k3ma", s) for s in (24, 17, 1, 63, 64, 65)]  # of 64 queries: 24 + 24 + 16, 17 + 17 + 17 + 13, 64 x 1, 63 + 1, unsplit


@pytest.mark.parametrize("name,sub", CASES_A, ids=[f"{n}-{s}" for n, s in CASES_A])
def test_pass_a_families(seq, name, sub):
    """3a.  The states of tests/test_gpu_call_sequence.py, split: K3q at its gate, K3h, K3, the single pass and the empty pass B, each
    with its 40 queries as 17 + 17 + 6, 5 x 8, 40 x 1, 39 + 1, and unsplit at 40 and 41; K3ma (forced, so no gate of its own) with
    its 64 queries as 24 + 24 + 16 and at five more sizes.  After the split call the dispatch describes the last sub-batch: six
    queries -- or one -- over five non-empty lists are below K3q's gate (4 nq >= 5 lists), so it says K3h where the unsplit call
    says K3q."""
    opts, k, w, qset, nq = STATES[name]
    Q = seq.data["Q"][qset][:nq]
    want = seq.want((qset, nq), Q, k, w)
    seq.options(opts, w)
    (got0, st0, d0), (got1, st1, d1) = whole_and_split(seq.ix, sub, lambda: seq.ix.search_batch(k, Q))
    seq.options({}, W)
    assert classify(d0, st0, nq, NONEMPTY) == name, (d0, st0["passb_items_last"])
    assert st0["passa_launches"] == 1
    assert_same(got1, want)
    same_bits(got1, got0)
    p = parts(nq, sub)
    assert st1["passa_launches"] == len(p), (p, st1["passa_launches"])
    if name in ("q_gate", "empty_b"):
        assert d0["pass_a"] == "K3q"
        assert d1["pass_a"] == ("K3q" if 4 * p[-1] >= 5 * NONEMPTY else "K3h"), (p, d1)
    else:
        assert d1["pass_a"] == d0["pass_a"], (d0, d1)
    if name == "empty_b":
        assert st1["passb_items_last"] == 0


# ---- 3b -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "device"])
def test_stale_hints_inside_one_call(mi, seq, entry):
    """3b.  Blocks of 16 queries: self, mid, self, mid, at sub_batch = 16 and k = 10, for which `self` keeps no pair for pass B and
    `mid` keeps some -- at most 32, so every count the pinned hint can hold says "at most 64 pairs".  The call is made three times in
    a row: from the third sub-batch of the first call on `hint_calls > 1` and `hint_prev_nq == nq` hold, and pass B goes through
    K3f's one looping launch on a count that describes another block's queries (one or two stages back: nothing waits for the
    device between two sub-batches, and on the device entry nothing waits between the three calls either).  Every call gives the
    oracle's answers; the last sub-batch (mid) reports the one-launch form, and the statistics count twelve sub-batches."""
    import torch

    k = 10
    Qs, Qm = seq.data["Q"]["self"], seq.data["Q"]["mid"]
    Q = np.concatenate([Qs[:16], Qm[:16], Qs[16:32], Qm[16:32]])
    want = seq.want("self/mid blocks", Q, k, W)
    assert np.all(want[2] == k)
    ix = seq.ix
    seq.options({}, W)
    ix.set_profiling(False)
    ix.set_option("sub_batch", 0)
    whole = ix.search_batch(k, Q)
    assert_same(whole, want)
    ix.set_option("sub_batch", 16)
    ix.set_profiling(True)  # (event records in the stream, no wait: the three calls below stay back to back)
    if entry == "host":
        res = [ix.search_batch(k, Q) for _ in range(3)]
    else:
        s1 = torch.cuda.Stream()
        dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")
        bufs = []
        for _ in range(3):  # (the output tensors of all three calls exist before the first launch: no fill, no wait in between)
            bufs.append((torch.full((64, k), -7, dtype=torch.int32, device="cuda"), torch.full((64, k), float("nan"), dtype=torch.float64, device="cuda"),
                         torch.full((64,), -7, dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()
        nat = importlib.import_module("multimedia-indexing_amd._native")
        for iid, dd, cc in bufs:
            nat.check(mi.lib().mmidx_search_device(ix._h, k, 64, dQ.data_ptr(), iid.data_ptr(), dd.data_ptr(), cc.data_ptr(), s1.cuda_stream))
        s1.synchronize()
        res = [host(b) for b in bufs]
    d, st = ix.get_dispatch(), ix.get_stats()
    ix.set_option("sub_batch", 0)
    ix.set_profiling(False)
    for r in res:
        assert_same(r, want)
        same_bits(r, whole)
    assert st["passa_launches"] == 12, st["passa_launches"]  # (three calls of four sub-batches)
    assert d["pass_b"].startswith(ONE_LAUNCH), d


# ---- 3c -------------------------------------------------------------------------------------------------------------------------
def _mfma_row(oracle, D_, m, C, n, w, k, tr, dup):
    """the index and the 74 queries test_mfma_pass_b builds for this row"""
    rng = np.random.default_rng(D_ + m + k)
    mu = 0.5 * rng.standard_normal((C, D_))
    base = mu[rng.integers(0, C, n // dup)] + rng.standard_normal((n // dup, D_))
    base = np.concatenate([base] * dup)[rng.permutation((n // dup) * dup)]
    ds = D_ // m
    pq = np.stack([synth.kmeans((mu[rng.integers(0, C, 3000)] - base[:3000])[:, s * ds:(s + 1) * ds], 256, iters=2, seed=s) for s in range(m)])
    Q = np.concatenate([0.5 * (base[:24] + base[100:124]), rng.standard_normal((8, D_)), base[:40] + 0.01 * rng.standard_normal((40, D_)), mu[:2]])
    return mu, pq, base, Q


def _smin_row(oracle, D_, m, C, n, w, k, tr, sep):
    """the index and the 68 queries test_smin_prefilter_forced builds for this row"""
    rng = np.random.default_rng(D_ + m + C)
    mu = sep * rng.standard_normal((C, D_))
    base = mu[rng.integers(0, C, n)] + 0.5 * rng.standard_normal((n, D_))
    pq = np.stack([synth.kmeans((mu[rng.integers(0, C, 2000)] - base[:2000])[:, s * (D_ // m):(s + 1) * (D_ // m)], 256, iters=1, seed=s)
                   for s in range(m)])
    Q = np.concatenate([base[:48] + 0.01 * rng.standard_normal((48, D_)), 0.5 * (base[100:116] + base[200:216]), mu[:4]])
    return mu, pq, base, Q


ROWS_C = {
    "K3m": (_mfma_row, (128, 16, 6, 30000, 6, 100, 0, 1), "K3m"),
    "K3mk": (_mfma_row, (256, 16, 5, 12000, 5, 50, 0, 1), "K3mk"),
    "ties": (_mfma_row, (128, 16, 5, 24000, 5, 50, 2, 3), "K3m"),
    "K3s": (_smin_row, (128, 16, 24, 30000, 24, 100, 0, 0.8), "K3m"),
}


@pytest.mark.parametrize("row", list(ROWS_C))
def test_pass_b_families_and_ties(mi, oracle, row):
    """3c.  The first rows of test_mfma_pass_b (K3m; K3mk; every vector three times under RandomPermutation, so that straddling ties
    reach the replay) and of test_smin_prefilter_forced, their own queries as 25 + 25 + 24 (25 + 25 + 18 for the K3s row, which
    builds 68), with pass B through K3m / K3mk, K3g (no_mfma) and K3f (no_mfma + no_grp: K3m stands in front of both).  The K3s row
    runs the pre-filter forced (1) and hint-driven (-1) in front of K3m and in front of K3g; it cannot stand in front of K3f, and the
    row's K3f run asserts that the forced option is then without effect.  The last sub-batch has another size than the one before
    it, so `passb_small` cannot take it and the reported pass B is the family itself."""
    build, (D_, m, C, n, w, k, tr, last), family = ROWS_C[row]
    mu, pq, base, Q = build(oracle, D_, m, C, n, w, k, tr, last)
    n = len(base)
    perm = oracle.random_permutation(1, D_) if tr == 2 else None
    ref = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D_, m, 256, C, w, tr=tr, perm=perm)
    sub = 25
    p = parts(len(Q), sub)
    assert len(p) == 3 and p[-1] != p[-2]
    ix = mi.IVFPQ(D_, n, False, "", m, 256, tr, C, 512)
    ix.loadCoarseQuantizer(mu)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ix.indexVectors([str(i) for i in range(n)], base)
    ref.load_lists(*ix.export())  # (the oracle takes the index's own records: the search is tested, not the encoder)
    if row == "ties":
        # some query of the second and some of the third sub-batch has its k-th and (k + 1)-th distances tie: reordered here, on
        # the CPU, until that holds (every vector is there three times and k = 3 x 16 + 2: nearly every query ties)
        w1 = ref.search_batch(Q, k + 1, nthreads=8)
        tie = (w1[2] > k) & (w1[1][:, k - 1] == w1[1][:, k])
        order = np.concatenate([np.nonzero(~tie)[0], np.nonzero(tie)[0]])  # (the ties fill the call from the back)
        Q, tie = Q[order], tie[order]
        assert tie[sub:2 * sub].any() and tie[2 * sub:].any(), tie
    want = ref.search_batch(Q, k, nthreads=8)
    runs = [({}, family), ({"no_mfma": 1}, "K3g"), ({"no_mfma": 1, "no_grp": 1}, "K3f")]
    if row == "K3s":
        # K3s stands in front of K3m and K3g only: k3s_decide asks for the grouped tables (`pre_ok` needs !no_grp), so there
        # is no K3s + K3f run to make -- checked below: under no_grp the forced option leaves the pre-filter off
        runs = [({"smin_pre": 1}, family), ({"smin_pre": -1}, family), ({"smin_pre": 1, "no_mfma": 1}, "K3g"), ({"smin_pre": -1, "no_mfma": 1}, "K3g"),
                ({"smin_pre": 1, "no_mfma": 1, "no_grp": 1}, "K3f")]
    whole = None
    for opts, fam in runs:
        for o, v in dict({"no_mfma": 0, "no_grp": 0, "smin_pre": -1}, **opts).items():
            ix.set_option(o, v)
        (got0, st0, d0), (got1, st1, d1) = whole_and_split(ix, sub, lambda: ix.search_batch(k, Q))
        assert_same(got1, want)
        same_bits(got1, got0)
        if whole is not None:
            same_bits(got0, whole)
        whole = got0
        assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3, (opts, st0["passa_launches"], st1["passa_launches"])
        assert d1["pass_b"] == fam, (opts, d1)
        if opts.get("smin_pre", -1) == 1:
            assert d0["pre"] == d1["pre"] == ("-" if opts.get("no_grp") else "K3s"), (opts, d0, d1)
        elif row == "K3s":
            # hint-driven: each sub-batch decides from the pinned figures of a stage that may lie one or two back, so which of them
            # take K3s is not determined (shown on failure); the answers above are, whichever do
            assert d0["pre"] in ("K3s", "-") and d1["pre"] in ("K3s", "-"), (opts, d0, d1)
            print("hint-driven K3s:", opts, "unsplit", d0["pre"], "last sub-batch", d1["pre"], "pairs left", st0["passb_items_last"], st1["passb_items_last"])
        if row == "ties":
            assert st1["tie_fallbacks"] >= int(tie.sum())  # (the replays of all three sub-batches accumulate)
    ix.close()


# ---- 3d -------------------------------------------------------------------------------------------------------------------------
def test_device_entry_as_a_caller_uses_it(mi, seq):
    """3d.  mmidx_search_device on a non-null torch stream: two calls with different query sets and different sub_batch (17, then 0)
    back to back, then one on a second stream (DeviceCall waits for the first), the host waiting only at the end.  The outputs
    start as -7 / NaN / -7 with a guard row in front and one behind.  The third call is the first 40 `mid` queries at w = 1 and
    sub_batch = 17: two of them (20, 21) lie next to the empty cell, so their count is 0 and their rows are the documented tail
    (-1, +inf) from the first entry on.

    The queries and the three guarded output triples exist before the first launch and the host waits once, for their fills.  Then
    a few milliseconds of element-wise work go onto the first stream, so that the two calls queue up behind it and are both still
    in flight when the third call arrives on the second stream: the only thing that keeps its kernels off the workspaces the first
    two are using is DeviceCall's wait.  The sequence runs twice: the first round may size the handle's workspaces (an allocation
    may wait for the device), the second finds them sized, nothing waits between its calls, and it asserts (hipStreamQuery, which
    asks without waiting) that the first stream was still busy when the third call was made."""
    import torch

    k = 100
    ix = seq.ix
    seq.options({}, W)
    ix.set_profiling(False)
    Qa, Qb, Qc = seq.data["Q"]["mid"][:40], seq.data["Q"]["self"], seq.data["Q"]["mid"][:40]
    wa, wb, wc = seq.want(("mid", 40), Qa, k, W), seq.want(("self", 40), Qb, k, W), seq.want(("mid", 40), Qc, k, 1)
    assert (wc[2] < k).any() and (wc[2] == k).any()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dA, dB, dC = (torch.tensor(q, dtype=torch.float64, device="cuda") for q in (Qa, Qb, Qc))
    ballast = torch.ones(1 << 27, dtype=torch.float32, device="cuda")  # (512 MiB: one pass over it is a good 0.2 ms of HBM traffic)
    for sized in (False, True):
        a, b, c = (device_outputs(40, k, guard=1) for _ in range(3))
        torch.cuda.synchronize()  # (the fills ran on torch's current stream; from here to the end of the round the host waits for nothing)
        with torch.cuda.stream(s1):
            for _ in range(60):
                ballast.mul_(1.0)
        ix.set_option("sub_batch", 17)
        device_launch(mi, ix, k, dA, a, s1, guard=1)
        ix.set_option("sub_batch", 0)
        device_launch(mi, ix, k, dB, b, s1, guard=1)
        in_flight = not s1.query()  # (asks, does not wait)
        ix.setW(1)
        ix.set_option("sub_batch", 17)
        device_launch(mi, ix, k, dC, c, s2, guard=1)
        s2.synchronize()
        s1.synchronize()
        ix.setW(W)
        ix.set_option("sub_batch", 0)
        assert in_flight or not sized, "the first stream had drained before the call on the second was made: this round tested no overlap"
        for t3, want in ((a, wa), (b, wb), (c, wc)):
            iid, dd, cc = (t.cpu().numpy() for t in t3)
            for g in (0, -1):
                assert np.all(iid[g] == -7) and np.all(np.isnan(dd[g])) and cc[g] == -7
            got = host(t3, guard=1)
            assert_same(got, want)
            for q in np.nonzero(got[2] < k)[0]:
                assert np.all(got[0][q, got[2][q]:] == -1) and np.all(np.isposinf(got[1][q, got[2][q]:]))


# ---- 3e -------------------------------------------------------------------------------------------------------------------------
def test_partial_lists(mi, seq):
    """3e.  mmidx_search_partial_device on the 40 `mid` queries with the cells of mmidx_coarse_device, as 17 + 17 + 6: the lists land
    at q0 (k + 1).  Counts and the valid entries of every list equal the unsplit call's bit for bit, and merged by
    mmidx_merge_partials_device (one shard) they are the oracle's answers.  The shard phases take one sub-batch per call:
    mmidx_shard_pass_a_device with 40 queries answers MMIDX_ERR_UNSUPPORTED, says so in mmidx_last_error and writes nothing."""
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    k, nq, K1 = 100, 40, 101
    ix = seq.ix
    seq.options({}, W)
    Q = seq.data["Q"]["mid"][:nq]
    want = seq.want(("mid", 40), Q, k, W)
    dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")
    cells = torch.empty(nq, W, dtype=torch.int32, device="cuda")
    nat.check(L.mmidx_coarse_device(ix._h, nq, dQ.data_ptr(), cells.data_ptr(), None, None))
    torch.cuda.synchronize()

    def run():
        pd = torch.full((nq, K1), float("nan"), dtype=torch.float64, device="cuda")
        pk = torch.full((nq, K1), -7, dtype=torch.int64, device="cuda")
        pc = torch.zeros(nq, dtype=torch.int32, device="cuda")  # (the merge below reads them: a count left unwritten is an empty list)
        torch.cuda.synchronize()
        nat.check(L.mmidx_search_partial_device(ix._h, k, nq, dQ.data_ptr(), cells.data_ptr(), pd.data_ptr(), pk.data_ptr(), pc.data_ptr(), None))
        iid = torch.empty(nq, k, dtype=torch.int32, device="cuda")
        dd = torch.empty(nq, k, dtype=torch.float64, device="cuda")
        cc = torch.empty(nq, dtype=torch.int32, device="cuda")
        nat.check(L.mmidx_merge_partials_device(0, k, nq, 1, pd.data_ptr(), pk.data_ptr(), pc.data_ptr(), None, iid.data_ptr(), dd.data_ptr(), cc.data_ptr(),
                                                None, None))
        torch.cuda.synchronize()
        return (pd.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()), (iid.cpu().numpy(), dd.cpu().numpy(), cc.cpu().numpy())

    ((l0, m0), st0, _), ((l1, m1), st1, _) = whole_and_split(ix, 17, run)
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
    assert np.array_equal(l1[2], l0[2]) and np.all(l1[2] >= k) and np.all(l1[2] <= K1)
    # "bit for bit" is asked of what a list defines: its count and the entries below it.  A list holds k or k + 1 entries, so the one
    # slot it may leave undefined is its last; whatever that slot holds (the fill, or a value the kernel parked there) is not compared
    valid = np.arange(K1)[None, :] < l1[2][:, None]
    assert valid[:, :k].all() and (~valid).sum(axis=1).max() <= 1
    assert np.array_equal(l1[0].view(np.uint64)[valid], l0[0].view(np.uint64)[valid])
    assert np.array_equal(l1[1][valid], l0[1][valid])
    assert np.all(l1[1][valid] >= 0) and not np.isnan(l1[0][valid]).any()
    assert_same(m1, want)
    same_bits(m1, m0)
    # one sub-batch per shard phase
    T = torch.full((nq,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ix.set_option("sub_batch", 17)
    rc = L.mmidx_shard_pass_a_device(ix._h, k, nq, dQ.data_ptr(), cells.data_ptr(), T.data_ptr(), None)
    msg = L.mmidx_last_error().decode()
    ok = L.mmidx_shard_pass_a_device(ix._h, k, 17, dQ.data_ptr(), cells.data_ptr(), T[20:].data_ptr(), None)
    torch.cuda.synchronize()
    ix.set_option("sub_batch", 0)
    assert rc == nat.ERR_UNSUPPORTED and "at most 17 queries" in msg, (rc, msg)
    assert ok == 0
    Th = T.cpu().numpy()
    assert np.all(Th[:20] == -7.0) and np.all(Th[37:] == -7.0) and np.all(Th[20:37] > 0)  # (the refused call wrote nothing; 17 queries pass)


# ---- 3f -------------------------------------------------------------------------------------------------------------------------
def test_id_queries(mi, oracle, seq):
    """3f.  mmidx_search_ids and mmidx_search_ids_device with 40 ids as 17 + 17 + 6: the decoded vectors are the queries (the twin
    of tests/decode_twin.py over the index's own export), the oracle searches them."""
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    k, ix = 20, seq.ix
    seq.options({}, W)
    n = len(seq.data["base"])
    ids = np.random.default_rng(5).integers(0, n, 40).astype(np.int32)
    ids[-1] = ids[0]
    off, eiids, codes = ix.export()
    X = dt.decode_exported(seq.data["pq"], off, eiids, codes, ids, seq.data["mu"], 0, None, None)
    want = seq.want("ids", X, k, W)
    (got0, st0, _), (got1, st1, _) = whole_and_split(ix, 17, lambda: ix.search_ids_batch(k, ids))
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
    assert_same(got1, want)
    same_bits(got1, got0)
    assert np.all(np.any(got1[0] == ids[:, None], axis=1))  # (every query's own record is among its answers)
    s1 = torch.cuda.Stream()
    d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")

    def dev():
        oi = torch.full((40, k), -7, dtype=torch.int32, device="cuda")
        od = torch.full((40, k), float("nan"), dtype=torch.float64, device="cuda")
        oc = torch.full((40,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nat.check(mi.lib().mmidx_search_ids_device(ix._h, k, 40, d_ids.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr(), s1.cuda_stream))
        s1.synchronize()
        return host((oi, od, oc))

    (dev0, st0, _), (dev1, st1, _) = whole_and_split(ix, 17, dev)
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
    assert_same(dev1, want)
    same_bits(dev1, dev0)


def test_refine(mi, oracle, seq):
    """3f.  mmidx_search_refine and its _device form at R = 150, k = 20 against a Linear index over the same rows: the compressed
    search for R candidates runs as 17 + 17 + 6 into the refinement's own buffers."""
    import torch

    k, R, ix = 20, 150, seq.ix
    seq.options({}, W)
    base = seq.data["base"]
    Q = seq.data["Q"]["mid"][:40]
    lin = mi.Linear(D, len(base) + 8)
    lin._add_vectors(base, None)
    want = rt.refine_batch(seq.want(("mid", 40), Q, R, W), base, Q, k)
    assert want[3] == 0
    (got0, st0, _), (got1, st1, _) = whole_and_split(ix, 17, lambda: ix.search_refine_batch(k, R, Q, lin))
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
    assert_same(got1[:3], want[:3])
    same_bits(got1, got0)
    assert got1[3] == 0
    dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")

    def dev():
        t = ix.search_refine_batch_device(k, R, dQ, lin)
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in t)

    (dev0, st0, _), (dev1, st1, _) = whole_and_split(ix, 17, dev)
    lin.close()
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
    assert_same(dev1[:3], want[:3])
    same_bits(dev1, dev0)
    assert int(dev1[3][0]) == 0


def test_flat_pq_adc(mi, oracle):
    """3f.  Flat PQ ADC at (D = 128, m = 8, 70000 codes, flat_chunk = 8192: nine chunks), the first row of test_mfma_flat_pq, its 100
    queries as 37 + 37 + 26: chunk 0 is pass A, the others go through K3m under pass A's thresholds."""
    D_, m, n, k, chunk = 128, 8, 70000, 100, 8192
    p = synth.make_pq_problem(n=8000, D=D_, m=m, ks=256, nq=12, seed=D_ + m, iters=2)
    rng = np.random.default_rng(n)
    base = rng.standard_normal((n, D_))
    ix = mi.PQ(D_, n, False, "", m, 256, 0, 512)
    ix.loadProductQuantizer(p["pq"])
    ix.set_option("flat_chunk", chunk)
    ref = oracle.OracleIndex(oracle.KIND_PQ, D_, m, 256)
    ref.set_pq(p["pq"])
    ix.indexVectors([str(i) for i in range(n)], base)
    ref.load_lists(*ix.export())
    Q = np.concatenate([base[:20] + 0.05 * rng.standard_normal((20, D_)), rng.standard_normal((80, D_))])
    want = ref.search_batch(Q, k, nthreads=8)
    assert sc.plan(D_, m, 256, 0, n, k, 100, chunk, sub_batch=37)["qb"] == 37
    for off in (0, 1):
        ix.set_option("no_mfma", off)
        (got0, st0, d0), (got1, st1, d1) = whole_and_split(ix, 37, lambda: ix.search_batch(k, Q))
        assert_same(got1, want)
        same_bits(got1, got0)
        assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3
        assert d1["pass_b"] == d0["pass_b"] and d1["pass_b"] in (("K3g", "K3f") if off else ("K3m",)), (d0, d1)
    ix.close()


def test_two_virtual_shards(mi, oracle, data):
    """3f.  A handle of two virtual shards on one device: the option reaches the shards like every other, and the group's
    collective rounds take the smallest `qb` of the shards rounded down to a multiple of their number -- 16, so 40 queries run as
    rounds of 16 + 16 + 8 (passa_launches of a sharded handle: the largest over the shards)."""
    s = Seq(mi, oracle, data, devices=[0, 0])
    k = 100
    Q = data["Q"]["mid"][:40]
    want = s.want(("mid", 40), Q, k, W)
    (got0, st0, _), (got1, st1, _) = whole_and_split(s.ix, 17, lambda: s.ix.search_batch(k, Q))
    s.ix.close()
    assert_same(got1, want)
    same_bits(got1, got0)
    assert st0["passa_launches"] == 1 and st1["passa_launches"] == 3


# ---- 3g -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup", [1, 3])
def test_table_slot_cap(mi, oracle, dup):
    """3g(i).  test_lookup_table_larger_than_lds's IVFPQ shape (D = 64, six cells, m = 32 x 1024: 256 KiB of table per (query,
    probe) in global scratch) at w = 6 with 1368 queries, option at 0: 2 GiB / (256 KiB x 6) = 1365 queries per sub-batch, so the
    call runs as 1365 + 3 -- plain, and with every vector three times, where k = 10 = 3 x 3 + 1 puts a straddling tie in nearly
    every query and the replay of the tail finds its tables at slots of its own sub-batch.  The call reserves about 2.1 GiB of
    device memory for the table slots ((1365 x 6 + 8) x 256 KiB), as the SDC case `sub_batches` does."""
    D_, C, m, ks, n, w, k, nq = 64, 6, 32, 1024, 4000, 6, 10, 1368
    pl = pm.ivf_plan(D_, m, ks, C, w, dup * n, dup * n, k, nq)
    assert pl["glut"] and pl["qb"] == 1365 and parts(nq, pl["qb"]) == [1365, 3]
    p = synth.make_ivfpq_problem(n=n, D=D_, C=C, m=m, ks=ks, nq=nq, seed=11)
    base = p["base"]
    if dup > 1:
        base = np.concatenate([base] * dup)[np.random.default_rng(2).permutation(dup * n)]
    ix = mi.IVFPQ(D_, len(base), False, "", m, ks, 0, C, 512)
    ix.loadCoarseQuantizer(p["coarse"])
    ix.loadProductQuantizer(p["pq"])
    ix.setW(w)
    ix.indexVectors([str(i) for i in range(len(base))], base)
    ref = oracle_ivfpq(oracle, p, D_, m, ks, C, w)
    ref.load_lists(*ix.export())
    Q = p["queries"]
    want = ref.search_batch(Q, k, nthreads=8)
    assert not np.array_equal(want[0][1365], want[0][0]) and not np.array_equal(Q[1365], Q[0])
    if dup > 1:
        w1 = ref.search_batch(Q, k + 1, nthreads=8)
        tie = (w1[2] > k) & (w1[1][:, k - 1] == w1[1][:, k])
        assert tie[1365:].any() and tie[:1365].any()
    ix.set_profiling(True)
    got = ix.search_batch(k, Q)
    st, d = ix.get_stats(), ix.get_dispatch()
    assert_same(got, want)
    assert st["passa_launches"] == 2 and d["pass_a"] == "K3(table in global scratch)", (st["passa_launches"], d)
    if dup > 1:
        assert st["tie_fallbacks"] >= int(tie.sum())  # (the replays of both sub-batches accumulate)
    same_bits(ix.search_batch(k, Q[1365:]), tuple(a[1365:] for a in got))  # (the tail alone: an unsplit call)
    ix.close()


def test_flat_table_slot_cap(mi, oracle):
    """3g(ii).  The SDC case `sub_batches` under ADC: 128 x 256 flat PQ, four chunks of 4096, 2 GiB / (256 KiB x 4) = 2048 queries
    per sub-batch, 2049 + 3 queries as 2048 + 4 (about 2.1 GiB of table slots)."""
    c = sc.case("sub_batches")
    D_, m, ks, n, k = c["D"], c["m"], c["ks"], c["n"], 10
    nq = 2049 + 3
    assert sc.plan(D_, m, ks, 0, n, k, nq, c["flat_chunk"])["qb"] == 2048
    ix = mi.PQ(D_, n, False, "", m, ks, 0, 512)
    ix.loadProductQuantizer(c["pq"])
    ix.set_option("flat_chunk", c["flat_chunk"])
    ix.loadIndex(mi.PQ.transformToByte(c["codes"]))
    ref = sc.oracle_index(c)
    rng = np.random.default_rng(77)
    X = np.concatenate([c["pq"][s][c["codes"][:, s]] for s in range(m)], axis=1)  # (the vectors the codes decode to)
    Q = X[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, D_))
    want = ref.search_batch(Q, k, nthreads=8)
    ix.set_profiling(True)
    got = ix.search_batch(k, Q)
    st = ix.get_stats()
    assert_same(got, want)
    assert st["passa_launches"] == 2
    same_bits(ix.search_batch(k, Q[2048:]), tuple(a[2048:] for a in got))
    ix.close()


@pytest.mark.parametrize("entry", ["host", "device"])
def test_exact_coarse_cap(mi, oracle, entry):
    """3g(iii).  C = 16390 cells (beyond the certified coarse stage's 64 x 256), D = 16, w = 9, 20000 records: the [nq][C] matrix of
    exact coarse distances is capped at 2 GiB, 16378 queries, so 16378 + 40 queries run as two sub-batches -- through mmidx_search
    (more than 4096 queries: search_host_big's slot path) and through mmidx_search_device.  Every query of the call is compared with
    the same queries given in two unsplit calls; the oracle is consulted for the 40 of the second sub-batch, the last 100 of the
    first and 372 drawn over the rest: 512 of 16418, a cap that exists only to keep the test to seconds (the oracle ranks 16390
    centroids per query)."""
    import torch

    D_, C, w, n, k, m, ks = 16, 16390, 9, 20000, 10, 2, 16
    qb, nq = 16378, 16378 + 40
    assert pm.ivf_plan(D_, m, ks, C, w, n, 64, k, nq)["qb"] == qb
    rng = np.random.default_rng(D_ * 7 + C)
    centers = 4.0 * rng.standard_normal((C // 40 + 2, D_))
    coarse = centers[rng.integers(0, len(centers), C)] + 0.7 * rng.standard_normal((C, D_))
    coarse[C // 2:C // 2 + 20] = coarse[:20]  # duplicates -> equal distances
    pq = rng.standard_normal((m, ks, D_ // m))
    base = coarse[rng.integers(0, C, n)] + 0.3 * rng.standard_normal((n, D_))
    Q = coarse[rng.integers(0, C, nq)] + 0.3 * rng.standard_normal((nq, D_))
    ix = mi.IVFPQ(D_, n, False, "", m, ks, 0, C, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ix.indexVectors([str(i) for i in range(n)], base)
    ref = oracle.OracleIndex(oracle.KIND_IVFPQ, D_, m, ks, C)
    ref.set_coarse(coarse)
    ref.set_pq(pq)
    ref.set_w(w)
    ref.load_lists(*ix.export())
    pick = np.concatenate([np.sort(rng.choice(qb - 100, 372, replace=False)), np.arange(qb - 100, nq)])
    assert len(pick) == 512
    want = ref.search_batch(Q[pick], k, nthreads=8)
    half = 8209

    if entry == "host":
        def run(q):
            return ix.search_batch(k, q)
    else:
        s1 = torch.cuda.Stream()

        def run(q):
            t3 = device_search(mi, ix, k, torch.tensor(q, dtype=torch.float64, device="cuda"), s1)
            s1.synchronize()
            return host(t3)

    ix.set_profiling(True)
    got = run(Q)
    st = ix.get_stats()
    assert st["passa_launches"] == 2
    two = [run(Q[:half]), run(Q[half:])]
    assert ix.get_stats()["passa_launches"] == 2  # (each of them unsplit)
    ix.close()
    same_bits(got, tuple(np.concatenate([a, b]) for a, b in zip(*two)))
    assert_same(tuple(a[pick] for a in got), want)
