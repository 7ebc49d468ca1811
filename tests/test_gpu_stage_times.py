"""The per-stage statistics of the matrix-core chains (K3m, K3mk, K3ma): `mfma_launches`, `mfma_scan_ms`, `mfma_verify_ms`,
`passa_mfma_launches` and the four `passa_mfma_*_ms` -- and, below, those of the search step's main event group: `total_ms`,
`coarse_ms`, `scan_ms`, `merge_ms`, `passa_ms`, `scan_launches` and `passa_launches`.

They come from groups of HIP events that every chain takes from a pool on the handle (take_events, csrc/mmidx_api.hip) and that
`get_stats` resolves and hands back to the pool; tests/bench_yfcc.py reports them.  One index per case, built once; every search
below is also compared with the oracle, so the profiled calls are the same calls that the parity tests make.
"""
import numpy as np
import pytest

import synth
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture)

pytestmark = pytest.mark.gpu

A_MS = ("passa_mfma_sweep1_ms", "passa_mfma_select_ms", "passa_mfma_sweep2_ms", "passa_mfma_verify_ms")


@pytest.mark.parametrize("D,m,C,n,w,k,chain", [
    (64, 8, 4, 16000, 4, 20, "K3m"),
    (256, 16, 5, 12000, 5, 50, "K3mk"),
    (32, 8, 3, 9000, 3, 10, "K3ma"),   # (pass A through K3ma, pass B through K3m behind it)
])
def test_stage_times(mi, oracle, D, m, C, n, w, k, chain):
    """Profiling on, two searches, one `get_stats`: two event groups of the pass-B chain (and, for K3ma, two of pass A's), every
    interval positive.  A second `get_stats` with no search in between finds the pools drained: the same fields are 0.  With
    profiling off two more searches take no events at all."""
    ks = 256
    rng = np.random.default_rng(D + m + k)
    mu = 0.5 * rng.standard_normal((C, D))
    base = mu[rng.integers(0, C, n)] + rng.standard_normal((n, D))
    ds = D // m
    pq = np.stack([synth.kmeans((mu[rng.integers(0, C, 3000)] - base[:3000])[:, s * ds:(s + 1) * ds], ks, iters=2, seed=s) for s in range(m)])
    ix = mi.IVFPQ(D, n, False, "", m, ks, 0, C, 512)
    ix.loadCoarseQuantizer(mu)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ref = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D, m, ks, C, w)
    ix.indexVectors([str(i) for i in range(n)], base)
    ref.add_vectors(base)
    Q = base[:40] + 0.01 * rng.standard_normal((40, D))
    want = ref.search_batch(Q, k)
    passa = chain == "K3ma"
    if passa:
        ix.set_option("passa_mfma", 1)

    ix.set_profiling(True)
    for _ in range(2):
        assert_same(ix.search_batch(k, Q), want)
        assert ix.get_dispatch()["pass_b"] == ("K3mk" if chain == "K3mk" else "K3m")
    st = ix.get_stats()
    print({f: st[f] for f in ("mfma_launches", "mfma_scan_ms", "mfma_verify_ms", "passa_mfma_launches") + A_MS})
    assert st["mfma_launches"] == 2
    assert st["mfma_scan_ms"] > 0
    assert st["mfma_verify_ms"] > 0
    if passa:
        assert st["passa_mfma_launches"] == 2
        for f in A_MS:
            assert st[f] > 0, f
    else:
        assert st["passa_mfma_launches"] == 0

    again = ix.get_stats()  # (no search in between: the pools were drained)
    for f in ("mfma_launches", "mfma_scan_ms", "mfma_verify_ms", "passa_mfma_launches") + A_MS:
        assert again[f] == 0, f

    ix.set_profiling(False)
    for _ in range(2):
        assert_same(ix.search_batch(k, Q), want)
    off = ix.get_stats()
    assert off["mfma_launches"] == 0
    assert off["mfma_scan_ms"] == 0 and off["mfma_verify_ms"] == 0
    ix.close()


# ---- the main event group of the search step (search_batch_device) ---------------------------------------------------------------
# Six events per step: start, coarse end, scan start, scan end, end, pass-A end.  Profiling 1 records all of them and counts the scan
# launches; profiling 2 records the pass-A pair alone.  A shard's phase 1 and phase 2 take a group each.
MAIN_MS = ("total_ms", "coarse_ms", "scan_ms", "merge_ms", "passa_ms")
MAIN = MAIN_MS + ("scan_launches", "passa_launches")
SLACK = 1e-3  # relative: the intervals are float differences of event times
CALLS = 2
D_, M_, KS_, C_, N_, K_, NQ_ = 32, 8, 256, 4, 9000, 10, 40


@pytest.fixture(scope="module")
def step_data(oracle):
    """one set of vectors and quantizers, and the oracle's answers, for every case below"""
    rng = np.random.default_rng(77)
    mu = 0.5 * rng.standard_normal((C_, D_))
    base = mu[rng.integers(0, C_, N_)] + rng.standard_normal((N_, D_))
    ds = D_ // M_
    pq = np.stack([synth.kmeans((mu[rng.integers(0, C_, 3000)] - base[:3000])[:, s * ds:(s + 1) * ds], KS_, iters=2, seed=s) for s in range(M_)])
    Q = base[:NQ_] + 0.01 * rng.standard_normal((NQ_, D_))
    want = {}
    for w in (3, 1):
        ref = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D_, M_, KS_, C_, w)
        ref.add_vectors(base)
        want[w] = ref.search_batch(Q, K_)
    ref = oracle.OracleIndex(oracle.KIND_PQ, D_, M_, KS_)
    ref.set_pq(pq)
    ref.add_vectors(base)
    want["flat"] = ref.search_batch(Q, K_)
    ref = oracle_ivfpq(oracle, {"coarse": mu, "pq": pq}, D_, M_, KS_, C_, 3)
    want["empty"] = ref.search_batch(Q, K_)
    return {"mu": mu, "pq": pq, "base": base, "Q": Q, "want": want}


# case: (kind, w, records?, devices, passes of a step that scans, the key of the oracle's answer)
STEP_CASES = {
    "ivfpq": ("ivf", 3, True, None, 2, 3),
    "flat_pq": ("flat", 0, True, None, 2, "flat"),       # flat_chunk = 4096: three chunks, chunk 0 is pass A
    "ivfpq_w1": ("ivf", 1, True, None, 1, 1),
    "empty": ("ivf", 3, False, None, 0, "empty"),        # quantizers set, no records: the scan stages are skipped
    "two_shards": ("ivf", 3, True, [0, 0], 2, 3),        # phase 1 and phase 2 on every shard
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_times(mi, step_data, case):
    """Two searches per profiling mode, each compared with the oracle, one `get_stats` behind them.

    Profiling 1: every interval that applies is positive, passa_ms <= scan_ms and coarse_ms + scan_ms + merge_ms <= total_ms;
    `passa_launches` is the number of calls and `scan_launches` that times the passes.  Profiling 2: `passa_ms` and `passa_launches`
    alone, the other four intervals exactly 0.  A second `get_stats` finds the pool drained; profiling 0 takes no events.

    What does not apply: `coarse_ms` on flat PQ (no coarse stage) and on the shards (they get their cells from the group, whose
    coarse stage lies outside their events); on the empty index the scan events are recorded back to back with no launch between
    them, so `scan_ms` and `passa_ms` may be 0 and no launch is counted -- the counts are the ones the library reports.  (A sharded
    handle reports the largest of each time and count over its shards.)"""
    kind, w, filled, devices, passes, key = STEP_CASES[case]
    d = step_data
    if kind == "ivf":
        ix = mi.IVFPQ(D_, N_, False, "", M_, KS_, 0, C_, 512, **({"devices": devices} if devices else {}))
        ix.loadCoarseQuantizer(d["mu"])
        ix.loadProductQuantizer(d["pq"])
        ix.setW(w)
    else:
        ix = mi.PQ(D_, N_, False, "", M_, KS_, 0, 512)
        ix.loadProductQuantizer(d["pq"])
        ix.set_option("flat_chunk", 4096)
    if filled:
        ix.indexVectors([str(i) for i in range(N_)], d["base"])
    want = d["want"][key]
    scans = passes > 0

    def searches():
        for _ in range(CALLS):
            assert_same(ix.search_batch(K_, d["Q"]), want)
        return ix.get_stats()

    ix.set_profiling(1)
    st = searches()
    print(case, "profiling 1", {f: st[f] for f in MAIN})
    assert st["total_ms"] > 0 and st["merge_ms"] > 0
    if kind == "ivf" and not devices:
        assert st["coarse_ms"] > 0
    if scans:
        assert st["scan_ms"] > 0 and st["passa_ms"] > 0
    assert st["passa_ms"] <= st["scan_ms"] * (1 + SLACK)
    assert st["coarse_ms"] + st["scan_ms"] + st["merge_ms"] <= st["total_ms"] * (1 + SLACK)
    assert st["passa_launches"] == (CALLS if scans else 0)
    assert st["scan_launches"] == CALLS * passes
    again = ix.get_stats()  # (no search in between: the pool was drained)
    for f in MAIN:
        assert again[f] == 0, f

    ix.set_profiling(2)
    st = searches()
    print(case, "profiling 2", {f: st[f] for f in MAIN})
    if scans:
        assert st["passa_ms"] > 0
    assert st["passa_launches"] == (CALLS if scans else 0)
    for f in ("total_ms", "coarse_ms", "scan_ms", "merge_ms"):
        assert st[f] == 0, f
    again = ix.get_stats()
    for f in MAIN:
        assert again[f] == 0, f

    ix.set_profiling(0)
    st = searches()
    for f in MAIN:
        assert st[f] == 0, f
    ix.close()
