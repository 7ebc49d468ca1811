"""The per-stage statistics of the matrix-core chains (K3m, K3mk, K3ma): `mfma_launches`, `mfma_scan_ms`, `mfma_verify_ms`,
`passa_mfma_launches` and the four `passa_mfma_*_ms`.

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
