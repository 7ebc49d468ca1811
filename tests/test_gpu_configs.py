"""Every BASELINE.json config at its STATED size under `-m gpu`, each checked against the CPU oracle:

  cfg1  Linear 10k x 128, k = 10                                   (tests/bench_configs.py, 1000 queries)
  cfg2  PQ ADC 1M x 128, m = 8 x 256, k = 100                      (256 oracle queries)
  cfg3  IVFPQ 1M x 128, C = 1024, w = 8, m = 16 x 256, k = 100     (2048 oracle queries)
  cfg4  IVFPQ 100M x 128, C = 8192, w = 32, m = 16 x 256, k = 100  single GPU: SURVEY 8d's generator (sigma 0.15: the coarse
        bound prunes 31 of 32 probes, pass A decides) AND overlapping clusters (sigma 1.0: all 32 probes go through the
        grouped filtered scan K3g / its hand-back K3f / K4 with a populated pool), 512 oracle queries each via mmidx_export
  cfg5  descriptors -> VLAD -> PCA -> IVFPQ, 100k synthetic images, device-resident front end

The 8-GPU leg of cfg4 needs 8 GPUs (the driver's SCALE run); its orchestration is covered by tests/test_sharded_gloo.py and
the virtual-shard tests in test_gpu_parity.py.
"""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture(scope="module")
def small_configs():
    import bench_configs

    return bench_configs.run_all()


def test_cfg1_linear_10k(small_configs):
    r = small_configs["cfg1_linear_10k"]
    assert r["ids_match"] and r["max_abs_ddist"] == 0.0, r


def test_cfg2_pq_adc_1m(small_configs):
    r = small_configs["cfg2_pq_adc_1M"]
    assert r["ids_match"] and r["max_abs_ddist"] == 0.0, r


def test_cfg3_ivfpq_1m(small_configs):
    r = small_configs["cfg3_ivfpq_1M"]
    assert r["ids_match"] and r["max_abs_ddist"] == 0.0 and r["recall_at_1"] >= 0.9, r


@pytest.mark.parametrize("sigma", [0.15, 1.0])
def test_cfg4_ivfpq_100m_single_gpu(sigma):
    """the bench's own builders (bench.py), 100M vectors, queries for the headline batch of 16384: oracle on 512 queries of a
    4096-query call (K3h: fewer than 1.25 queries per list) and on 512 queries drawn over the whole 16384-query call (K3q, the
    headline's pass A); batch-wide properties of both"""
    import argparse

    import torch

    import bench

    cx = bench.Ctx()
    cx.torch = torch
    cx.args = argparse.Namespace(n=100_000_000, dim=128, cells=8192, w=32, m=16, k=100, chunk=2_000_000, opt=[])
    cx.mi = importlib.import_module("multimedia-indexing_amd")
    cx.nat = importlib.import_module("multimedia-indexing_amd._native")
    cx.L = cx.mi.lib()
    cx.chk = cx.nat.check
    cx.world, cx.rank, cx.local, cx.dist = 1, 0, 0, None
    cx.dev = torch.device("cuda", 0)
    cx.stream = torch.cuda.current_stream().cuda_stream
    k, B, BH, ns, N = 100, 4096, 16384, 512, 100_000_000
    mu, coarse_h, pq_h = bench.learn_codebooks(cx, sigma)
    h, Q = bench.build_index(cx, mu, sigma, coarse_h, pq_h, BH, sharded_build=False)
    # (the vector each query perturbs: build_index's own draw)
    gq = torch.Generator(device=cx.dev)
    gq.manual_seed(4321)
    qsrc = torch.randint(0, N, (BH,), generator=gq, device=cx.dev).cpu().numpy()

    def search(nq):
        iid = torch.empty(nq, k, dtype=torch.int32, device=cx.dev)
        dd = torch.empty(nq, k, dtype=torch.float64, device=cx.dev)
        cc = torch.empty(nq, dtype=torch.int32, device=cx.dev)
        cx.chk(cx.L.mmidx_search_device(h, k, nq, Q.data_ptr(), iid.data_ptr(), dd.data_ptr(), cc.data_ptr(), cx.stream))
        torch.cuda.synchronize()
        buf = C.create_string_buffer(512)
        cx.chk(cx.L.mmidx_get_dispatch(h, buf, 512))
        disp = dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))
        return iid.cpu().numpy(), dd.cpu().numpy(), cc.cpu().numpy(), disp

    hits = []

    def batch_props(i_all, d_all, nq):
        # size-independent properties on the whole batch: ascending distances, ids inside the index, self hit (asserted at the end)
        assert np.all(np.diff(d_all, axis=1) >= 0.0)
        assert i_all.min() >= 0 and i_all.max() < N
        hits.append(float(np.mean((i_all == qsrc[:nq, None]).any(axis=1))))
        print(f"cfg4 sigma {sigma}: self hit in the top {k} of {nq} queries: {hits[-1]:.4f}")

    try:
        cx.chk(cx.L.mmidx_set_profiling(h, 1))
        i4, d4, c4, disp4 = search(B)
        st = cx.nat.Stats()
        cx.chk(cx.L.mmidx_get_stats(h, C.byref(st)))
        cx.chk(cx.L.mmidx_set_profiling(h, 0))
        print(f"cfg4 sigma {sigma}: dispatch of {B} queries: {disp4}")
        assert disp4["pass_a"] == "K3h", disp4  # (4096 queries on 8192 lists: below K3q's gate)
        pairs_per_query = st.passb_items_last / B
        if sigma >= 1.0:
            assert pairs_per_query > 0.5 * 31, "the hard workload must defeat the coarse bound"
        else:
            assert pairs_per_query < 1.0
        ref = bench.oracle_of_index(cx, h, coarse_h, pq_h)
        rid, rd, rc = ref.search_batch(Q[:ns].cpu().numpy(), k, nthreads=bench.usable_cpus()[0])
        assert np.array_equal(c4[:ns], rc)
        assert np.array_equal(i4[:ns], rid), "neighbour ids differ from the oracle at 100M"
        assert np.array_equal(d4[:ns], rd), "distances are not bit-equal at 100M"
        batch_props(i4, d4, B)
        # the headline batch through the default dispatch: K3q
        t_head = time.time()
        ih, dh, ch, disph = search(BH)
        print(f"cfg4 sigma {sigma}: dispatch of {BH} queries: {disph}")
        assert disph["pass_a"] == "K3q", disph
        # a sample over the WHOLE batch (not a prefix): many nearest lists, every position of a K3q group of four
        sel = np.sort(np.random.default_rng(16384).choice(BH, ns, replace=False))
        rid, rd, rc = ref.search_batch(Q[torch.as_tensor(sel, device=cx.dev)].cpu().numpy(), k, nthreads=bench.usable_cpus()[0])
        assert np.array_equal(ch[sel], rc)
        assert np.array_equal(ih[sel], rid), "neighbour ids of the headline batch differ from the oracle at 100M"
        assert np.array_equal(dh[sel], rd), "distances of the headline batch are not bit-equal at 100M"
        batch_props(ih, dh, BH)
        # the first 4096 queries: K3q's answers are K3h's
        assert np.array_equal(ch[:B], c4) and np.array_equal(ih[:B], i4) and np.array_equal(dh[:B], d4)
        print(f"cfg4 sigma {sigma}: the headline batch's call and checks took {time.time() - t_head:.1f} s")
        assert min(hits) >= 0.9, hits
        del ref
    finally:
        cx.chk(cx.L.mmidx_destroy(h))
        torch.cuda.empty_cache()


def test_cfg5_end_to_end_100k_images():
    import config5_pipeline as c5
    from oracle import oracle as o

    out, chk = c5.run_device(n_images=100_000, n_queries=256, k=10, cells=1024, w=8)
    # front end against the oracle on a sample of images (VLAD + PCA, 1e-12 relative to the unit row norm)
    Vw = o.pca_whiten(chk["Vt"], chk["eig"])  # (whitening folded into the basis, PCA.java:275-313)
    for j, descs in zip(chk["sample_ids"], chk["sample_descs"]):
        xo = o.pca_project(Vw, chk["means"], o.vlad_aggregate_multi([chk["codebook"]], descs, True), True)
        assert np.max(np.abs(chk["X"][j] - xo)) <= 1e-12
    assert np.allclose(np.linalg.norm(chk["X"], axis=1), 1.0, atol=1e-12)
    # index / search half bit-exact against the oracle fed with the same projected vectors
    ref = o.OracleIndex(o.KIND_IVFPQ, 128, 16, 256, chk["cells"])
    ref.set_coarse(chk["coarse"])
    ref.set_pq(chk["pq"])
    ref.set_w(chk["w"])
    ref.add_vectors(chk["X"])
    rid, rd, rc = ref.search_batch(chk["Q"], chk["k"], nthreads=8)
    assert np.array_equal(chk["iids"], rid) and np.array_equal(chk["dists"], rd) and np.array_equal(chk["counts"], rc)
    assert out["self_hit_rate"] >= 0.9, out
