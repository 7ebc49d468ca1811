"""GPU parity of the config-5 front end: batched VLAD (K8) and the f64-MFMA PCA projection (K7)
against the CPU oracle.  VLAD without normalisation is bit-exact (accumulation in descriptor
order); normalised VLAD and PCA carry the stated 1e-12 tolerance (Math.pow / EJML order, A2)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def mi():
    try:
        import torch

        torch.cuda.init()
    except Exception:
        pass
    m = importlib.import_module("multimedia-indexing_amd")
    if m.lib().mmidx_device_count() < 1:
        pytest.fail("libmmidx_hip.so found no HIP device: GPU tests must run the native path")
    return m


@pytest.mark.parametrize("nc,dl", [(128, 64), (32, 64), (20, 12)])
def test_vlad_raw_bit_exact(mi, oracle, nc, dl):
    rng = np.random.default_rng(nc + dl)
    cb = rng.standard_normal((nc, dl))
    sets = [rng.standard_normal((n, dl)) for n in (0, 1, 7, 300, 777, 256, 513)]
    for s in sets:  # SURF-like: L2-normalised descriptors
        if len(s):
            s /= np.linalg.norm(s, axis=1, keepdims=True)
    agg = mi.VladAggregator(cb)
    # (0, 0): K8'' where it applies (dl = 64, <= 128 centroids: one kernel -- certified bf16-MFMA argmin, flagged descriptors redone in
    # fp64 by the image's block, ordered accumulation), else K8'; (0, 1): K8' (assignment kernel over all descriptors of the call +
    # accumulation kernel); (1, 0): fp64 brute force in the block
    for exact, two in ((0, 0), (0, 1), (1, 0)):
        agg.set_option("exact", exact)
        agg.set_option("two_pass", two)
        out = agg.aggregate_batch(sets)
        assert out.shape == (len(sets), nc * dl)
        for i, s in enumerate(sets):
            ref = oracle.vlad_aggregate(cb, s)
            assert np.array_equal(out[i], ref), (exact, two, i)
        assert np.array_equal(agg.aggregate(sets[3]), oracle.vlad_aggregate(cb, sets[3]))
    agg.close()


def test_vlad_single_centroid_vocabulary(mi, oracle):
    """nc = 1: the assignment handle needs two centroids, so the vocabulary's slot stays empty and k_vlad serves it.  An empty
    slot is no error of mmidx_vlad_create: no text is left behind (the error text is per thread, so the case runs in a thread of
    its own, where no earlier test's refusal can be what is read)."""
    import threading

    rng = np.random.default_rng(1)
    dl = 64
    cb = rng.standard_normal((1, dl))
    sets = [rng.standard_normal((n, dl)) for n in (0, 1, 70)]
    res = {}

    def run():
        try:
            agg = mi.VladAggregator(cb)
            res["out"] = agg.aggregate_batch(sets)
            res["err"] = mi.lib().mmidx_last_error()
            agg.close()
        except Exception as e:  # noqa: BLE001
            res["exc"] = e

    th = threading.Thread(target=run)
    th.start()
    th.join()
    assert "exc" not in res, res.get("exc")
    for i, s in enumerate(sets):
        assert np.array_equal(res["out"][i], oracle.vlad_aggregate(cb, s)), i
    assert res["err"] == b""


def test_vlad_assignment_ties_first_centroid_wins(mi, oracle):
    """computeNearestCentroid (AFA:136-155) updates on `<` only: of several equally near centroids the FIRST wins.  Duplicate
    centroids and descriptors that coincide with centroids: the MFMA assignment cannot certify those and redoes them in fp64."""
    rng = np.random.default_rng(9)
    nc, dl = 64, 64
    cb = rng.standard_normal((nc, dl))
    cb[40] = cb[3]
    cb[41] = cb[3]
    cb[10] = cb[50]
    sets = [np.concatenate([cb[[3, 50, 7]], cb[3:4] + 1e-9, rng.standard_normal((200, dl))]), cb[[40, 41, 10, 50]].copy()]
    agg = mi.VladAggregator(cb)
    for exact, two in ((0, 0), (0, 1), (1, 0)):
        agg.set_option("exact", exact)
        agg.set_option("two_pass", two)
        out = agg.aggregate_batch(sets)
        for i, s in enumerate(sets):
            assert np.array_equal(out[i], oracle.vlad_aggregate(cb, s)), (exact, two, i)
    # more uncertifiable descriptors in one image than the fused kernel's list holds (64): every descriptor of the image is redone
    many = [np.concatenate([cb[[3, 50]]] * 60 + [rng.standard_normal((30, dl))])]
    agg.set_option("exact", 0)
    agg.set_option("two_pass", 0)
    assert np.array_equal(agg.aggregate_batch(many)[0], oracle.vlad_aggregate(cb, many[0]))
    agg.close()


def test_vlad_multi_vocab_normalised(mi, oracle):
    rng = np.random.default_rng(5)
    dl = 64
    cbs = [rng.standard_normal((128, dl)), rng.standard_normal((64, dl)), rng.standard_normal((16, dl))]
    sets = [rng.standard_normal((n, dl)) for n in (0, 5, 400)]
    agg = mi.VladAggregatorMultipleVocabularies(cbs)
    assert agg.getVectorLength() == (128 + 64 + 16) * dl
    out = agg.aggregate_batch(sets)
    for i, s in enumerate(sets):
        ref = oracle.vlad_aggregate_multi(cbs, s, True)
        assert np.max(np.abs(out[i] - ref)) <= TOL, i
    # single vocabulary with normalisation: no second L2 (VladAggregatorMultipleVocabularies.java:97)
    one = mi.VladAggregatorMultipleVocabularies([cbs[0]])
    o1 = one.aggregate_batch(sets)
    for i, s in enumerate(sets):
        assert np.max(np.abs(o1[i] - oracle.vlad_aggregate_multi([cbs[0]], s, True))) <= TOL
    # zero descriptors + normalisation -> all ones / sqrt... (zero norm -> ones, Normalization.java:29-30)
    assert np.all(o1[0] == 1.0)
    agg.close()
    one.close()


@pytest.mark.parametrize("nc,ss,n,whiten", [(128, 8192, 300, True), (128, 8192, 65, False), (40, 1000, 130, True), (7, 33, 5, False)])
def test_pca_projection_mfma(mi, oracle, nc, ss, n, whiten):
    rng = np.random.default_rng(nc + ss)
    Vt = np.linalg.qr(rng.standard_normal((ss, nc)))[0].T.copy()          # orthonormal rows
    mu = 0.01 * rng.standard_normal(ss)
    eig = np.sort(rng.uniform(0.5, 4.0, nc))[::-1].copy()
    X = rng.standard_normal((n, ss)) / np.sqrt(ss)
    X[1] = mu  # projects to the zero vector: whitening then yields all ones (Normalization.java:29-30)
    pca = mi.PCA(nc, 0, ss, whiten)
    pca.load(mu, eig if whiten else None, Vt)
    Y = pca.project(X)
    Vw = oracle.pca_whiten(Vt, eig) if whiten else Vt
    for i in range(n):
        ref = oracle.pca_project(Vw, mu, X[i], whiten)
        scale = max(1.0, float(np.linalg.norm(ref)))
        assert np.max(np.abs(Y[i] - ref)) <= TOL * scale, (i, np.max(np.abs(Y[i] - ref)))
    if whiten:
        assert np.all(Y[1] == 1.0)
    # A = I check with an asymmetric B (catches a transposed C/D layout)
    y1 = pca.sampleToEigenSpace(X[0])
    assert np.array_equal(y1, Y[0])
    with pytest.raises(mi.MmidxError):
        pca.project(np.zeros((2, ss + 1)))
    pca.close()


def test_pca_layout_identity(mi):
    """Transpose-detecting check of the MFMA fragment maps: X = I-like rows against an asymmetric V_t."""
    nc, ss = 32, 48
    Vt = np.arange(nc * ss, dtype=np.float64).reshape(nc, ss) / 7.0
    pca = mi.PCA(nc, 0, ss, False)
    pca.load(np.zeros(ss), None, Vt)
    X = np.zeros((ss, ss))
    X[np.arange(ss), np.arange(ss)] = 1.0
    Y = pca.project(X)            # Y[i][c] = Vt[c][i]
    assert np.array_equal(Y, Vt.T)
    pca.close()


def test_config5_pipeline_end_to_end(mi, oracle):
    """descriptors -> VLAD -> PCA -> IVFPQ through the C ABI (BASELINE config 5, scaled down); the
    index/search half is checked bit-exactly against the oracle fed with the same projected vectors."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import config5_pipeline as c5

    out, (X, Q, iids, dists, counts, coarse, pq, cells, w, k) = c5.run(n_images=3000, n_queries=64, k=10, cells=64, w=8, verbose=False)
    assert X.shape == (3000, 128) and np.allclose(np.linalg.norm(X, axis=1), 1.0, atol=1e-12)  # whitening -> unit rows
    ref = oracle.OracleIndex(oracle.KIND_IVFPQ, 128, 16, 256, cells)
    ref.set_coarse(coarse)
    ref.set_pq(pq)
    ref.set_w(w)
    ref.add_vectors(X)
    rid, rd, rc = ref.search_batch(Q, k)
    assert np.array_equal(iids, rid) and np.array_equal(dists, rd) and np.array_equal(counts, rc)
    assert out["recall_at_1_vs_exact"] >= 0.9 and out["self_hit_rate"] >= 0.9, out


def test_fused_vectorize_equals_the_two_stages(mi):
    """mmidx_vectorize (descriptors -> VLAD -> PCA, VLAD vectors kept on the device) = aggregate_batch + project,
    bit for bit: the same two kernels run on the same data (ImageVectorization.java:169-208)."""
    rng = np.random.default_rng(42)
    nc, dl, ncomp = 32, 16, 24
    cb = rng.standard_normal((nc, dl)) / 4.0
    sets = [rng.standard_normal((n, dl)) for n in (5, 0, 300, 41, 1, 800)]
    agg = mi.VladAggregatorMultipleVocabularies([cb], normalizationsOn=True)
    ss = nc * dl
    pca = mi.PCA(ncomp, 0, ss, True)
    pca.load(rng.standard_normal(ss) * 0.01, np.linspace(3.0, 0.4, ncomp), np.linalg.qr(rng.standard_normal((ss, ncomp)))[0].T.copy())
    two = pca.project(agg.aggregate_batch(sets))
    vec = mi.frontend.ImageVectorizer(agg, pca)
    one = vec.transform_batch(sets)
    assert one.shape == (len(sets), ncomp) and np.array_equal(one, two)
    assert np.array_equal(vec.transformToVector(sets[2]), two[2])
    bad = mi.PCA(ncomp, 0, ss + 1, False)
    with pytest.raises(mi.MmidxError):
        mi.frontend.ImageVectorizer(agg, bad)
