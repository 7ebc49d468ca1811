"""GPU parity of the re-indexing walk (mmidx_truncate_l2_device, mmidx_linear_reindex, Linear.reindex; csrc/mmidx_reindex.h,
DESIGN.md section 5.12).  The yardstick is tests/reindex_twin.py (np_twin.normalize_l2 row by row, itself compared with the oracle
in tests/test_reindex_cpu.py), the oracle's encoder for the compressed targets and tests/refine_twin.py for the re-ranking at the
end.  Every comparison of vectors is np.array_equal on uint64 views: there is no tolerance in this file."""
import ctypes as C
import importlib

import numpy as np
import pytest

import build_cases as bc
import id_query_cases as cases
import refine_twin as rt
import reindex_twin as rx

pytestmark = pytest.mark.gpu


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


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
def run_kernel(mi, X, ncols, lens, modes, skew=0):
    """X [n][ld] on the host -> the targets as the device wrote them.  The columns from max(lens) on (the padding up to ld included)
    are NaN on the device: this shows that none of them reaches an output or a norm.  That they are never LOADED, as the contract
    says, no test can see; the kernel's `c < L` guards establish it.  Every output has a guard row behind it.  skew = 1: the rows
    start 8 bytes off a 16-byte boundary."""
    import torch

    n, ld = X.shape
    dev = X.copy()
    dev[:, max(lens):] = np.nan
    flat = torch.empty(n * ld + 2, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    dX = flat[skew:skew + n * ld]
    dX.copy_(torch.from_numpy(dev.reshape(-1)))
    outs = [torch.full((n + 1, T), -7.5, dtype=torch.float64, device="cuda") for T in lens]
    ptrs = (C.c_void_p * len(lens))(*[o.data_ptr() for o in outs])
    la, ma = np.array(lens, np.int32), np.array(modes, np.int32)
    st = torch.cuda.current_stream().cuda_stream
    rc = mi.lib().mmidx_truncate_l2_device(0, n, ncols, ld, dX.data_ptr(), len(lens), la.ctypes.data, ma.ctypes.data, C.addressof(ptrs), st)
    assert rc == 0, mi.lib().mmidx_last_error()
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h in host:
        assert (h[n] == -7.5).all()  # nothing behind the last row
    return [h[:n] for h in host]


# (n, ncols, ld, lens, modes, skew); the first six are the specified shapes; then every size at which the host picks another form: 128 / 129
# columns (rows kept in LDS / streamed twice), 288 / 289 (the last length that could be kept, see the forced forms below), an odd ld and
# a base off the 16-byte boundary (8-byte loads), 64 / 65 rows (one block / two)
KERNEL_CASES = [
    (1, 1, 1, [1], [1], 0),
    (67, 40, 40, [40, 33, 32, 31, 1], [2, 2, 1, 0, 1], 0),
    (130, 130, 136, [130, 129, 128], [2, 2, 1], 0),
    (130, 1024, 1024, [1024, 512, 96], [1, 2, 2], 0),
    (5, 4096, 4100, [2048, 3], [2, 2], 0),
    (200, 24, 24, [24, 23, 17, 16, 12, 8, 2, 1], [2, 2, 1, 0, 2, 1, 2, 1], 0),
    (70, 140, 140, [128, 5], [2, 1], 0),
    (70, 140, 140, [129, 5], [2, 1], 0),
    (70, 300, 300, [288, 5], [2, 1], 0),
    (70, 300, 300, [289, 5], [2, 1], 0),
    (67, 40, 41, [40, 7], [1, 2], 0),
    (67, 40, 40, [39, 33], [2, 2], 1),
    (64, 34, 34, [34, 13], [1, 1], 0),
    (65, 34, 34, [34, 13], [1, 1], 0),
]


@pytest.mark.parametrize("n,ncols,ld,lens,modes,skew", KERNEL_CASES, ids=[f"{c[0]}x{c[1]}ld{c[2]}t{len(c[3])}max{max(c[3])}s{c[5]}" for c in KERNEL_CASES])
def test_kernel_against_the_twin(mi, n, ncols, ld, lens, modes, skew):
    rng = np.random.default_rng(n * 7919 + ncols)
    X = rng.standard_normal((n, ld))
    r0 = None
    if n >= rx.EDGE_ROWS and ncols >= 2:
        r0 = rx.plant_edge_rows(X[:, :ncols], 1 if n > rx.EDGE_ROWS else 0)
    got = run_kernel(mi, X, ncols, lens, modes, skew)
    want = rx.truncate_l2(X[:, :ncols], lens, modes)
    for t, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero((np.ascontiguousarray(g).view(np.uint64) != w.view(np.uint64)).any(axis=1))[0]
        assert bad.size == 0, f"target {t} (length {lens[t]}, mode {modes[t]}): rows {bad[:8].tolist()} differ"
        if not rx.normalises(lens[t], ncols, modes[t]):
            assert rx.same_bits(g, X[:, :lens[t]])  # a bit copy
    if (n, ncols) == (67, 40) and skew == 0 and ld == 40:
        # the row that is zero up to a shorter target's length and not within a longer one: its two targets part ways
        one, longer = got[lens.index(1)], got[lens.index(32)]
        assert one[r0, 0] == 1.0 and longer[r0, 0] == 0.0 and (longer[r0, 12:] != 0.0).all()
        assert rx.same_bits(got[0], X[:, :40])  # the full-length mode-2 target


def test_kernel_forms_forced(mi, monkeypatch):
    """Rows of 129 .. 288 columns could stay in LDS (one block per CU) and are streamed by default; MMIDX_TRL_CACHED_MAX moves the
    limit.  Both forms give the twin's bits at L = 200, and at 288 / 289, the last length that fits and the first that does not."""
    rng = np.random.default_rng(200)
    X = rng.standard_normal((70, 300))
    rx.plant_edge_rows(X, 1)
    modes = [2, 1, 2]
    for lens in ([200, 130, 12], [288, 130, 12], [289, 130, 12]):
        want = rx.truncate_l2(X, lens, modes)
        for limit in (None, "288", "0"):
            if limit is None:
                monkeypatch.delenv("MMIDX_TRL_CACHED_MAX", raising=False)
            else:
                monkeypatch.setenv("MMIDX_TRL_CACHED_MAX", limit)
            for g, w in zip(run_kernel(mi, X, 300, lens, modes), want):
                assert rx.same_bits(g, w), (lens, limit)


# ---- the walk --------------------------------------------------------------------------------------------------------------------
def walk(mi, src, iid0, n, targets, modes, chunk=0, pca=None):
    """mmidx_linear_reindex on the mirrors' handles; returns the status"""
    kinds = np.array([0 if isinstance(t, mi.Linear) else 1 for t in targets], np.int32)
    hs = (C.c_void_p * len(targets))(*[t._h for t in targets])
    ma = np.array(modes, np.int32)
    return mi.lib().mmidx_linear_reindex(src._h, iid0, n, pca._h if pca is not None else None, len(targets), kinds.ctypes.data, C.addressof(hs),
                                         ma.ctypes.data, chunk)


def source(mi, X, cap=None):
    src = mi.Linear(X.shape[1], cap or len(X))
    src._add_vectors(X, None)
    return src


def rows_of(lin, ids):
    return np.stack([lin.getVector(int(i)) for i in ids])


def test_walk_small(mi):
    """D = 24, n = 300 in chunks of 128 (two full ones and a partial one) into Linear 24 and Linear 10, mode 2"""
    rng = np.random.default_rng(24)
    X = rng.standard_normal((300, 24))
    rx.plant_edge_rows(X, 126)  # (across the first chunk boundary)
    src, t24, t10 = source(mi, X), mi.Linear(24, 300), mi.Linear(10, 300)
    assert walk(mi, src, 0, 300, [t24, t10], [2, 2], 128) == 0, mi.lib().mmidx_last_error()
    assert t24.size() == 300 and t10.size() == 300 and src.size() == 300
    w24, w10 = rx.truncate_l2(X, [24, 10], [2, 2])
    assert rx.same_bits(rows_of(t24, range(300)), w24) and rx.same_bits(w24, X)
    assert rx.same_bits(rows_of(t10, range(300)), w10)
    assert rx.same_bits(rows_of(src, range(300)), X)  # the source is untouched
    # the targets search like any Linear index: a stored row finds itself
    ii, dd, cc = t10.search_batch(1, w10[200:204])
    assert ii[:, 0].tolist() == [200, 201, 202, 203] and (dd[:, 0] == 0.0).all()
    for ix in (src, t24, t10):
        ix.close()


def test_walk_past_the_small_path(mi):
    """n = 20000, D = 8 -> 5: source and target are beyond Linear's 16384-row small path (no host mirror)"""
    n, chunk = 20000, 4096
    rng = np.random.default_rng(8)
    X = rng.standard_normal((n, 8))
    src, t5 = source(mi, X), mi.Linear(5, n)
    assert walk(mi, src, 0, n, [t5], [2], chunk) == 0, mi.lib().mmidx_last_error()
    assert t5.size() == n
    edges = [r for c0 in range(0, n, chunk) for r in (c0, min(c0 + chunk, n) - 1)]
    ids = np.unique(np.concatenate([rng.choice(n, 512, replace=False), edges]))
    assert rx.same_bits(rows_of(t5, ids), rx.truncate_l2(X[ids], [5], [2])[0])
    src.close()
    t5.close()


def quantized_case(kind, tr, n=500):
    """a 24-long source, the twin's 16-long vectors and codebooks over 16 dimensions: m = 4, ks = 16, C = 8"""
    p = cases.problem(160 + 10 * kind + tr, kind, 16, 8, 4, 16, 600, tr)
    X = np.random.default_rng(1600 + tr).standard_normal((n, 24))
    Y = rx.truncate_l2(X, [16], [2])[0]
    return p, X, Y


@pytest.mark.parametrize("tr", [cases.TR_NONE, cases.TR_ROTATION, cases.TR_PERMUTATION], ids=["none", "rot", "perm"])
@pytest.mark.parametrize("kind", [cases.KIND_PQ, cases.KIND_IVFPQ], ids=["pq", "ivfpq"])
def test_walk_into_pq_and_ivfpq(mi, oracle, kind, tr):
    """T = 16 of D = 24: the target's export equals that of a handle filled by mmidx_add_vectors with the twin's vectors, and the
    records the oracle makes of those vectors; then (ivfpq) mmidx_search_refine over the Linear 16 and the IVFPQ 16 of the same walk"""
    n = 500
    p, X, Y = quantized_case(kind, tr, n)
    nl = 8 if kind == cases.KIND_IVFPQ else 1
    src = source(mi, X)
    ix = bc.make_index(mi, kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])
    lin16 = mi.Linear(16, n)
    assert walk(mi, src, 0, n, [lin16, ix], [2, 2], 192) == 0, mi.lib().mmidx_last_error()
    assert ix.size() == n and lin16.size() == n
    got = ix.export()
    # a second handle, filled the old way with the twin's vectors
    ix2 = bc.make_index(mi, kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])
    ix2._add_vectors(Y, np.arange(n, dtype=np.int32))
    for a, b in zip(got, ix2.export()):
        assert np.array_equal(a, b)
    # the oracle's records of the same vectors
    ref, _ = bc.oracle_index(kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])
    cells, codes = ref.encode_batch(Y)
    for a, b in zip(got, bc.expected_export(cells, codes, np.arange(n), nl, 16)):
        assert np.array_equal(a, b)
    assert rx.same_bits(rows_of(lin16, range(n)), Y)
    if kind == cases.KIND_IVFPQ:
        ix.setW(8)
        ref.set_w(8)
        ref.load_lists(*got)
        rng = np.random.default_rng(5)
        Q = Y[rng.integers(0, n, 20)] + 0.02 * rng.standard_normal((20, 16))
        k, R = 5, 40
        want = rt.refine_batch(ref.search_batch(Q, R), Y, Q, k)
        res = ix.search_refine_batch(k, R, Q, lin16)
        assert want[3] == 0 and int(res[3]) == 0
        assert np.array_equal(res[2], want[2]) and np.array_equal(res[0], want[0])
        assert np.array_equal(res[1].view(np.uint64), want[1].view(np.uint64))
    for h in (src, ix, ix2, lin16):
        h.close()


@pytest.mark.parametrize("whitening", [False, True], ids=["plain", "whitened"])
def test_walk_through_a_pca(mi, whitening):
    """ss = 24, nc = 12 into Linear 12 / 8 / 4: the rows equal the twin applied to mmidx_pca_project's output for the same rows"""
    rng = np.random.default_rng(12)
    n = 300
    X = rng.standard_normal((n, 24)) @ rng.standard_normal((24, 24))
    Vt = np.linalg.qr(rng.standard_normal((24, 24)))[0][:12]
    means, eig = X.mean(0), np.linspace(9.0, 0.5, 12)
    pca = mi.PCA(12, 1, 24, whitening)
    pca.load(means, eig, Vt)
    P = pca.project(X)
    src = source(mi, X)
    for modes in ([0, 0, 0], [1, 1, 1], [0, 1, 0]):
        tg = [mi.Linear(T, n) for T in (12, 8, 4)]
        assert walk(mi, src, 0, n, tg, modes, 128, pca) == 0, mi.lib().mmidx_last_error()
        for t, w in zip(tg, rx.truncate_l2(P, [12, 8, 4], modes)):
            assert t.size() == n and rx.same_bits(rows_of(t, range(n)), w), modes
            t.close()
    src.close()
    pca.close()


def test_incremental_walk(mi):
    """rows [0, 200), 100 more rows into the source, rows [200, 300): the same targets as one walk of 300"""
    kind, tr = cases.KIND_IVFPQ, cases.TR_NONE
    p, X, Y = quantized_case(kind, tr, 300)

    def targets():
        return mi.Linear(16, 300), bc.make_index(mi, kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])

    src = mi.Linear(24, 300)
    src._add_vectors(X[:200], None)
    la, ia = targets()
    assert walk(mi, src, 0, 200, [la, ia], [2, 2], 64) == 0, mi.lib().mmidx_last_error()
    src._add_vectors(X[200:], None)
    assert walk(mi, src, 0, 100, [la, ia], [2, 2], 64) == 6 and b"holds 200 records, iid0 = 0" in mi.lib().mmidx_last_error()
    assert walk(mi, src, 200, 100, [la, ia], [2, 2], 64) == 0, mi.lib().mmidx_last_error()
    lb, ib = targets()
    assert walk(mi, src, 0, 300, [lb, ib], [2, 2], 0) == 0, mi.lib().mmidx_last_error()
    assert rx.same_bits(rows_of(la, range(300)), rows_of(lb, range(300))) and rx.same_bits(rows_of(la, range(300)), Y)
    for a, b in zip(ia.export(), ib.export()):
        assert np.array_equal(a, b)
    for h in (src, la, ia, lb, ib):
        h.close()


def test_refusals_on_live_handles(mi):
    """every refusal leaves every target's size as it was; n = 0 is fine after the checks"""
    L = mi.lib()
    kind, tr = cases.KIND_IVFPQ, cases.TR_NONE
    p, X, Y = quantized_case(kind, tr, 100)
    src = source(mi, X)
    lin16, lin16b, lin30 = mi.Linear(16, 100), mi.Linear(16, 100), mi.Linear(30, 100)
    held = mi.Linear(16, 100)
    held._add_vectors(Y[:1], None)
    small = mi.Linear(16, 40)  # room for 40 vectors
    ix = bc.make_index(mi, kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])
    bare = mi.IVFPQ(16, 100, False, "", 4, 16, tr, 8, 512)  # no codebooks
    sh = mi.IVFPQ(16, 100, False, "", 4, 16, tr, 8, 512, devices=[0])  # one virtual shard
    sh.loadCoarseQuantizer(p["coarse"])
    sh.loadProductQuantizer(p["pq"])
    pca9 = mi.PCA(4, 1, 9, False)
    pca9.load(np.zeros(9), np.ones(4), np.eye(9)[:4])
    everyone = {"lin16": (lin16, 0), "lin16b": (lin16b, 0), "lin30": (lin30, 0), "held": (held, 1), "small": (small, 0), "ix": (ix, 0), "bare": (bare, 0),
                "sh": (sh, 0), "src": (src, 100)}

    def refused(status, text, *a, **kw):
        rc = walk(mi, src, *a, **kw)
        msg = L.mmidx_last_error()
        assert rc == status and text in msg, (rc, msg)
        for name, (h, size) in everyone.items():
            assert h.size() == size, name

    refused(6, b"holds vectors of length 30, the walk delivers 24", 0, 100, [lin16, lin30], [2, 2])      # longer than the source
    refused(6, b"targets[1] holds 1 records, iid0 = 0", 0, 100, [lin16, held], [2, 2])                   # already holds a row
    refused(6, b"100 rows from row 50 are asked for, the source holds 100", 50, 100, [lin16], [2])       # past the source
    refused(6, b"rows from row 4611686018427387904 are asked for", 2 ** 62, 2 ** 62, [lin16], [2])       # (iid0 + n would overflow)
    refused(6, b"samples of length 9, the source holds vectors of length 24", 0, 100, [lin16], [2], pca=pca9)
    refused(6, b"are the same handle", 0, 100, [lin16, ix, lin16], [2, 2, 2])                            # the same target twice
    refused(6, b"targets[1] is the source handle", 0, 100, [lin16, src], [2, 2])                         # the source among the targets
    refused(7, b"targets[1] has no codebooks yet", 0, 100, [lin16, bare], [2, 2])                        # NOT_READY
    refused(10, b"targets[1] is a sharded handle", 0, 100, [lin16, sh], [2, 2])                          # UNSUPPORTED
    refused(6, b"targets[1] has room for 40 more vectors, n = 100", 0, 100, [lin16, small], [2, 2])      # capacity
    # n = 0 after the checks; and the handles still work
    assert walk(mi, src, 0, 0, [lin16, ix], [2, 2]) == 0
    assert walk(mi, src, 100, 0, [held], [2]) == 6  # (the identity check holds for n = 0 too)
    assert lin16.size() == 0 and ix.size() == 0
    assert walk(mi, src, 0, 100, [lin16, ix, lin16b], [2, 2, 0]) == 0, L.mmidx_last_error()
    assert rx.same_bits(rows_of(lin16, range(100)), Y) and ix.size() == 100
    assert rx.same_bits(rows_of(lin16b, range(100)), X[:, :16])  # mode 0: the bit copy of the truncation
    for h in (src, lin16, lin16b, lin30, held, small, ix, bare, sh):
        h.close()
    pca9.close()


def test_walk_beside_refine_calls(mi):
    """An index that grows is brought up to date walk by walk while another thread re-ranks over the same pair: the two calls take
    the index handle before the Linear handle, both of them, so neither waits for the other for ever; and because a walk holds
    both targets from its checks to its last append, a refine call always sees the pair at one size: nothing is ever missing."""
    import threading

    kind, tr, n, step = cases.KIND_IVFPQ, cases.TR_NONE, 2000, 200
    p, X, Y = quantized_case(kind, tr, n)
    src = source(mi, X)
    lin16 = mi.Linear(16, n)
    ix = bc.make_index(mi, kind, 16, 4, 16, 8, tr, p["coarse"], p["pq"], p["rot"])
    ix.setW(8)
    assert walk(mi, src, 0, step, [lin16, ix], [2, 2]) == 0, mi.lib().mmidx_last_error()
    Q = Y[:16] + 0.01
    errors, missing = [], []

    def walker():
        try:
            for i0 in range(step, n, step):
                rc = walk(mi, src, i0, step, [lin16, ix], [2, 2], 64)  # (the Linear target first in the argument list)
                if rc:
                    errors.append((i0, rc, mi.lib().mmidx_last_error()))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def refiner():
        try:
            for _ in range(40):
                missing.append(int(ix.search_refine_batch(5, 40, Q, lin16)[3]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=f, daemon=True) for f in (walker, refiner, refiner)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "the walk and the refine calls wait for each other"
    assert errors == [] and len(missing) == 80 and set(missing) == {0}
    assert lin16.size() == n and ix.size() == n and rx.same_bits(rows_of(lin16, range(0, n, 7)), Y[::7])
    for h in (src, lin16, ix):
        h.close()


# ---- the Python face -------------------------------------------------------------------------------------------------------------
def test_python_face_carries_the_ids(mi):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((120, 24))
    ids = [f"img{i}" for i in range(120)]
    src = mi.Linear(24, 200)
    assert src.indexVectors(ids[:80], X[:80]) == 80
    t10, t24 = mi.Linear(10, 200), mi.Linear(24, 200)
    assert src.reindex([t10, t24], chunk_rows=64) == 80
    assert t10.loadCounter == 80 and t24.getLoadCounter() == 80 and t10.size() == 80
    assert [t10.getId(i) for i in range(80)] == ids[:80] and all(t24.getInternalId(ids[i]) == i for i in range(80))
    # the source grows: the second call brings the targets up to date
    assert src.indexVectors(ids[80:], X[80:]) == 40
    assert mi.IndexTransformation.transform(src, t10) == 40
    assert t10.loadCounter == 120 and t10.getId(119) == "img119" and t10.getInternalId("img100") == 100
    assert rx.same_bits(rows_of(t10, range(120)), rx.truncate_l2(X, [10], [2])[0])
    ans = t10.computeNearestNeighbors(1, t10.getVector(90))
    assert ans.getIds() == ["img90"]
    # refusals before the native call: the maps and the counters stay as they were
    dup = mi.Linear(10, 200)
    assert dup.indexVector("img5", np.ones(10))
    with pytest.raises(mi.MmidxError, match="Vector 'img5' already indexed!"):
        src.reindex([dup], iid0=1, n=10)
    with pytest.raises(mi.MmidxError, match="Vector 'img5' already indexed!"):
        src.reindex([dup])
    full = mi.Linear(10, 100)
    with pytest.raises(mi.MmidxError, match="Maximum index capacity reached, no more vectors can be indexed!"):
        src.reindex([full])
    with pytest.raises(mi.MmidxError, match="different numbers of vectors"):
        src.reindex([t10, t24])
    for t, size in ((dup, 1), (full, 0), (t24, 80), (t10, 120)):
        assert t.loadCounter == size and t.size() == size and len(t._iid_to_id) == size and len(t._id_to_iid) == size
    for h in (src, t10, t24, dup, full):
        h.close()


def test_pca_projection_driver(mi):
    rng = np.random.default_rng(4)
    X = rng.standard_normal((90, 24))
    pca = mi.PCA(12, 1, 24, False)
    pca.load(X.mean(0), np.ones(12), np.linalg.qr(rng.standard_normal((24, 24)))[0][:12])
    full = mi.Linear(24, 90)
    full.indexVectors([str(i) for i in range(90)], X)
    proj = [mi.Linear(T, 90) for T in (4, 8, 12)]
    assert mi.PCAProjection.project(full, pca, proj, L2Normalization=True) == 90
    for t, w in zip(proj, rx.truncate_l2(pca.project(X), [4, 8, 12], [1, 1, 1])):
        assert t.loadCounter == 90 and t.getId(89) == "89" and rx.same_bits(rows_of(t, range(90)), w)
        t.close()
    full.close()
    pca.close()
