"""Linear beyond the small path on the GPU: HBM-resident rows and the certified scan, against the oracle byte
for byte -- ids, distance bits and counts with np.array_equal in every case, ties included."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

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


_DATA = {}
_WANT = {}


def _data(n, D, dup=False, scale=1.0):
    """the recipe of test_linear_exact_search: Gaussian rows, optionally 30 duplicated; 20 stored rows + noise, 4 verbatim, 8 random"""
    key = (n, D, dup, scale)
    if key not in _DATA:
        rng = np.random.default_rng(n)
        X = rng.standard_normal((n, D))
        if dup:
            X[n // 2:n // 2 + 30] = X[:30]
        Q = np.concatenate([X[rng.choice(n, 20, replace=False)] + 0.05 * rng.standard_normal((20, D)), X[:4], rng.standard_normal((8, D))])
        X, Q = X * scale, Q * scale
        X.setflags(write=False)
        Q.setflags(write=False)
        _DATA[key] = (X, Q)
    return _DATA[key]


def _want(oracle, n, D, k, dup=False, scale=1.0):
    key = (n, D, k, dup, scale)
    if key not in _WANT:
        X, Q = _data(n, D, dup, scale)
        _WANT[key] = oracle.linear_search_batch(X, Q, k, nthreads=8)
    return _WANT[key]


def _tied(oracle, n, D, k, dup):
    """queries whose k-th and (k+1)-th oracle distances are equal"""
    _, d1, c1 = _want(oracle, n, D, k + 1, dup)
    return [q for q in range(len(c1)) if c1[q] == k + 1 and d1[q, k - 1] == d1[q, k]]


def _filled(mi, X, cap=None):
    ix = mi.Linear(X.shape[1], cap or X.shape[0] + 8)
    ix._add_vectors(X, None)
    return ix


def _same(got, want):
    assert np.array_equal(got[2], want[2]), "counts"
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]


SHAPES = [(16385, 128, 10), (20011, 24, 100), (50000, 128, 1), (33000, 64, 300), (3000, 16, 400), (20000, 1024, 5), (20000, 16, 1500)]


@pytest.mark.parametrize("n,D,k", SHAPES)
def test_scan_parity(mi, oracle, n, D, k):
    """tie-free Gaussian data: the scan serves every query itself (a hand-back here would be the scan hiding behind the exact path)"""
    X, Q = _data(n, D)
    assert _tied(oracle, n, D, k, False) == []  # confirmed on the CPU: no query has d_k == d_{k+1}
    ix = _filled(mi, X)
    got = ix.search_batch(k, Q)
    st = ix.get_stats()
    print(st)
    _same(got, _want(oracle, n, D, k))
    assert st["path"] == 3 and st["redo_queries"] == 0, st
    assert st["rows_scanned"] == n and (st["segments"] > 0) == (n > max(k + 1, 1024))
    ix.close()


@pytest.mark.parametrize("n,D,k", [(20011, 24, 100), (50000, 128, 1)])
def test_ties_are_handed_back_exactly(mi, oracle, n, D, k):
    X, Q = _data(n, D, dup=True)
    F = _tied(oracle, n, D, k, True)
    if k == 1:
        assert set(range(20, 24)) <= set(F)  # the verbatim queries: the row and its duplicate at distance 0
    ix = _filled(mi, X)
    got = ix.search_batch(k, Q)
    st = ix.get_stats()
    _same(got, _want(oracle, n, D, k, dup=True))
    assert st["path"] == 3 and st["redo_queries"] == len(F), (st, F)
    ix.close()


def test_forced_overflow_and_exact_switch(mi, oracle):
    n, D, k = 20011, 24, 100
    X, Q = _data(n, D)
    want = _want(oracle, n, D, k)
    ix = _filled(mi, X)
    ix.set_option("mfma_qcap", 64)
    _same(ix.search_batch(k, Q), want)
    assert ix.get_stats()["redo_queries"] > 0
    ix.set_option("mfma_qcap", 0)
    scan = ix.search_batch(k, Q)
    _same(scan, want)
    st = ix.get_stats()
    assert st["redo_queries"] == 0 and st["path"] == 3 and st["survivors"] > 0
    ix.set_option("exact", 1)
    exact = ix.search_batch(k, Q)
    assert ix.get_stats()["path"] == 2
    for a, b in zip(exact, scan):
        assert a.tobytes() == b.tobytes()
    ix.set_option("exact", 0)
    ix.set_option("debug_sync", 1)
    _same(ix.search_batch(k, Q), want)
    st = ix.get_stats()
    assert st["scan_ms"] > 0 and st["verify_ms"] > 0
    with pytest.raises(mi.MmidxError) as ei:
        ix.set_option("no_such_option", 1)
    assert ei.value.status == 6
    ix.close()


@pytest.mark.parametrize("scale", [1e-25, 1e140])
def test_magnitudes_outside_the_filter(mi, oracle, scale):
    """fp32 squares are all zero / all infinite: the norm guard certifies nothing and the exact path serves every query"""
    n, D, k = 20011, 24, 10
    X, Q = _data(n, D, scale=scale)
    ix = _filled(mi, X)
    got = ix.search_batch(k, Q)
    st = ix.get_stats()
    _same(got, _want(oracle, n, D, k, scale=scale))
    assert st["path"] == 3 and st["redo_queries"] == len(Q), st
    ix.close()


def test_growth(mi, oracle):
    D, k = 32, 10
    rng = np.random.default_rng(99)
    X = rng.standard_normal((20005, D))
    Q = np.concatenate([X[[5, 9000, 12000, 19990, 20003]] + 0.01 * rng.standard_normal((5, D)), rng.standard_normal((6, D))])
    ix = mi.Linear(D, 30000)
    ix._add_vectors(X[:10000], None)
    _same(ix.search_batch(k, Q), oracle.linear_search_batch(X[:10000], Q, k))
    assert ix.get_stats()["path"] == 1 and ix.get_stats()["uploaded_rows"] == 10000
    ix._add_vectors(X[10000:20000], None)
    got = ix.search_batch(k, Q)
    _same(got, oracle.linear_search_batch(X[:20000], Q, k))
    assert ix.get_stats()["path"] == 3 and (got[0] >= 10000).any()
    ix._add_vectors(X[20000:], None)
    assert ix.get_stats()["uploaded_rows"] == 5 and ix.size() == 20005
    got = ix.search_batch(k, Q)
    _same(got, oracle.linear_search_batch(X, Q, k))
    assert (got[0] >= 20000).any()
    # the host mirror is gone: rows come back from HBM
    assert ix.getVector(3).tobytes() == X[3].tobytes() and ix.getVector(20004).tobytes() == X[20004].tobytes()
    ix.close()


def test_device_entry_points(mi, oracle):
    import torch

    n, D, k = 20011, 24, 100
    X, Q = _data(n, D)
    host = _filled(mi, X)
    want = host.search_batch(k, Q)
    _same(want, _want(oracle, n, D, k))
    dev = mi.Linear(D, n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dX = torch.from_numpy(np.array(X)).cuda()
        dev.add_device(dX[:9000])   # (small: the mirror is filled from the device)
        dev.add_device(dX[9000:])
        assert dev.get_stats()["uploaded_rows"] == n - 9000
        dQ = torch.from_numpy(np.array(Q)).cuda()
        ti, td, tc = dev.search_batch_device(k, dQ)
        rows = dev.copy_rows_device(8990, torch.empty((40, D), dtype=torch.float64, device="cuda"))
    s.synchronize()
    for a, b in zip((ti, td, tc), want):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    assert rows.cpu().numpy().tobytes() == X[8990:9030].tobytes()
    assert dev.size() == n and dev.getVector(17).tobytes() == X[17].tobytes()
    ids = np.array([0, 17, 10005, n - 1, 17], np.int32)
    by_id = dev.search_ids_batch(k, ids)
    by_vec = host.search_batch(k, X[ids])
    for a, b in zip(by_id, by_vec):
        assert a.tobytes() == b.tobytes()
    a, b = dev.computeNearestNeighborsInternalById(3, 11)
    assert a[0] == 11 and b[0] == 0.0
    for bad in (-1, n):
        with pytest.raises(mi.MmidxError) as ei:
            dev.search_ids_batch(k, [3, bad])
        assert ei.value.status == 6 and "out of range" in str(ei.value)
    _same(dev.search_batch(k, Q), want)  # still usable
    host.close()
    dev.close()


def test_concurrent_single_query_callers(mi, oracle):
    n, D, k = 20011, 24, 10
    X, Q = _data(n, D)
    want = _want(oracle, n, D, k)
    ix = mi.Linear(D, n)
    assert ix.indexVectors([f"v{i}" for i in range(n)], X) == n
    errors = []
    start = threading.Barrier(8)

    def worker(t):
        try:
            start.wait()
            for rep in range(4):
                q = (t * 4 + rep) % len(Q)
                ans = ix.computeNearestNeighbors(k, Q[q])
                if ans.getIds() != [f"v{i}" for i in want[0][q]] or not np.array_equal(ans.getDistances(), want[1][q]):
                    errors.append((t, rep, q))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []
    ix.close()
