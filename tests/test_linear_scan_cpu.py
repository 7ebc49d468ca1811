"""Linear's certified scan without a GPU: the logic (tests/linear_scan_twin.py) against the oracle, byte for byte, and the
refusals of the new entry points that are reachable before any device call."""
import ctypes as C
import importlib

import numpy as np
import pytest

from linear_scan_twin import scan_twin


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    m.build()
    return m


def _data(kind):
    rng = np.random.default_rng(5)
    n, D = 3000, 8
    X = rng.standard_normal((n, D))
    if kind == "dup":
        X[n // 2:n // 2 + 30] = X[:30]
    if kind == "equal":
        X[:] = X[0]
    Q = np.concatenate([X[rng.choice(n, 6, replace=False)] + 0.05 * rng.standard_normal((6, D)), X[:3], rng.standard_normal((3, D))])
    return X, Q


@pytest.mark.parametrize("kind", ["gauss", "dup", "equal"])
@pytest.mark.parametrize("k", [1, 10, 300])
def test_twin_equals_oracle(oracle, kind, k):
    X, Q = _data(kind)
    for qi, q in enumerate(Q):
        rid, rd = oracle.linear_search(X, q, k)
        ids, ds, info = scan_twin(X, q, k, segment=512, rng=np.random.default_rng(qi))
        assert np.array_equal(ids, rid), (kind, k, qi, info)
        assert np.array_equal(ds, rd), (kind, k, qi, info)
        if kind == "equal":
            assert info["handed_back"] == "tie"


@pytest.mark.parametrize("k", [1, 10, 300])
def test_worst_sign_drops_no_true_neighbour(oracle, k):
    """d~ = d + eps on every row: the filter value that makes a row look as far as the bound allows.  No row of the answer is
    dropped (the bytes equal the oracle's with no hand-back), although most rows are."""
    X, Q = _data("gauss")
    for qi, q in enumerate(Q[:6]):  # (the perturbed queries: no exact tie)
        rid, rd = oracle.linear_search(X, q, k)
        ids, ds, info = scan_twin(X, q, k, segment=512, sloppy="worst", eps=0.05)
        assert info["handed_back"] is None and info["dropped"] > 0
        assert np.array_equal(ids, rid) and np.array_equal(ds, rd)


def test_overflow_hands_back(oracle):
    X, Q = _data("gauss")
    rid, rd = oracle.linear_search(X, Q[0], 10)
    ids, ds, info = scan_twin(X, Q[0], 10, segment=512, eps=5.0, record_cap=8)
    assert info["handed_back"] == "overflow" and np.array_equal(ids, rid) and np.array_equal(ds, rd)


def test_new_entry_points_refuse_bad_arguments(mi):
    """null handles and null arguments are MMIDX_ERR_INVALID_ARG before any device call"""
    L = mi.lib()
    buf = (C.c_double * 8)()
    i32 = (C.c_int32 * 8)()
    p, ip = C.addressof(buf), C.addressof(i32)
    st = mi._native.LinearStats() if hasattr(mi, "_native") else importlib.import_module("multimedia-indexing_amd._native").LinearStats()
    assert L.mmidx_linear_add_device(None, 1, p, None) == 6
    assert L.mmidx_linear_search_device(None, 1, 1, p, ip, p, ip, None) == 6
    assert b"null handle" in L.mmidx_last_error()
    assert L.mmidx_linear_search_ids(None, 1, 1, ip, ip, p, ip) == 6
    assert L.mmidx_linear_copy_rows_device(None, 0, 1, p, None) == 6
    assert L.mmidx_linear_set_option(None, b"exact", 1) == 6
    assert L.mmidx_linear_get_stats(None, C.byref(st)) == 6
    assert all(v == 0.0 for v in buf) and all(v == 0 for v in i32)
    assert L.mmidx_abi_version() == 8
