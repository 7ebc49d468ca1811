"""CPU checks of the id queries (mmidx_search_ids, mmidx_reconstruct and their _device forms): the symbols,
the refusals that need no GPU, the decoder's twin (tests/decode_twin.py) by hand and against the CPU oracle, and the Java side."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import decode_twin as dt
import id_query_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["mmidx_reconstruct", "mmidx_reconstruct_device", "mmidx_search_ids", "mmidx_search_ids_device"]


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    m.build()
    return m


def test_symbols_declared_exported_and_bound(mi):
    hdr = open(os.path.join(ROOT, "include", "mmidx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nat = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), f"{name} is not declared in include/mmidx.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in nat.SIGNATURES
    assert L.mmidx_abi_version() == 8  # (adding symbols breaks no caller)
    assert len(nat.SIGNATURES["mmidx_reconstruct"][1]) == 4 and len(nat.SIGNATURES["mmidx_reconstruct_device"][1]) == 6
    assert len(nat.SIGNATURES["mmidx_search_ids"][1]) == 7 and len(nat.SIGNATURES["mmidx_search_ids_device"][1]) == 8


def test_argument_errors_without_touching_the_gpu(mi):
    """a null handle, and null arrays on a handle that is never looked into: the refusals come before any device call"""
    L = mi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert L.mmidx_reconstruct(None, 1, p, p) == 6 and b"null handle" in L.mmidx_last_error()
    assert L.mmidx_reconstruct_device(None, 1, p, p, None, None) == 6
    assert L.mmidx_search_ids(None, 3, 1, p, p, p, p) == 6 and b"null handle" in L.mmidx_last_error()
    assert L.mmidx_search_ids_device(None, 3, 1, p, p, p, p, None) == 6
    fake = (C.c_char * (1 << 20))()  # stands in for a handle: the argument checks return before they read it
    h = C.addressof(fake)
    assert L.mmidx_reconstruct(h, 1, None, p) == 6 and b"null argument" in L.mmidx_last_error()
    assert L.mmidx_reconstruct(h, 1, p, None) == 6
    assert L.mmidx_reconstruct(h, -1, p, p) == 6
    assert L.mmidx_reconstruct_device(h, 1, None, p, None, None) == 6
    assert L.mmidx_reconstruct_device(h, 1, p, None, None, None) == 6
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        assert L.mmidx_search_ids(h, 3, 1, *args) == 6 and b"null argument" in L.mmidx_last_error()
        assert L.mmidx_search_ids_device(h, 3, 1, *args, None) == 6
    assert L.mmidx_search_ids(h, 0, 1, p, p, p, p) == 6 and b"k must be in" in L.mmidx_last_error()
    assert L.mmidx_search_ids_device(h, 0, 1, p, p, p, p, None) == 6
    assert all(v == 0.0 for v in buf)


def test_hand_kat():
    """KAT-2's quantizers (tests/golden/kat_hand.json): the record (cell 0, indices [0, 1]) is the vector (0, 0, 1, 1) -- the
    residual is centroid - vector, so the codebook row (-1, -1) comes back with its sign turned.  A permutation [2, 0, 1] sends
    z = (a, b, c) to y = (b, c, a): permuted[i] = v[perm[i]], so y[perm[i]] = z[i]."""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_hand.json")))
    k2 = kat["kat2_ivfpq_residual_sign"]
    coarse, pq = np.array(k2["coarse"], np.float64), np.array(k2["pq"], np.float64)
    assert np.array_equal(coarse, [[0] * 4, [10] * 4]) and np.array_equal(pq[1], [[0, 0], [-1, -1]])
    x = dt.decode(pq, [[0, 1]], [0], coarse)
    assert np.array_equal(x, [[0.0, 0.0, 1.0, 1.0]])
    assert np.array_equal(dt.decode(pq, [[1, 1]], [1], coarse), [[9.0, 9.0, 11.0, 11.0]])
    assert np.array_equal(dt.decode(pq, [[1, 1]]), [[1.0, 1.0, -1.0, -1.0]])  # PQ: the rows themselves
    assert np.array_equal(dt.stored_to_index(np.array([[-128, -127]], np.int8)), [[0, 1]])  # PQ.java:555
    assert np.array_equal(dt.stored_to_index(np.array([[300, 7]], np.int16)), [[300, 7]])
    a, b, c = 3.0, 5.0, 7.0
    pq3 = np.array([[[a, b, c]]])  # m = 1, ks = 1, dsub = 3
    assert np.array_equal(dt.decode(pq3, [[0]], transform=dt.TR_PERMUTATION, perm=[2, 0, 1]), [[b, c, a]])
    # KAT-3's own permutation of three (seed 1) is [1, 2, 0]: y = (c, a, b), and permuting y again gives z back
    p3 = kat["kat3_jdk"]["perm_seed1_dim3"]
    y = dt.decode(pq3, [[0]], transform=dt.TR_PERMUTATION, perm=p3)
    assert np.array_equal(y, [[c, a, b]]) and np.array_equal(y[0][p3], [a, b, c])
    # rotation by a quarter turn R = [[0, 1], [-1, 0]]: rotated = v R = (-v1, v0), so z = (1, 2) came from y = (2, -1)
    R = np.array([[0.0, 1.0], [-1.0, 0.0]])
    y = dt.decode(np.array([[[1.0, 2.0]]]), [[0]], transform=dt.TR_ROTATION, rot=R)
    assert np.array_equal(y, [[2.0, -1.0]]) and np.array_equal(y[0] @ R, [1.0, 2.0])


@pytest.mark.parametrize("name,kind,D,C_,m,ks,n,k,tr,seed", cases.TABLE, ids=[c[0] for c in cases.TABLE])
def test_twin_against_the_oracle(oracle, name, kind, D, C_, m, ks, n, k, tr, seed):
    """Every decoded record sits on top of its own code: searched for, with every list probed, it comes first, at a distance that
    is rounding residue, and nothing in the top k + 1 ties.  200 random ids per shape."""
    p = cases.problem(seed, kind, D, C_, m, ks, n, tr)
    ref, perm = cases.oracle_index(oracle, p, kind, D, C_, m, ks, tr)
    ref.add_vectors(p["base"])
    rng = np.random.default_rng(D)
    ids = rng.choice(n, 200, replace=False)
    recs = [ref.get_record(int(i)) for i in ids]
    cells = np.array([r[0] for r in recs])
    stored = np.array([r[1] for r in recs]).astype(np.int8 if ks <= 256 else np.int16)
    X = dt.decode(p["pq"], dt.stored_to_index(stored), cells, p["coarse"], tr, perm, p["rot"])
    worst = 0.0
    for iid, x in zip(ids, X):
        got, d = ref.search(x, k + 1)
        assert got[0] == iid
        assert 0.0 <= d[0] <= 1e-24
        assert not synth_tie(d)
        worst = max(worst, d[0])
    print(f"{name}: largest own distance {worst:.3g}")


def synth_tie(d):
    d = np.asarray(d)
    return bool(np.any(d[1:] == d[:-1]))


def test_java_side_declares_and_uses_the_natives():
    jdir = os.path.join(ROOT, "multimedia-indexing_amd", "jni", "java", "gr", "iti", "mklab", "visual", "datastructures")
    nat = open(os.path.join(jdir, "MmidxNative.java")).read()
    assert re.search(r"native void searchIds\(", nat) and re.search(r"native void reconstruct\(", nat)
    ivf = open(os.path.join(jdir, "GpuIVFPQ.java")).read()
    hook = ivf[ivf.index("computeNearestNeighborsInternal(int k, int iid)"):]
    hook = hook[:hook.index("\n\t}\n")]
    assert "return null" not in hook and "MmidxNative.searchIds(" in hook
    assert "reconstructVector(String id)" in ivf
    assert "reconstructVector(String id)" in open(os.path.join(jdir, "GpuPQ.java")).read()
    shim = open(os.path.join(ROOT, "multimedia-indexing_amd", "jni", "mmidx_jni.c")).read()
    assert "JFN(searchIds)" in shim and "JFN(reconstruct)" in shim
