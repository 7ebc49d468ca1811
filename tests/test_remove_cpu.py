"""CPU checks of the removal (mmidx_remove, mmidx_remove_device): the numpy twin against the CPU oracle --
which pins "as if never added" --, the symbols and the refusals that need no GPU, the mirror's id maps, and the Java side."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import decode_twin as dt
import id_query_cases as cases
import remove_twin as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [cases.TABLE[0], cases.EXTRA[0], cases.EXTRA[2]]  # d16, d24_perm, pq32
assert [r[0] for r in ROWS] == ["d16", "d24_perm", "pq32"]


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    m.build()
    return m


def test_twin_by_hand():
    """three lists (2, 0 and 3 records), the id 7 stored twice in two lists"""
    off = np.array([0, 2, 2, 5], np.int64)
    iids = np.array([4, 7, 1, 7, 9], np.int32)
    codes = np.arange(10, dtype=np.int8).reshape(5, 2)
    o2, i2, c2, found, removed = rt.filter_export(off, iids, codes, [7, 7, -3, 100, 4, 5])
    assert np.array_equal(o2, [0, 0, 0, 2]) and np.array_equal(i2, [1, 9]) and np.array_equal(c2, [[4, 5], [8, 9]])
    assert np.array_equal(found, [1, 1, 0, 0, 1, 0]) and removed == 3
    o3, i3, c3, found, removed = rt.filter_export(off, iids, codes, [])
    assert np.array_equal(o3, off) and np.array_equal(i3, iids) and np.array_equal(c3, codes) and removed == 0 and found.shape == (0,)
    o4, i4, _, _, removed = rt.filter_export(off, iids, codes, iids)
    assert np.array_equal(o4, [0, 0, 0, 0]) and len(i4) == 0 and removed == 5
    assert np.array_equal(rt.list_of_position(off, 5), [0, 0, 2, 2, 2])


@pytest.mark.parametrize("dup", [1, 2])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_filtered_lists_answer_as_if_never_added(oracle, row, dup):
    """The oracle loaded with the twin's filtered lists answers exactly as an oracle to which only the survivors were ever added,
    in arrival order (under their ids).  With dup = 2 every vector is there twice, so equal distances are everywhere and the
    order inside the lists decides the answers."""
    name, kind, D, C_, m, ks, n, k, tr, seed = row
    p = cases.problem(seed, kind, D, C_, m, ks, n, tr, dup)
    n = len(p["base"])
    full, _ = cases.oracle_index(oracle, p, kind, D, C_, m, ks, tr)
    full.add_vectors(p["base"])
    recs = [full.get_record(i) for i in range(n)]
    cells = np.array([max(r[0], 0) for r in recs], np.int32)
    stored = np.array([r[1] for r in recs]).astype(np.int8 if ks <= 256 else np.int16)
    nl = C_ if kind == cases.KIND_IVFPQ else 1
    order = np.argsort(cells, kind="stable")  # list-major, arrival order inside every list: what an export is
    off = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=nl))]).astype(np.int64)
    iids, codes = order.astype(np.int32), stored[order]
    rng = np.random.default_rng(seed + dup)
    gone = rng.choice(n, n // 3, replace=False).astype(np.int32)
    request = np.concatenate([gone, gone[:5], [-1, n, n + 77]]).astype(np.int32)
    off2, iids2, codes2, found, removed = rt.filter_export(off, iids, codes, request)
    assert removed == len(gone) and np.array_equal(found, [1] * (len(gone) + 5) + [0, 0, 0])
    assert off2[-1] == n - removed == len(iids2) and not np.isin(iids2, gone).any()
    loaded, _ = cases.oracle_index(oracle, p, kind, D, C_, m, ks, tr)
    loaded.load_lists(off2, iids2, codes2)
    never, _ = cases.oracle_index(oracle, p, kind, D, C_, m, ks, tr)
    keep = np.ones(n, bool)
    keep[gone] = False
    idx = dt.stored_to_index(stored)
    for i in np.nonzero(keep)[0]:
        never.add_code(int(i), int(cells[i]), idx[i])
    assert np.array_equal(loaded.list_sizes(), never.list_sizes())
    Q = np.concatenate([p["base"][gone[:20]], p["base"][np.nonzero(keep)[0][:20]], rng.standard_normal((20, D))])
    for w in ((1, C_) if kind == cases.KIND_IVFPQ else (None,)):
        if w is not None:
            loaded.set_w(w)
            never.set_w(w)
        for kk in (1, k, 2 * k + 1):
            a, b = loaded.search_batch(Q, kk), never.search_batch(Q, kk)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0])
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
            assert not np.isin(a[0], gone).any()
    if dup == 2:
        d = loaded.search_batch(Q[20:40], 4)[1]
        assert (d[:, 0] == d[:, 1]).any()  # (the ties are there)


def _kernel_model(off, iids, gone_mask, tile):
    """The arithmetic of K13b-K13e (csrc/mmidx_remove.h) restated on the host: 64-bit keep words, survivor counts per tile, their
    exclusive prefix, a list's new start = tile prefix + popcounts of the words in front of it in its tile + a masked popcount, a
    record's new place = tile prefix + words in front + popcount of its word below its bit."""
    n = len(iids)
    keep = ~gone_mask
    nwords, ntiles, wpt = (n + 63) // 64, (n + tile - 1) // tile, tile // 64
    words = [sum(1 << l for l in range(64) if 64 * w + l < n and keep[64 * w + l]) for w in range(nwords)]
    pop = [bin(w).count("1") for w in words]
    cnt = [sum(pop[t * wpt:(t + 1) * wpt]) for t in range(ntiles)]
    pre = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)

    def rank(p):  # survivors in front of position p
        if p >= n:
            return int(pre[ntiles])
        t, wp, b = p // tile, p >> 6, p & 63
        return int(pre[t]) + sum(pop[t * wpt:wp]) + bin(words[wp] & ((1 << b) - 1)).count("1")

    off_new = np.array([rank(int(p)) for p in off], np.int64)
    dst = np.full(n, -1, np.int64)
    for p in range(n):
        if (words[p >> 6] >> (p & 63)) & 1:
            dst[p] = rank(p)
    return off_new, dst


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097])
def test_design_model_against_the_twin(n):
    """A model of the DESIGN only: the keep-word / tile-prefix arithmetic of DESIGN.md section 5.13, restated in Python, gives the
    twin's offsets and a stable, gap-free placement.  It runs no kernel -- only RM_TILE is read from the header -- and says nothing
    about the HIP code, which tests/test_gpu_remove.py checks on the device."""
    hdr = open(os.path.join(ROOT, "multimedia-indexing_amd", "csrc", "mmidx_remove.h")).read()
    tile = int(re.search(r"#define RM_TILE (\d+)", hdr).group(1))
    assert tile & (tile - 1) == 0 and 64 <= tile <= 8192
    rng = np.random.default_rng(n)
    nl = 5
    cells = np.sort(rng.integers(0, nl, n))
    off = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=nl))]).astype(np.int64)
    iids = rng.permutation(3 * n)[:n].astype(np.int32)
    for frac in (0.0, 0.3, 1.0):
        gone = rng.random(n) < frac
        off_new, dst = _kernel_model(off, iids, gone, tile)
        want = rt.filter_export(off, iids, np.zeros((n, 1), np.int8), iids[gone])
        assert np.array_equal(off_new, want[0])
        assert np.array_equal(dst[~gone], np.arange((~gone).sum())) and (dst[gone] == -1).all()


def test_symbols_declared_exported_and_bound(mi):
    hdr = open(os.path.join(ROOT, "include", "mmidx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nat = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    want = {
        "mmidx_remove": r"int mmidx_remove\(mmidx_index \*h, int64_t n, const int32_t \*iids,\s*int32_t \*found_out,\s*int64_t \*removed_out\);",
        "mmidx_remove_device": r"int mmidx_remove_device\(mmidx_index \*h, int64_t n, const int32_t \*d_iids,\s*int32_t \*d_found_out,\s*"
                               r"int64_t \*removed_out,\s*void \*stream\);",
    }
    for name, decl in want.items():
        assert re.search(decl, hdr), f"{name} is not declared with the stated signature"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in nat.SIGNATURES
    assert len(nat.SIGNATURES["mmidx_remove"][1]) == 5 and len(nat.SIGNATURES["mmidx_remove_device"][1]) == 6
    assert L.mmidx_abi_version() == 8  # (adding symbols breaks no caller)
    assert "#define MMIDX_ABI_VERSION 8" in hdr


def test_argument_errors_without_touching_the_gpu(mi):
    L = mi.lib()
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    removed = C.c_int64(-5)
    assert L.mmidx_remove(None, 1, p, p, C.byref(removed)) == 6 and b"null handle" in L.mmidx_last_error()
    assert L.mmidx_remove_device(None, 1, p, p, C.byref(removed), None) == 6 and b"null handle" in L.mmidx_last_error()
    assert L.mmidx_remove(None, 0, None, None, None) == 6
    fake = (C.c_char * (1 << 20))()  # stands in for a handle: the argument checks return before they read it
    h = C.addressof(fake)
    assert L.mmidx_remove(h, -1, p, p, C.byref(removed)) == 6 and b"n < 0" in L.mmidx_last_error()
    assert L.mmidx_remove_device(h, -1, p, p, C.byref(removed), None) == 6 and b"n < 0" in L.mmidx_last_error()
    assert L.mmidx_remove(h, 2, None, p, C.byref(removed)) == 6 and b"null argument" in L.mmidx_last_error()
    assert L.mmidx_remove_device(h, 2, None, p, C.byref(removed), None) == 6
    assert removed.value == -5 and all(v == 0 for v in buf)


class _HostOnly(importlib.import_module("multimedia-indexing_amd").index.AbstractSearchStructure):
    """the mirror's base class over two Python lists in place of the device: what removeVectors / replaceVector do to the id maps
    does not depend on the device"""

    def __init__(self, cap):
        super().__init__(4, cap)
        self.rows, self.removed_calls = {}, []

    def indexVectorInternal(self, vector):
        self.rows[self.loadCounter] = np.array(vector)

    def remove_batch(self, iids):
        self.removed_calls.append([int(i) for i in iids])
        found = np.array([int(i) in self.rows for i in iids], np.int32)
        for i in iids:
            self.rows.pop(int(i), None)
        return found, int(found.sum())


def test_mirror_id_maps(capsys):
    ix = _HostOnly(6)
    for i in range(4):
        assert ix.indexVector(f"img{i}", np.full(4, float(i)))
    assert ix.removeVector("img1") is True
    assert not ix.isIndexed("img1") and ix.getInternalId("img1") == -1 and ix.getId(1) is None
    assert ix.getLoadCounter() == 4 and sorted(ix.rows) == [0, 2, 3]
    assert ix.removeVector("img1") is False and "Vector 'img1' is not indexed!" in capsys.readouterr().out
    assert ix.removeVectors(["img0", "nope", "img0", "img3"]) == 2  # a repeat is one removal, an unknown id a printed line
    assert "Vector 'nope' is not indexed!" in capsys.readouterr().out
    assert ix.removed_calls[-1] == [0, 3] and sorted(ix.rows) == [2]
    assert ix.removeVectors([]) == 0 and ix.removeVectors(["nope"]) == 0 and len(ix.removed_calls) == 2
    # replace: the record gets a fresh internal id
    assert ix.replaceVector("img2", np.full(4, 9.0)) is True
    assert ix.getInternalId("img2") == 4 and ix.getId(2) is None and ix.getId(4) == "img2" and ix.getLoadCounter() == 5
    assert sorted(ix.rows) == [4] and (ix.rows[4] == 9.0).all()
    assert ix.replaceVector("img7", np.zeros(4)) is False and ix.getLoadCounter() == 5
    with pytest.raises(Exception, match="dimensionality"):
        ix.replaceVector("img2", np.zeros(3))
    assert ix.getInternalId("img2") == 4  # (refused before the removal)
    # a removed record does not give its capacity back: the sixth id is the last
    assert ix.indexVector("img1", np.zeros(4)) and ix.getInternalId("img1") == 5
    capsys.readouterr()
    assert ix.replaceVector("img1", np.ones(4)) is False and ix.isIndexed("img1")  # (full: nothing was removed)
    assert "Maximum index capacity reached" in capsys.readouterr().out
    assert ix.replaceVector("img7", np.ones(4)) is False  # full AND unknown: the unknown id is what is reported
    out = capsys.readouterr().out
    assert "Vector 'img7' is not indexed!" in out and "capacity" not in out
    assert ix.indexVector("more", np.zeros(4)) is False


def test_linear_has_no_removal():
    mi = importlib.import_module("multimedia-indexing_amd")
    with pytest.raises(mi.MmidxError) as ei:
        mi.index.Linear.remove_batch(object.__new__(mi.index.Linear), [0])
    assert ei.value.status == mi._native.ERR_UNSUPPORTED


def test_java_side_declares_and_uses_the_native():
    jdir = os.path.join(ROOT, "multimedia-indexing_amd", "jni", "java", "gr", "iti", "mklab", "visual", "datastructures")
    nat = open(os.path.join(jdir, "MmidxNative.java")).read()
    assert re.search(r"native long remove\(", nat)
    shim = open(os.path.join(ROOT, "multimedia-indexing_amd", "jni", "mmidx_jni.c")).read()
    assert "JFN(remove)" in shim and "mmidx_remove(" in shim
    for f in ("GpuIVFPQ.java", "GpuPQ.java"):
        src = open(os.path.join(jdir, f)).read()
        assert re.search(r"public synchronized int removeVectors\(String\[\] ids\)", src), f
        assert "MmidxNative.remove(" in src, f
