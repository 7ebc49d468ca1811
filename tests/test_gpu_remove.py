"""GPU parity of the removal (mmidx_remove / mmidx_remove_device; csrc/mmidx_remove.h).  After a removal
the index must be, array for array, the index the removed records were never added to: every export is compared with the numpy
twin (tests/remove_twin.py) applied to the export taken before, and every search with the CPU oracle loaded with the twin's lists.
Every comparison is np.array_equal on ids, on distance bits and on counts: there is no tolerance in this file."""
import ctypes as C
import importlib
import os
import re
import threading

import numpy as np
import pytest

import decode_twin as dt
import id_query_cases as cases
import refine_twin as rf
import remove_twin as rt

pytestmark = pytest.mark.gpu

ROWS = {r[0]: r for r in cases.TABLE + cases.EXTRA}


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


def assert_same(res, ref):
    iids, dists, counts = res
    rid, rd, rc = ref
    assert np.array_equal(counts, rc)
    assert np.array_equal(iids, rid)
    assert np.array_equal(dists.view(np.uint64), rd.view(np.uint64))


def assert_export(got, want):
    for g, w, what in zip(got, want, ("list_off", "ids", "codes")):
        assert g.shape == w.shape and np.array_equal(g, w), what


def make_index(mi, p, kind, D, C_, m, ks, cap, tr, w=None):
    if kind == cases.KIND_IVFPQ:
        ix = mi.IVFPQ(D, cap, False, "", m, ks, tr, C_, 512, rot=p["rot"])
        ix.loadCoarseQuantizer(p["coarse"])
        ix.setW(C_ if w is None else w)
    else:
        ix = mi.PQ(D, cap, False, "", m, ks, tr, 512, rot=p["rot"])
    ix.loadProductQuantizer(p["pq"])
    return ix


def append_export(exp, iids, cells, codes):
    """the export after these records arrived, in this order, behind the ones of `exp`"""
    off, eiids, ecodes = exp
    nl = len(off) - 1
    lists = np.concatenate([rt.list_of_position(off, len(eiids)), np.asarray(cells, np.int32).clip(0)])
    order = np.argsort(lists, kind="stable")
    off2 = np.concatenate([[0], np.cumsum(np.bincount(lists, minlength=nl))]).astype(np.int64)
    return off2, np.concatenate([eiids, np.asarray(iids, np.int32)])[order], np.concatenate([ecodes, codes])[order]


class Case:
    """one shape: its vectors encoded once on the GPU; every test loads a fresh handle from that export (removal changes the index)"""

    def __init__(self, mi, oracle, row, dup=1):
        self.mi, self.oracle = mi, oracle
        self.name, self.kind, self.D, self.C, self.m, self.ks, self.n, self.k, self.tr, seed = row
        self.ivf = self.kind == cases.KIND_IVFPQ
        self.p = cases.problem(seed, self.kind, self.D, self.C, self.m, self.ks, self.n, self.tr, dup)
        self.base = self.p["base"]
        self.n = len(self.base)
        ix = self.empty()
        assert ix.indexVectors([str(i) for i in range(self.n)], self.base) == self.n
        self.exported = ix.export()
        ix.close()
        if not self.ivf:
            assert np.array_equal(self.exported[1], np.arange(self.n))
        self.perm = oracle.random_permutation(1, self.D) if self.tr == cases.TR_PERMUTATION else None

    def empty(self, w=None):
        return make_index(self.mi, self.p, self.kind, self.D, self.C, self.m, self.ks, self.n + 64, self.tr, w)

    def fresh(self, w=None):
        """a handle holding the shape's records, loaded list by list (the order inside every list is the arrival order)"""
        ix = self.empty(w)
        off, iids, codes = self.exported
        if self.ivf:
            ix.loadIndex(iids, rt.list_of_position(off, len(iids)), codes)
        else:
            ix.loadIndex(codes)
        return ix

    def ref(self, exp, w=None):
        """the CPU oracle over the lists of an export"""
        r, _ = cases.oracle_index(self.oracle, self.p, self.kind, self.D, self.C, self.m, self.ks, self.tr, w)
        r.load_lists(*exp)
        return r

    def decode(self, exp, ids):
        return dt.decode_exported(self.p["pq"], exp[0], exp[1], exp[2], ids, self.p["coarse"], self.tr, self.perm, self.p["rot"])


_built = {}


@pytest.fixture(scope="module")
def built(mi, oracle):
    def get(name, dup=1):
        if (name, dup) not in _built:
            _built[(name, dup)] = Case(mi, oracle, ROWS[name], dup)
        return _built[(name, dup)]

    yield get
    _built.clear()


def remove_and_check(ix, before, request, ivf):
    """remove_batch(request) on ix, whose export was `before`: everything the call reports and leaves against the twin"""
    request = np.asarray(request, np.int32)
    want = rt.filter_export(*before, request)
    found, removed = ix.remove_batch(request)
    assert np.array_equal(found, want[3]), "found"
    assert removed == want[4], "removed"
    after = ix.export()
    assert_export(after, want[:3])
    assert ix.size() == len(want[1])
    if ivf:
        assert np.array_equal(ix.listSizes(), np.diff(want[0]))
    return after


def request_sets(exp, rng):
    off, iids, _ = exp
    n = len(iids)
    big = [c for c in range(len(off) - 1) if off[c + 1] - off[c] >= 2]
    c = big[len(big) // 2]
    absent = np.array([-1, -(2 ** 31), int(iids.max()) + 1, int(iids.max()) + 1000, 2 ** 31 - 1], np.int32)
    rep = rng.choice(iids, 40, replace=False)
    return {
        "empty": np.zeros(0, np.int32),
        "one": iids[[n // 3]],
        "first_last_of_index": iids[[0, n - 1]],
        "first_last_of_list": iids[[off[c], off[c + 1] - 1]],
        "whole_list": iids[off[c]:off[c + 1]],
        "every_second": iids[::2],
        "everything": rng.permutation(iids),
        "absent_only": absent,
        "repeats": np.concatenate([rep, rep[:17], absent[:2], rep[5:9]]),
    }


@pytest.mark.parametrize("name", ["d16", "d24_perm", "d64_short", "d1024_rot", "pq32"])
def test_record_for_record(built, name):
    """1. records of 4, 6, 16 (short codes), 64 and 8 bytes; each request set on a handle of its own"""
    c = built(name)
    rng = np.random.default_rng(c.D)
    for label, req in request_sets(c.exported, rng).items():
        ix = c.fresh()
        try:
            after = remove_and_check(ix, c.exported, req, c.ivf)
            if label in ("empty", "absent_only"):
                assert_export(after, c.exported)  # (nothing moved)
            if label == "everything":
                assert ix.size() == 0 and len(after[1]) == 0
                # ... and the empty index answers found = 0 to the same ids
                remove_and_check(ix, after, req[:3], c.ivf)
        except AssertionError as e:
            raise AssertionError(f"{name}: request '{label}': {e}") from e
        finally:
            ix.close()


SIZES = [1, 63, 64, 65] + [v for j in range(7, 14) for v in (2 ** j - 1, 2 ** j, 2 ** j + 1)]


@pytest.mark.parametrize("kind", ["ivfpq", "pq"])
def test_every_tile_and_word_edge(mi, built, kind):
    """1. index sizes around every power of two up to 8192 (a tile is a power of two of at most 8192 records, a keep word 64): random
    4-byte records, a random third removed; one handle serves all sizes -- the rest is removed before the next size is loaded"""
    c = built("d16")
    rng = np.random.default_rng(5)
    if kind == "ivfpq":
        ix = c.empty()
    else:
        ix = mi.PQ(c.D, 10 ** 6, False, "", c.m, c.ks, cases.TR_NONE, 512)
        ix.loadProductQuantizer(c.p["pq"])
    try:
        for n in SIZES:
            codes = (rng.integers(0, c.ks, (n, c.m)) - 128).astype(np.int8)
            if kind == "ivfpq":
                iids = rng.choice(3 * n, n, replace=False).astype(np.int32)
                ix.loadIndex(iids, rng.integers(0, c.C, n).astype(np.int32), codes)
            else:
                ix.loadIndex(codes)
            before = ix.export()
            assert len(before[1]) == n and np.array_equal(np.sort(before[2].view(np.int32).ravel()), np.sort(codes.view(np.int32).ravel()))
            third = rng.choice(before[1], max(n // 3, 1), replace=False)
            try:
                after = remove_and_check(ix, before, third, kind == "ivfpq")
                remove_and_check(ix, after, rng.permutation(after[1]), kind == "ivfpq")
            except AssertionError as e:
                raise AssertionError(f"{kind}, n = {n}: {e}") from e
            assert ix.size() == 0
    finally:
        ix.close()


def test_more_tiles_than_one_scan_round(mi, built):
    """1. K13c's block takes 1024 tile counts per round and carries their sum into the next: 2 x 1024 x 2048 + 12345 records are
    2055 tiles, three rounds with a carry into the second and the third (4-byte records, 17 MB; no smaller index reaches the carry)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "multimedia-indexing_amd", "csrc", "mmidx_remove.h")).read()
    tile, scan_nt = (int(re.search(r"#define %s (\d+)" % s, hdr).group(1)) for s in ("RM_TILE", "RM_SCAN_NT"))
    c = built("d16")
    n = 2 * scan_nt * tile + 12345
    assert (n + tile - 1) // tile > 2 * scan_nt and n <= 5_000_000
    rng = np.random.default_rng(13)
    iids = rng.permutation(n).astype(np.int32)
    cells = rng.integers(0, c.C, n).astype(np.int32)
    codes = (rng.integers(0, c.ks, (n, c.m)) - 128).astype(np.int8)  # (stored form: index - 128)
    ix = c.empty()
    try:
        mi._native.check(mi.lib().mmidx_add_codes(ix._h, n, iids.ctypes.data, cells.ctypes.data, codes.ctypes.data))
        before = ix.export()
        assert len(before[1]) == n
        # a third of the ids, with every record of the last tile of the first round and the first of the second among them
        edge = before[1][scan_nt * tile - tile:scan_nt * tile + tile]
        after = remove_and_check(ix, before, np.concatenate([rng.choice(n, n // 3, replace=False).astype(np.int32), edge]), True)
        remove_and_check(ix, after, after[1][::2], True)
    finally:
        ix.close()


def test_an_iid_stored_twice(built):
    """2. mmidx_add_codes does not forbid it: the same iid in two lists.  Both records go; one request entry, two records"""
    c = built("d16")
    off, iids, codes = c.exported
    ix = c.fresh()
    twice = int(iids[off[1]])  # the first record of list 1 ...
    ix.loadIndex(np.array([twice], np.int32), np.array([3], np.int32), codes[:1])  # ... once more, at the end of list 3
    before = ix.export()
    assert (before[1] == twice).sum() == 2
    found, removed = ix.remove_batch([twice])
    assert np.array_equal(found, [1]) and removed == 2
    assert_export(ix.export(), rt.filter_export(*before, [twice])[:3])
    assert ix.size() == c.n - 1
    ix.close()


def test_pending_records(built):
    """3. records that were appended and not folded into the lists yet can be removed, together with old ones"""
    c = built("d16")
    h = 300
    ix = c.empty()
    ix.indexVectors([str(i) for i in range(h)], c.base[:h])
    ix.export()  # (folds the first batch)
    ix.indexVectors([str(i) for i in range(h, c.n)], c.base[h:])
    req = np.array([5, h - 1, h, h + 7, c.n - 1, 123, c.n + 3], np.int32)
    want = rt.filter_export(*c.exported, req)  # (two batches leave the lists the one batch of the Case left)
    found, removed = ix.remove_batch(req)
    assert np.array_equal(found, want[3]) and removed == want[4] == 6
    assert_export(ix.export(), want[:3])
    ix.close()


# (shape, w, dup): d128 at w = C goes through K3m for pass B; dup = 2 is the tie fixture (every vector twice: equal distances
# everywhere, resolved by the order inside the lists, under the default queue rule)
SEARCHES = [("d128", None, 1), ("d128", 1, 1), ("d64_short", None, 1), ("d24_perm", None, 1), ("pq32", None, 1), ("d128", None, 2)]


@pytest.mark.parametrize("name,w,dup", SEARCHES, ids=[f"{s[0]}-w{s[1] or 'C'}-dup{s[2]}" for s in SEARCHES])
def test_searches_after_a_removal(built, name, w, dup):
    """4. 300 queries, among them the removed vectors themselves: the oracle over the twin's lists, bit for bit"""
    c = built(name, dup)
    rng = np.random.default_rng(c.D + dup)
    gone = rng.choice(c.n, c.n // 4, replace=False).astype(np.int32)
    keep = np.setdiff1d(np.arange(c.n), gone)
    Q = np.concatenate([c.base[gone[:120]], c.base[keep[:120]], 0.5 * (c.base[gone[120:180]] + c.base[keep[120:180]])])
    assert len(Q) == 300
    k = 100 if name == "d128" else c.k
    ix = c.fresh(w)
    try:
        assert_same(ix.search_batch(k, Q[:40]), c.ref(c.exported, w).search_batch(Q[:40], k))  # (before: the per-code norms are built)
        after = remove_and_check(ix, c.exported, gone, c.ivf)
        ref = c.ref(after, w)
        want = ref.search_batch(Q, k)
        got = ix.search_batch(k, Q)
        d = ix.get_dispatch()
        print(f"{name} w={w} dup={dup}: {d}")
        assert not np.isin(got[0], gone).any()  # the removed vectors' own records are gone from their answers
        assert_same(got, want)
        if dup == 2:
            # (the ties are there: a surviving vector whose copy survived too meets both at the same distance)
            assert (want[1][120:240, 0] == want[1][120:240, 1]).sum() >= 30
        if name == "d128" and w is None:
            # pass B on the matrix cores reads the per-code norms, which the removal invalidated: they were rebuilt from the new codes
            assert d["pass_b"] == "K3m", d
            ix.set_option("passb_small", 0)  # (so that no hint of the call before can take the second call away from K3m)
            assert_same(ix.search_batch(k, Q), want)
            assert ix.get_dispatch()["pass_b"] == "K3m"
            ix.set_option("no_mfma", 1)
            assert_same(ix.search_batch(k, Q), want)
            assert ix.get_dispatch()["pass_b"] != "K3m"
    finally:
        ix.close()


def test_id_paths(mi, built):
    """5. a removed id is unknown to every per-id call; a surviving one answers from the new lists; the exact re-ranking still
    finds its rows, because internal ids do not move"""
    c = built("d128")
    nat = importlib.import_module("multimedia-indexing_amd._native")
    rng = np.random.default_rng(3)
    gone = rng.choice(c.n, 500, replace=False).astype(np.int32)
    keep = np.setdiff1d(np.arange(c.n), gone).astype(np.int32)
    ix = c.fresh()
    lin = mi.Linear(c.D, c.n)
    try:
        after = remove_and_check(ix, c.exported, gone, True)  # (remove_batch: the mirror's maps still know the ids)
        ref = c.ref(after)
        for call in (lambda: ix.search_ids_batch(5, [int(keep[0]), int(gone[0])]), lambda: ix.reconstruct([int(gone[1])]),
                     lambda: ix.getPQCodeByte(str(int(gone[2]))), lambda: ix.getInvertedListId(str(int(gone[3])))):
            with pytest.raises(mi.MmidxError) as ei:
                call()
            assert ei.value.status == nat.ERR_INVALID_ARG and "Id does not exist!" in str(ei.value)
        ids = keep[rng.choice(len(keep), 60, replace=False)]
        X = c.decode(after, ids)
        assert np.array_equal(ix.reconstruct(ids).view(np.uint64), X.view(np.uint64))
        assert_same(ix.search_ids_batch(20, ids), ref.search_batch(X, 20))
        pos = {int(v): i for i, v in enumerate(after[1])}
        for i in ids[:5]:
            assert np.array_equal(ix.getPQCodeByte(str(int(i))), after[2][pos[int(i)]])
            assert ix.getInvertedListId(str(int(i))) == rt.list_of_position(after[0], len(after[1]))[pos[int(i)]]
        # the Linear index is untouched: row iid is still the vector of record iid
        lin.indexVectors([str(i) for i in range(c.n)], c.base)
        Q = np.concatenate([c.base[gone[:30]], c.base[keep[:30]]])
        k, R = 10, 50
        want = rf.refine_batch(ref.search_batch(Q, R), c.base, Q, k)
        got = ix.search_refine_batch(k, R, Q, lin)
        assert_same(got[:3], want[:3])
        assert got[3] == want[3] == 0 and not np.isin(got[0], gone).any()
    finally:
        ix.close()
        lin.close()


def test_ids_are_used_again(built):
    """6. after a removal: new vectors under fresh ids, one record under a removed iid, and replaceVector through the mirror"""
    c = built("d32_perm")
    ix = c.fresh()
    try:
        gone = [str(i) for i in (0, 7, 500, c.n - 1)]
        assert ix.removeVectors(gone + ["never indexed"]) == 4
        assert not ix.isIndexed("7") and ix.getInternalId("7") == -1 and ix.getLoadCounter() == c.n
        exp = rt.filter_export(*c.exported, [0, 7, 500, c.n - 1])[:3]
        assert_export(ix.export(), exp)
        # new vectors: the next internal ids
        rng = np.random.default_rng(8)
        X = c.base[:20] + 0.05 * rng.standard_normal((20, c.D))
        cells, codes = ix.encode(X)
        assert ix.indexVectors([f"new{i}" for i in range(20)], X) == 20
        exp = append_export(exp, np.arange(c.n, c.n + 20), cells, codes)
        # a record under the removed iid 7 (loadIndex takes the iid as given)
        ix.loadIndex(np.array([7], np.int32), cells[:1], codes[:1])
        exp = append_export(exp, [7], cells[:1], codes[:1])
        assert_export(ix.export(), exp)
        assert ix.isIndexed("7") and np.array_equal(ix.getPQCodeByte("7"), codes[0])
        # replaceVector: the record of "11" goes, its new vector arrives under a fresh internal id
        counter = ix.getLoadCounter()
        v = c.base[11] + 0.05 * rng.standard_normal(c.D)
        vc, vk = ix.encode(v.reshape(1, -1))
        assert ix.replaceVector("11", v) is True
        assert ix.getInternalId("11") == counter and ix.getId(11) is None and ix.getLoadCounter() == counter + 1
        exp = append_export(rt.filter_export(*exp, [11])[:3], [counter], vc, vk)
        assert_export(ix.export(), exp)
        ref = c.ref(exp)
        Q = np.concatenate([X[:10], c.base[[0, 7, 500, 11]], v.reshape(1, -1)])
        got = ix.search_batch(c.k, Q)
        assert_same(got, ref.search_batch(Q, c.k))
        a = ix.computeNearestNeighbors(3, v)
        wi, _, wc = ref.search_batch(v.reshape(1, -1), 3)
        assert a.getIds() == [ix.getId(i) for i in wi[0, :wc[0]]] and None not in a.getIds()
        assert ix.getId(counter) == "11"
        assert ix.replaceVector("never indexed", v) is False
    finally:
        ix.close()


def test_snapshot_after_a_removal(built, tmp_path):
    """7. the snapshot holds the smaller index, and its id map has forgotten the removed ids"""
    c = built("d24_perm")
    ix = c.fresh()
    ix2 = c.empty()
    try:
        assert ix.removeVectors([str(i) for i in range(0, c.n, 3)]) == len(range(0, c.n, 3))
        path = str(tmp_path / "removed.snap")
        ix.saveSnapshot(path)
        ix2.loadSnapshot(path)
        want = rt.filter_export(*c.exported, np.arange(0, c.n, 3))[:3]
        assert_export(ix.export(), want)
        assert_export(ix2.export(), want)
        assert ix2.size() == len(want[1]) and not ix2.isIndexed("3") and ix2.isIndexed("4") and ix2.getLoadCounter() == c.n
        Q = c.base[:16]
        assert_same(ix2.search_batch(c.k, Q), ix.search_batch(c.k, Q))
    finally:
        ix.close()
        ix2.close()


def test_sharded_handle_is_refused(mi, built):
    """8. DESIGN.md section 9 freezes the sharded code: one virtual shard answers UNSUPPORTED, and keeps its records"""
    nat = importlib.import_module("multimedia-indexing_amd._native")
    c = built("d16")
    ix = mi.IVFPQ(c.D, c.n, False, "", c.m, c.ks, c.tr, c.C, 512, devices=[0])
    try:
        ix.loadCoarseQuantizer(c.p["coarse"])
        ix.loadProductQuantizer(c.p["pq"])
        ix.indexVectors([str(i) for i in range(c.n)], c.base)
        before = ix.export()
        with pytest.raises(mi.MmidxError) as ei:
            ix.remove_batch([0, 1])
        assert ei.value.status == nat.ERR_UNSUPPORTED and "plain handle" in str(ei.value)
        buf = (C.c_int32 * 16)()
        removed = C.c_int64(-1)
        assert mi.lib().mmidx_remove_device(ix._h, 2, C.addressof(buf), None, C.byref(removed), None) == nat.ERR_UNSUPPORTED
        assert removed.value == -1
        with pytest.raises(mi.MmidxError):
            ix.removeVectors(["0"])
        assert ix.isIndexed("0")  # (the mirror's maps follow the native call)
        assert_export(ix.export(), before)
        assert ix.size() == c.n
    finally:
        ix.close()


def test_device_form(mi, built):
    """the ids and the found flags in HBM, on a torch stream that is not the default one; found may be null; the call has
    synchronised when it returns"""
    import torch

    c = built("d24_perm")
    L = mi.lib()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    ix = c.fresh()
    try:
        req = np.concatenate([np.arange(0, c.n, 5), [-4, c.n + 9, 10, 10]]).astype(np.int32)
        want = rt.filter_export(*c.exported, req)
        removed = C.c_int64(-1)
        with torch.cuda.stream(s):
            d_req = torch.from_numpy(req).to(dev, non_blocking=True)
            d_found = torch.full((len(req),), 9, dtype=torch.int32, device=dev)
            assert L.mmidx_remove_device(ix._h, len(req), d_req.data_ptr(), d_found.data_ptr(), C.byref(removed), s.cuda_stream) == 0
            found = d_found.cpu().numpy()
        assert removed.value == want[4] and np.array_equal(found, want[3])
        assert_export(ix.export(), want[:3])
        with torch.cuda.stream(s):
            d_req = torch.tensor([1, 2, 3, 10], dtype=torch.int32, device=dev)
            assert L.mmidx_remove_device(ix._h, 4, d_req.data_ptr(), None, None, s.cuda_stream) == 0
        assert_export(ix.export(), rt.filter_export(*want[:3], [1, 2, 3])[:3])
        assert L.mmidx_remove_device(ix._h, 0, None, None, C.byref(removed), None) == 0 and removed.value == 0
    finally:
        ix.close()


def test_a_search_thread_beside_one_removal(built):
    """9. one thread searches the same 64 queries in a loop while the main thread removes once: every answer is the oracle's
    answer before or the oracle's answer after, whole.  Bounded: 200 searches at most, a join with a timeout."""
    c = built("d32_perm")
    rng = np.random.default_rng(21)
    gone = rng.choice(c.n, c.n // 2, replace=False).astype(np.int32)
    Q = c.base[np.concatenate([gone[:32], np.setdiff1d(np.arange(c.n), gone)[:32]])]
    after_exp = rt.filter_export(*c.exported, gone)[:3]
    before, after = c.ref(c.exported).search_batch(Q, c.k), c.ref(after_exp).search_batch(Q, c.k)
    assert not np.array_equal(before[0], after[0])
    ix = c.fresh()
    answers, errors = [], []
    started, done = threading.Event(), threading.Event()

    def searcher():
        try:
            tail = 0
            for _ in range(200):
                answers.append(ix.search_batch(c.k, Q))
                if len(answers) >= 3:
                    started.set()
                if done.is_set():
                    tail += 1
                    if tail >= 3:
                        break
        except Exception as e:  # noqa: BLE001
            errors.append(e)
        finally:
            started.set()

    t = threading.Thread(target=searcher, daemon=True)
    t.start()
    try:
        assert started.wait(timeout=60), "the search thread did not start"
        found, removed = ix.remove_batch(gone)
        done.set()
        t.join(timeout=60)
        assert not t.is_alive(), "the search thread did not finish"
        assert not errors, errors
        assert removed == len(gone) and found.all()
        assert 3 <= len(answers) <= 200
        kinds = []
        for a in answers:
            is_before = all(np.array_equal(x, y) for x, y in zip((a[0], a[1].view(np.uint64), a[2]), (before[0], before[1].view(np.uint64), before[2])))
            is_after = all(np.array_equal(x, y) for x, y in zip((a[0], a[1].view(np.uint64), a[2]), (after[0], after[1].view(np.uint64), after[2])))
            assert is_before or is_after, "an answer that is neither the one before nor the one after the removal"
            kinds.append(is_after)
        assert kinds == sorted(kinds) and kinds[-1] and not kinds[0]  # before ... before, after ... after
        assert_export(ix.export(), after_exp)
    finally:
        done.set()
        t.join(timeout=60)
        ix.close()
