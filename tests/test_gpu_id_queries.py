"""GPU parity of the id queries (mmidx_reconstruct, mmidx_search_ids and their _device forms; csrc/mmidx_decode.h, DESIGN.md
section 5.9).  The decoder is compared bit for bit with its numpy twin (tests/decode_twin.py), fed from the index's own export, so the
decode is tested and not the encoder; the searches are compared with the CPU oracle searching the twin's vectors, under its default
queue rule.  Every comparison is np.array_equal on ids, on distance bits and on counts: there is no tolerance in this file."""
import ctypes as C
import importlib

import numpy as np
import pytest

import decode_twin as dt
import id_query_cases as cases

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


def assert_same(res, ref):
    iids, dists, counts = res
    rid, rd, rc = ref
    assert np.array_equal(counts, rc)
    assert np.array_equal(iids, rid)
    assert np.array_equal(dists.view(np.uint64), rd.view(np.uint64))


def make_index(mi, p, kind, D, C_, m, ks, n, tr, w=None):
    if kind == cases.KIND_IVFPQ:
        ix = mi.IVFPQ(D, n, False, "", m, ks, tr, C_, 512, rot=p["rot"])
        ix.loadCoarseQuantizer(p["coarse"])
        ix.setW(C_ if w is None else w)
    else:
        ix = mi.PQ(D, n, False, "", m, ks, tr, 512, rot=p["rot"])
    ix.loadProductQuantizer(p["pq"])
    return ix


class Case:
    """one shape: the index on the GPU, the oracle over the same records, and the twin fed from the index's own export"""

    def __init__(self, mi, oracle, row, dup=1):
        self.name, self.kind, self.D, self.C, self.m, self.ks, self.n, self.k, self.tr, seed = row
        self.p = cases.problem(seed, self.kind, self.D, self.C, self.m, self.ks, self.n, self.tr, dup)
        self.n = len(self.p["base"])
        self.ix = make_index(mi, self.p, self.kind, self.D, self.C, self.m, self.ks, self.n, self.tr)
        self.ref, self.perm = cases.oracle_index(oracle, self.p, self.kind, self.D, self.C, self.m, self.ks, self.tr)
        assert self.ix.indexVectors([str(i) for i in range(self.n)], self.p["base"]) == self.n
        self.exported = self.ix.export()
        # (the oracle takes the index's own records, list by list: what is tested is the decode and the search, not the encoder --
        #  and at D = 1024 the oracle's encoder alone would take several seconds)
        self.ref.load_lists(*self.exported)

    def twin(self, ids):
        off, iids, codes = self.exported
        return dt.decode_exported(self.p["pq"], off, iids, codes, ids, self.p["coarse"], self.tr, self.perm, self.p["rot"])

    def set_w(self, w):
        if self.kind == cases.KIND_IVFPQ:
            self.ix.setW(w)
            self.ref.set_w(w)

    def ids(self, count, seed=0):
        """`count` ids with repeats inside the batch"""
        rng = np.random.default_rng(self.D + count + seed)
        ids = rng.integers(0, self.n, count).astype(np.int32)
        if count >= 3:
            ids[-1] = ids[0]
            ids[count // 2] = ids[0]
        return ids


ALL = cases.TABLE + cases.EXTRA
_built = {}


@pytest.fixture(scope="module")
def built(mi, oracle):
    """the nine shapes, each built once for the module"""

    def get(row):
        if row[0] not in _built:
            _built[row[0]] = Case(mi, oracle, row)
        return _built[row[0]]

    yield get
    for c in _built.values():
        c.ix.close()
    _built.clear()


@pytest.mark.parametrize("row", ALL, ids=[r[0] for r in ALL])
def test_reconstruct_bit_for_bit(built, row):
    """1. batches of 1, 7 and 300 ids (40 at D = 1024), ids repeated inside a batch"""
    c = built(row)
    for count in (1, 7, 40 if c.D >= 1024 else 300):
        ids = c.ids(count)
        got = c.ix.reconstruct(ids)
        want = c.twin(ids)
        assert got.shape == want.shape == (count, c.D)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{c.name}: {count} ids"
    # and by external id
    assert np.array_equal(c.ix.reconstructVector(str(5)), c.twin([5])[0])


def test_reconstruct_noncontiguous_iids(mi, oracle):
    """the records carry the internal ids 3 i + 7: the position table has holes, and the ids between them do not exist"""
    row = cases.TABLE[1]
    _, kind, D, C_, m, ks, n, k, tr, seed = row
    p = cases.problem(seed, kind, D, C_, m, ks, n, tr)
    ix = make_index(mi, p, kind, D, C_, m, ks, 4 * n, tr)
    iids = (3 * np.arange(n) + 7).astype(np.int32)
    ix._add_vectors(p["base"], iids)
    off, eiids, codes = ix.export()
    perm = oracle.random_permutation(1, D)
    ask = iids[[0, 5, n - 1, 17, 5]]
    want = dt.decode_exported(p["pq"], off, eiids, codes, ask, p["coarse"], tr, perm, None)
    assert np.array_equal(ix.reconstruct(ask).view(np.uint64), want.view(np.uint64))
    for bad in (8, 0, 3 * n + 7):  # between two records, below the first, just past the last
        with pytest.raises(mi.MmidxError) as ei:
            ix.reconstruct([7, bad])
        assert ei.value.status == mi._native.ERR_INVALID_ARG and "Id does not exist!" in str(ei.value)
    ix.close()


def test_unknown_and_negative_ids_fail_and_write_nothing(mi, built):
    c = built(cases.TABLE[0])
    nat = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    for bad in (c.n, c.n + 1000, -1, -(2 ** 31)):
        ids = np.array([3, bad, 4], np.int32)
        out = np.full((3, c.D), 7.5)
        st = L.mmidx_reconstruct(c.ix._h, 3, ids.ctypes.data, out.ctypes.data)
        assert st == nat.ERR_INVALID_ARG and b"Id does not exist!" in L.mmidx_last_error()
        assert (out == 7.5).all()
        oi, od, oc = np.full((3, 2), 9, np.int32), np.full((3, 2), 7.5), np.full(3, 9, np.int32)
        st = L.mmidx_search_ids(c.ix._h, 2, 3, ids.ctypes.data, oi.ctypes.data, od.ctypes.data, oc.ctypes.data)
        assert st == nat.ERR_INVALID_ARG and b"Id does not exist!" in L.mmidx_last_error()
        assert (oi == 9).all() and (od == 7.5).all() and (oc == 9).all()
        with pytest.raises(mi.MmidxError) as ei:
            c.ix.reconstruct(ids)
        assert ei.value.status == nat.ERR_INVALID_ARG
    with pytest.raises(mi.MmidxError) as ei:
        c.ix.reconstructVector("no such image")
    assert "Id does not exist!" in str(ei.value)


@pytest.mark.parametrize("row", ALL, ids=[r[0] for r in ALL])
def test_search_ids_against_the_oracle(built, row):
    """2. k = 1, the shape's k and (on the 500-record shape with w = 1) a k beyond the candidates; w = 1 and w = C; and the same
    bytes as a vector search with the reconstructed vectors"""
    c = built(row)
    ids = c.ids(40 if c.D >= 1024 else 60, seed=1)
    X = c.twin(ids)
    ws = (1, c.C) if c.kind == cases.KIND_IVFPQ else (None,)
    for w in ws:
        if w is not None:
            c.set_w(w)
        ks_ = [1, c.k] + ([400] if c.name == "d16" and w == 1 else [])
        for k in ks_:
            want = c.ref.search_batch(X, k)
            got = c.ix.search_ids_batch(k, ids)
            assert_same(got, want)
            if k == 400:
                assert (want[2] < k).all()  # (a list of ~125 records: fewer candidates than k)
            assert_same(got, c.ix.search_batch(k, c.ix.reconstruct(ids)))
    if c.kind == cases.KIND_IVFPQ:
        # computeNearestNeighbors(k, "id"): the id's own record first
        a = c.ix.computeNearestNeighbors(c.k, str(int(ids[0])))
        want = c.ref.search_batch(X[:1], c.k)
        assert a.getIds() == [str(int(i)) for i in want[0][0, :want[2][0]]]
        assert np.array_equal(a.getDistances(), want[1][0, :want[2][0]])
        assert a.getIds()[0] == str(int(ids[0]))


def _family_case(mi, oracle, D, m, C_, n, w, dup=1, seed=5):
    row = ("family", cases.KIND_IVFPQ, D, C_, m, 256, n, 0, cases.TR_NONE, seed)
    c = Case(mi, oracle, row, dup)
    c.set_w(w)
    return c


def test_pass_a_k3q_under_id_queries(mi, oracle):
    """3. the first row of test_passa_q_forced: every query sits on a stored code, through K3q's integer table, then without it"""
    c = _family_case(mi, oracle, 128, 16, 6, 30000, 3)
    ids = c.ids(90)
    want = c.ref.search_batch(c.twin(ids), 100)
    c.ix.set_option("passa_q", 1)
    got = c.ix.search_ids_batch(100, ids)
    assert c.ix.get_dispatch()["pass_a"] == "K3q"
    assert_same(got, want)
    c.ix.set_option("passa_q", 0)
    off = c.ix.search_ids_batch(100, ids)
    assert c.ix.get_dispatch()["pass_a"] != "K3q"
    assert_same(off, want)
    c.ix.close()


def test_pass_a_k3ma_under_id_queries(mi, oracle):
    """3. the smallest forced shape of tests/test_gpu_passa_mfma.py (D 32, m 8, 9000 records, w 3, k 10)"""
    c = _family_case(mi, oracle, 32, 8, 3, 9000, 3)
    ids = c.ids(40)
    c.ix.set_option("passa_mfma", 1)
    got = c.ix.search_ids_batch(10, ids)
    assert c.ix.get_dispatch()["pass_a"] == "K3ma"
    assert_same(got, c.ref.search_batch(c.twin(ids), 10))
    c.ix.close()


def test_pass_b_k3m_under_id_queries(mi, oracle):
    """3. w = C on the shape of test_mfma_pass_b's first row: pass B on the matrix cores, then the exact scan on the same handle"""
    c = _family_case(mi, oracle, 128, 16, 6, 30000, 6)
    ids = c.ids(72)
    want = c.ref.search_batch(c.twin(ids), 100)
    got = c.ix.search_ids_batch(100, ids)
    assert c.ix.get_dispatch()["pass_b"] == "K3m"
    assert_same(got, want)
    c.ix.set_option("no_filter", 1)
    assert_same(c.ix.search_ids_batch(100, ids), want)
    c.ix.close()


def test_flagged_ties(mi, oracle):
    """4. every vector three times: a query's own triplicates tie at the top, and so does every other neighbour"""
    c = _family_case(mi, oracle, 128, 16, 5, 24000, 5, dup=3)
    ids = c.ids(120)
    X = c.twin(ids)
    for k in (50, 2):
        want = c.ref.search_batch(X, k)
        assert (want[1][:, 0] == want[1][:, 1]).all()  # (the tie is there)
        assert_same(c.ix.search_ids_batch(k, ids), want)
    c.ix.close()


def test_device_forms(mi, built):
    """5. on a torch stream that is not the default one: equal to the host forms; two unknown ids in the batch leave found = 0 and
    rows of zeros (reconstruct), count -1, ids -1, +inf (search), every other row as without them"""
    import torch

    c = built(cases.TABLE[3])  # rotation
    c.set_w(c.C)
    L = mi.lib()
    k = 10
    ids = c.ids(64, seed=2)
    host_X = c.ix.reconstruct(ids)
    host_res = c.ix.search_ids_batch(k, ids)
    bad = ids.copy()
    bad[3], bad[40] = c.n + 5, -7
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        for use, unknown in ((ids, []), (bad, [3, 40])):
            nq = len(use)
            d_ids = torch.from_numpy(use).to(dev)
            dX = torch.full((nq, c.D), 3.25, dtype=torch.float64, device=dev)
            d_found = torch.full((nq,), 9, dtype=torch.int32, device=dev)
            oi = torch.full((nq, k), 9, dtype=torch.int32, device=dev)
            od = torch.full((nq, k), 3.25, dtype=torch.float64, device=dev)
            oc = torch.full((nq,), 9, dtype=torch.int32, device=dev)
            assert L.mmidx_reconstruct_device(c.ix._h, nq, d_ids.data_ptr(), dX.data_ptr(), d_found.data_ptr(), s.cuda_stream) == 0
            assert L.mmidx_search_ids_device(c.ix._h, k, nq, d_ids.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr(), s.cuda_stream) == 0
            s.synchronize()
            X, found = dX.cpu().numpy(), d_found.cpu().numpy()
            gi, gd, gc = oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()
            keep = np.ones(nq, bool)
            keep[unknown] = False
            assert np.array_equal(found, keep.astype(np.int32))
            assert np.array_equal(X[keep].view(np.uint64), host_X[keep].view(np.uint64))
            assert (X[~keep] == 0.0).all() and not np.signbit(X[~keep]).any()
            assert_same((gi[keep], gd[keep], gc[keep]), tuple(a[keep] for a in host_res))
            assert (gc[~keep] == -1).all() and (gi[~keep] == -1).all() and np.isposinf(gd[~keep]).all()
        # found may be null
        d_ids = torch.from_numpy(ids).to(dev)
        dX = torch.empty((len(ids), c.D), dtype=torch.float64, device=dev)
        assert L.mmidx_reconstruct_device(c.ix._h, len(ids), d_ids.data_ptr(), dX.data_ptr(), None, s.cuda_stream) == 0
        s.synchronize()
        assert np.array_equal(dX.cpu().numpy().view(np.uint64), host_X.view(np.uint64))


def test_position_table_follows_the_index(mi, oracle, tmp_path):
    """6. half the records, id queries; the other half, id queries into both halves; snapshot -> fresh handle -> the same answers"""
    row = cases.TABLE[1]
    _, kind, D, C_, m, ks, n, k, tr, seed = row
    p = cases.problem(seed, kind, D, C_, m, ks, n, tr)
    ref, perm = cases.oracle_index(oracle, p, kind, D, C_, m, ks, tr, w=3)
    ix = make_index(mi, p, kind, D, C_, m, ks, n, tr, w=3)
    h = n // 2

    def check(index, ids):
        off, eiids, codes = index.export()
        X = dt.decode_exported(p["pq"], off, eiids, codes, ids, p["coarse"], tr, perm, None)
        assert np.array_equal(index.reconstruct(ids).view(np.uint64), X.view(np.uint64))
        res = index.search_ids_batch(k, ids)
        assert_same(res, ref.search_batch(X, k))
        return res

    ix.indexVectors([str(i) for i in range(h)], p["base"][:h])
    ref.add_vectors(p["base"][:h])
    check(ix, np.array([0, 1, h - 1, 77, h // 2], np.int32))
    with pytest.raises(mi.MmidxError):
        ix.reconstruct([h])  # (not there yet)
    ix.indexVectors([str(i) for i in range(h, n)], p["base"][h:])
    ref.add_vectors(p["base"][h:])
    ids = np.array([0, h - 1, h, n - 1, 77, h + 77, h // 2], np.int32)
    before = check(ix, ids)
    path = str(tmp_path / "idq.snap")
    ix.saveSnapshot(path)
    ix2 = make_index(mi, p, kind, D, C_, m, ks, n, tr, w=3)
    ix2.loadSnapshot(path)
    assert_same(check(ix2, ids), before)
    assert ix2.reconstructVector(str(h + 77)).shape == (D,)
    ix.close()
    ix2.close()


def test_sharded_handle_is_refused(mi):
    """7. DESIGN.md section 9 freezes the sharded code: one virtual shard answers both host calls with UNSUPPORTED"""
    nat = importlib.import_module("multimedia-indexing_amd._native")
    _, kind, D, C_, m, ks, n, k, tr, seed = cases.TABLE[0]
    p = cases.problem(seed, kind, D, C_, m, ks, n, tr)
    ix = mi.IVFPQ(D, n, False, "", m, ks, tr, C_, 512, devices=[0])
    ix.loadCoarseQuantizer(p["coarse"])
    ix.loadProductQuantizer(p["pq"])
    ix.setW(2)
    ix.indexVectors([str(i) for i in range(n)], p["base"])
    with pytest.raises(mi.MmidxError) as ei:
        ix.reconstruct([0, 1])
    assert ei.value.status == nat.ERR_UNSUPPORTED
    with pytest.raises(mi.MmidxError) as ei:
        ix.search_ids_batch(3, [0, 1])
    assert ei.value.status == nat.ERR_UNSUPPORTED
    L = mi.lib()
    buf = (C.c_double * 64)()
    p_ = C.addressof(buf)
    assert L.mmidx_reconstruct_device(ix._h, 1, p_, p_, None, None) == nat.ERR_UNSUPPORTED
    assert L.mmidx_search_ids_device(ix._h, 3, 1, p_, p_, p_, p_, None) == nat.ERR_UNSUPPORTED
    ix.close()
