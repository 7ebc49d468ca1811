"""GPU parity of the exact re-ranking (mmidx_search_refine, _device, _ids; csrc/mmidx_refine.h).  The
yardstick is never the code under test: the CPU oracle searches the index's own records with k = R, the candidates' rows come from the
test's own base array, their distances from np_twin.sq_dists_rows and the queue from np_twin.bpq_result (tests/refine_twin.py).
Every comparison is np.array_equal on ids, on distance bits, on counts and on `missing`: there is no tolerance in this file."""
import ctypes as C
import importlib

import numpy as np
import pytest

import id_query_cases as cases
import refine_twin as rt

pytestmark = pytest.mark.gpu

ROWS = {r[0]: r for r in cases.TABLE + cases.EXTRA}
TABLE1 = ["d16", "d32_perm", "d128", "d64_short", "d24_perm", "d1024_rot", "pq32", "pq32_rot"]


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


def assert_same(res, ref, what=""):
    iids, dists, counts = res[:3]
    rid, rd, rc = ref[:3]
    assert np.array_equal(counts, rc), what
    assert np.array_equal(iids, rid), what
    assert np.array_equal(dists.view(np.uint64), rd.view(np.uint64)), what
    if len(ref) > 3:
        assert int(res[3]) == int(ref[3]), what


def make_index(mi, p, kind, D, C_, m, ks, n, tr, **kw):
    if kind == cases.KIND_IVFPQ:
        ix = mi.IVFPQ(D, n, False, "", m, ks, tr, C_, 512, rot=p["rot"], **kw)
        ix.loadCoarseQuantizer(p["coarse"])
        ix.setW(C_)
    else:
        ix = mi.PQ(D, n, False, "", m, ks, tr, 512, rot=p["rot"])
    ix.loadProductQuantizer(p["pq"])
    return ix


class Case:
    """one shape: the compressed index and a Linear index over the same vectors on the GPU, the oracle over the index's own records"""

    def __init__(self, mi, oracle, row, dup=1, seed=None):
        self.name, self.kind, self.D, self.C, self.m, self.ks, n, self.k, self.tr, s = row
        self.p = cases.problem(s if seed is None else seed, self.kind, self.D, self.C, self.m, self.ks, n, self.tr, dup)
        self.base = self.p["base"]
        self.base.setflags(write=False)
        self.n = len(self.base)
        self.ix = make_index(mi, self.p, self.kind, self.D, self.C, self.m, self.ks, self.n, self.tr)
        self.ref, _ = cases.oracle_index(oracle, self.p, self.kind, self.D, self.C, self.m, self.ks, self.tr)
        assert self.ix.indexVectors([str(i) for i in range(self.n)], self.base) == self.n
        self.ref.load_lists(*self.ix.export())  # (the oracle takes the index's own records: the search is tested, not the encoder)
        self.lin = mi.Linear(self.D, self.n + 8)
        self.lin._add_vectors(self.base, None)
        self.nq = 40 if self.D >= 1024 else 300
        rng = np.random.default_rng(1000 + self.D)
        self.Q = self.base[rng.integers(0, self.n, self.nq)] + 0.05 * rng.standard_normal((self.nq, self.D))
        self.Q.setflags(write=False)
        self._cands = {}
        self.w = self.C

    def set_w(self, w):
        if self.kind == cases.KIND_IVFPQ and w != self.w:
            self.ix.setW(w)
            self.ref.set_w(w)
            self._cands.clear()
            self.w = w

    def cands(self, R, Q=None):
        """the oracle's answer for k = R: computed once per R for the shape's own queries"""
        if Q is not None:
            return self.ref.search_batch(Q, R, nthreads=8)
        if R not in self._cands:
            self._cands[R] = self.ref.search_batch(self.Q, R, nthreads=8)
        return self._cands[R]

    def close(self):
        self.ix.close()
        self.lin.close()


_built = {}


@pytest.fixture(scope="module")
def built(mi, oracle):
    """each shape built once for the module"""

    def get(name):
        if name not in _built:
            _built[name] = Case(mi, oracle, ROWS[name])
        return _built[name]

    yield get
    for c in _built.values():
        c.close()
    _built.clear()


def kr_pairs(k):
    return [(1, 1), (k, k), (k, 4 * k + 1), (k, 257), (k, 1000)]


@pytest.mark.parametrize("name", TABLE1)
def test_shape_table(built, oracle, name):
    """1. batches of 1, 7 and 300 queries (40 at D = 1024) for five (k, R) pairs; and 7. the property: for every tie-free query the
    refined top k holds every exact top-k id that the plain compressed top k holds"""
    c = built(name)
    c.set_w(c.C)
    xi, xd, _ = oracle.linear_search_batch(c.base, c.Q, c.k + 1, nthreads=8)  # exact neighbours, for the property
    for k, R in kr_pairs(c.k):
        want = rt.refine_batch(c.cands(R), c.base, c.Q, k)
        assert want[3] == 0
        for nq in (1, 7, c.nq):
            got = c.ix.search_refine_batch(k, R, c.Q[:nq], c.lin)
            assert_same(got, tuple(a[:nq] for a in want[:3]) + (0,), f"{name} k={k} R={R} nq={nq}")
        # the property.  Tie-free: the k-th and (k + 1)-th exact distances differ (the exact top k is a set), and so do the k-th and
        # (k + 1)-th code distances (the plain top k is a set, and a subset of the R candidates).  An exact top-k record among the
        # candidates then has at most k candidates at or below its distance, so the queue of size k keeps it.
        pi, pd, pc = c.cands(k)
        p1 = c.cands(k + 1)
        checked = 0
        for q in range(c.nq):
            if xd[q, k - 1] == xd[q, k] or (p1[2][q] == k + 1 and p1[1][q, k - 1] == p1[1][q, k]):
                continue
            both = set(xi[q, :k].tolist()) & set(pi[q, :pc[q]].tolist())
            assert both <= set(want[0][q, :want[2][q]].tolist()), (name, k, R, q)
            checked += 1
        assert checked >= c.nq // 2, (name, k, R)


def test_tile_and_capacity_edges(built):
    """2. d128, w = C: the largest R, k = R, R around K11a's tile of 256 and around the capacities K11b's LDS arrays come in"""
    c = built("d128")
    c.set_w(c.C)
    for k, R, nq in [(100, 4095, 300), (4095, 4095, 60), (100, 255, 60), (100, 256, 60), (100, 257, 60), (100, 512, 60), (100, 513, 60),
                     (100, 1024, 60), (100, 1025, 60)]:
        want = rt.refine_batch(tuple(a[:nq] for a in c.cands(R)), c.base, c.Q[:nq], k)
        got = c.ix.search_refine_batch(k, R, c.Q[:nq], c.lin)
        assert_same(got, want, f"k={k} R={R}")
        assert (want[2] == k).all()


def test_short_lists(built):
    """3. d16, w = 1, R = 300: a list holds about 125 records, so the counts fall below R, and below k for k = 200"""
    c = built("d16")
    c.set_w(1)
    try:
        cands = c.cands(300)
        assert (cands[2] < 300).all()
        for k in (3, 200):
            want = rt.refine_batch(cands, c.base, c.Q, k)
            assert_same(c.ix.search_refine_batch(k, 300, c.Q, c.lin), want, f"k={k}")
        assert (want[2] < 200).any() and (want[2] == cands[2])[want[2] < 200].all()
    finally:
        c.set_w(c.C)


TIE_SEED = 12  # chosen on the CPU (the oracle over its own encoding of this problem): all 200 queries tie at the k boundary; asserted below


def test_ties(mi, oracle):
    """4. every vector four times on the d32_perm shape, k = 10, R = 101, 200 queries: the copies of a vector share their exact
    distance, and 10 = 4 + 4 + 2 cuts a group of four"""
    c = Case(mi, oracle, ROWS["d32_perm"], dup=4, seed=TIE_SEED)
    try:
        Q = c.Q[:200]
        cands = c.cands(101, Q)
        tied = rt.boundary_ties(cands, c.base, Q, 10)
        assert len(tied) >= 1, "no query has its 10th and 11th exact distances equal among its candidates"
        want = rt.refine_batch(cands, c.base, Q, 10)
        assert_same(c.ix.search_refine_batch(10, 101, Q, c.lin), want)
    finally:
        c.close()


def test_missing_rows(mi, built):
    """5. a Linear index with the first half of the vectors: the answers are the twin's on the filtered sequence and `missing` is
    its count; and an empty Linear index: everything is missing, every count 0"""
    c = built("d32_perm")
    c.set_w(c.C)
    half = c.n // 2
    lin = mi.Linear(c.D, c.n)
    lin._add_vectors(c.base[:half], None)
    empty = mi.Linear(c.D, c.n)
    try:
        for k, R in ((c.k, 4 * c.k + 1), (c.k, 257), (1, 1)):
            want = rt.refine_batch(c.cands(R), c.base, c.Q, k, n_lin=half)
            assert want[3] > 0
            assert_same(c.ix.search_refine_batch(k, R, c.Q, lin), want, f"k={k} R={R}")
            got = c.ix.search_refine_batch(k, R, c.Q, empty)
            assert (got[2] == 0).all() and (got[0] == -1).all() and np.isposinf(got[1]).all()
            assert got[3] == int(c.cands(R)[2].sum())
    finally:
        lin.close()
        empty.close()


@pytest.mark.parametrize("name", ["d16", "d64_short"])
def test_against_linear_itself(built, name):
    """6. R = n and w = C on tie-free data: the refined answer is mmidx_linear_search's on the same Linear handle, ids and bits"""
    c = built(name)
    c.set_w(c.C)
    assert c.n <= 4095
    Q = c.Q[:60]
    li, ld, lc = c.lin.search_batch(c.k + 1, Q)
    assert (lc == c.k + 1).all() and (ld[:, c.k - 1] != ld[:, c.k]).all()  # (tie-free at the boundary)
    got = c.ix.search_refine_batch(c.k, c.n, Q, c.lin)
    assert got[3] == 0
    assert_same(got, (li[:, :c.k], ld[:, :c.k], np.minimum(lc, c.k)))


def test_device_form(mi, built):
    """8. on a torch stream that is not the default one: bit-equal to the host form, with and without the missing counter; then an
    mmidx_linear_add_device on another stream, and a second refine sees the new rows"""
    import torch

    c = built("d128")
    c.set_w(c.C)
    L = mi.lib()
    k, R, nq = 10, 257, 64
    Q = c.Q[:nq]
    half = c.n // 2
    lin = mi.Linear(c.D, c.n)
    lin._add_vectors(c.base[:half], None)
    dev = torch.device("cuda", 0)
    s, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    try:
        host_half = c.ix.search_refine_batch(k, R, Q, lin)
        assert_same(host_half, rt.refine_batch(tuple(a[:nq] for a in c.cands(R)), c.base, Q, k, n_lin=half))
        assert host_half[3] > 0
        dQ = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        rest = torch.from_numpy(np.ascontiguousarray(c.base[half:])).to(dev)
        torch.cuda.synchronize()

        def run(with_missing):
            oi = torch.full((nq, k), 9, dtype=torch.int32, device=dev)
            od = torch.full((nq, k), 3.25, dtype=torch.float64, device=dev)
            oc = torch.full((nq,), 9, dtype=torch.int32, device=dev)
            om = torch.full((1,), 77, dtype=torch.int64, device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            st = L.mmidx_search_refine_device(c.ix._h, lin._h, k, R, nq, dQ.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                              om.data_ptr() if with_missing else None, s.cuda_stream)
            assert st == 0, L.mmidx_last_error()
            s.synchronize()
            return oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy(), int(om.cpu()[0])

        got = run(True)
        assert_same(got, host_half)
        got = run(False)
        assert_same(got[:3], host_half[:3])
        assert got[3] == 77  # (a null counter: nothing was written)
        # the other half arrives on another stream; the refine that follows on `s` waits for it
        assert L.mmidx_linear_add_device(lin._h, c.n - half, rest.data_ptr(), s2.cuda_stream) == 0
        got = run(True)
        assert_same(got, rt.refine_batch(tuple(a[:nq] for a in c.cands(R)), c.base, Q, k))
        assert got[3] == 0
        # and the wrapper
        with torch.cuda.stream(s):
            ti, td, tc, tm = c.ix.search_refine_batch_device(k, R, dQ, lin)
        s.synchronize()
        assert_same((ti.cpu().numpy(), td.cpu().numpy(), tc.cpu().numpy(), int(tm.cpu()[0])), got)
    finally:
        torch.cuda.synchronize()
        lin.close()


@pytest.mark.parametrize("name", ["d32_perm", "pq32_rot", "d24_perm"])
def test_ids_form(built, name):
    """9. the query is row iids[q] of the Linear index: parity with the twin fed that row, ids repeated inside the batch; an id
    outside the Linear index gives count 0 and padding and leaves the other rows alone"""
    c = built(name)
    c.set_w(c.C)
    rng = np.random.default_rng(7)
    ids = rng.integers(0, c.n, 50).astype(np.int32)
    ids[-1] = ids[0]
    ids[25] = ids[0]
    k, R = c.k, 4 * c.k + 1
    X = c.base[ids]
    cands = c.cands(R, X)
    want = rt.refine_batch(cands, c.base, X, k)
    got = c.ix.search_refine_ids_batch(k, R, ids, c.lin)
    assert_same(got, want)
    for bad in (c.n, -1, c.n + 1000):
        ids2 = ids.copy()
        ids2[3] = bad
        known = np.ones(len(ids), bool)
        known[3] = False
        got = c.ix.search_refine_ids_batch(k, R, ids2, c.lin)
        assert_same(got, rt.refine_batch(cands, c.base, X, k, known=known))
        assert got[2][3] == 0 and (got[0][3] == -1).all() and np.isposinf(got[1][3]).all()
    a = c.ix.computeNearestNeighborsRefined(k, R, str(int(ids[0])), c.lin)
    assert a.getIds() == [str(int(i)) for i in want[0][0, :want[2][0]]]
    assert np.array_equal(a.getDistances(), want[1][0, :want[2][0]])
    b = c.ix.computeNearestNeighborsRefined(k, R, X[1], c.lin)
    assert b.getIds() == [str(int(i)) for i in want[0][1, :want[2][1]]]


def test_refusals(mi, built):
    """10. every refused condition, each naming the offending value; both handles stay usable"""
    nat = importlib.import_module("multimedia-indexing_amd._native")
    c = built("d16")
    c.set_w(c.C)
    L = mi.lib()
    Q = np.ascontiguousarray(c.Q[:5])
    nq, k, R = 5, 3, 13
    oi, od, oc = np.full((nq, 8), 9, np.int32), np.full((nq, 8), 7.5), np.full(nq, 9, np.int32)
    miss = C.c_int64(55)
    ids = np.arange(nq, dtype=np.int32)
    other = mi.Linear(c.D + 1, 10)

    def calls(h, l, kk, RR):
        a = (oi.ctypes.data, od.ctypes.data, oc.ctypes.data)
        yield L.mmidx_search_refine(h, l, kk, RR, nq, Q.ctypes.data, *a, C.byref(miss))
        yield L.mmidx_search_refine_ids(h, l, kk, RR, nq, ids.ctypes.data, *a, C.byref(miss))
        yield L.mmidx_search_refine_device(h, l, kk, RR, nq, Q.ctypes.data, *a, None, None)  # (refused before a pointer is used)

    refused = [(None, c.lin._h, k, R, nat.ERR_INVALID_ARG, b"null index handle"), (c.ix._h, None, k, R, nat.ERR_INVALID_ARG, b"null Linear handle"),
               (c.ix._h, c.lin._h, 0, R, nat.ERR_INVALID_ARG, b"got 0"), (c.ix._h, c.lin._h, 5, 4, nat.ERR_INVALID_ARG, b"R = 4 is below k = 5"),
               (c.ix._h, c.lin._h, k, 4096, nat.ERR_INVALID_ARG, b"got 4096"),
               (c.ix._h, other._h, k, R, nat.ERR_INVALID_ARG, f"length {c.D}, the Linear handle of length {c.D + 1}".encode())]
    try:
        for h, l, kk, RR, status, text in refused:
            for st in calls(h, l, kk, RR):
                assert st == status and text in L.mmidx_last_error(), (kk, RR, text, L.mmidx_last_error())
        if L.mmidx_device_count() >= 2:  # handles on different devices
            far = mi.Linear(c.D, 10, device=1)
            for st in calls(c.ix._h, far._h, k, R):
                assert st == nat.ERR_INVALID_ARG and b"on device 0, the Linear handle on device 1" in L.mmidx_last_error()
            far.close()
        # a sharded handle (one virtual shard)
        sh = make_index(mi, c.p, c.kind, c.D, c.C, c.m, c.ks, c.n, c.tr, devices=[0])
        for st in calls(sh._h, c.lin._h, k, R):
            assert st == nat.ERR_UNSUPPORTED and b"takes a plain handle" in L.mmidx_last_error()
        sh.close()
        assert (oi == 9).all() and (od == 7.5).all() and (oc == 9).all() and miss.value == 55  # nothing was written
        # nq == 0
        assert L.mmidx_search_refine(c.ix._h, c.lin._h, k, R, 0, None, None, None, None, C.byref(miss)) == 0 and miss.value == 0
        assert L.mmidx_search_refine_device(c.ix._h, c.lin._h, k, R, 0, None, None, None, None, None, None) == 0
        # both handles still answer
        assert_same(c.ix.search_batch(k, c.Q), c.cands(k))
        li, ld, lc = c.lin.search_batch(1, c.base[:4])
        assert li[:, 0].tolist() == [0, 1, 2, 3] and (ld[:, 0] == 0.0).all()
        assert_same(c.ix.search_refine_batch(k, R, c.Q, c.lin), rt.refine_batch(c.cands(R), c.base, c.Q, k))
    finally:
        other.close()
