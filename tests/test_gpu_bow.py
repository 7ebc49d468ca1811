"""GPU parity of the bag-of-words aggregation (mmidx_bow_*, frontend.BowAggregator) against the restatement of
BowAggregator.java:39-74 in tests/bow_twin.py.  Every value is an integer far below 2^53, so every comparison is np.array_equal:
there is no tolerance in this file."""
import ctypes as C
import importlib

import numpy as np
import pytest

from bow_twin import BowTwin

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 7, 300, 777, 20011)
LDS_MAX_NC = 40960  # K9a's envelope: 160 KiB of 32-bit counters


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


def _sets(rng, dl, sizes):
    sets = [rng.standard_normal((n, dl)) for n in sizes]
    for s in sets:  # SURF-like: L2-normalised descriptors
        if len(s):
            s /= np.linalg.norm(s, axis=1, keepdims=True)
    return sets


# compared images: all of them at the small vocabularies; at the two large ones the CPU twin costs 0.3 / 2 ms per descriptor, so the
# 20011-descriptor image is compared at 4096 words only and checked by its row sum at 65536
@pytest.mark.parametrize("nc,dl,compare", [(128, 64, range(6)), (20, 12, range(6)), (1, 8, range(6)), (4096, 64, range(6)),
                                           (65536, 32, range(5))])
def test_bow_hard_bit_exact(mi, oracle, nc, dl, compare):
    rng = np.random.default_rng(nc + dl)
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, SIZES)
    tw = BowTwin(oracle, cb)
    ref = {i: tw.aggregate(sets[i]) for i in compare}
    agg = mi.BowAggregator(cb)
    assert (agg.getVectorLength(), agg.getNumCentroids(), agg.getDescriptorLength()) == (nc, nc, dl)
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    assert mi.lib().mmidx_bow_get_dims(agg._h, C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (nc, dl, 1)
    variants = [(0, 0), (1, 0)] + ([(0, 1)] if nc <= LDS_MAX_NC else [])
    for exact, hist_global in variants:
        agg.set_option("exact", exact)
        agg.set_option("hist_global", hist_global)
        out = agg.aggregate_batch(sets)
        assert out.shape == (len(sets), nc)
        for i, r in ref.items():
            assert np.array_equal(out[i], r), (exact, hist_global, i)
        assert np.array_equal(out.sum(axis=1), [float(len(s)) for s in sets]), (exact, hist_global)  # hard: row sum = n_i
        assert np.array_equal(out, np.floor(out)) and out.min() >= 0.0
    agg.set_option("exact", 0)
    agg.set_option("hist_global", 0)
    assert np.array_equal(agg.aggregate(sets[3]), ref[3])
    with pytest.raises(mi.MmidxError) as ei:  # AFA:72-79
        agg.aggregate(np.zeros((3, dl + 1)))
    assert ei.value.status == 2 and str(ei.value) == "Descriptor length is incompatible with codebook centroid length!"
    with pytest.raises(mi.MmidxError):
        agg.set_option("no_such_option", 1)
    agg.close()


def test_bow_assignment_ties_first_centroid_wins(mi, oracle):
    """computeNearestCentroid (AFA:136-155) updates on `<` only: of several equally near centroids the FIRST wins.  Duplicate
    centroids and descriptors that coincide with centroids (the construction of test_vlad_assignment_ties_first_centroid_wins)."""
    rng = np.random.default_rng(9)
    nc, dl = 64, 64
    cb = rng.standard_normal((nc, dl))
    cb[40] = cb[3]
    cb[41] = cb[3]
    cb[10] = cb[50]
    sets = [np.concatenate([cb[[3, 50, 7]], cb[3:4] + 1e-9, rng.standard_normal((200, dl))]), cb[[40, 41, 10, 50]].copy(),
            np.concatenate([cb[[3, 50]]] * 60 + [rng.standard_normal((30, dl))])]
    tw = BowTwin(oracle, cb)
    ref = tw.aggregate_batch(sets)
    assert ref[1][3] == 2.0 and ref[1][10] == 2.0 and ref[1][40] == ref[1][41] == ref[1][50] == 0.0  # the first of the equals
    agg = mi.BowAggregator(cb)
    for exact, hist_global in ((0, 0), (1, 0), (0, 1), (1, 1)):
        agg.set_option("exact", exact)
        agg.set_option("hist_global", hist_global)
        assert np.array_equal(agg.aggregate_batch(sets), ref), (exact, hist_global)
    agg.close()


@pytest.mark.parametrize("nc,dl,k", [(128, 64, 2), (128, 64, 3), (128, 64, 10), (4096, 64, 2), (4096, 64, 3), (4096, 64, 10), (20, 12, 20)])
def test_bow_soft_bit_exact(mi, oracle, nc, dl, k):
    rng = np.random.default_rng(nc + dl + k)
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, (0, 1, 7, 300, 777))
    ref = BowTwin(oracle, cb, k).aggregate_batch(sets)
    agg = mi.BowAggregator(cb, k)
    for exact, hist_global in ((0, 0), (1, 0), (0, 1)):
        agg.set_option("exact", exact)
        agg.set_option("hist_global", hist_global)
        out = agg.aggregate_batch(sets)
        assert np.array_equal(out, ref), (exact, hist_global)
        assert np.array_equal(np.mod(out, dl), np.zeros_like(out))  # every (descriptor, neighbour) hit is worth dl (:47-51)
        assert np.array_equal(out.sum(axis=1), [float(len(s) * k * dl) for s in sets])
    if k == nc:  # every word is among the k nearest of every descriptor
        assert np.array_equal(out, np.outer([len(s) * dl for s in sets], np.ones(nc)))
    agg.close()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_bow_soft_ties_at_the_kth_position_follow_a1(mi, oracle, k):
    """Three identical centroids (3, 40, 41) and a pair (10, 50): for descriptors at or next to them the equal distances straddle the
    k-th position, and which of the equals is counted is the bounded queue's choice -- assumption A1, the oracle's default rule,
    the guarantee the coarse stage gives."""
    rng = np.random.default_rng(17)
    nc, dl = 64, 16
    cb = rng.standard_normal((nc, dl))
    cb[40] = cb[3]
    cb[41] = cb[3]
    cb[10] = cb[50]
    near = np.concatenate([cb[[3, 50, 40, 10]], cb[3:4] + 1e-3 * rng.standard_normal((20, dl)), cb[50:51] + 1e-3 * rng.standard_normal((20, dl))])
    sets = [near, rng.standard_normal((400, dl)), near[::-1].copy()]
    assert oracle.get_queue_rule() == 0
    ref = BowTwin(oracle, cb, k).aggregate_batch(sets)
    agg = mi.BowAggregator(cb, k)
    for exact, hist_global in ((0, 0), (1, 0), (0, 1)):
        agg.set_option("exact", exact)
        agg.set_option("hist_global", hist_global)
        assert np.array_equal(agg.aggregate_batch(sets), ref), (exact, hist_global)
    agg.close()


@pytest.mark.parametrize("nc,dl,k", [(128, 64, 1), (128, 64, 3), (50000, 16, 1), (1, 8, 1)])
def test_bow_device_form_equals_host_form(mi, nc, dl, k):
    """torch tensors, a non-default stream, inputs unchanged afterwards"""
    import torch

    rng = np.random.default_rng(nc + k)
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, (5, 0, 300, 41, 1, 800, 0))
    agg = mi.BowAggregator(cb, k)
    host = agg.aggregate_batch(sets)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    descs = np.concatenate(sets)
    dev = torch.device("cuda:0")
    d_off, d_descs = torch.from_numpy(off).to(dev), torch.from_numpy(descs).to(dev)
    d_out = torch.full((len(sets), nc), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        mi._native.check(mi.lib().mmidx_bow_aggregate_device(agg._h, len(sets), d_off.data_ptr(), d_descs.data_ptr(), 800, d_out.data_ptr(),
                                                             C.c_void_p(st.cuda_stream)))
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), host)
    assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_descs.cpu().numpy(), descs)
    # a sub-range of the images: the offsets stay absolute into d_descs
    d_out2 = torch.full((3, nc), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    mi._native.check(mi.lib().mmidx_bow_aggregate_device(agg._h, 3, d_off.data_ptr() + 8 * 2, d_descs.data_ptr(), 300, d_out2.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(d_out2.cpu().numpy(), host[2:5])
    agg.close()


@pytest.mark.parametrize("k", [1, 2])
def test_bow_chunked_images_equal_one_round(mi, k):
    rng = np.random.default_rng(23 + k)
    nc, dl = 300, 24
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, (12, 0, 0, 150, 1, 33, 0, 64, 7, 90, 2))
    assert len(sets) == 11
    agg = mi.BowAggregator(cb, k)
    one = agg.aggregate_batch(sets)
    for hist_global in (0, 1):
        agg.set_option("hist_global", hist_global)
        for chunk in (3, 1, 11, 0):
            agg.set_option("chunk_images", chunk)
            assert np.array_equal(agg.aggregate_batch(sets), one), (hist_global, chunk)
    with pytest.raises(mi.MmidxError):
        agg.set_option("chunk_images", -1)
    agg.close()


@pytest.mark.parametrize("nc,dl,k", [(128, 64, 1), (128, 64, 4), (50000, 8, 1), (1, 4, 1)])
def test_bow_only_empty_images(mi, nc, dl, k):
    agg = mi.BowAggregator(np.random.default_rng(1).standard_normal((nc, dl)), k)
    for hist_global in (0, 1):
        agg.set_option("hist_global", hist_global)
        out = agg.aggregate_batch([np.zeros((0, dl)), None, []])
        assert out.shape == (3, nc) and not out.any()
    assert agg.aggregate_batch([]).shape == (0, nc)
    agg.close()


@pytest.mark.parametrize("nc,dl,k", [(128, 64, 1), (128, 64, 3), (45000, 8, 1)])
def test_bow_repeat_calls_on_one_handle(mi, oracle, nc, dl, k):
    """two calls with different batch shapes: counters of the first must not show in the second"""
    rng = np.random.default_rng(nc + 7 * k)
    cb = rng.standard_normal((nc, dl))
    a = _sets(rng, dl, (400, 30, 0, 9))
    b = _sets(rng, dl, (2, 50))
    tw = BowTwin(oracle, cb, k)
    ra, rb = tw.aggregate_batch(a), tw.aggregate_batch(b)
    agg = mi.BowAggregator(cb, k)
    for hist_global in (0, 1):
        agg.set_option("hist_global", hist_global)
        assert np.array_equal(agg.aggregate_batch(a), ra)
        assert np.array_equal(agg.aggregate_batch(b), rb)
        assert np.array_equal(agg.aggregate_batch(a), ra)
    agg.close()


# K9a's second configuration: counters above 32 KiB run in 1024-thread blocks, above 64 KiB beyond the default limit of dynamic LDS
# (the launch raises it), up to nc = 40960 where they fill the 160 KiB.  10000 words = 40000 B (1024 threads, default limit),
# 20000 = 80000 B and 40960 = 163840 B (raised limit).  dl = 8 keeps the twin at 0.1 - 0.3 ms per descriptor: every image is
# compared, the 20011-descriptor one included.
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nc", [10000, 20000, 40960])
def test_bow_lds_form_large_vocabularies(mi, oracle, nc, k):
    dl = 8
    rng = np.random.default_rng(nc + k)
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, SIZES)
    ref = BowTwin(oracle, cb, k).aggregate_batch(sets)
    weight = 1 if k == 1 else dl
    assert np.array_equal(ref.sum(axis=1), [float(len(s) * k * weight) for s in sets])
    agg = mi.BowAggregator(cb, k)
    outs = {}
    for exact, hist_global in ((0, 0), (0, 1), (1, 0)):
        agg.set_option("exact", exact)
        agg.set_option("hist_global", hist_global)
        outs[exact, hist_global] = out = agg.aggregate_batch(sets)
        for i in range(len(sets)):
            assert np.array_equal(out[i], ref[i]), (exact, hist_global, i)
    assert np.array_equal(outs[0, 0], outs[0, 1])  # LDS form against the global form
    # a second call of another shape on the same handle: stale counters would show
    agg.set_option("exact", 0)
    agg.set_option("hist_global", 0)
    assert np.array_equal(agg.aggregate_batch(sets[:4]), ref[:4])
    agg.close()


def test_bow_soft_largest_k(mi, oracle):
    """k = 5459, the largest the create call accepts (the coarse stage's selection holds k + 1 entries in a 64 KiB block)"""
    nc, dl, k = 6000, 4, 5459
    rng = np.random.default_rng(5459)
    cb = rng.standard_normal((nc, dl))
    sets = _sets(rng, dl, (0, 3, 40))
    ref = BowTwin(oracle, cb, k).aggregate_batch(sets)
    agg = mi.BowAggregator(cb, k)
    for hist_global in (0, 1):
        agg.set_option("hist_global", hist_global)
        out = agg.aggregate_batch(sets)
        assert np.array_equal(out, ref), hist_global
        assert np.array_equal(out.sum(axis=1), [float(len(s) * k * dl) for s in sets])
    agg.close()
    with pytest.raises(mi.MmidxError) as ei:
        mi.BowAggregator(cb, k + 1)
    assert ei.value.status == 10


def test_bow_device_calls_on_two_streams_and_one_image(mi):
    """two device calls on one handle from different streams, back to back, share the cell buffer: the second waits for the first;
    nimg = 1 takes the single 16-byte read-back of its descriptor range"""
    import torch

    rng = np.random.default_rng(77)
    nc, dl = 512, 32
    cb = rng.standard_normal((nc, dl))
    a, b = _sets(rng, dl, (3000, 10, 0, 2500)), _sets(rng, dl, (1700,))
    agg = mi.BowAggregator(cb, 2)
    ha, hb = agg.aggregate_batch(a), agg.aggregate_batch(b)
    dev = torch.device("cuda:0")

    def pack(sets):
        off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
        return torch.from_numpy(off).to(dev), torch.from_numpy(np.concatenate(sets)).to(dev), torch.full((len(sets), nc), -1.0, dtype=torch.float64, device=dev)

    (oa, da, ra), (ob, db, rb) = pack(a), pack(b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    L = mi.lib()
    for hist_global in (0, 1):
        agg.set_option("hist_global", hist_global)
        ra.fill_(-1.0)
        rb.fill_(-1.0)
        torch.cuda.synchronize()
        mi._native.check(L.mmidx_bow_aggregate_device(agg._h, len(a), oa.data_ptr(), da.data_ptr(), 3000, ra.data_ptr(), C.c_void_p(s1.cuda_stream)))
        mi._native.check(L.mmidx_bow_aggregate_device(agg._h, 1, ob.data_ptr(), db.data_ptr(), 1700, rb.data_ptr(), C.c_void_p(s2.cuda_stream)))
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(ra.cpu().numpy(), ha) and np.array_equal(rb.cpu().numpy(), hb), hist_global
    agg.close()
