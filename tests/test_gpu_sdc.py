"""mmidx_search_sdc (PQ.computeKnnSDC, PQ.java:334-374) on every scan form it reaches, against the CPU oracle: ids, distance bits and
counts compared with ==.  The cases, what each is meant to reach and the host mirrors that prove it on the CPU are in
tests/sdc_cases.py (checked by tests/test_sdc_cases_cpu.py); the oracle's answers are computed once per case and shared.

second_round needs about 1 GiB of device memory for its term tables, sub_batches about 2.6 GiB (2 GiB of it table slots the
symmetric scan reserves and never reads)."""
import numpy as np
import pytest

import sdc_cases as sc
from test_gpu_parity import mi  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 6, 10


def make_handle(mi, c, ks=None):
    ix = mi.PQ(c["D"], 1 << 30, False, "", c["m"], ks or c["ks"], c["transform"], 512, rot=c["rot"])
    if ks is None:
        ix.loadProductQuantizer(c["pq"])
    if c["flat_chunk"]:
        ix.set_option("flat_chunk", c["flat_chunk"])
    return ix


def load(mi, ix, c, lo, hi):
    """records lo .. hi: the stored codes through loadIndex, or (after_adds) their vectors through indexVectors, a batch a call"""
    if c["by_vectors"]:
        for a in range(lo, hi, c["by_vectors"]):
            b = min(hi, a + c["by_vectors"])
            assert ix.indexVectors([str(i) for i in range(a, b)], c["X"][a:b]) == b - a
    else:
        ix.loadIndex(mi.PQ.transformToByte(c["codes"][lo:hi]))


def same(got, want):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc)
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64))


@pytest.mark.parametrize("name", sc.NAMES)
def test_sdc_case(mi, oracle, name):
    c = sc.case(name)
    exp = sc.expected(name)
    ix = make_handle(mi, c)
    loaded = 0
    try:
        for call, (nl, k, ids) in enumerate(c["calls"]):
            if loaded < nl:
                load(mi, ix, c, loaded, nl)
                loaded = nl
            got = ix.search_sdc_batch(k, ids)
            d = ix.get_dispatch()
            same(got, exp[call])
            if k > nl:  # the tail past the count stays as the caller left it
                assert np.all(got[0][:, nl:] == -1) and np.all(np.isinf(got[1][:, nl:]))
            assert (d["pass_a"], d["pass_b"], d["pre"]) == sc.labels(sc.case_plan(c, call), c["m"], c["ks"]) + ("-",), d
    finally:
        ix.close()


# every one of these is gated off for symmetric distances (pass_a_rung and k3s_decide of the search step, launch_scan_grouped_flat, launch_scan_filtered):
# forced in turn, none may change an answer.  (name, forced value, default)
SWEEP = [("passa_hist", 1, -1), ("no_filter", 1, 0), ("no_grp", 1, 0), ("no_mfma", 1, 0), ("smin_pre", 1, -1), ("passb_small", 1, 1),
         ("passb_small", 0, 1), ("debug_sync", 1, 0)]


@pytest.mark.parametrize("name", ["m8_chunks", "m16_chunks_ties"])
def test_option_sweep(mi, oracle, name):
    c = sc.case(name)
    nl, k, ids = c["calls"][0]
    want = sc.expected(name)[0]
    ix = make_handle(mi, c)
    try:
        load(mi, ix, c, 0, nl)
        for opt, forced, default in SWEEP:
            ix.set_option(opt, forced)
            got = ix.search_sdc_batch(k, ids)
            d = ix.get_dispatch()
            ix.set_option(opt, default)
            same(got, want)
            assert (d["pass_a"], d["pass_b"], d["pre"]) == ("K3", sc.PASSB_SDC, "-"), (opt, d)
    finally:
        ix.close()


def test_sdc_interleaved_with_adc(mi, oracle):
    """ADC, SDC, the same ADC batch, SDC with another nq on one handle of four chunks: the two share ws_Q, the pool and the hint state"""
    c = sc.case("m8_chunks")
    nl, k, ids = c["calls"][0]
    ref = sc.oracle_index(c)
    rng = np.random.default_rng(99)
    Q = np.concatenate([rng.standard_normal((20, c["D"])),
                        np.concatenate([c["pq"][s][c["codes"][:20, s]] for s in range(c["m"])], axis=1) + 0.01 * rng.standard_normal((20, c["D"]))])
    want_adc = ref.search_batch(Q, k)
    ids2 = np.asarray([(j * 541) % nl for j in range(23)] + [int(c["groups"][0][3])], np.int32)
    want2 = sc.padded([ref.search_sdc(int(i), k) for i in ids2], k)
    ix = make_handle(mi, c)
    try:
        load(mi, ix, c, 0, nl)
        adc1 = ix.search_batch(k, Q)
        sdc1 = ix.search_sdc_batch(k, ids)
        adc2 = ix.search_batch(k, Q)
        sdc2 = ix.search_sdc_batch(k, ids2)
    finally:
        ix.close()
    same(adc1, want_adc)
    same(adc2, want_adc)
    same(adc2, adc1)
    same(sdc1, sc.expected("m8_chunks")[0])
    same(sdc2, want2)


def test_sdc_refusals(mi, oracle):
    c = sc.case("generic_m4")
    nl, k, ids = c["calls"][0]
    ix = make_handle(mi, c)
    try:
        load(mi, ix, c, 0, nl)
        for bad_k in (0, sc.K_MAX + 1):
            with pytest.raises(mi.MmidxError) as ei:
                ix.search_sdc_batch(bad_k, ids)
            assert ei.value.status == INVALID_ARG
        for bad_id in (nl, -1, -2 ** 31):
            with pytest.raises(mi.MmidxError) as ei:
                ix.search_sdc_batch(k, np.array([0, bad_id, 1], np.int32))
            assert ei.value.status == INVALID_ARG
        # nq = 0: OK, and nothing is written
        N = mi._native
        oi = np.full((2, k), -7, np.int32)
        od = np.full((2, k), -7.0)
        oc = np.full(2, -7, np.int32)
        q = np.zeros(2, np.int32)
        assert N.lib().mmidx_search_sdc(ix._h, k, 0, q.ctypes.data, oi.ctypes.data, od.ctypes.data, oc.ctypes.data) == 0
        assert np.all(oi == -7) and np.all(od == -7.0) and np.all(oc == -7)
        # ... and the handle still answers
        same(ix.search_sdc_batch(k, ids), sc.expected("generic_m4")[0])
    finally:
        ix.close()
    # short codes: the reference dereferences pqByteCodes unconditionally (PQ.java:350)
    sh = make_handle(mi, c, ks=512)
    try:
        rng = np.random.default_rng(3)
        sh.loadProductQuantizer(rng.standard_normal((c["m"], 512, c["dsub"])))
        sh.loadIndex(mi.PQ.transformToShort(rng.integers(0, 512, (300, c["m"]))))
        with pytest.raises(mi.MmidxError) as ei:
            sh.search_sdc_batch(3, np.array([0], np.int32))
        assert ei.value.status == UNSUPPORTED
    finally:
        sh.close()
    # IVFPQ: computeKnnIVFSDC is a stub (IVFPQ.java:509-511)
    iv = mi.IVFPQ(c["D"], 1 << 30, False, "", c["m"], c["ks"], 0, 4, 512)
    try:
        rng = np.random.default_rng(4)
        iv.loadCoarseQuantizer(rng.standard_normal((4, c["D"])))
        iv.loadProductQuantizer(c["pq"])
        iv.indexVectors([str(i) for i in range(200)], rng.standard_normal((200, c["D"])))
        with pytest.raises(mi.MmidxError) as ei:
            iv.search_sdc_batch(3, np.array([0], np.int32))
        assert ei.value.status == UNSUPPORTED
    finally:
        iv.close()
