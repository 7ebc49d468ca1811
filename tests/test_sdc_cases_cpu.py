"""The fixtures of tests/sdc_cases.py, checked on the CPU: the oracle's mmo_pq_search_sdc (with the reference's early abandon) equals
the plain twin on every case, every claimed tie is one, the host mirrors place every case in the kernel form it names, and the twin
tells itself from three wrong restatements."""
from fractions import Fraction

import numpy as np
import pytest

import np_twin
import sdc_cases as sc


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_equals_twin(oracle, name):
    """ids, distance bits and counts of every call"""
    c = sc.case(name)
    exp = sc.expected(name)
    for call, (nl, k, ids) in enumerate(c["calls"]):
        ti, td, tc = sc.twin_expected(name, call)
        oi, od, oc = exp[call]
        assert np.array_equal(oc, tc) and np.array_equal(oc, np.full(len(ids), min(k, nl)))
        assert np.array_equal(oi, ti)
        assert np.array_equal(od.view(np.uint64), td.view(np.uint64))
        assert np.all(oi[:, min(k, nl):] == -1) and np.all(np.isinf(od[:, min(k, nl):]))
        # the query's own record is at distance 0 (among more than k duplicates it need not be one of those kept)
        assert np.all(od[:, 0] == 0.0)


def test_single_query_twin_is_the_batched_one():
    c = sc.case("m16_chunks_ties")
    nl, k, ids = c["calls"][0]
    ti, td, _ = sc.twin_expected("m16_chunks_ties", 0)
    for j in (0, 2):
        i1, d1 = sc.sdc_twin(c["pq"], c["codes"], int(ids[j]), k)
        assert np.array_equal(i1, ti[j]) and np.array_equal(d1, td[j])


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.CASES[n].get("ties")])
def test_claimed_ties_are_ties(name):
    """the k-th and (k + 1)-th distances are equal; where the case says so the tied records lie in at least two chunks"""
    c = sc.case(name)
    for call, j in c["ties"]:
        nl, k, ids = c["calls"][call]
        d, uniq = sc.twin_dists(name, call)
        row = d[list(uniq).index(ids[j])]
        srt = np.sort(row)
        assert srt[k - 1] == srt[k], (name, call, j)
        if c["tie_chunks"]:
            chunks = np.unique(np.nonzero(row == srt[k - 1])[0] // sc.case_plan(c, call)["chunk"])
            assert len(chunks) >= 2, (name, call, j)


def test_tie_details(oracle):
    # m8_chunks: the 25 duplicates cover all four chunks
    c = sc.case("m8_chunks")
    assert sorted(set(int(p) // 4096 for p in c["groups"][0])) == [0, 1, 2, 3]
    # m16_chunks_ties: a member ties at 0 with more than k records; for `straddle` the group sits at one non-zero distance across rank k
    c = sc.case("m16_chunks_ties")
    nl, k, ids = c["calls"][0]
    d, uniq = sc.twin_dists("m16_chunks_ties", 0)
    member, straddle = d[list(uniq).index(ids[0])], d[list(uniq).index(ids[2])]
    assert np.count_nonzero(member == 0.0) >= 120 > k
    g = straddle[c["groups"][0]]
    assert np.all(g == g[0]) and g[0] > 0.0
    assert np.count_nonzero(straddle < g[0]) < k < np.count_nonzero(straddle <= g[0])
    # ks_small: 16 distinct codes of about 3000 / 16 = 187 records each, so the k-th distance of every id is 0 and more than k = 100 hold it
    c = sc.case("ks_small")
    nl, k, ids = c["calls"][0]
    assert len(np.unique(c["codes"], axis=0)) == 16
    d, uniq = sc.twin_dists("ks_small", 0)
    for row in d:
        assert np.sort(row)[k - 1] == 0.0 and k < np.count_nonzero(row == 0.0) < 2 * k
    # glut_big_k: 2500 duplicates, more than k = 2000
    c = sc.case("glut_big_k")
    d, uniq = sc.twin_dists("glut_big_k", 0)
    assert np.count_nonzero(d[0] == 0.0) >= 2500 > c["calls"][0][1]
    # many_ids: three flag blocks, the last one partial; about a third of the queries tie at rank k; ids repeat
    c = sc.case("many_ids")
    nl, k, ids = c["calls"][0]
    assert len(ids) == 600 and 2 * 256 < len(ids) < 3 * 256 and len(np.unique(ids)) < len(ids)
    d, uniq = sc.twin_dists("many_ids", 0)
    srt = np.sort(d, axis=1)
    tied = dict(zip(uniq.tolist(), (srt[:, k - 1] == srt[:, k]).tolist()))
    flagged = sum(tied[int(i)] for i in ids)
    assert 180 <= flagged <= 270, flagged
    for blk in range(3):  # every block of 256 flags has flagged and unflagged queries
        fl = [tied[int(i)] for i in ids[blk * 256:(blk + 1) * 256]]
        assert any(fl) and not all(fl)
    # second_round / sub_batches: the id that starts the second round / sub-batch differs from id 0 (a wrong q0 offset shows)
    for name, at in (("second_round", 512), ("sub_batches", 2048)):
        c = sc.case(name)
        ids = c["calls"][0][2]
        assert len(ids) == at + 1 and ids[at] != ids[0]
        e = sc.expected(name)[0]
        assert not np.array_equal(e[0][at], e[0][0])


@pytest.mark.parametrize("name", sc.NAMES)
def test_mirrors_place_the_case(name):
    """GLUT or not, number of chunks, M instance, host rounds, sub-batches, merge instance -- and the labels they imply"""
    c = sc.case(name)
    r = c["reach"]
    for call, (nl, k, ids) in enumerate(c["calls"]):
        pl = sc.case_plan(c, call)
        assert pl["glut"] == r["glut"]
        assert pl["nchunks"] == r["nchunks"]
        assert sc.scan_instance(c["m"]) == r["M"]
        threads, mcap = sc.merge_instance(k)
        assert threads == (r["merge"][call] if isinstance(r["merge"], tuple) else r["merge"]) and mcap == r.get("mcap", mcap)
        rounds, batches = sc.rounds_and_batches(lambda nb: sc.plan(c["D"], c["m"], c["ks"], c["transform"], nl, k, nb, c["flat_chunk"]),
                                                c["m"], c["ks"], c["dsub"], len(ids))
        assert rounds == r.get("rounds", 1) and batches == r.get("sub_batches", 1)
        assert not sc.split_applies(pl, c["m"], c["ks"], sdc=True)
        a, b = sc.labels(pl, c["m"], c["ks"])
        assert a == ("K3(table in global scratch)" if r["glut"] else ("K3" if r["nchunks"] > 1 else "K3(single pass)"))
        assert b == (sc.PASSB_SDC if r["nchunks"] > 1 else "-")


def test_mirror_values():
    assert [sc.cap_rule(k) for k in (1, 10, 511, 512, 2000, 3583, 3584, 4095)] == [1024, 1024, 1024, 2048, 4096, 4096, 8192, 8192]
    assert sc.scan_lds_bytes(64, 64, 256, 0, 4096) == 131072 + 512 + 49152 + 16 > sc.LDS_BYTES
    assert sc.scan_lds_bytes(32, 8, 256, 2, 1024) - sc.scan_lds_bytes(32, 8, 256, 0, 1024) == 32 * 8  # the transform's second vector
    assert sc.sdc_round(8, 256, 128) == 512 and sc.sdc_round(128, 256, 1) == 4096 and sc.sdc_round(8, 256, 4) == 16384
    assert sc.merge_instance(127) == (128, 512) and sc.merge_instance(128) == (256, 512) and sc.merge_instance(4095) == (256, 8192)
    assert sc.plan(128, 128, 256, 0, sc.N4, 10, 4096, 4096)["qb"] == 2048
    # the two-halves kernel: ADC only, and only while a chunk's partial sums fit the block's table slot (chunk <= m * ks = 32768)
    for chunk, sdc, want in ((4096, False, True), (32768, False, True), (36864, False, False), (4096, True, False)):
        pl = sc.plan(128, 128, 256, 0, 40000, 10, 12, chunk)
        assert pl["glut"] and sc.split_applies(pl, 128, 256, sdc) == want
    assert not sc.split_applies(sc.plan(128, 128, 256, 0, 9000, 10, 12, 4096), 128, 256, False, no_split_table=1)
    # ... and not where k + 1 + 512 candidates do not fit next to half a table
    assert not sc.split_applies(sc.plan(128, 128, 256, 0, 9000, 4095, 12, 4096), 128, 256, False)


def _dists_t_descending(pq, codes, iid):
    """s outer, t from dsub - 1 down to 0"""
    m, ks, dsub = pq.shape
    d = np.zeros(codes.shape[0])
    for s in range(m):
        for t in range(dsub - 1, -1, -1):
            df = pq[s][codes[:, s], t] - pq[s][codes[iid, s], t]
            d += df * df
    return d


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.CASES[n].get("straddle")])
def test_straddle_tie_shows_the_inner_order(name):
    """The record next to the group: the group is at one non-zero distance across rank k, and that distance has other bits when every
    sub-quantizer's terms are added last to first -- a tie replay that recomputes the distances in another order cannot find the tie.
    (A tie at distance 0 cannot show this: all its terms are 0.)"""
    c = sc.case(name)
    nl, k, ids = c["calls"][0]
    assert c["straddle"] in ids
    d, uniq = sc.twin_dists(name, 0)
    row = d[list(uniq).index(c["straddle"])]
    g = row[c["groups"][0]]
    assert np.all(g == g[0]) and g[0] > 0.0
    assert np.count_nonzero(row < g[0]) < k < np.count_nonzero(row <= g[0])
    assert _dists_t_descending(c["pq"], c["codes"], c["straddle"])[c["groups"][0][0]] != g[0]
    # it is offered after k members of the group: it evicts the tie inserted first, so the kept ties are not the first k - 1 offered
    members = c["groups"][0]
    assert np.count_nonzero(members < c["straddle"]) >= k
    ti = sc.twin_expected(name, 0)[0][list(ids).index(c["straddle"])]
    assert members[0] not in ti and np.count_nonzero(np.isin(ti, members)) == k - np.count_nonzero(row < g[0])


# ---- three wrong restatements ---------------------------------------------------------------------------------------------------
def _dists_t_outer(pq, codes, iid):
    m, ks, dsub = pq.shape
    d = np.zeros(codes.shape[0])
    for t in range(dsub):
        for s in range(m):
            df = pq[s][codes[:, s], t] - pq[s][codes[iid, s], t]
            d += df * df
    return d


def _dists_fma(pq, codes, iid):
    """d = fma(df, df, d): the product unrounded (exact rational arithmetic, one rounding per step)"""
    m, ks, dsub = pq.shape
    out = np.zeros(codes.shape[0])
    for i in range(codes.shape[0]):
        acc = 0.0
        for s in range(m):
            for t in range(dsub):
                df = float(pq[s][codes[i, s], t] - pq[s][codes[iid, s], t])
                acc = float(Fraction(df) * Fraction(df) + Fraction(acc))
        out[i] = acc
    return out


def test_twin_rejects_wrong_restatements():
    # t outer, s inner: other distance bits (dsub = 4, m = 16)
    c = sc.case("m16_chunks_ties")
    nl, k, ids = c["calls"][0]
    ti, td, _ = sc.twin_expected("m16_chunks_ties", 0)
    j = 3  # id 0: no tie, the answer is decided by the distances alone
    d = _dists_t_outer(c["pq"], c["codes"], int(ids[j]))
    pos = np_twin.bpq_result(d, k)
    assert not np.array_equal(d[pos], td[j])
    # a fused multiply-add: other distance bits
    c = sc.case("generic_m4")
    nl, k, ids = c["calls"][0]
    ti, td, _ = sc.twin_expected("generic_m4", 0)

    def fma_differs(j):
        d = _dists_fma(c["pq"], c["codes"], int(ids[j]))
        return not np.array_equal(d[np_twin.bpq_result(d, k)], td[j])

    assert any(fma_differs(j) for j in range(len(ids)))  # (16 terms a distance: not every answer of seven has a bit to lose)
    # a queue whose ties go to the later offer (the same queue fed from the far end): other ids among the 25 duplicates
    c = sc.case("m8_chunks")
    nl, k, ids = c["calls"][0]
    ti, td, _ = sc.twin_expected("m8_chunks", 0)
    d, uniq = sc.twin_dists("m8_chunks", 0)
    row = d[list(uniq).index(ids[0])]
    late = (nl - 1 - np_twin.bpq_result(row[::-1], k)).astype(np.int32)
    assert np.array_equal(row[late], td[0]) and not np.array_equal(np.sort(late), np.sort(ti[0]))
    assert np.array_equal(np.sort(ti[0]), c["groups"][0][:k])  # (the rule keeps the k members offered first)


def test_by_vectors_case_encodes_to_its_codes(oracle):
    """after_adds: the vectors are the codebook rows of their codes, so the encoder returns those codes"""
    c = sc.case("after_adds")
    ref = oracle.OracleIndex(oracle.KIND_PQ, c["D"], c["m"], c["ks"])
    ref.set_pq(c["pq"])
    for i in (0, 1499, 1500, 2999, 3000, 4499):
        assert np.array_equal(ref.encode(c["X"][i])[1], c["codes"][i])
