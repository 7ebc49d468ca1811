"""Fixtures of the symmetric-distance id queries (mmidx_search_sdc = PQ.computeKnnSDC, PQ.java:334-374), shared by
tests/test_sdc_cases_cpu.py and tests/test_gpu_sdc.py.  Pure numpy plus the oracle.

mmidx_search_sdc has no scan of its own: k_sdc_terms writes a [nq][m][ks][dsub] table of squared terms and search_common runs the
SDC = true instances of the exact scan and of the tie replay over it.  Every case below names the form it is meant to reach
(`reach`); the host mirrors (`plan`, `sdc_round`, `scan_instance`, `merge_instance`, `split_applies`, `labels`) restate the gates
of csrc/mmidx_api.hip (make_plan, launch_scan, the step's stage_pass_a / stage_pass_b_flat / stage_merge / stage_tie_replay, mmidx_search_sdc) and the CPU test holds every case to them.

The TWIN (`sdc_dists`, `sdc_twin`) is the independent statement of the answer: the full distance of every record as ONE chain
(s outer, t inner, one rounding per operation, no early abandon), then the bounded queue of np_twin.  The oracle
(mmo_pq_search_sdc, with the reference's early abandon) must equal it, and the library must equal the oracle.

The GENERATOR draws codes directly (no encoding, no k-means over the base) and plants groups of identical codes: identical codes
are the only exact ties of a continuous codebook, and they tie at every distance, not only at 0.  The codebook is one k-means
iteration over 2000 Gaussian rows."""
import functools

import numpy as np

import np_twin
import synth
from oracle import oracle as o

TR_NONE, TR_ROTATION, TR_PERMUTATION = 0, 1, 2
K_MAX = 4095           # MMIDX_K_MAX
SEG = 512              # MMIDX_SEG: codes per segment of k_scan (256 threads x 2)
HKEEP = 256            # MMIDX_HKEEP
LDS_BYTES = 160 * 1024
MIN_FLAT_CHUNK = 4096  # the smallest chunk option "flat_chunk" accepts
PASSB_SDC = "K3(exact scan: symmetric distances)"


# ---- host mirrors (csrc/mmidx_api.hip) ------------------------------------------------------------------------------------------
def cap_rule(k):
    """make_plan: the candidate buffer, the smallest power of two >= k + 1 + a segment"""
    cap = 1
    while cap < k + 1 + SEG:
        cap <<= 1
    return cap


def scan_lds_bytes(D, m, ks, transform, cap):
    """scan_lds_bytes: table + one vector (two with a transform) + (key, value) buffer + counters"""
    return m * ks * 8 + (2 if transform else 1) * D * 8 + cap * 12 + 16


def plan(D, m, ks, transform, n, k, nq, flat_chunk=0, sub_batch=0):
    """make_plan for a flat PQ handle of byte codes: dict(cap, lds, glut, chunk, nchunks, qb).  Without the option the chunk is 32768
    or 65536 codes (by batch size and the K3m tables): every case that leaves it alone has fewer codes than either.  sub_batch: the
    option of that name (tests/plan_model.py has the IVFPQ side)."""
    cap = cap_rule(k)
    lds = scan_lds_bytes(D, m, ks, transform, cap)
    glut = lds > LDS_BYTES  # the pl.glut predicate
    assert lds - m * ks * 8 <= LDS_BYTES
    if flat_chunk >= MIN_FLAT_CHUNK:
        chunk = min(flat_chunk, 1 << 23)
    else:
        chunk = 32768
        assert n <= chunk
    nchunks = (max(n, 1) + chunk - 1) // chunk
    poolq = min(nchunks * (k + 1) + HKEEP, max(n, k + 1))
    qb = min(nq, 1 << 30, max(1, (16 << 30) // (poolq * 16)))
    if glut:  # one table slot per block in global scratch: at most 2 GiB of it
        qb = min(qb, max(1, (2 << 30) // (m * ks * 8 * nchunks)))
    if sub_batch > 0:
        qb = min(qb, sub_batch)
    return dict(cap=cap, lds=lds, glut=glut, chunk=chunk, nchunks=nchunks, qb=qb)


def sdc_round(m, ks, dsub):
    """mmidx_search_sdc: ids per host round, at most 1 GiB of term tables"""
    return max(1, 2 ** 30 // (m * ks * dsub * 8))


def rounds_and_batches(pl_of, m, ks, dsub, nq):
    """(host rounds of mmidx_search_sdc, the largest number of sub-batches search_common makes of one round); pl_of(nb) = plan"""
    QB = sdc_round(m, ks, dsub)
    rounds = (nq + QB - 1) // QB
    most = 0
    for q0 in range(0, nq, QB):
        nb = min(QB, nq - q0)
        qb = pl_of(nb)["qb"]
        most = max(most, (nb + qb - 1) // qb)
    return rounds, most


def scan_instance(m):
    """launch_scan, SDC: the M of k_scan<M, uchar, 2, 256, true> (0: codes loaded without CodeVec)"""
    return m if m in (8, 16) else 0


def merge_instance(k):
    """(threads of k_merge, its buffer): <128> up to K1 = k + 1 = 128, else <256>; the smallest power of two >= 2 K1, 512 at least"""
    mcap = 512
    while mcap < 2 * (k + 1):
        mcap <<= 1
    return (128 if k + 1 <= 128 else 256), mcap


def split_applies(pl, m, ks, sdc, code_bytes=1, no_split_table=0):
    """scan_split_applies: k_scan_split (the table in two halves) serves pass A"""
    return bool(pl["glut"] and not sdc and not no_split_table and code_bytes == 1 and ks == 256 and m == 128 and
                pl["chunk"] <= m * ks and pl["lds"] - m * ks * 8 + 64 * 256 * 8 <= LDS_BYTES)


def labels(pl, m, ks, sdc=True):
    """(pass_a, pass_b) mmidx_get_dispatch reports after an SDC call (ADC calls of the same handle have more kernels to choose from)"""
    assert sdc
    if pl["glut"]:
        a = "K3(table in two halves)" if split_applies(pl, m, ks, sdc) else "K3(table in global scratch)"
    else:
        a = "K3" if pl["nchunks"] > 1 else "K3(single pass)"
    return a, (PASSB_SDC if pl["nchunks"] > 1 else "-")


# ---- the twin -------------------------------------------------------------------------------------------------------------------
def sdc_dists(pq, codes, iids):
    """[len(iids)][n] distances of every record to the records `iids`: (pq[s][c_s][t] - pq[s][q_s][t])^2 added s outer, t inner into
    one accumulator (numpy's elementwise a * a then += is one rounding per operation, no FMA)"""
    m, ks, dsub = pq.shape
    codes = np.asarray(codes)
    iids = np.asarray(iids, np.int64).reshape(-1)
    d = np.zeros((iids.shape[0], codes.shape[0]))
    for s in range(m):
        A = pq[s][codes[:, s]]        # [n][dsub]
        B = pq[s][codes[iids, s]]     # [nq][dsub]
        for t in range(dsub):
            df = A[None, :, t] - B[:, t, None]
            d += df * df
    return d


def sdc_twin(pq, codes, iid, k):
    """(ids best -> worst, distances) of computeKnnSDC(k, iid): full distances, then the bounded queue (np_twin.bpq_result)"""
    d = sdc_dists(pq, codes, [iid])[0]
    pos = np_twin.bpq_result(d, k)
    return pos.astype(np.int32), d[pos]


def padded(answers, k):
    """[(ids, dists)] -> (ids [nq][k] padded with -1, dists [nq][k] padded with +inf, counts [nq]): search_sdc_batch's layout"""
    ids = np.full((len(answers), k), -1, np.int32)
    ds = np.full((len(answers), k), np.inf)
    cnt = np.zeros(len(answers), np.int32)
    for j, (i, d) in enumerate(answers):
        cnt[j] = len(i)
        ids[j, :len(i)] = i
        ds[j, :len(i)] = d
    return ids, ds, cnt


# ---- the cases ------------------------------------------------------------------------------------------------------------------
N4 = 3 * MIN_FLAT_CHUNK + 77  # 12365: four chunks of 4096, the last one ragged
USUAL = lambda n: [0, 1, n // 2, n - 1, 17, 17, 3]  # noqa: E731


def _spread(n, g):
    return [int(x) for x in np.linspace(100, n - 10, g)]


# name -> dict(D, m, ks, n, flat_chunk, transform, groups [(positions)], calls [(n loaded, k, ids or a name resolved in case())],
#              ties [(call, query index)] claimed to tie at rank k, tie_chunks: those ties have members in >= 2 chunks,
#              reach dict(glut, nchunks, M, rounds, sub_batches, merge (a tuple: per call)))
CASES = {
    # <8> in pass A, the exact pass B over chunks 1-3; 25 duplicates over all four chunks: a tie at 0 for a member, and for `straddle`
    # (a few sub-quantizers away from the group: the group is its nearest neighbour) the whole group at one non-zero distance across
    # rank k.  A tie at 0 survives any order of the additions -- every term is 0 --, the one at a non-zero distance does not.
    "m8_chunks": dict(D=32, m=8, ks=256, n=N4, flat_chunk=4096, groups=[_spread(N4, 25)], straddle=(7000, 6), calls=[(N4, 10, "group+edges")],
                      ties=[(0, 0), (0, 1), (0, 2), (0, 3)], tie_chunks=True, reach=dict(glut=False, nchunks=4, M=8, merge=128)),
    # <16>, dsub 4; 120 duplicates: a tie at 0 of more than k for a member, and for `straddle` the whole group at one non-zero
    # distance across rank k
    "m16_chunks_ties": dict(D=64, m=16, ks=16, n=N4, flat_chunk=4096, groups=[_spread(N4, 120)], straddle=(7000, 8),
                            calls=[(N4, 50, "group+straddle")], ties=[(0, 0), (0, 1), (0, 2)], tie_chunks=True,
                            reach=dict(glut=False, nchunks=4, M=16, merge=128)),
    # <0> without GLUT, dsub 4, 4, 2, 1
    "generic_m4": dict(D=16, m=4, ks=16, n=3000, calls=[(3000, 7, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    "generic_m6": dict(D=24, m=6, ks=64, n=3000, calls=[(3000, 7, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    "generic_m32": dict(D=64, m=32, ks=256, n=3000, calls=[(3000, 7, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    "generic_m64": dict(D=64, m=64, ks=256, n=3000, calls=[(3000, 7, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    # 16 distinct codes of about 187 records: every answer is ties, the replay decides all of it -- at distance 0 with k = 100, inside
    # the records of the second nearest code with k = 250
    "ks_small": dict(D=8, m=4, ks=2, n=3000, calls=[(3000, 100, [0, 1, 2, 3, 1500, 2999]), (3000, 250, [0, 1, 2, 3, 1500, 2999])],
                     ties=[(c, j) for c in range(2) for j in range(6)],
                     reach=dict(glut=False, nchunks=1, M=0, merge=(128, 256))),
    # ks neither a power of two nor 256, dsub 5
    "ks_odd": dict(D=30, m=6, ks=100, n=3000, calls=[(3000, 10, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    # 128 KiB of table + a 4096-entry buffer > 160 KiB: the GLUT scan; 2500 duplicates > k: the GLUT tie replay
    "glut_big_k": dict(D=64, m=64, ks=256, n=5000, groups=[list(range(0, 5000, 2))], calls=[(5000, 2000, [0, 2, 4998, 1, 4999, 2501])],
                       ties=[(0, 0), (0, 1), (0, 2)], reach=dict(glut=True, nchunks=1, M=0, merge=256)),
    # ... and with dsub = 2 (at dsub = 1 there is no inner order to get wrong): the GLUT replay of a tie at a non-zero distance.  The
    # record next to the group is the last one, so it is offered when k ties are held and evicts the earliest of them: the kept ties
    # are not simply the first ones
    "glut_big_k_dsub2": dict(D=128, m=64, ks=256, n=5000, groups=[list(range(0, 5000, 2))], straddle=(4999, 24),
                             calls=[(5000, 2000, [0, 4999, 4998, 1])], ties=[(0, 0), (0, 1), (0, 2)], reach=dict(glut=True, nchunks=1, M=0, merge=256)),
    # 256 KiB of table: GLUT over three chunks (k_scan_split must not run); 25 duplicates
    "glut_m128": dict(D=128, m=128, ks=256, n=9000, flat_chunk=4096, groups=[_spread(9000, 25)], calls=[(9000, 10, "group+edges")],
                      ties=[(0, 0), (0, 1), (0, 2)], tie_chunks=True, reach=dict(glut=True, nchunks=3, M=0, merge=128)),
    # the largest buffers: k_merge<256> with 8192 entries; k > n: the count is n and the tail stays (-1, +inf)
    "k_max": dict(D=32, m=8, ks=256, n=5000, calls=[(5000, K_MAX, [0, 4999, 2500])], reach=dict(glut=False, nchunks=1, M=8, merge=256, mcap=8192)),
    "k_over_n": dict(D=32, m=8, ks=256, n=200, calls=[(200, 300, [0, 199, 100])], reach=dict(glut=False, nchunks=1, M=8, merge=256)),
    # K1 = 128 / 129: k_merge<128> against k_merge<256>
    "k_merge_127": dict(D=32, m=8, ks=256, n=3000, calls=[(3000, 127, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=8, merge=128)),
    "k_merge_128": dict(D=32, m=8, ks=256, n=3000, calls=[(3000, 128, USUAL(3000))], reach=dict(glut=False, nchunks=1, M=8, merge=256)),
    # nq = 600 = 2 x 256 + 88: three flag blocks of the replay, the last one partial; every third id is one of 10 duplicates or the
    # record two sub-quantizers away from them (k = 5)
    "many_ids": dict(D=16, m=4, ks=16, n=3000, groups=[_spread(3000, 10)], straddle=(2900, 2), calls=[(3000, 5, "every_third")],
                     reach=dict(glut=False, nchunks=1, M=0, merge=128)),
    # 2 MiB of terms per id: 512 ids per host round, id 513 is round two (about 1 GiB of device memory for the term tables)
    "second_round": dict(D=1024, m=8, ks=256, n=600, calls=[(600, 5, list(range(513)))], reach=dict(glut=False, nchunks=1, M=8, merge=128, rounds=2)),
    # GLUT with four chunks: 2 GiB / (256 KiB x 4) = 2048 ids per sub-batch of search_common, id 2049 starts the second one at
    # q0 = 2048 of the term table (about 2.6 GiB of device memory: table slots and terms)
    "sub_batches": dict(D=128, m=128, ks=256, n=N4, flat_chunk=4096, calls=[(N4, 10, "four_then_fifth")],
                        reach=dict(glut=True, nchunks=4, M=0, merge=128, sub_batches=2)),
    # three indexVectors calls (pending buffer, build_csr); SDC before and after the third, ids from the batch added last
    "after_adds": dict(D=32, m=8, ks=256, n=4500, by_vectors=1500, calls=[(3000, 10, [1500, 2999, 2000, 1499]), (4500, 10, [3000, 4499, 3700, 2999])],
                       reach=dict(glut=False, nchunks=1, M=8, merge=128)),
    # SDC ignores the transform; the LDS layout moves with it
    "transformed_perm": dict(D=32, m=8, ks=256, n=3000, transform=TR_PERMUTATION, calls=[(3000, 10, USUAL(3000))],
                             reach=dict(glut=False, nchunks=1, M=8, merge=128)),
    "transformed_rot": dict(D=32, m=8, ks=256, n=3000, transform=TR_ROTATION, calls=[(3000, 10, USUAL(3000))],
                            reach=dict(glut=False, nchunks=1, M=8, merge=128)),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, D, m, ks, dsub, n, flat_chunk, transform, rot, pq [m][ks][dsub], codes [n][m] (indices), X (after_adds: the vectors
    that encode to `codes`), groups, straddle (the record next to group 0, or None), calls [(n loaded, k, ids int32 array)], ties, tie_chunks, reach)"""
    spec = CASES[name]
    D, m, ks, n = spec["D"], spec["m"], spec["ks"], spec["n"]
    dsub = D // m
    rng = np.random.default_rng(5000 + NAMES.index(name))
    rows = rng.standard_normal((2000, D))
    pq = np.stack([synth.kmeans(rows[:, s * dsub:(s + 1) * dsub], ks, iters=1, seed=s) for s in range(m)])
    codes = rng.integers(0, ks, (n, m))
    groups = [np.asarray(g, np.int64) for g in spec.get("groups", [])]
    for g in groups:
        codes[g] = codes[g[0]]
    straddle = None
    if "straddle" in spec:
        # the group's code with the first `moved` sub-quantizers moved to their nearest other centroid: near enough for the group to be
        # this record's nearest neighbour, and `moved` * dsub non-zero terms, so that the order of the additions shows in the sum
        straddle, moved = spec["straddle"]
        codes[straddle] = codes[groups[0][0]]
        for s in range(moved):
            ds = ((pq[s] - pq[s][codes[straddle, s]]) ** 2).sum(1)
            ds[codes[straddle, s]] = np.inf
            codes[straddle, s] = int(np.argmin(ds))
    calls = []
    for nl, k, ids in spec["calls"]:
        if ids == "group+edges":
            g = groups[0]
            ids = [g[0], g[len(g) // 2], g[-1]] + ([straddle] if straddle is not None else []) + [0, 4095, 4096, 8191, 8192, nl - 1]
        elif ids == "group+straddle":
            g = groups[0]
            ids = [g[0], g[-1], straddle, 0, nl - 1]
        elif ids == "every_third":
            g = list(groups[0]) + [straddle]
            other = np.setdiff1d(np.arange(nl), g)
            pick = other[rng.integers(0, len(other), 40)]  # (40 distinct at most: the list repeats ids)
            ids = [g[(j // 3) % len(g)] if j % 3 == 0 else pick[rng.integers(0, 40)] for j in range(600)]
        elif ids == "four_then_fifth":
            four = [0, 4096, 8191, nl - 1]
            ids = [four[j % 4] for j in range(2048)] + [6000]
        calls.append((nl, k, np.asarray(ids, np.int32)))
    rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if spec.get("transform", 0) == TR_ROTATION else None
    X = None
    if "by_vectors" in spec:  # every vector IS the codebook rows of its code: distance 0 to them, so it encodes to that code
        X = np.concatenate([pq[s][codes[:, s]] for s in range(m)], axis=1)
    return dict(name=name, D=D, m=m, ks=ks, dsub=dsub, n=n, flat_chunk=spec.get("flat_chunk", 0), transform=spec.get("transform", TR_NONE),
                rot=rot, pq=pq, codes=codes, X=X, by_vectors=spec.get("by_vectors", 0), groups=groups, straddle=straddle, calls=calls,
                ties=spec.get("ties", []), tie_chunks=spec.get("tie_chunks", False), reach=spec["reach"])


def case_plan(c, call):
    """the plan of the first sub-batch of a call's first host round"""
    nl, k, ids = c["calls"][call]
    nb = min(len(ids), sdc_round(c["m"], c["ks"], c["dsub"]))
    return plan(c["D"], c["m"], c["ks"], c["transform"], nl, k, nb, c["flat_chunk"])


def oracle_index(c, n=None):
    """the oracle over the first n records of a case"""
    perm = o.random_permutation(1, c["D"]) if c["transform"] == TR_PERMUTATION else None  # (the library's own: java.util.Random seed 1)
    ref = o.OracleIndex(o.KIND_PQ, c["D"], c["m"], c["ks"], transform=c["transform"], perm=perm, rot=c["rot"])
    ref.set_pq(c["pq"])
    n = c["n"] if n is None else n
    ref.add_codes(np.arange(n), None, c["codes"][:n])
    return ref


def _by_unique(ids, k, one):
    """one(iid) for every distinct id, laid out for the whole list"""
    memo = {}
    return padded([memo[i] if i in memo else memo.setdefault(i, one(i)) for i in (int(x) for x in ids)], k)


@functools.lru_cache(maxsize=None)
def expected(name):
    """[(ids [nq][k], distances [nq][k], counts [nq])] per call: the oracle's search_sdc, computed once and left unchanged"""
    c = case(name)
    out = []
    for nl, k, ids in c["calls"]:
        ref = oracle_index(c, nl)
        res = _by_unique(ids, k, lambda i: ref.search_sdc(i, k))
        for a in res:
            a.setflags(write=False)
        out.append(res)
    return out


@functools.lru_cache(maxsize=None)
def twin_dists(name, call):
    """[distinct ids of the call][n loaded] full distances (the twin's), and the distinct ids"""
    c = case(name)
    nl, k, ids = c["calls"][call]
    uniq = np.unique(ids)
    return sdc_dists(c["pq"], c["codes"][:nl], uniq), uniq


def twin_expected(name, call):
    c = case(name)
    nl, k, ids = c["calls"][call]
    d, uniq = twin_dists(name, call)
    row = {int(u): j for j, u in enumerate(uniq)}

    def one(i):
        pos = np_twin.bpq_result(d[row[i]], k)
        return pos.astype(np.int32), d[row[i]][pos]

    return _by_unique(ids, k, one)
