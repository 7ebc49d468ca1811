"""Host mirror of make_plan (csrc/mmidx_api.hip) for an IVFPQ handle: how many queries `search_common` serves per sub-batch.

tests/sdc_cases.py::plan restates the flat PQ side; this is the IVFPQ side, with the caps in the order the source applies them:

  1. 2^30 / w pairs per sub-batch;
  2. a candidate pool of at most 16 GiB (16 bytes per entry, `poolq` entries per query);
  3. when the coarse stage runs inside the call: the [nq][C] matrix of exact coarse distances, 2 GiB where every row is written
     and read (the exact stage), 16 GiB where the certified stage only touches the rows that overflow -- but then never more than
     a quarter of the free device memory, never less than 2 GiB, and the free figure is only asked for when the call's own matrix
     would pass 2 GiB;
  4. when the lookup table lives in global scratch: 2 GiB of table slots, w x chunks of them per query;
  5. option "sub_batch" (> 0): at most that many.

Pure arithmetic: tests/test_plan_model_cpu.py pins the figures, tests/test_gpu_sub_batches.py sizes its calls by them."""
from sdc_cases import HKEEP, LDS_BYTES, cap_rule, scan_lds_bytes

BLOCK = 256        # MMIDX_BLOCK
CSEL_CAP = 1024    # MMIDX_CSEL_CAP
CAND_CHUNK = 24    # MMIDX_CAND_CHUNK
TERM_PAD = 1       # MMIDX_TERM_PAD
IVF_CHUNK = 16384  # codes per chunk of an inverted list
GIB = 1 << 30


def coarse_certified(D, C, w, exact_coarse=0):
    """coarse_certified: the certified coarse stage (K1c ... K1f) applies -- run_coarse's own test"""
    sel_fixed = CSEL_CAP * 12 + (w + 1) * 8 + ((w + 2) & ~1) * 4 + 16
    row_bytes = (D + TERM_PAD) * 8
    cch = CAND_CHUNK
    if sel_fixed + cch * row_bytes > 64 * 1024:
        cch = (64 * 1024 - sel_fixed) // row_bytes if sel_fixed < 64 * 1024 else 0
    alds = sel_fixed + max(cch, 1) * row_bytes
    return bool(not exact_coarse and C >= BLOCK and w + 1 <= BLOCK and C <= 64 * BLOCK and w >= 1 and cch >= 1 and alds <= 64 * 1024)


def ivf_plan(D, m, ks, C, w, n, max_list_len, k, nq, transform=0, need_coarse=True, exact_coarse=0, free_bytes=None, sub_batch=0):
    """make_plan for an IVFPQ handle of n records whose longest list has max_list_len: dict(cap, lds, glut, nchunks, nitems, poolq,
    certified, asks_free, qb).  free_bytes: what hipMemGetInfo would report free (None: enough for every cap)."""
    cap = cap_rule(k)
    lds = scan_lds_bytes(D, m, ks, transform, cap)
    glut = lds > LDS_BYTES
    assert not glut or lds - m * ks * 8 <= LDS_BYTES  # (else make_plan refuses the call)
    K1 = k + 1
    nchunks = (max(max_list_len, 1) + IVF_CHUNK - 1) // IVF_CHUNK
    nitems = w * nchunks
    poolq = min(nitems * K1 + HKEEP, max(n, K1))
    qb = min(nq, (1 << 30) // max(w, 1))
    qb = min(qb, max(1, (16 * GIB) // max(poolq * 16, 1)))
    certified = coarse_certified(D, C, w, exact_coarse)
    asks_free = False
    if need_coarse:
        cap_bytes = (16 if certified else 2) * GIB
        if cap_bytes > 2 * GIB and nq * C * 8 > 2 * GIB:
            asks_free = True
            if free_bytes is not None:
                cap_bytes = max(2 * GIB, min(cap_bytes, free_bytes // 4))
        qb = min(qb, max(1, cap_bytes // (C * 8)))
    if glut:
        qb = min(qb, max(1, (2 * GIB) // (m * ks * 8 * max(nitems, 1))))
    if sub_batch > 0:
        qb = min(qb, sub_batch)
    return dict(cap=cap, lds=lds, glut=glut, nchunks=nchunks, nitems=nitems, poolq=poolq, certified=certified, asks_free=asks_free, qb=qb)


def sub_batches(nq, qb):
    """[(q0, nb)] of search_common's loop"""
    return [(q0, min(qb, nq - q0)) for q0 in range(0, nq, qb)]
