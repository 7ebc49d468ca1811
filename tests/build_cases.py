"""Fixtures of the index BUILD path, shared by tests/test_build_cases_cpu.py and tests/test_gpu_build.py: the assignment (K6a' from
rows / from copies, K6a, the exact kernel), the product quantisation (K6b' / K6b) and the CSR placement.  Pure numpy plus the oracle.

Expected cells and codes are the oracle's (OracleIndex.encode_batch: sequential fp64, the first index wins a tie); the expected
export is the stable sort of the oracle's (cell, stored code, id) records by cell.  The numpy twin below accumulates dimension by
dimension in the oracle's order (one rounding per operation, no np.sum): it stands in for the oracle on the one fixture of more than
2^18 rows, and with last_wins=True it is the wrong encoder the tie fixtures must tell from the right one.

ENCODER rows: every codebook carries duplicated rows, and the first TIE_ROWS vectors are built so that a duplicated row is the
nearest in one sub-quantizer -- the transformed residual is that row plus noise far below the row spacing, mapped back through the
permutation / rotation and subtracted from a coarse centroid far from all others.
ASSIGN rows: the inputs of test_gpu_parity.test_assignment_kernel_ties_and_padding (duplicated centroids, rows on them, a 1e-13 near
tie, noisy rows, far rows) plus 300 near_ties.midpoints."""
import functools

import numpy as np

import near_ties
from oracle import oracle as o
from test_coarse_bound_cpu import filter_eps_split16, filter_norms_usable, filter_underflow_eps

KIND_PQ, KIND_IVFPQ = 1, 2
TR_NONE, TR_ROTATION, TR_PERMUTATION = 0, 1, 2
ENC_N, ENC_C, TIE_ROWS = 521, 7, 64  # 521 = 2 * 256 + 9 = 65 * 8 + 1: K6b' (256 rows a block) and K6b (8) both end on a partial block

# (name, kind, D, m, ks, transform, expected `encode`)
ENCODER = [
    ("d4_byte", KIND_IVFPQ, 16, 4, 256, TR_NONE, "K6b'"),
    ("d8_byte_ks64_perm", KIND_IVFPQ, 32, 4, 64, TR_PERMUTATION, "K6b'"),
    ("d16_byte_flat", KIND_PQ, 32, 2, 256, TR_NONE, "K6b'"),
    ("d4_short_perm", KIND_IVFPQ, 16, 4, 300, TR_PERMUTATION, "K6b'"),
    ("d8_short_flat", KIND_PQ, 32, 4, 512, TR_NONE, "K6b'"),
    ("d16_short_under_64k", KIND_IVFPQ, 32, 2, 500, TR_NONE, "K6b'"),  # 500 * 128 + 256 * 2 * 2 = 65024 <= 65536
    ("d16_short_over_64k", KIND_IVFPQ, 32, 2, 512, TR_NONE, "K6b"),    # the same shape 1024 bytes over the limit
    ("d8_rot", KIND_IVFPQ, 32, 4, 256, TR_ROTATION, "K6b"),
    ("d3", KIND_IVFPQ, 24, 8, 256, TR_NONE, "K6b"),
    ("d3_short_3strides", KIND_IVFPQ, 24, 8, 700, TR_NONE, "K6b"),     # three strides of 256 per thread
    ("d12_flat_perm", KIND_PQ, 96, 8, 64, TR_PERMUTATION, "K6b"),
    ("d32_ks16", KIND_IVFPQ, 64, 2, 16, TR_NONE, "K6b"),               # most lanes own no centroid
    ("d1_ks2_flat", KIND_PQ, 8, 8, 2, TR_NONE, "K6b"),
]

# (name, D, C, options, rows 8 bytes past a 16-byte boundary through mmidx_assign_device, expected `assign`)
ASSIGN = [
    ("d128", 128, 1000, (), False, "K6a'(rows)"),
    ("d24_one_step", 24, 5000, (), False, "K6a'(rows)"),     # one k step, the last 8-lane group zero-filled
    ("d64_pad127", 64, 257, (), False, "K6a'(rows)"),        # 127 padding centroids
    ("d100", 100, 384, (), False, "K6a'(copies)"),           # D % 8 != 0, one chunk, zero fill
    ("d130_two_chunks", 130, 260, (), False, "K6a'(copies)"),
    ("d260_three_chunks", 260, 300, (), False, "K6a'(copies)"),
    ("d128_misaligned", 128, 1000, (), True, "K6a'(copies)"),
    ("d32_v1", 32, 300, (("coarse_v1", 1),), False, "K6a"),
    ("d32_exact", 32, 300, (("exact_coarse", 1),), False, "exact"),
    ("d32_one_cell", 32, 1, (), False, "exact"),
]
ASSIGN_SIZES = (1, 127, 128, 129, None)  # None: the full set
CERTIFIED = ("K6a'(rows)", "K6a'(copies)", "K6a")


# ---- the two gates, as assign_device / encode_device have them (csrc/mmidx_api.hip; DESIGN.md section 5.0, "build") -------------
def assign_gate(kind, D, C, options=(), aligned=True):
    if kind != KIND_IVFPQ:
        return "-"
    opt = dict(options)
    split16 = not opt.get("coarse_v1", 0)
    asg_lds = ((64 * (D + 2) + 3) & ~3) * 4 + 32 * 256 * 4  # K6a holds 64 whole vectors and a 32 x 256 centroid tile in LDS
    if not opt.get("exact_coarse", 0) and (split16 or asg_lds <= 160 * 1024) and C >= 2:
        if not split16:
            return "K6a"
        Dp = (D + 31) // 32 * 32
        return "K6a'(rows)" if Dp <= 128 and D % 8 == 0 and aligned else "K6a'(copies)"
    return "exact"


def code_bytes(ks):
    return 1 if ks <= 256 else 2


def encode_gate(D, m, ks, transform):
    dsub = D // m
    if transform in (TR_NONE, TR_PERMUTATION) and dsub in (4, 8, 16) and ks * dsub * 8 + 256 * m * code_bytes(ks) <= 65536:
        return "K6b'"
    return "K6b"


# ---- the numpy twin -------------------------------------------------------------------------------------------------------------
def sqdist_seq(X, Cn):
    """[n][C] squared distances, accumulated dimension by dimension in fp64 as the oracle's loops do"""
    d = np.zeros((X.shape[0], Cn.shape[0]))
    for j in range(X.shape[1]):
        df = Cn[None, :, j] - X[:, j, None]
        d += df * df
    return d


def _argmin(d, last_wins):
    return d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1) if last_wins else np.argmin(d, axis=1)


def twin_assign(X, coarse, last_wins=False):
    return _argmin(sqdist_seq(X, coarse), last_wins).astype(np.int32)


def twin_encode(X, coarse, pq, transform=TR_NONE, perm=None, rot=None, last_wins=False, chunk=1 << 16):
    """(cells [n] (-1 without a coarse quantizer), code indices [n][m]) of mmo_index_encode, vectorised over the rows; last_wins
    breaks the tie rule of both argmins on purpose"""
    X = np.ascontiguousarray(X, np.float64)
    m, ks, dsub = pq.shape
    cells = np.full(X.shape[0], -1, np.int32)
    codes = np.zeros((X.shape[0], m), np.int32)
    for i0 in range(0, X.shape[0], chunk):
        x = X[i0:i0 + chunk]
        if coarse is not None:
            c = twin_assign(x, coarse, last_wins)
            cells[i0:i0 + chunk] = c
            r = coarse[c] - x  # (the reference's sign: centroid - vector)
        else:
            r = x
        if transform == TR_PERMUTATION:
            r = r[:, perm]
        elif transform == TR_ROTATION:
            t = np.zeros_like(r)
            for i in range(r.shape[1]):  # sequential over the row index of the matrix, as mmo_rotate
                t += r[:, i, None] * rot[i][None, :]
            r = t
        for s in range(m):
            codes[i0:i0 + chunk, s] = _argmin(sqdist_seq(r[:, s * dsub:(s + 1) * dsub], pq[s]), last_wins)
    return cells, codes


def stored(codes, ks):
    """code indices -> the stored form (PQ.java:544-558): int8 index - 128 / int16 index"""
    codes = np.asarray(codes, np.int32)
    return (codes - 128).astype(np.int8) if ks <= 256 else codes.astype(np.int16)


def expected_export(cells, codes, ids, nlists, ks):
    """(list_off [nlists + 1], ids, stored codes) of records that arrived in the given order: the stable sort by cell (flat PQ: one list)"""
    cells = np.zeros(len(ids), np.int64) if nlists == 1 else np.asarray(cells, np.int64)
    order = np.argsort(cells, kind="stable")
    off = np.zeros(nlists + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(cells, minlength=nlists))
    return off, np.asarray(ids, np.int32)[order], stored(codes, ks)[order]


# ---- the oracle over a fixture -------------------------------------------------------------------------------------------------
def oracle_index(kind, D, m, ks, C, transform, coarse, pq, rot):
    perm = o.random_permutation(1, D) if transform == TR_PERMUTATION else None  # (the library's own: java.util.Random seed 1)
    ref = o.OracleIndex(kind, D, m, ks, C if kind == KIND_IVFPQ else 0, transform=transform, perm=perm, rot=rot)
    if kind == KIND_IVFPQ:
        ref.set_coarse(coarse)
    ref.set_pq(pq)
    return ref, perm


def make_index(mi, kind, D, m, ks, C, transform, coarse, pq, rot, options=()):
    """the GPU handle over the same quantizers (mi: the package)"""
    if kind == KIND_IVFPQ:
        ix = mi.IVFPQ(D, 1 << 30, False, "", m, ks, transform, C, 512, rot=rot)
        ix.loadCoarseQuantizer(coarse)
    else:
        ix = mi.PQ(D, 1 << 30, False, "", m, ks, transform, 512, rot=rot)
    ix.loadProductQuantizer(pq)
    for name, v in options:
        ix.set_option(name, v)
    return ix


# ---- encoder fixtures -----------------------------------------------------------------------------------------------------------
def dup_pairs(ks, s):
    """(j1, j2), j1 < j2, with pq[s][j2] = pq[s][j1]: always (3, ks - 1); (3, 200) too where ks > 200 -- two waves of K6b -- and
    (10, 300) where ks > 300 -- two threads and strides.  Below five centroids there is no row 3: (0, ks - 1), and only in the even
    sub-quantizers, so that the odd ones still have something to decide."""
    if ks < 5:
        return [(0, ks - 1)] if s % 2 == 0 else []
    pairs = [(3, ks - 1)]
    if ks > 200:
        pairs.append((3, 200))
    if ks > 300:
        pairs.append((10, 300))
    return pairs


def codebook(rng, m, ks, dsub):
    pq = rng.standard_normal((m, ks, dsub))
    for s in range(m):
        for j1, j2 in dup_pairs(ks, s):
            pq[s, j2] = pq[s, j1]
    return pq


@functools.lru_cache(maxsize=None)
def encoder_case(name):
    """dict(kind, D, m, ks, C, transform, coarse, pq, rot, perm, X [521][D], cells, codes (the oracle's, as indices), tie_sub [TIE_ROWS]
    the sub-quantizer in which row i sits on a duplicated codebook row, tie_low / tie_high its two indices)"""
    _, kind, D, m, ks, transform, expect = next(r for r in ENCODER if r[0] == name)
    rng = np.random.default_rng(1000 + [r[0] for r in ENCODER].index(name))
    dsub = D // m
    C = ENC_C if kind == KIND_IVFPQ else 0
    pq = codebook(rng, m, ks, dsub)
    coarse = 20.0 * rng.standard_normal((C, D)) if C else None  # (far apart: a residual of codebook size never changes the cell)
    rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if transform == TR_ROTATION else None
    ref, perm = oracle_index(kind, D, m, ks, C, transform, coarse, pq, rot)
    # the usual mixture: a centroid plus noise of the codebook's scale
    X = rng.standard_normal((ENC_N, D)) + (coarse[rng.integers(0, C, ENC_N)] if C else 0.0)
    subs = [s for s in range(m) if dup_pairs(ks, s)]
    tie_sub = np.array([subs[i % len(subs)] for i in range(TIE_ROWS)])
    tie_low = np.zeros(TIE_ROWS, np.int64)
    tie_high = np.zeros(TIE_ROWS, np.int64)
    for i in range(TIE_ROWS):
        s = int(tie_sub[i])
        pairs = dup_pairs(ks, s)
        j1, _ = pairs[(i // len(subs)) % len(pairs)]
        tie_low[i], tie_high[i] = j1, max(j2 for a, j2 in pairs if a == j1)
        t = rng.standard_normal(D)  # the transformed residual: ordinary everywhere but in sub-quantizer s
        t[s * dsub:(s + 1) * dsub] = pq[s, j1] + 1e-7 * rng.standard_normal(dsub)
        if transform == TR_PERMUTATION:  # t[i] = r[perm[i]]
            r = np.zeros(D)
            r[perm] = t
        elif transform == TR_ROTATION:  # t = r R, R orthogonal
            r = rot @ t
        else:
            r = t
        X[i] = coarse[rng.integers(0, C)] - r if C else r
    cells, codes = ref.encode_batch(X)
    return dict(kind=kind, D=D, m=m, ks=ks, C=C, transform=transform, coarse=coarse, pq=pq, rot=rot, perm=perm, X=X, cells=cells,
                codes=codes, expect=expect, tie_sub=tie_sub, tie_low=tie_low, tie_high=tie_high)


# ---- assignment fixtures --------------------------------------------------------------------------------------------------------
def filter_eps_fp32(D, xnorm, xn2, cnorm_max, cn2_max):
    """mirror of the __device__ function of the same name (csrc/mmidx_device_util.h), operation for operation: K6a's bound"""
    sumn = cnorm_max + xnorm
    return (2.0 * (D + 3) * 2.0 ** -24 * 1.01 * xnorm * cnorm_max + 1e-12 * (cn2_max + xn2) + 2.0 ** -23 * sumn * sumn +
            filter_underflow_eps(D, sumn)) * (1.0 + 1e-9)


@functools.lru_cache(maxsize=None)
def _assign_data(D, C):
    """the inputs of a (D, C) pair, the oracle's cells and everything the tests take from the one [n][C] matrix of fp64 distances"""
    rng = np.random.default_rng(C + D)
    coarse = rng.standard_normal((C, D))
    if C >= 40:
        coarse[C // 2:C // 2 + 25] = coarse[10:35]  # duplicates of earlier rows
        coarse[C - 3] = coarse[C - 4] + 1e-13         # a near tie far below any fp32 / bf16 resolution
        pq = rng.standard_normal((2, 16, D // 2))
        X = np.concatenate([coarse[10:35], coarse[C // 2:C // 2 + 25] + 1e-12, coarse[[C - 3, C - 4]], 0.5 * (coarse[C - 3] + coarse[C - 4])[None],
                            coarse[rng.integers(0, C, 3000)] + 0.3 * rng.standard_normal((3000, D)), 3.0 * rng.standard_normal((500, D))])
        X = np.concatenate([X, near_ties.midpoints(rng, coarse, 300)])
        dup_low, dup_high = np.arange(10, 35), np.arange(C // 2, C // 2 + 25)
    else:  # one cell: nothing to duplicate, nothing to sit between
        pq = rng.standard_normal((2, 16, D // 2))
        X = np.concatenate([coarse[[0]], coarse[rng.integers(0, C, 3000)] + 0.3 * rng.standard_normal((3000, D)), 3.0 * rng.standard_normal((500, D))])
        dup_low = dup_high = np.zeros(0, np.int64)
    ref, _ = oracle_index(KIND_IVFPQ, D, 2, 16, C, TR_NONE, coarse, pq, None)
    cells, _ = ref.encode_batch(X)
    d = sqdist_seq(X, coarse)
    gap = None
    if C >= 2:
        two = np.partition(d, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    return dict(D=D, C=C, coarse=coarse, pq=pq, X=X, cells=cells, dup_low=dup_low, dup_high=dup_high, gap=gap,
                twin_first=_argmin(d, False).astype(np.int32), twin_last=_argmin(d, True).astype(np.int32))


@functools.lru_cache(maxsize=None)
def assign_case(name):
    """dict(D, C, options, misaligned, expect, coarse, pq [2][16][D / 2], X, cells (the oracle's), dup_low / dup_high (the duplicated
    centroid pairs), twin_first / twin_last (the numpy twin's cells under either tie rule), lo, hi (the window of `flagged` for the
    full set; None for the exact rows))"""
    _, D, C, options, misaligned, expect = next(r for r in ASSIGN if r[0] == name)
    c = dict(_assign_data(D, C), options=options, misaligned=misaligned, expect=expect, lo=None, hi=None)
    if expect in CERTIFIED:
        c["lo"], c["hi"] = flagged_window(c["X"], c["coarse"], c["gap"], expect)
    return c


def flagged_window(X, coarse, gap, kernel):
    """(lo, hi), gap = the difference of every row's two smallest fp64 distances (accumulated as the oracle does).  The certified
    kernels flag a row when second~ - best~ <= 2 eps over d~ with |d~ - d| <= eps, or
    when its norms are outside the filter's range.  A row whose two smallest fp64 distances are exactly equal has second~ - best~ <=
    2 eps: it MUST be flagged (lo).  A row with gap > 4 eps has second~ - best~ >= gap - 2 eps > 2 eps: it MUST be certified, so at
    most the rows with gap <= 4.04 eps are flagged (hi; the 1 % covers the last-place differences between the kernel's and numpy's
    evaluation of eps).  eps is evaluated with the quantities the host and the kernels keep: squared norms rounded up by 1e-12."""
    D = X.shape[1]
    cn2 = np.zeros(coarse.shape[0])
    for j in range(D):
        cn2 += coarse[:, j] * coarse[:, j]
    xn2 = np.zeros(X.shape[0])
    for j in range(D):
        xn2 += X[:, j] * X[:, j]
    xn2 *= 1.0 + 1e-12
    xnorm = np.sqrt(xn2)
    cn2_max = (cn2 * (1.0 + 1e-12)).max()
    cnorm_max = (np.sqrt(cn2) * (1.0 + 1e-12)).max()
    if kernel == "K6a":
        eps = filter_eps_fp32(D, xnorm, xn2, cnorm_max, cn2_max)
    else:
        eps = filter_eps_split16((D + 31) // 32 * 32, 2.0 ** -21, xnorm, xn2, cnorm_max, cn2_max)
    usable = filter_norms_usable(cnorm_max + xnorm)
    return int(((gap == 0.0) | ~usable).sum()), int(((gap <= 4.04 * eps) | ~usable).sum())


# ---- placement ------------------------------------------------------------------------------------------------------------------
PLACE_D, PLACE_M, PLACE_C = 32, 4, 300


@functools.lru_cache(maxsize=None)
def placement_case(ks, n):
    """IVFPQ D = 32, m = 4, C = 300: n vectors around 90 of the 300 centroids, so that many lists stay empty; cells and codes from the
    oracle once, shared by every test that adds these vectors in whatever batches"""
    rng = np.random.default_rng(7000 + ks + n)
    coarse = 3.0 * rng.standard_normal((PLACE_C, PLACE_D))
    pq = codebook(rng, PLACE_M, ks, PLACE_D // PLACE_M)
    used = rng.choice(PLACE_C, 90, replace=False)
    X = coarse[used[rng.integers(0, 90, n)]] + rng.standard_normal((n, PLACE_D))
    ref, _ = oracle_index(KIND_IVFPQ, PLACE_D, PLACE_M, ks, PLACE_C, TR_NONE, coarse, pq, None)
    cells, codes = ref.encode_batch(X)
    return dict(kind=KIND_IVFPQ, D=PLACE_D, m=PLACE_M, ks=ks, C=PLACE_C, transform=TR_NONE, coarse=coarse, pq=pq, rot=None, X=X,
                cells=cells, codes=codes)


# ---- the 2^18-row chunk edge of the host entry points ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_edge_case():
    """D = 8, m = 2, ks = 16, C = 4, n = 2^18 + 3: the second chunk of mmidx_encode / mmidx_add_vectors holds three rows.  Expected
    values from the twin (a 262147-row loop over ctypes is too slow); its first 2000 rows are checked against the oracle here."""
    rng = np.random.default_rng(218)
    D, m, ks, C, n = 8, 2, 16, 4, (1 << 18) + 3
    coarse = 2.0 * rng.standard_normal((C, D))
    pq = codebook(rng, m, ks, D // m)
    X = coarse[rng.integers(0, C, n)] + rng.standard_normal((n, D))
    cells, codes = twin_encode(X, coarse, pq)
    ref, _ = oracle_index(KIND_IVFPQ, D, m, ks, C, TR_NONE, coarse, pq, None)
    rc, rk = ref.encode_batch(np.concatenate([X[:2000], X[-3:]]))
    assert np.array_equal(rc, np.concatenate([cells[:2000], cells[-3:]])) and np.array_equal(rk, np.concatenate([codes[:2000], codes[-3:]]))
    return dict(kind=KIND_IVFPQ, D=D, m=m, ks=ks, C=C, transform=TR_NONE, coarse=coarse, pq=pq, rot=None, X=X, cells=cells, codes=codes)
