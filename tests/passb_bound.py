"""A numpy model of the certificate behind K3g (`k_scan_grp`, csrc/mmidx_scan_grp.h) and K3s (`k_pair_smin`, `k_pair_smin_mfma`,
`k_pair_smin_bf16`), replayed operation for operation from the kernel source, for tests/test_passb_bound_cpu.py.

What is replayed, per (query, cell) pair and sub-quantizer s:
  host tables   pq32T = fl32(p), pn = fp64 sum of p^2 (t ascending), pn32 = fl32(pn) (+inf beyond ks), pnmax = sqrt(max pn) (1 + 1e-12)
                and max pn (1 + 1e-12)                                                      (k_pq32_table, k_pn_max)
  residuals     r = centroid - q in fp64, r32 = fl32(r), nr = fp64 sum of r^2 in each kernel's own order -- t ascending in K3g's
                phase (c), a butterfly over the dimensions in k_pair_smin, two halves summed in turn and added in the matrix-core
                forms --, nrf = fl32(nr)                                                            (phases (b), (c) / (i))
  VALU entry    dot = fma(r32_t, p32_t, dot), t ascending from 0;  entry = fma(-2, dot, fl(nrf + pn32))  (grp_rows, grp_entries, k_pair_smin)
  matrix cores  acc = -pn32 / 2;  acc = fma(r32_t, p32_t, acc), t ascending;  row minimum = fma(-2, max_j acc_j, nrf)  (k_pair_smin_mfma)
  bf16 stage    r32 = head + tail in bf16, p's bf16 head; the 32 products [head | tail] x [p_hi | p_hi] of the one
                v_mfma_f32_16x16x32_bf16 are accumulated as a chain of fused fp32 steps, k ascending, from -pn32 / 2 (the order inside
                the instruction is not documented; a rounding per step is the reading the kernel's own error analysis -- "33 fp32
                accumulation steps" -- assumes)                                                            (k_pair_smin_bf16)
  quantisation  q8 = RNE-and-saturate(fma(entry, inv, fma(-mn, inv, -0.5))) (clamped to QMAX first when QMAX < 255), and the generic
                form (u32) fminf((entry - mn) * inv, QMAX) of the run-time-dsub instance                    (grp_q / phase (d))
  phase (e)     s_err, es, Smin_lo, the state (0 scan, 1 nothing to do, 2 hand back to K3f), th
  K3s           term = fl64(mn) - err, lowered by 2^-40, -inf unless err < 1e22; their sum in the kernel's order

A fused fp32 step fma(a, b, c) is modelled as the exact product in fp64 (two fp32 factors: 48 bits), the sum in np.longdouble (64-bit
significand), rounded ONCE to fp32.  Every fp32 result is produced in two readings of what happens below 2^-126: gradual underflow
(IEEE subnormals, numpy's own conversion) and flush to zero (applied by hand to every result; a flushed result is also what a
flushed operand looks like to the next step).  A build or a chip may apply either at any step; a sound bound holds under both.
The flush reading is evaluated only where the gradual one produced a result below 2^-126 at all (otherwise the two are the same
numbers).  Exact values -- entries, distances, sums of minima -- are np.longdouble sums of squared differences of the fp64 inputs.

Where this is NOT the kernels' arithmetic: every r * r and every addition of an fp64 sum is rounded on its own, where the compiler
may contract `nr += r * r` (and the host's `pn += p * p`) into fused fp64 steps -- a difference of 2^-53 relative, which the
bounds' factor 1.01 is there for; the bf16 instruction's inner order (above).  Not modelled at all: the UNION instances'
`256 / T0 < 1e300` bucket map of the per-query histogram and what follows from `th`'s 32000 clamp beyond "a clamped th passes
more" -- whether those stay monotone at the edges is settled by the device runs only (`no_union` = -1 in
tests/test_gpu_passb_magnitudes.py), not here.

Inputs: residual-like Gaussian data at unit scale from a seed, multiplied by the scale under test; see `unit_problem`, `MIXES`."""
import functools
import multiprocessing
import os

import numpy as np

import near_ties

LD, F64, F32 = np.longdouble, np.float64, np.float32
TINY = F32(2.0 ** -126)
INF = np.inf

SHAPES = [(16, 8), (8, 16), (32, 4), (8, 12)]  # (m, dsub)
KS = (256, 200)  # 200: the +inf padding entries beyond ks are present
NPAIR, NCODE, NCELL = 64, 512, 8
LOW = [10.0 ** (-e / 2.0) for e in range(20, 41)]   # 1e-10 .. 1e-20 in half decades
HIGH = [10.0 ** (e / 2.0) for e in range(24, 41)]   # 1e12 .. 1e20
EXTREME = [1e-25, 1e-45, 1e25, 1e140]
SCALES = list(near_ties.ORDINARY) + LOW + HIGH + EXTREME
MIXES = ("plain", "far_query", "tiny_codebook", "zero_residual")
T_FACTORS = (1.0, 1.0 + 1e-6, 4.0)  # of the exact 20th-smallest distance among the pair's codes
# (QMAX, fused): the plain and flat-PQ instances, the IVF UNION instances, the run-time-dsub instance
QFORMS = ((127, True), (255, True), (127, False))
G_VARIANTS = ("kernel", "no_es_guard", "no_abs_term", "no_iv_guard")
S_VARIANTS = ("kernel", "no_err_guard", "no_abs_term")


class Reading:
    """fp32 results under one reading of underflow; `touched`: some result fell below 2^-126 (the readings differ from here on)"""

    def __init__(self, ftz):
        self.ftz, self.touched = ftz, False

    def rnd(self, x):
        y = np.asarray(x).astype(F32)
        small = np.abs(y) < TINY
        if small.any():
            small &= np.asarray(x) != 0
            if small.any():
                self.touched = True
                if self.ftz:
                    y = np.where(small, F32(0.0), y)
        return y

    def rnd_sum(self, p, c):
        """fl32(p + c), p an fp64 array holding an exact product (or an fp32 value), c fp32: the sum in np.longdouble, one rounding.
        (Infinities and NaNs take the same sum in fp64 -- the result is the same inf / NaN, and extended-precision arithmetic on
        them is an order of magnitude slower.)"""
        p, c = np.broadcast_arrays(np.asarray(p, F64), np.asarray(c, F32).astype(F64))
        fin = np.isfinite(p) & np.isfinite(c)
        if fin.all():
            return self.rnd(p.astype(LD) + c.astype(LD))
        y = self.rnd(np.where(fin, p, 0.0).astype(LD) + np.where(fin, c, 0.0).astype(LD))
        return np.where(fin, y, (p + c).astype(F32))

    def fma(self, a, b, c):
        return self.rnd_sum(np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64), c)  # (the product is exact)

    def add(self, a, b):
        return self.rnd_sum(np.asarray(a, F32).astype(F64), b)

    def mul(self, a, b):
        return self.rnd(np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64))


def _bf16(f):
    """fp32 -> bf16 (round to nearest even), returned as fp32"""
    b = np.ascontiguousarray(f, F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F32)


@functools.lru_cache(maxsize=None)
def unit_problem(m, dsub):
    """centroids [NCELL][D], queries [NPAIR][D] (a cell's centroid plus N(0, 1): near and far probes alike), the probed cell of every
    pair, a codebook [m][256][dsub] of residual-like entries, and uniform draws [NPAIR][NCODE][m] the random codes are made from"""
    rng = np.random.default_rng(1000 * m + dsub)
    D = m * dsub
    cent = 0.5 * rng.standard_normal((NCELL, D))
    Q = cent[rng.integers(0, NCELL, NPAIR)] + rng.standard_normal((NPAIR, D))
    cell = rng.integers(0, NCELL, NPAIR)
    pq = rng.standard_normal((m, 256, dsub))
    u = rng.random((NPAIR, NCODE, m))
    return cent, Q, cell, pq, u


def scaled_inputs(m, dsub, scale, mix):
    """fp64 residuals [NPAIR][m][dsub] (centroid - q, as the kernels form them) and the fp64 codebook at `scale` under `mix`"""
    cent, Q, cell, pq, _ = unit_problem(m, dsub)
    c = (cent * scale)[cell]
    q = Q * scale
    p = pq * scale
    if mix == "far_query":        # the query a million times the data's scale; codebook and centroids as they are
        q = q * 1e6
    elif mix == "tiny_codebook":  # the codebook eight orders below the residuals
        p = p * 1e-8
    elif mix == "zero_residual":  # the query IS the centroid (flat PQ: the zero query)
        q = c.copy()
    return (c - q).reshape(NPAIR, m, dsub), p


def _seq_sum(x):
    acc = np.zeros(x.shape[:-1], F64)
    for t in range(x.shape[-1]):
        acc = acc + x[..., t]
    return acc


def _tree_sum(v):
    """the butterfly of phase (e) over M = 2^k lanes (x[i] + x[i ^ off], off = M/2 .. 1: the same value in every lane)"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def host_tables(p, rd):
    """k_pq32_table / k_pn_max at ks = 256; `pad(ks)` below turns the tail into the padding of a smaller codebook"""
    pn = _seq_sum(p * p)  # [m][256]
    return rd.rnd(p), rd.rnd(pn), pn


def pnmax(pn, ks):
    a = pn[:, :ks].max(1)
    return np.sqrt(a) * (1.0 + 1e-12), a * (1.0 + 1e-12)


def exact_entries(r, p):
    E = np.zeros((r.shape[0], r.shape[1], p.shape[1]), LD)
    rl, pl = r.astype(LD), p.astype(LD)
    for t in range(r.shape[2]):
        d = rl[:, :, None, t] - pl[None, :, :, t]
        E += d * d
    return E


def fp32_entries(r, p32, pn32, rd, bf16=False):
    """(entries of the VALU form [P][m][256], accumulators of the matrix-core form, accumulators of the bf16 stage or None,
    nr fp64 [P][m], nrf)"""
    r32 = rd.rnd(r)
    nr = _seq_sum(r * r)
    nrf = rd.rnd(nr)
    P_, m, dsub = r.shape
    # ||r_s||^2 in K3s's own orders: k_pair_smin's butterfly over the dimensions' lanes (x[i] + x[i ^ off], off = 1, 2, ..: dsub a
    # power of two), the matrix-core forms' two halves (each summed in turn, then added)
    sq = r * r
    nr_bfly = sq
    while dsub & (dsub - 1) == 0 and nr_bfly.shape[-1] > 1:
        nr_bfly = nr_bfly[..., 0::2] + nr_bfly[..., 1::2]
    nr_bfly = nr_bfly[..., 0] if nr_bfly.shape[-1] == 1 else nr
    nr_half = _seq_sum(sq[..., :dsub // 2]) + _seq_sum(sq[..., dsub // 2:])
    dot = np.zeros((P_, m, 256), F32)
    ph = rd.mul(F32(-0.5), pn32)[None]
    acc = np.broadcast_to(ph, dot.shape)
    for t in range(dsub):
        prod = r32[:, :, None, t].astype(F64) * p32[None, :, :, t].astype(F64)  # exact; shared by the two chains
        dot = rd.rnd_sum(prod, dot)
        acc = rd.rnd_sum(prod, acc)
    a = rd.fma(F32(-2.0), dot, rd.add(nrf[:, :, None], pn32[None]))
    nrf_bfly = rd.rnd(nr_bfly)
    a_s = a if np.array_equal(nrf_bfly, nrf) else rd.fma(F32(-2.0), dot, rd.add(nrf_bfly[:, :, None], pn32[None]))  # k_pair_smin's entries
    accb = None
    if bf16:
        rh = rd.rnd(_bf16(r32))
        rlo = rd.rnd(_bf16(rd.rnd(r32.astype(F64) - rh.astype(F64))))  # (f - head is exact in fp32)
        phi = rd.rnd(_bf16(p32))
        accb = np.broadcast_to(ph, dot.shape)
        for part in (rh, rlo):
            for t in range(dsub):
                accb = rd.fma(part[:, :, None, t], phi[None, :, :, t], accb)
    return a, acc, accb, nr, nrf, dict(a_s=a_s, nr_bfly=nr_bfly, nr_half=nr_half, nrf_half=rd.rnd(nr_half))


def pad(x, ks, value):
    if ks == 256:
        return x
    x = x.copy()
    x[..., ks:] = value
    return x


def err_k3g(nr, pm, pm2, dsub, abs_term=True):
    """s_err of phase (c) (and of k_pair_smin's phase (i))"""
    return 2.0 ** -24 * 1.01 * (3.0 * (nr + pm2) + (2.0 * dsub + 9.0) * np.sqrt(nr) * pm) + (1e-30 if abs_term else 0.0)


def err_mfma(nr, pm, pm2, dsub, abs_term=True):
    return 2.0 ** -24 * 1.01 * (3.0 * nr + (dsub + 3.0) * pm2 + (2.0 * dsub + 9.0) * np.sqrt(nr) * pm) + (1e-30 if abs_term else 0.0)


def err_bf16(nr, pm, pm2, abs_term=True):
    cross = np.sqrt(nr) * pm
    return 2.0 ** -24 * 1.01 * (3.0 * nr + 36.0 * pm2 + 72.0 * cross) + 2.0 ** -8 * 1.02 * cross + (1e-30 if abs_term else 0.0)


def k3s_smin(mn32, err, guard=True):
    """the sum k_pair_smin* leaves in smin[]: eight terms per slice group in turn, the groups' parts added (atomicAdd from zero)"""
    term = mn32.astype(F64) - err
    term = term - np.abs(term) * 2.0 ** -40
    if guard:
        term = np.where(err < 1e22, term, -INF)
    total = np.zeros(term.shape[0], F64)
    for g0 in range(0, term.shape[1], 8):
        s = np.zeros(term.shape[0], F64)
        for i in range(g0, g0 + 8):
            s = s + term[:, i]
        total = s if term.shape[1] == 8 else total + s
    return total


def k3g_inv(Td, qmax, rd, guard=True):
    """phase (a): the quantisation step's inverse, 0 = none"""
    iv = (qmax - 1.0) / Td
    return np.where((iv < 1e30) | (not guard), rd.rnd(iv), F32(0.0)).astype(F32)


def k3g_phase_e(mn32, err, Td, invf, es_guard=True):
    """(state [P], th [P], Smin_lo [P]) as phase (e) decides them (every T here is finite)"""
    smin = _tree_sum(mn32.astype(F64) - err)
    es = _tree_sum(err)
    smin_lo = smin - np.abs(smin) * 2.0 ** -40
    bad = ~(np.abs(smin_lo) < 1e30) | ~(invf > 0)
    if es_guard:
        bad |= ~(es < 1e24)
    t = (Td - smin_lo) * invf.astype(F64) * (1.0 + 2.0 ** -20) + 0.02
    small = t < 32000.0
    th = np.where(small, np.floor(np.where(small, t, 0.0)), 32000.0)
    state = np.where(bad, 2, np.where(~(smin_lo < Td), 1, 0))
    return state, th, smin_lo


def quantise(a, mn, invf, qmax, fused, rd):
    """byte sums of K codes: entries a [K][m], the row minima mn [K][m] and inv [K] of each code's pair"""
    if fused:
        c = rd.fma(-mn, invf[:, None], F32(-0.5))
        x = rd.fma(a, invf[:, None], c)
        if qmax < 255:
            x = np.fmin(x, F32(qmax))
        x = np.where(np.isnan(x), F32(0.0), x)  # (v_cvt_pk_u8_f32: NaN -> 0)
        return np.clip(np.rint(x), 0.0, 255.0).sum(-1)
    x = np.fmin(rd.mul(rd.add(a, -mn), invf[:, None]), F32(qmax))  # (fminf: NaN -> QMAX)
    return np.floor(np.maximum(x, F32(0.0))).sum(-1)


def _gather(E, codes):
    P_, N, m = codes.shape
    return E[np.arange(P_)[:, None, None], np.arange(m)[None, None, :], codes]


def _nanmax(x):
    """maximum over the last axis, NaN if any element is"""
    return np.where(np.isnan(x).any(-1), LD(np.nan), np.max(np.where(np.isnan(x), LD(0.0), x), axis=-1))


def stage1(m, dsub, scale, mix, ftz):
    """what depends on neither ks nor T: host tables, exact entries, the fp32 entries of every form"""
    rd = Reading(ftz)
    r, p = scaled_inputs(m, dsub, scale, mix)
    with np.errstate(all="ignore"):
        p32, pn32, pn = host_tables(p, rd)
        a, acc, accb, nr, nrf, K = fp32_entries(r, p32, pn32, rd, bf16=(dsub == 16))
        E = exact_entries(r, p)
        # K3s's matrix-core forms: entry_j = fl(nrf - 2 acc_j)
        ent = {"k3g": a, "valu": K["a_s"], "mfma": rd.fma(F32(-2.0), acc, K["nrf_half"][:, :, None])}
        if accb is not None:
            ent["bf16"] = rd.fma(F32(-2.0), accb, K["nrf_half"][:, :, None])
        # worst |entry32 - exact| of every row, over the entries below each ks (a NaN stays a NaN: it fails every comparison)
        worst = {}
        for name, x in ent.items():
            dif = np.abs(x.astype(LD) - E)
            lo = _nanmax(dif[:, :, :KS[1]])
            worst[name] = {KS[1]: lo, KS[0]: _nanmax(np.stack([lo, _nanmax(dif[:, :, KS[1]:])], axis=-1))}
    return dict(m=m, dsub=dsub, pn=pn, E=E, a=a, acc=acc, accb=accb, nr=nr, nrf=nrf, worst=worst, K=K), rd.touched


def stage2(S, ftz):
    """For both ks: violations of B1 .. B4 per variant, the regime counts of the kernel's own rule.  Returns (results, touched)."""
    rd = Reading(ftz)
    m, dsub, pn, nr, nrf = S["m"], S["dsub"], S["pn"], S["nr"], S["nrf"]
    u = unit_problem(m, dsub)[4]
    out = {}
    with np.errstate(all="ignore"):
        for ks in KS:
            pm, pm2 = pnmax(pn, ks)
            E = pad(S["E"], ks, LD(INF))
            a = pad(S["a"], ks, F32(INF))
            # the pair's codes: NCODE random ones, the nearest entry of every sub-quantizer, the second nearest
            two = np.argsort(E.astype(F64), axis=-1, kind="stable")[:, :, :2]
            codes = np.concatenate([np.floor(u * ks).astype(np.int64), two[:, None, :, 0], two[:, None, :, 1]], axis=1)
            d = _gather(E, codes).sum(-1)  # exact distances [P][N]
            smin_exact = E.min(-1).sum(-1)
            T20 = np.sort(d, axis=1)[:, 19].astype(F64)
            mn = np.fmin.reduce(a, axis=-1)  # (fminf / v_min_f32: a NaN loses)
            a_codes = _gather(a, codes)
            errs = {ab: err_k3g(nr, pm[None], pm2[None], dsub, ab) for ab in (True, False)}
            g = {v: dict(B1=0, B2=0, B4=0) for v in G_VARIANTS}
            regime, handed = None, 0
            state0_any = {v: np.zeros(NPAIR, bool) for v in G_VARIANTS}
            for tf in T_FACTORS:
                Td = T20 * tf
                inside = d <= Td.astype(LD)[:, None]
                for qmax, fused in QFORMS:
                    invs = {True: k3g_inv(Td, qmax, rd, True), False: k3g_inv(Td, qmax, rd, False)}
                    dec = {}
                    for v in G_VARIANTS:
                        invf = invs[v != "no_iv_guard"]
                        state, th, _ = k3g_phase_e(mn, errs[v != "no_abs_term"], Td, invf, es_guard=(v != "no_es_guard"))
                        dec[v] = (state, th)
                        state0_any[v] |= state == 0
                        g[v]["B4"] += int(((state == 1) & ~(smin_exact >= Td.astype(LD))).sum())
                    state, th = dec["kernel"]
                    handed += int((state == 2).sum())
                    if tf == 1.0 and (qmax, fused) == QFORMS[0]:
                        blind = (state == 0) & (th >= m * qmax)
                        regime = (int(((state == 0) & ~blind).sum()), int(blind.sum()), int((state == 2).sum()), int((state == 1).sum()))
                    # B2: the byte sums of the codes with d <= T, for the pairs some variant scans
                    for guard in (True, False):
                        vs = [v for v in G_VARIANTS if (v != "no_iv_guard") == guard]
                        need = inside & np.any([dec[v][0] == 0 for v in vs], axis=0)[:, None]
                        pi, ci = np.nonzero(need)
                        if len(pi) == 0:
                            continue
                        qs = quantise(a_codes[pi, ci], mn[pi], invs[guard][pi], qmax, fused, rd)
                        for v in vs:
                            state, th = dec[v]
                            g[v]["B2"] += int(((state[pi] == 0) & ~(qs <= th[pi])).sum())
            worst = {name: w[ks] for name, w in S["worst"].items()}
            for v in G_VARIANTS:  # (B1 is counted in rows: a (pair, sub-quantizer) with an entry outside the bound)
                g[v]["B1"] = int((~(worst["k3g"] <= errs[v != "no_abs_term"].astype(LD)) & state0_any[v][:, None]).sum())
            s = {v: dict(B1=0, B3=0) for v in S_VARIANTS}
            k3s = None
            if dsub in (4, 8, 16):  # (K3s sits out at any other width)
                K = S["K"]
                nrb, nrh, nrfh = K["nr_bfly"], K["nr_half"], K["nrf_half"]
                mn_s = mn if K["a_s"] is S["a"] else np.fmin.reduce(pad(K["a_s"], ks, F32(INF)), axis=-1)
                forms = [("valu", None, mn_s, lambda ab: err_k3g(nrb, pm[None], pm2[None], dsub, ab)),
                         ("mfma", S["acc"], None, lambda ab: err_mfma(nrh, pm[None], pm2[None], dsub, ab))]
                if dsub == 16:
                    forms.append(("bf16", S["accb"], None, lambda ab: err_bf16(nrh, pm[None], pm2[None], ab)))
                for name, x, mins, errf in forms:
                    if mins is None:  # the matrix-core forms: minimum = fl(nrf - 2 max_j acc_j)
                        mins = rd.fma(F32(-2.0), np.fmax.reduce(pad(x, ks, F32(-INF)), axis=-1), nrfh)
                    for v in S_VARIANTS:
                        err = errf(v != "no_abs_term")
                        ok_pair = np.all(err < 1e22, axis=1) if v != "no_err_guard" else np.ones(NPAIR, bool)
                        s[v]["B1"] += int((~(worst[name] <= err.astype(LD)) & ok_pair[:, None]).sum())
                        if v == "kernel" and name == "mfma":  # pairs it bounds / pairs with a term of -inf (never dropped)
                            k3s = (int(ok_pair.sum()), int((~ok_pair).sum()))
                        sm = k3s_smin(mins, err, guard=(v != "no_err_guard"))
                        s[v]["B3"] += int((~(sm.astype(LD) <= smin_exact)).sum())
            out[ks] = dict(g=g, s=s, regime=regime, handed=handed, k3s=k3s)
    return out, rd.touched


def _both_readings(job):
    m, dsub, scale, mix = job
    S, t1 = stage1(m, dsub, scale, mix, False)
    grad, t2 = stage2(S, False)
    flush = grad
    if t1 or t2:  # (stage 1 again only if one of ITS results fell below 2^-126)
        flush = stage2(stage1(m, dsub, scale, mix, True)[0] if t1 else S, True)[0]
    return grad, flush


@functools.lru_cache(maxsize=None)
def sweep(m, dsub):
    """{(scale, mix, ks, ftz): result} over SCALES x MIXES x KS x the two readings (the configurations are independent: a few
    worker processes share them)"""
    jobs = [(m, dsub, scale, mix) for scale in SCALES for mix in MIXES]
    workers = max(1, min(8, (os.cpu_count() or 1) // 2))
    if workers > 1:
        # (fresh interpreters, not forks: the suite's process may hold a GPU runtime and its threads by now)
        with multiprocessing.get_context("spawn").Pool(workers) as pool:
            done = pool.map(_both_readings, jobs, chunksize=4)
    else:
        done = [_both_readings(j) for j in jobs]
    res = {}
    for (_, _, scale, mix), (grad, flush) in zip(jobs, done):
        for ks in KS:
            res[(scale, mix, ks, False)] = grad[ks]
            res[(scale, mix, ks, True)] = flush[ks]
    return res


def regime_name(counts):
    sharp, blind, back, idle = counts
    return " + ".join(n for n, c in (("state 0", sharp), ("blind", blind), ("handed back", back), ("state 1", idle)) if c)


def intervals(m, dsub, ks=256, mix="plain", ftz=False, k3s=False):
    """[(first scale, last scale, regime)] over the sorted scales: K3g at T = the 20th-smallest distance, QMAX 127; or K3s (matrix-core
    form): "bounds" where every term passes `err < 1e22`, "-inf" where one does not"""
    sw = sweep(m, dsub)
    runs = []
    for scale in sorted(SCALES):
        r = sw[(scale, mix, ks, ftz)]
        name = " + ".join(n for n, c in zip(("bounds", "-inf"), r["k3s"]) if c) if k3s else regime_name(r["regime"])
        if runs and runs[-1][2] == name:
            runs[-1][1] = scale
        else:
            runs.append([scale, scale, name])
    return [tuple(r) for r in runs]
