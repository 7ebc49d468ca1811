"""The head-only screen of the one-probe certificate (K1s: k_coarse_screen16 + k_coarse_near_cert, DESIGN.md section 5.1 "The
screen") restated in numpy.

d~ = fl32(fl32(|c|^2 - 2 S) + |q|^2) with S = the fp32 sum of the products of the bf16 HEADS of the fp32 copies of q and c (each
product is exact in fp32), three low mantissa bits of the first result borrowed for a position.  The certificate asks only that
|d~ - d| <= eps1 = filter_eps_head16 (csrc/mmidx_device_util.h), restated here term for term.  From a = the smallest d~ (at c0) and
b = the smallest d~ of every other centroid -- two equal minima give b = a -- L = b - eps1 bounds every centroid but c0 from below,
and the tests of coarse_near_model.certificate follow with that L."""
import numpy as np

import coarse_near_model as cm
import np_twin as nt
from passb_bound import _bf16

F32 = np.float32
U126 = 2.0 ** -126


def underflow_eps_head(Dk, sumn):
    """two roundings per element (the fp32 copy, its head): 6 U sqrt(Dk) sumn in d~; Dk products and Dk additions, doubled: 4 Dk U;
    the epilogue's 16 U"""
    return (4.0 * Dk + 16.0 + 6.0 * np.sqrt(float(Dk)) * sumn) * U126


def eps_head16(Dp, xnorm, xn2, cnorm_max, cn2_max, epi=cm.EPI_K1E, cross=True):
    """filter_eps_head16, term for term; cross = False drops the dropped-cross-terms term (a mutation the tests must catch)"""
    sumn = cnorm_max + xnorm
    t_cross = 2.0 * 2.01 * 2.0 ** -8 * xnorm * cnorm_max if cross else 0.0
    t_acc = 2.0 * 1.01 * (Dp + 16.0) * 2.0 ** -22 * xnorm * cnorm_max
    return (t_cross + t_acc + 1e-12 * (cn2_max + xn2) + epi * sumn * sumn + underflow_eps_head(Dp, sumn)) * (1.0 + 1e-9)


def head_dists(coarse, q):
    """the screen's d~ row, fp32: heads of the fp32 copies, products and their running sum in fp32, the kernel's epilogue"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ch, qh = _bf16(coarse.astype(F32)), _bf16(q.astype(F32))
        S = np.zeros(len(coarse), F32)
        for j in range(coarse.shape[1]):
            S = (S + ch[:, j] * qh[j]).astype(F32)
        cn = (coarse * coarse).sum(1).astype(F32)
        qn = F32((q * q).sum() * (1.0 + 1e-12))
        t = (cn.astype(np.float64) - 2.0 * S.astype(np.float64)).astype(F32)  # one rounding: the fma
        t = ((t.view(np.uint32) & ~np.uint32(7)) | (np.arange(len(coarse), dtype=np.uint32) >> 4 & np.uint32(7))).view(F32)
        d = (t + qn).astype(F32)
    return np.where(d < 0, F32(0), d)


def norms_of(coarse, q):
    qn = float((q * q).sum()) * (1.0 + 1e-12)
    cn_max = float((coarse * coarse).sum(1).max()) * (1.0 + 1e-12)
    return np.sqrt(qn), qn, np.sqrt(cn_max), cn_max


def a_b_c0(dt, splits=1, other_a=True):
    """(a, b, c0) as the certificate kernel merges the records of `splits` equal ranges of centroids: per range (best, rest, where);
    b = the smallest of every other range's best and of all the rests; strict <.  other_a = False leaves the other ranges' bests
    out of b (a mutation the tests must catch)"""
    a, b, c0 = np.inf, np.inf, 0
    for part in np.array_split(np.arange(len(dt)), splits):
        v = dt[part]
        i = int(v.argmin())
        ra, rb = float(v[i]), float(np.delete(v, i).min()) if len(v) > 1 else np.inf
        lt = ra < a
        hi = (a if lt else ra) if other_a else np.inf
        b = min(hi, min(b, rb))
        if lt:
            a, c0 = ra, int(part[i])
    return a, b, c0


def certificate(coarse, q, list_len, near_min, rmax, dt=None, splits=1, cross=True, other_a=True):
    """coarse_near_model.certificate with L = b - eps1 from the head-only row; -> the same dict (eps1 under "eps16" too)"""
    C, D = coarse.shape
    Dp = (D + 127) // 128 * 128
    dt = head_dists(coarse, q) if dt is None else dt
    qnorm, qn, cnorm_max, cn_max = norms_of(coarse, q)
    eps1 = eps_head16(Dp, qnorm, qn, cnorm_max, cn_max, cross=cross)
    a, b, c0 = a_b_c0(dt, splits, other_a)
    L = b - eps1
    gap, lb = cm.pair_keep_bound(np.float64(L), rmax)
    out = dict(ok=False, c0=c0, a=a, b=b, L=L, d0=np.nan, U=np.nan, lb=float(lb), eps1=eps1, eps16=eps1)
    if not (c0 < C and b < np.inf and cm.norms_usable(cnorm_max + qnorm) and gap > 0.0 and list_len[c0] >= near_min):
        return out
    d0 = float(nt.sq_dists_rows(coarse[c0:c0 + 1], q)[0])
    su = np.sqrt(d0) + rmax
    U = su * su * (1.0 + 1e-9)
    out.update(d0=d0, U=float(U), ok=bool(lb > U))
    return out


class ScreenAuto:
    """the auto rule of option "coarse_screen" (ScreenAuto::step, csrc/mmidx_host.h)"""

    def __init__(self):
        self.skip, self.fresh, self.nq = 0, False, 0

    def step(self, handed, nq_now):
        if self.skip > 0:
            self.skip -= 1
            return False
        if self.fresh:
            self.fresh = False
            if handed * 4 > self.nq:
                self.skip = 6
                return False
        self.fresh, self.nq = True, nq_now
        return True


def run_auto(handed_of_call, nq=100):
    """on / off decisions of a sequence of calls; handed_of_call[i] = the queries call i would hand on if it ran the screen.  The
    pinned word keeps the figure of the last screened call"""
    s, word, out = ScreenAuto(), 0, []
    for h in handed_of_call:
        on = s.step(word, nq)
        if on:
            word = h
        out.append(on)
    return out
