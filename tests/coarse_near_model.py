"""The coarse stage's one-probe certificate (k_coarse_front_sel) restated in numpy.

Per query the kernel holds, for every group of 8 centroids, the smallest approximate distance d~ (fp32), the runner-up with its
three low mantissa bits replaced by the position of the smallest (so: rounded towards zero), and the error bound eps16 of d~.
From these alone:

    a  = the smallest d~, at centroid c0 of group g0
    b  = the smallest d~ of every other centroid = min(min over g != g0 of m1[g], m2[g0])
    L  = b - eps16            every centroid but c0 lies at L or farther
    d0 = |c0 - q|^2           exact, dimensions ascending

The query is answered with c0 alone when
    (1) list c0 holds at least `near_min` codes (the kernel's host passes K1 * chunks + 1 >= K1 + 1),
    (2) r = sqrt(L) (1 - 1e-12) > Rmax,
    (3) (r - Rmax)^2 (1 - 1e-9) > (sqrt(d0) + Rmax)^2 (1 + 1e-9).
The left side of (3) is pair_keep()'s lower bound of a cell at distance L.  `weaken` drops one of the three, for the tests that
show what each is there for.

d~ here is an fp32 stand-in (fp32 copies, fp32 dot product, the kernel's epilogue): the certificate only asks that
|d~ - d| <= eps16, which the tests assert of it."""
import numpy as np

import np_twin as nt

EPI_K1E = 2.0 ** -21 + 2.0 ** -20
GROUP_TILE = 128  # centroids per tile: group g = 16 t + fr holds the centroids 128 t + fr + 16 ct, ct = 0 .. 7


def underflow_eps(Dk, sumn):
    return (12.0 * Dk + 16.0 + 8.0 * np.sqrt(float(Dk)) * sumn) * 2.0 ** -126


def eps_split16(Dp, xnorm, xn2, cnorm_max, cn2_max, epi=EPI_K1E):
    """filter_eps_split16 (csrc/mmidx_device_util.h), term for term"""
    sumn = cnorm_max + xnorm
    return (2.0 * 3.1 * 2.0 ** -16 * xnorm * cnorm_max + 2.0 * (3.0 * Dp + 16.0) * 2.0 ** -22 * xnorm * cnorm_max +
            1e-12 * (cn2_max + xn2) + epi * sumn * sumn + underflow_eps(Dp, sumn)) * (1.0 + 1e-9)


def norms_usable(sumn):
    return sumn * sumn < 1e37 and sumn * sumn > 1e-37


def rmax_of(pq):
    """sqrt(sum_s max_j |pq[s][j]|^2) (1 + 1e-12), as the handle keeps it"""
    return float(np.sqrt((pq * pq).sum(2).max(1).sum()) * (1.0 + 1e-12))


def approx_dists(coarse, q):
    """an fp32 d~ row: fl32((|c|^2 + |q|^2) - 2 S), S the fp32 dot product of the fp32 copies"""
    S = (coarse.astype(np.float32) @ q.astype(np.float32)).astype(np.float64)
    return (((coarse * coarse).sum(1) + (q * q).sum()) - 2.0 * S).astype(np.float32)


def group_pairs(dt):
    """the K1e record of every group: (m1, m2 with the position of m1 in its three low bits) -- fp32, [G]"""
    C = len(dt)
    Cp = (C + GROUP_TILE - 1) // GROUP_TILE * GROUP_TILE
    row = np.full(Cp, np.inf, np.float32)
    row[:C] = dt
    G = Cp // 8
    g = np.arange(G)
    cent = ((g >> 4) * GROUP_TILE + (g & 15))[:, None] + 16 * np.arange(8)[None, :]  # [G][8]
    v = row[cent]
    pos = v.argmin(1)
    m1 = v[g, pos]
    v2 = v.copy()
    v2[g, pos] = np.inf
    m2 = v2.min(1)
    ry = ((m2.view(np.uint32) & ~np.uint32(7)) | pos.astype(np.uint32)).view(np.float32)
    return m1, ry, cent


def pair_keep_bound(cd, rmax):
    """(gap, lower bound) as pair_keep() computes them from a cell's squared distance (no rotation: shrink = 1)"""
    with np.errstate(invalid="ignore"):
        gap = np.sqrt(cd) * (1.0 - 1e-12) - rmax
    return gap, gap * gap * (1.0 - 1e-9)


def certificate(coarse, q, list_len, near_min, rmax, dt=None, weaken=0):
    """-> dict(ok, c0, a, b, L, d0, U, lb, eps16); list_len[c] = codes in list c"""
    C, D = coarse.shape
    Dp = (D + 127) // 128 * 128
    dt = approx_dists(coarse, q) if dt is None else dt
    qn = float((q * q).sum()) * (1.0 + 1e-12)
    qnorm = np.sqrt(qn)
    cn = (coarse * coarse).sum(1)
    cn_max = float(cn.max()) * (1.0 + 1e-12)
    cnorm_max = np.sqrt(cn_max)
    eps16 = eps_split16(Dp, qnorm, qn, cnorm_max, cn_max)
    m1, ry, cent = group_pairs(dt)
    m1 = np.fmax(m1, np.float32(0.0))  # exact distances are >= 0
    g0 = int(m1.argmin())
    a = float(m1[g0])
    rb = ry.view(np.uint32)
    m2 = (rb & ~np.uint32(7)).view(np.float32)[g0]
    m2c = float(m2) if m2 > 0.0 else 0.0  # (a negative or NaN runner-up: b = 0)
    rest = np.delete(m1, g0)
    b = min(float(rest.min()) if len(rest) else np.inf, m2c)
    c0 = int(cent[g0, int(rb[g0] & 7)])
    L = b - eps16
    gap, lb = pair_keep_bound(np.float64(L), rmax)
    out = dict(ok=False, c0=c0, a=a, b=b, L=L, d0=np.nan, U=np.nan, lb=float(lb), eps16=eps16)
    if not (c0 < C and b < np.inf and norms_usable(cnorm_max + qnorm)):
        return out
    if weaken != 2 and not gap > 0.0:
        return out
    if weaken != 1 and not list_len[c0] >= near_min:
        return out
    d0 = float(nt.sq_dists_rows(coarse[c0:c0 + 1], q)[0])
    su = np.sqrt(d0) + rmax
    U = su * su * (1.0 + 1e-9)
    out.update(d0=d0, U=float(U))
    out["ok"] = bool(L > d0) if weaken == 3 else bool(lb > U)
    return out
