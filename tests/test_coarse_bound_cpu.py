"""The certificate of the bf16-split coarse / assignment filters (csrc/mmidx_device_util.h: filter_eps_split16, filter_norms_usable;
DESIGN.md section 5.1), checked numerically on the CPU where fp32 squares underflow.

K6a' (k_assign_gmin16_t) and K8'' (k_vlad_fused) certify a row when `second - best > 2 eps` over d~ = (|c|^2 + |x|^2) - 2 S, S the sum
of three bf16 products accumulated in fp32; K1f selects with the same eps.  The claim is |d~ - d| <= eps.  This file replays that
arithmetic in numpy -- fp64 rows rounded to fp32, split into a bf16 head and tail, the products head.head, head.tail, tail.head per
block of 32 dimensions accumulated in fp32, fp32 copies of the (rounded-up) squared norms, the epilogue in the kernel's order -- in
two readings of what happens to a result below 2^-126: gradual underflow (IEEE subnormals) and flush to zero.  A build or a chip may
apply either at any step; a sound bound holds under both.

The inputs are near ties of the two nearest centroids (tests/near_ties.py), swept from 1e-17 to 1e-25 in half decades, plus 1e-9, 1
and 1e9.  Three assertions:
  A  the inputs have teeth: with the bound as it stood before the absolute term and the lower guard, the model certifies wrong
     argmins in the band, in each reading;
  B  with the bound as the kernels have it now, no certified argmin is wrong and |d~ - d| <= eps holds for every centroid of every
     row that passes the guard, in both readings;
  C  nothing was bought by certifying less: at 1e-9, 1 and 1e9 both bounds certify exactly the same rows."""
import functools

import numpy as np
import pytest

import near_ties

C, NQ = 1200, 400
TINY = np.float32(2.0 ** -126)


# ---- the two bounds -------------------------------------------------------------------------------------------------------------
def eps_before_this_change(Dp, xnorm, xn2, cnorm_max, cn2_max):
    """the formula every copy carried: relative terms only"""
    sumn = cnorm_max + xnorm
    return (2.0 * 3.1 * 2.0 ** -16 * xnorm * cnorm_max + 2.0 * (3.0 * Dp + 16.0) * 2.0 ** -22 * xnorm * cnorm_max +
            1e-12 * (cn2_max + xn2) + 2.0 ** -21 * sumn * sumn) * (1.0 + 1e-9)


def usable_before_this_change(sumn):
    return sumn * sumn < 1e37


def filter_underflow_eps(Dk, sumn):
    return (12.0 * Dk + 16.0 + 8.0 * np.sqrt(float(Dk)) * sumn) * 2.0 ** -126


def filter_eps_split16(Dp, epi, xnorm, xn2, cnorm_max, cn2_max):
    """mirror of the __device__ function of the same name, operation for operation"""
    sumn = cnorm_max + xnorm
    return (2.0 * 3.1 * 2.0 ** -16 * xnorm * cnorm_max + 2.0 * (3.0 * Dp + 16.0) * 2.0 ** -22 * xnorm * cnorm_max +
            1e-12 * (cn2_max + xn2) + epi * sumn * sumn + filter_underflow_eps(Dp, sumn)) * (1.0 + 1e-9)


def filter_norms_usable(sumn):
    return (sumn * sumn < 1e37) & (sumn * sumn > 1e-37)


# ---- the kernels' arithmetic ----------------------------------------------------------------------------------------------------
# fp32 arithmetic on subnormal operands is an order of magnitude slower on a CPU, and the band is nothing but subnormals.  Scaling by
# a power of two commutes with every fp32 rounding except underflow, so in the band the model works on rows times 2^74 and centroids
# times 2^75: products, sums, norms and d~ are then in units of 2^-149 -- the subnormal step is 1 (np.rint; sums of integers need no
# further rounding, exactly as subnormal additions are exact) and the smallest normal number is 2^23 -- and underflow is applied by
# hand.  At 1e-9, 1 and 1e9 the arrays are used as they are (K = 0: the hardware's own gradual underflow, a flush by hand).
def _bf16(f):
    """fp32 -> bf16 (round to nearest even), returned as fp32"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _flush_small(a, ftz):
    if ftz:
        a[np.abs(a) < TINY] = 0.0
    return a


def _split(X, ftz):
    """bf16 head and tail of fl32(X), as k_split_bf16 and the kernels that split in registers form them (unscaled: small arrays)"""
    with np.errstate(under="ignore"):
        f = _flush_small(X.astype(np.float32), ftz)
        h = _flush_small(_bf16(f), ftz)
        l = _flush_small(_bf16(_flush_small(f - h, ftz)), ftz)
    return h, l


class _Underflow:
    """what a square-sized fp32 result (product, sum, norm, d~) suffers below 2^-126, on arrays scaled by 2^K"""

    def __init__(self, K, ftz, shape):
        self.K, self.ftz = K, ftz
        self.tiny = np.float32(2.0 ** (K - 126))
        self.half_step = 2.0 ** (K - 150)
        self.tmp = np.empty(shape, np.float32)
        self.mask = np.empty(shape, bool)

    def product_is_zero(self, amax, bmax):
        """every product of the step underflows to zero (sound shortcut: the step leaves the accumulators as they are)"""
        return amax * bmax < (float(self.tiny) if self.ftz else self.half_step)

    def __call__(self, v, is_sum=False):
        if self.ftz:
            if v.shape == self.tmp.shape:
                np.abs(v, out=self.tmp)
                np.greater_equal(self.tmp, self.tiny, out=self.mask)
                np.multiply(v, self.mask, out=v)
            else:
                v[np.abs(v) < self.tiny] = 0.0
        elif self.K and not is_sum:
            np.rint(v, out=v)  # (K = 149: a no-op at and above 2^23, the subnormal grid below)
        return v


def filter_distances(X, Cn, ftz, band):
    """d~[n][C] (fp64 copy of the fp32 values) as K6a' / K8'' form it, and the fp64 squared norms the bound is evaluated with"""
    ka, kb = (74, 75) if band else (0, 0)
    K = ka + kb
    xh, xl = (np.ldexp(v, ka) for v in _split(X, ftz))
    ch, cl = (np.ldexp(v, kb) for v in _split(Cn, ftz))
    n, D = X.shape
    acc = np.zeros((n, Cn.shape[0]), np.float32)
    p = np.empty_like(acc)
    uf = _Underflow(K, ftz, acc.shape)
    with np.errstate(under="ignore"):
        for k0 in range(0, D, 32):  # one matrix-core step = 32 dimensions; head.head, head.tail, tail.head of a step in turn
            for a, b in ((xh, ch), (xh, cl), (xl, ch)):
                for j in range(k0, min(k0 + 32, D)):
                    if uf.product_is_zero(float(np.abs(a[:, j]).max()), float(np.abs(b[:, j]).max())):
                        continue
                    np.multiply(a[:, j, None], b[None, :, j], out=p)
                    uf(p)
                    np.add(acc, p, out=acc)
                    uf(acc, is_sum=True)
        xn2 = (X * X).sum(1) * (1.0 + 1e-12)  # rounded up, as the kernels keep it
        cn2 = (Cn * Cn).sum(1)
        xf = np.ldexp(_flush_small(xn2.astype(np.float32), ftz), K)
        cf = np.ldexp(_flush_small(cn2.astype(np.float32), ftz), K)
        s = uf(cf[None, :] + xf[:, None], is_sum=True)
        t = uf(np.float32(2.0) * acc, is_sum=True)
        dv = uf(s - t, is_sum=True)
    return np.ldexp(dv.astype(np.float64), -K), xn2, cn2


@functools.lru_cache(maxsize=None)
def _sweep(D, ftz):
    """per scale: certified rows and wrongly certified rows under either bound, and the worst excess of |d~ - d| over the new eps"""
    cent1, X1 = near_ties.problem(D, C, NQ, seed=100 + D)
    Dp = (D + 31) // 32 * 32
    out = {}
    for scale in near_ties.SWEEP:
        Cn, X = cent1 * scale, X1 * scale
        d = near_ties.sqdist(X, Cn)
        two = np.argsort(d, axis=1)[:, :2]
        # the two nearest, re-evaluated as the reference does (sum of squared differences): distinct, so no tie rule is involved
        d2 = np.stack([((X - Cn[two[:, i]]) ** 2).sum(1) for i in range(2)], axis=1)
        assert np.all(d2[:, 0] != d2[:, 1]), scale
        exact = np.where(d2[:, 0] < d2[:, 1], two[:, 0], two[:, 1])
        dv, xn2, cn2 = filter_distances(X, Cn, ftz, band=scale in near_ties.BAND)
        ix = dv.argmin(1)
        part = np.partition(dv, 1, axis=1)
        gap = part[:, 1] - part[:, 0]
        xnorm = np.sqrt(xn2)
        cn2_max = cn2.max() * (1.0 + 1e-12)
        cnorm_max = np.sqrt(cn2.max()) * (1.0 + 1e-12)
        sumn = cnorm_max + xnorm
        eps_old = eps_before_this_change(Dp, xnorm, xn2, cnorm_max, cn2_max)
        eps_new = filter_eps_split16(Dp, 2.0 ** -21, xnorm, xn2, cnorm_max, cn2_max)
        sure_old = (gap > 2.0 * eps_old) & usable_before_this_change(sumn)
        sure_new = (gap > 2.0 * eps_new) & filter_norms_usable(sumn)
        ok = filter_norms_usable(sumn)
        # (d above is good to ~1e-15 sumn^2: far inside every term of eps)
        excess = (np.abs(dv - d) - eps_new[:, None] - 1e-14 * (sumn * sumn)[:, None])[ok]
        out[scale] = dict(sure_old=sure_old, sure_new=sure_new, wrong_old=int((sure_old & (ix != exact)).sum()),
                          wrong_new=int((sure_new & (ix != exact)).sum()), excess=float(excess.max()) if ok.any() else -np.inf)
    return out


MODES = [pytest.param(False, id="gradual"), pytest.param(True, id="flush")]


@pytest.mark.parametrize("ftz", MODES)
def test_a_the_old_bound_certifies_wrong_argmins_in_the_band(ftz):
    wrong = {(D, s): r["wrong_old"] for D in (32, 64, 128) for s, r in _sweep(D, ftz).items()}
    print({k: v for k, v in wrong.items() if v})
    assert sum(wrong.values()) >= 1
    assert all(v == 0 for (D, s), v in wrong.items() if s in near_ties.ORDINARY)  # (it was right where nothing underflows)


@pytest.mark.parametrize("ftz", MODES)
@pytest.mark.parametrize("D", [32, 64, 128])
def test_b_the_bound_holds_and_no_certified_argmin_is_wrong(D, ftz):
    for scale, r in _sweep(D, ftz).items():
        print(scale, int(r["sure_new"].sum()), r["wrong_new"], r["excess"])
        assert r["wrong_new"] == 0, scale
        assert r["excess"] <= 0.0, scale


@pytest.mark.parametrize("ftz", MODES)
@pytest.mark.parametrize("D", [32, 64, 128])
def test_c_ordinary_magnitudes_certify_the_same_rows(D, ftz):
    sw = _sweep(D, ftz)
    for scale in near_ties.ORDINARY:
        assert np.array_equal(sw[scale]["sure_old"], sw[scale]["sure_new"]), scale
        assert sw[scale]["sure_new"].sum() > NQ // 2  # (and most near ties are still decided by the filter)
