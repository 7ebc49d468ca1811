"""The certificate of pass B's table filters -- K3g (`k_scan_grp`: fp32 table entries, u8 rows, the survivor bound th) and K3s
(`k_pair_smin`, `k_pair_smin_mfma`, `k_pair_smin_bf16`: a lower bound of a pair's Smin) -- checked numerically on the CPU where fp32
and fp64 scales run out (csrc/mmidx_scan_grp.h; DESIGN.md sections 5.2 / 5.3).  tests/passb_bound.py replays the kernels' arithmetic
in numpy, in two readings of results below 2^-126 (gradual underflow, flush to zero); exact values are np.longdouble.

Sweep (passb_bound.SCALES x MIXES x KS x SHAPES): 64 (query, cell) residuals per shape, 512 random codes per pair plus the codes of
every sub-quantizer's nearest and second-nearest entry, ks = 256 and 200 (the +inf padding), the scales near_ties.ORDINARY, 1e-10 ..
1e-20 and 1e12 .. 1e20 in half decades, 1e-25, 1e-45, 1e25, 1e140, and at each scale three mixed cases (query x 1e6, codebook x 1e-8,
a zero residual).  T per pair: the exact 20th-smallest distance among its codes, that times 1 + 1e-6, that times 4.

  B1  |entry32 - exact| <= s_err for every entry j < ks of every row of a pair in state 0 (K3g; VALU form), and of every pair whose
      terms all pass `err < 1e22` (K3s; VALU, matrix-core and bf16 forms), in both readings
  B2  state 0 and exact d <= T  =>  the code's byte sum is at most th (QMAX 127 and 255 fused, QMAX 127 generic)
  B3  K3s's smin <= the exact sum of row minima (= the smallest exact d over all ks^m codes), every form
  B4  a pair not in state 0 is handed back (state 2), or is in state 1 with exact Smin >= T
  A   teeth: each guard / term weakened on its own.  Over this sweep
        K3s  without `err < 1e22`: B1 and B3 fail (far queries from scale 1e13 on: fp32 entries overflow to inf / NaN);
             without `+ 1e-30`:    B1 and B3 fail in the flush reading from scale 1e-17 down (entries flushed to zero, relative terms
                                   of the bound below what was lost);
        K3g  without `+ 1e-30`:    B1 fails in the flush reading at scale 1e-15 with the codebook x 1e-8 (m = 32, dsub 4: ||p||^2 ~
                                   1e-46 is flushed from a row whose relative terms are smaller than that);
             without `es < 1e24` and without `iv < 1e30`: NOTHING fails.  Both are redundant over this sweep, because another guard
             of phase (a) / (e) closes the same range: without `iv` (T < 1.3e-28, scale ~3e-16 down) the m x 1e-30 of es push
             Smin_lo below zero and th into its 32000 clamp -- a blind scan, not a wrong one -- and `|Smin_lo| < 1e30` trips half a
             decade of scale after `es < 1e24` does, eight decades of squares before fp32 overflows.  The kernel is left as it is.
  C   at the ordinary scales (and in every mixed case at scale 1) no pair is handed back and every pair is filtered (th below the
      blind value m x QMAX): nothing is bought by handing back more.

The test prints, per shape, the scale intervals of the three regimes (state 0 / blind / handed back) for T = the 20th-smallest
distance, and where K3s bounds; DESIGN.md section 5.3 carries them and tests/test_gpu_passb_magnitudes.py takes its bands from them.

Run time: 180 configurations per shape (each for both ks), both readings where they differ, ~0.5 s apiece in longdouble -- six minutes in one
process.  passb_bound.sweep shares them among up to eight spawned workers (half the CPUs at most): about two and a half minutes
for the module, the sweep of a shape computed once and shared by the tests."""
import pytest

import near_ties
import passb_bound as pb

SHAPES = [pytest.param(m, dsub, id=f"m{m}x{dsub}") for m, dsub in pb.SHAPES]
TEETH = {("s", "no_err_guard"), ("s", "no_abs_term"), ("g", "no_abs_term")}
REDUNDANT = {("g", "no_es_guard"), ("g", "no_iv_guard")}


def _violations(m, dsub, fam, variant):
    """{(scale, mix, ks, ftz): {assertion: count}} of the entries of the sweep where `variant` breaks something"""
    return {k: {b: n for b, n in r[fam][variant].items() if n} for k, r in pb.sweep(m, dsub).items() if any(r[fam][variant].values())}


@pytest.mark.parametrize("m,dsub", SHAPES)
def test_b_the_certificate_holds(m, dsub):
    for ftz in (False, True):
        for ks in pb.KS:
            for mix in pb.MIXES:
                print(f"K3g m={m} dsub={dsub} ks={ks} {mix} {'flush' if ftz else 'gradual'}:",
                      "; ".join(f"{lo:.3g} .. {hi:.3g} {name}" for lo, hi, name in pb.intervals(m, dsub, ks, mix, ftz)))
                if dsub in (4, 8, 16):
                    print(f"K3s m={m} dsub={dsub} ks={ks} {mix} {'flush' if ftz else 'gradual'}:",
                          "; ".join(f"{lo:.3g} .. {hi:.3g} {name}" for lo, hi, name in pb.intervals(m, dsub, ks, mix, ftz, k3s=True)))
    assert _violations(m, dsub, "g", "kernel") == {}
    assert _violations(m, dsub, "s", "kernel") == {}


def test_a_teeth():
    found = {}
    for fam, variants in (("g", pb.G_VARIANTS[1:]), ("s", pb.S_VARIANTS[1:])):
        for v in variants:
            bad = {}
            for m, dsub in pb.SHAPES:
                bad.update({(m, dsub) + k: c for k, c in _violations(m, dsub, fam, v).items()})
            found[(fam, v)] = bad
            print(fam, v, len(bad), "entries of the sweep fail;", sorted(bad.items(), key=str)[:4])
    assert {k for k, bad in found.items() if bad} == TEETH
    assert {k for k, bad in found.items() if not bad} == REDUNDANT  # (the docstring says so: keep it true)


@pytest.mark.parametrize("m,dsub", SHAPES)
def test_c_ordinary_magnitudes_are_filtered(m, dsub):
    sw = pb.sweep(m, dsub)
    keys = [(s, "plain") for s in near_ties.ORDINARY] + [(1.0, mix) for mix in pb.MIXES[1:]]
    for scale, mix in keys:
        for ks in pb.KS:
            for ftz in (False, True):
                r = sw[(scale, mix, ks, ftz)]
                assert r["handed"] == 0, (scale, mix, ks, ftz)
                assert r["regime"] == (pb.NPAIR, 0, 0, 0), (scale, mix, ks, ftz)
