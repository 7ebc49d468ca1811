"""Pass B's table filters and the kernels behind them where fp32 and fp64 scales run out: K3g (`k_scan_grp`: the plain, UNION, flat-PQ
and run-time-dsub instances, m = 8 .. 64), K3s in front of it (`k_pair_smin`, `k_pair_smin_mfma`, the bf16 first stage), K3f as the
main scan (the `nofilter` branch of its `rebuild`) and K3h in front of them all (the `inv = 0` branch of its bucket map), against the
oracle bit for bit: ids, distance bits and counts of every query, no row filtered.

One index per (shape, scale); the oracle is loaded with the device's own lists (encode parity is asserted on 500 rows at scale 1),
then the public switches are walked on that handle -- none of them changes a result -- and mmidx_get_dispatch must name the kernel
each set is there for.  The scales: the ordinary ones, the two bands the CPU model (tests/test_passb_bound_cpu.py)
reports in half decades -- 1e-14 .. 1e-17, where K3g goes from state 0 to "handed back" (`iv < 1e30`), and 1e13 .. 1e15, where `es
< 1e24` hands back -- and the far ends 1e-19 .. 1e-160 and 3e18 .. 1e140, where fp32 squares flush or overflow, K3f's threshold
reaches fp64's subnormals and K3h's bucket width leaves [0, 1e300).

What these runs can catch: on random data the byte filter has a slack of about m quantisation steps, so a bound a few ulps short
does not show here.  The GPU runs catch the gross failures -- inf or NaN in a table, a blind or dead filter, a wrong hand-back, a
list overflow.  The subtle ones are the CPU model's job; that is why it checks B1 .. B4 per entry.

Regime checks use the existing statistics.  mmidx_stats::verified_codes is fed by K3g (and K3m / K3ma) only -- K3f and the exact
scan have no counter, their figure is 0 whatever they evaluate.  They are made on a call of their own without the query 1e6 times
the data's scale (at 1e-19 its threshold is one fp32 still carries: its pairs are scanned, blind, as the model's far-query case
says; flat PQ also leaves out the query x 1e-6, which there is its own residual), for `no_union` = 1 and -1:
  - hand_back_forecast() evaluates K3g's own guards on the host for every far pair of the call -- `iv < 1e30` from the bracket the
    query's threshold lies in during pass B, `es < 1e24` and `|Smin_lo| < 1e30` from the pair's residual -- and says whether every
    pair is certainly handed back, or some pair certainly is not;
  - at EVERY scale the model calls "handed back" (1e-17 .. 3.16e-16, 1e14 .. 1e15, the far ends) the forecast must say "all handed
    back", and at every scale it calls state 0 (the ordinary ones, 1e-14 .. 1e-15, 1e13, 3.16e13) "some pair scanned"; where the
    data's edge is not the model's -- T grows with D and the cut with QMAX, es with D -- the exception is listed with its reason
    (NOT_ALL_STATE0, NOT_ALL_HANDED_BACK);
  - wherever the forecast says "all handed back", K3g's figure equals that of K3f as the main scan of the same call: every item
    went there, K3g itself verified nothing.  A guard that fires half a decade late on the device fails this;
  - wherever it says "some pair scanned" at a state-0 scale, pass B had items and K3g verified something: a guard that fires early;
  - at scale 1 K3g verifies fewer codes than the unfiltered scan (`no_filter`) of the same call evaluates: at most the lengths of
    the shortest far lists, as many as pairs survived the coarse bound -- which is that run's own scan_codes - passa_codes where
    no pair fell to the coarse bound (asserted).
The figures are printed; no ratio is fixed.

What the library cannot do is not asserted: m = 64 has no K3f instance (with `no_grp` its pass B is the exact scan, and the dispatch
text says so); K3h keeps at most 256 entries per item, so it does not serve k = 300; its table must fit 64 KiB next to the
position buffer, which 32 x 256 doubles do not -- the m = 32 shape runs twice, at ks = 200 with the K3h sets (which also puts K3g's
+inf padding entries on the device) and at ks = 256 without them; and with w = 1 there is no pass A at all (one exact pass), so the
K3h runs at 1e-160 and 1e140 are those at w = 6 and the w = 1 call checks the answers."""
import functools
import importlib

import numpy as np
import pytest

import near_ties
import passb_bound as pb
import synth

pytestmark = pytest.mark.gpu

# name: kind, D, m, C, n, w, k, transform, ks, what the shape reaches
SHAPES = {
    "m16x8": ("ivfpq", 128, 16, 6, 12000, 6, 20, 0, 256),    # K3g <16, 8, 8>, K3s dsub 8
    "m8x16": ("ivfpq", 128, 8, 6, 12000, 6, 20, 0, 256),     # K3g dsub 16, K3s with the bf16 stage
    "m32x4": ("ivfpq", 128, 32, 4, 8000, 4, 20, 0, 200),     # K3g groups of four, dsub 4, K3s in two slice groups (atomicAdd)
    "m32x4_ks256": ("ivfpq", 128, 32, 4, 8000, 4, 20, 0, 256),  # the same at ks = 256 (K3h cannot hold that table: no K3h sets)
    "m8x12": ("ivfpq", 96, 8, 4, 8000, 4, 10, 0, 256),       # K3g's run-time-dsub instance; K3s sits out
    "perm_k300": ("ivfpq", 64, 16, 4, 8000, 4, 300, 2, 256),  # candidate buffers of 512, the permuted residual path (K1 > 256: no K3h)
    "flat_m8": ("pq", 64, 8, 1, 20000, 1, 20, 0, 256),       # K3g's flat-PQ instance (k_flat_lut, QMAX 127), chunks of 4096
    "m64x8": ("ivfpq", 512, 64, 4, 4000, 4, 10, 0, 256),     # K3g m = 64
}
LOW_BAND = [10.0 ** (-e / 2.0) for e in range(28, 35)]   # 1e-14 .. 1e-17
HIGH_BAND = [10.0 ** (e / 2.0) for e in range(26, 31)]   # 1e13 .. 1e15
FAR = [1e-19, 1e-22, 1e-25, 1e-160, 3e18, 1e19, 1e25, 1e140]
# the model's regimes of the plain case, the same for every shape: state 0 from 1e-15 to 3.16e13, handed back outside
STATE0 = set(near_ties.ORDINARY) | {s for s in LOW_BAND if s > 0.9e-15} | {s for s in HIGH_BAND if s < 3.2e13}
HANDED_BACK = set(FAR) | {s for s in LOW_BAND if s < 0.9e-15} | {s for s in HIGH_BAND if s > 3.2e13}
# Where this data's edges are not the model's (the model's T is the 20th of 514 random codes of a 128-dimensional pair, QMAX 127).
# `iv < 1e30` hands back once T <= (QMAX - 1) 1e-30 and T grows with D: at 1e-15 the thresholds of the D = 128 shapes lie between
# 1.26e-28 and 2.54e-28 -- the QMAX 127 instances scan, the UNION ones (QMAX 255) hand back -- and those of the D = 64 shapes lie
# below both.  `es < 1e24` trips at a scale ~ 1 / sqrt(D): D = 512 is handed back at 3.16e13 already, flat PQ (D = 64, the residual
# is the query itself) still scans a few of its pairs at 1e14.  hand_back_forecast() computes all of this from the guards; these
# sets only say where the model's regime is not expected, and the forecast is asserted against the device everywhere.
_D128 = ("m16x8", "m8x16", "m32x4", "m32x4_ks256")
NOT_ALL_STATE0 = ({(n, 1e-15, "K3g-1") for n in _D128} | {(n, 1e-15, key) for n in ("perm_k300", "flat_m8") for key in ("K3g1", "K3g-1")} |
                  {("m64x8", 10.0 ** 13.5, key) for key in ("K3g1", "K3g-1")})
NOT_ALL_HANDED_BACK = {("flat_m8", 1e14, "K3g1"), ("flat_m8", 1e14, "K3g-1")}
NO_K3F = "K3(exact scan: no K3f instance for this shape)"
SCALES = list(near_ties.ORDINARY) + LOW_BAND + HIGH_BAND + FAR
DEFAULTS = dict(no_mfma=1, no_grp=0, no_union=1, no_filter=0, smin_pre=0, smin_valu=0, smin_bf16=1, passa_q=-1, passa_hist=-1,
                passb_small=0)  # (passb_small = 0: a call that kept <= 64 pairs must not turn the next one into K3f's looping launch)


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    if m.lib().mmidx_device_count() < 1:
        pytest.fail("libmmidx_hip.so found no HIP device: GPU tests must run the native path")
    return m


@functools.lru_cache(maxsize=None)
def unit_data(name):
    """(centroids or None, base, pq, queries) at unit scale, as test_mfma_pass_b_magnitudes draws them (everything is multiplied
    by the scale afterwards, the self-queries' 0.01 N offset included); computed once per shape"""
    kind, D, m, C, n, w, k, tr, KS = SHAPES[name]
    rng = np.random.default_rng(11 + D + m)
    ds = D // m
    if kind == "ivfpq":
        mu = 0.5 * rng.standard_normal((C, D))
        lab = rng.integers(0, C, n)
        base = mu[lab] + rng.standard_normal((n, D))
        res = mu[rng.integers(0, C, 3000)] - base[:3000]
    else:
        mu, lab = None, np.arange(n) % 2
        base = rng.standard_normal((n, D))
        res = base[:3000]
    pq = np.stack([synth.kmeans(res[:, s * ds:(s + 1) * ds], KS, iters=2, seed=s) for s in range(m)])
    # 24 midpoints of vectors of different cells (far probes feed pass B), 24 self-queries, one far out, one far in, a centroid
    a = np.arange(24)
    b = np.array([int(np.nonzero(lab[100:] != lab[i])[0][0]) + 100 for i in a])
    mid = 0.5 * (base[a] + base[b])
    own = base[200:224] + 0.01 * rng.standard_normal((24, D))
    Q = [mid, own, 1e6 * mid[:1], 1e-6 * own[:1]]
    Q.append(mu[:1] if kind == "ivfpq" else np.zeros((1, D)))  # (flat PQ: the zero vector is its zero residual)
    return mu, base, pq, np.concatenate(Q)


def option_sets(name):
    """(options, expected dispatch) of every search on a handle, in order"""
    kind, D, m, C, n, w, k, tr, KS = SHAPES[name]
    pre_applies = kind == "ivfpq" and (D // m) in (4, 8, 16)
    sets = []
    for union in (1, -1):
        sets.append((dict(no_union=union), dict(pass_b="K3g", pre="-")))
        if kind == "ivfpq":
            for valu, b16 in ((0, 1), (1, 1), (0, 0)) if pre_applies else ((0, 1),):
                sets.append((dict(no_union=union, smin_pre=1, smin_valu=valu, smin_bf16=b16), dict(pass_b="K3g", pre="K3s" if pre_applies else "-")))
    sets.append((dict(no_grp=1), dict(pass_b="K3f" if m < 64 else NO_K3F, pre="-")))  # K3f as the main scan
    if k + 1 <= 256 and m * KS * 8 < 65536:  # K3h (an item keeps at most 256 entries; its table and buffers share 64 KiB) in front of each of the above
        sets += [(dict(o, passa_q=0, passa_hist=1), dict(e, pass_a="K3h")) for o, e in list(sets)]
    sets.append((dict(passa_q=0, passa_hist=0), dict(pass_b="K3g", pre="-")))  # the control: pass A by the exact scan
    return sets


def run(ix, opts, Q, k):
    for key, v in dict(DEFAULTS, **opts).items():
        ix.set_option(key, v)
    ix.set_profiling(True)
    got = ix.search_batch(k, Q)
    return got, ix.get_stats(), ix.get_dispatch()


def same(got, want):
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)


def hand_back_forecast(name, Qk, mu, pq, ref, oracle, k, qmax, cds):
    """K3g's own guards evaluated on the host for the pairs of a call (tests/passb_bound.py has the formulas): `iv = (QMAX - 1) / T <
    1e30` needs the query's threshold, which pass B sees somewhere between the (k + 1)-th distance over all probed lists (where it
    ends) and that of the nearest list alone (where pass A leaves it; flat PQ: of the first chunk, computed here in numpy); `es <
    1e24` and `|Smin_lo| < 1e30` need the pair's residual (Smin is bounded by the exact sum of row minima and by es).  Returns (all_handed, some_scanned): every far pair certainly in state 2 / some
    far pair certainly not, each with a margin of 1e-3 so that the fp64 details of the kernel's sums do not matter."""
    kind, D, m, C, n, w, k_, tr, KS = SHAPES[name]
    ds = D // m
    pn = (pq * pq).sum(-1)  # [m][ks]
    pm2 = pn.max(1) * (1.0 + 1e-12)
    pm = np.sqrt(pn.max(1)) * (1.0 + 1e-12)
    t_lo = ref.search_batch(Qk, k + 1)[1][:, k]
    t_hi = np.full(len(Qk), np.inf)
    if kind == "ivfpq":
        ref.set_w(1)
        t_hi = ref.search_batch(Qk, k + 1)[1][:, k]
        ref.set_w(w)
    else:  # flat PQ: pass A is the first chunk of 4096 codes
        idx = cds[:4096].astype(np.int64) + 128
        with np.errstate(all="ignore"):
            for i, q in enumerate(Qk):
                tab = ((q.reshape(m, 1, ds) - pq) ** 2).sum(-1)  # [m][ks]
                t_hi[i] = np.sort(tab[np.arange(m)[None, :], idx].sum(1))[k]
    cut = (qmax - 1.0) * 1e-30
    perm = oracle.random_permutation(1, D) if tr == 2 else np.arange(D)
    all_handed, some_scanned = True, False
    with np.errstate(all="ignore"):
        for i, q in enumerate(Qk):
            cells = ref.nearest_coarse(q, w)[1:] if kind == "ivfpq" else [None]
            for c in cells:
                r = ((mu[c] - q) if kind == "ivfpq" else q)[perm].reshape(m, ds)
                nr = (r * r).sum(1)
                es = float(pb.err_k3g(nr, pm, pm2, ds).sum())
                smin_ub = float(((r[:, None, :] - pq) ** 2).sum(-1).min(1).sum()) + es
                handed = (t_hi[i] <= cut * (1 - 1e-3)) or not (es < 1e24 * (1 + 1e-3))
                scanned = t_lo[i] > cut * (1 + 1e-3) and es < 1e24 * (1 - 1e-3) and smin_ub < 1e30 * (1 - 1e-3)
                all_handed &= bool(handed)
                some_scanned |= bool(scanned)
    return all_handed, some_scanned


CASES = [pytest.param(name, scale, id=f"{name}-{scale:.3g}") for name in SHAPES for scale in SCALES]


@pytest.mark.parametrize("name,scale", CASES)
def test_pass_b_filters_at_every_magnitude(mi, oracle, name, scale):
    kind, D, m, C, n, w, k, tr, KS = SHAPES[name]
    mu1, base1, pq1, Q1 = unit_data(name)
    base, pq, Q = base1 * scale, pq1 * scale, Q1 * scale
    if kind == "ivfpq":
        mu = mu1 * scale
        ix = mi.IVFPQ(D, n, False, "", m, KS, tr, C, 512)
        ix.loadCoarseQuantizer(mu)
        ix.setW(w)
        ref = oracle.OracleIndex(oracle.KIND_IVFPQ, D, m, KS, C, transform=tr, perm=oracle.random_permutation(1, D) if tr == 2 else None)
        ref.set_coarse(mu)
        ref.set_w(w)
    else:
        ix = mi.PQ(D, n, False, "", m, KS, tr, 512)
        ix.set_option("flat_chunk", 4096)
        ref = oracle.OracleIndex(oracle.KIND_PQ, D, m, KS, transform=tr)
    ix.loadProductQuantizer(pq)
    ref.set_pq(pq)
    ix.indexVectors(list(range(n)), base)
    off, iids, cds = ix.export()
    ref.load_lists(off, iids, cds)
    if scale == 1.0:  # the lists are the device's own: the encoder is held to the oracle's here
        cells, codes = ix.encode(base[:500])
        rcells, rcodes = ref.encode_batch(base[:500])
        assert np.array_equal(codes.astype(np.int32) + 128, rcodes)
        assert kind == "pq" or np.array_equal(cells, rcells)
    try:
        _walk(ix, ref, oracle, name, scale, Q, off, mu if kind == "ivfpq" else None, pq, cds)
    finally:
        ix.close()


def _walk(ix, ref, oracle, name, scale, Q, off, mu, pq, cds):
    kind, D, m, C, n, w, k, tr, KS = SHAPES[name]
    k3f = "K3f" if m < 64 else NO_K3F
    want = ref.search_batch(Q, k)
    stats = {}
    for opts, expect in option_sets(name):
        got, st, disp = run(ix, opts, Q, k)
        stats[tuple(sorted(opts.items()))] = st
        print(name, scale, opts, {f: disp[f] for f in ("pass_a", "pre", "pass_b")}, "items", st["passb_items_last"], "verified", st["verified_codes"])
        for field, label in expect.items():
            assert disp[field] == label, (opts, disp)
        same(got, want)
    if scale == 1.0:  # the filter filters: fewer codes verified than the unfiltered scan of the same call evaluates
        st1 = stats[(("no_union", 1),)]
        items = st1["passb_items_last"]
        got, st, disp = run(ix, dict(no_filter=1), Q, k)
        assert disp["pass_b"] == NO_K3F, disp  # (`no_filter`: pass B by the exact scan)
        same(got, want)
        if kind == "pq":
            floor = len(Q) * (n - 4096)  # (every chunk but the first of every query)
            all_pairs = True
        else:
            lens = np.diff(off)
            far = sorted(int(lens[c]) for q in Q for c in ref.nearest_coarse(q, w)[1:])
            floor = sum(far[:items])  # the shortest far lists, as many as pairs survived the coarse bound
            all_pairs = items == len(far)
        print(name, "K3g verified", st1["verified_codes"], "unfiltered: at least", floor, "in", items, "pairs; scan_codes - passa_codes",
              st["scan_codes"] - st["passa_codes"])
        if all_pairs:  # no pair fell to the coarse bound: the unfiltered run's own figures say what it evaluated
            assert st["scan_codes"] - st["passa_codes"] == floor
        assert 0 < st1["verified_codes"] < floor
    # the regime of the call without the rescaled queries (a query x 1e6 keeps a threshold fp32 carries twenty decades further down
    # and is dropped for every shape; the query x 1e-6 is dropped for flat PQ only, where it is its own residual)
    keep = [i for i in range(len(Q)) if i != 48 and not (kind == "pq" and i == 49)]
    fig = {}
    for opts, label in ((dict(no_union=1), "K3g"), (dict(no_union=-1), "K3g"), (dict(no_grp=1), k3f)):
        got, st, disp = run(ix, opts, Q[keep], k)
        assert disp["pass_b"] == label, (opts, disp)
        same(got, tuple(a[keep] for a in want))
        fig[label + str(opts.get("no_union", ""))] = (st["verified_codes"], st["passb_items_last"])
    # (QMAX: 255 in the IVF UNION instances, which the run-time-dsub shape does not have; 127 everywhere else)
    qmax = {"K3g1": 127, "K3g-1": 255 if kind == "ivfpq" and (D // m) in (4, 8, 16) else 127}
    cast = {key: hand_back_forecast(name, Q[keep], mu, pq, ref, oracle, k, qm, cds) for key, qm in qmax.items()}
    print(name, scale, "regime figures (verified, items):", fig, "forecast (all handed back, some scanned):", cast)
    if name == "m16x8" and scale in (1e-160, 1e140):  # the scales of K3h's inv = 0 branch (every code a candidate) at w = 1 as well
        ix.setW(1)
        ref.set_w(1)
        got, st, disp = run(ix, dict(passa_q=0, passa_hist=1), Q, k)
        assert disp["pass_a"] == "K3(single pass)" and disp["pass_b"] == "-", disp
        same(got, ref.search_batch(Q, k))
        ix.setW(w)
        ref.set_w(w)
    got, st, disp = run(ix, {}, Q[:1], k)  # a one-query call: groups of one pair
    assert disp["pass_b"] == "K3g", disp
    same(got, tuple(a[:1] for a in want))
    for key in ("K3g1", "K3g-1"):
        all_handed, some_scanned = cast[key]
        if scale in HANDED_BACK and (name, scale, key) not in NOT_ALL_HANDED_BACK:
            assert all_handed, (key, cast)  # (the model's regime holds for this data: the check below is not void)
        if scale in STATE0 and (name, scale, key) not in NOT_ALL_STATE0:
            assert some_scanned, (key, cast)
        if all_handed:  # every item of K3g went to K3f: its figure is that of K3f as the main scan of the same call
            assert fig[key][0] == fig[k3f][0], (key, fig)
        if some_scanned and scale in STATE0:
            assert kind == "pq" or fig[key][1] > 0
            assert fig[key][0] > 0, (key, fig)
