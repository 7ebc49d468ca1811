"""The certified coarse / assignment filters where fp32 squares underflow, against the oracle, bit for bit.

Every filter in front of an exact fp64 stage decides on d~ = |c|^2 + |x|^2 - 2 x.c in fp32 and an error bound eps.
Coordinates between 1e-17 and 1e-25 put |x|^2, |c|^2 and x.c into fp32's subnormal range, where a relative bound no longer holds;
above and below that band the suite already had cases (1e-9: everything normal; 1e-25: everything zero, nothing certified), inside
it none.  The inputs are near ties (tests/near_ties.py): rows a relative 1e-3 off the middle of two neighbouring centroids, and rows
whose k-th and (k+1)-th nearest centroids are that close -- far from an fp64 tie, so the oracle's answer leans on no tie rule, and
close enough that a bound which is too small certifies the wrong centroid (tests/test_coarse_bound_cpu.py shows it on the CPU).
The same sweep runs through the coarse top-w (one row per kernel family of DESIGN 5.0), the encoder's assignment, VLAD (K8'' with
ragged vocabularies, K8'), bag of words (hard and soft) and the k-means learner; VLAD and BoW also run at the upper guard.
Every comparison is np.array_equal; no scale and no row is filtered."""
import importlib

import numpy as np
import pytest

import near_ties
from bow_twin import BowTwin
from test_gpu_learning import _case, _check, _host, _twin
from test_gpu_parity import _coarse_cells

pytestmark = pytest.mark.gpu

SWEEP = near_ties.SWEEP
UPPER = [1e17, 1.5e18, 1e25, 1e140]


@pytest.fixture(scope="module")
def mi():
    try:
        import torch

        torch.cuda.init()
    except Exception:
        pass
    m = importlib.import_module("multimedia-indexing_amd")
    if m.lib().mmidx_device_count() < 1:
        pytest.fail("libmmidx_hip.so found no HIP device: GPU tests must run the native path")
    return m


def _index(mi, oracle, D, C, w, opts=()):
    """a handle and its oracle twin with a throw-away product quantizer (the coarse stage and the assignment do not read it)"""
    pq = np.random.default_rng(1).standard_normal((2, 16, D // 2))
    ix = mi.IVFPQ(D, 10, False, "", 2, 16, 0, C, 512)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    for name, v in opts:
        ix.set_option(name, v)
    ref = oracle.OracleIndex(oracle.KIND_IVFPQ, D, 2, 16, C)
    ref.set_pq(pq)
    ref.set_w(w)
    return ix, ref


def _assign_cells(mi, ix, X):
    """mmidx_assign_device on device buffers (torch only holds them)"""
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    dX = torch.tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda")
    cells = torch.empty(dX.shape[0], dtype=torch.int32, device="cuda")
    nat.check(mi.lib().mmidx_assign_device(ix._h, dX.shape[0], dX.data_ptr(), cells.data_ptr(), None))
    torch.cuda.synchronize()
    return cells.cpu().numpy()


COARSE = [
    (128, 1024, 8, (), "K1e'+K1f(front_sel)"),
    (32, 1200, 6, (), "K1e'+K1f(front+select_list)"),
    (32, 1200, 1, (), "K1e'+K1f(front+select_list)"),
    (16, 8200, 9, (), "K1e'+K1f(select_grp)"),  # C / 8 > 1024 groups
    (32, 1200, 6, (("coarse_v1", 1),), "K1c+K1d"),  # the fp32 chain and its own formula
]


@pytest.mark.parametrize("D,C,w,opts,family", COARSE, ids=[f"D{r[0]}-C{r[1]}-w{r[2]}" + ("-v1" if r[3] else "") for r in COARSE])
def test_coarse_topw_in_the_band(mi, oracle, D, C, w, opts, family):
    """(a) mmidx_coarse_device: 256 rows at a near tie of ranks 1 / 2 and 16 at a near tie of ranks w / w + 1, ordered cells"""
    rng = np.random.default_rng(D + C + w)
    cent = rng.standard_normal((C, D))
    Q = near_ties.midpoints(rng, cent, 256)
    cent, Qw = near_ties.tie_at_rank(rng, cent, cent[rng.integers(0, C, 64)] + 0.7 * rng.standard_normal((64, D)), w, 16)
    assert len(Qw) == 16
    Q = np.concatenate([Q, Qw])
    ix, ref = _index(mi, oracle, D, C, w, opts)
    for scale in SWEEP:
        ix.loadCoarseQuantizer(cent * scale)
        ref.set_coarse(cent * scale)
        got = _coarse_cells(mi, ix, Q * scale)
        assert ix.get_dispatch()["coarse"] == family, scale
        exp = np.stack([ref.nearest_coarse(q, w) for q in Q * scale])
        bad = np.flatnonzero((got != exp).any(1))
        print(f"coarse {family} D={D} C={C} w={w} scale={scale:.3g}: {len(bad)} of {len(Q)} rows differ")
        assert np.array_equal(got, exp), (scale, bad[:8])
    ix.close()


@pytest.mark.parametrize("D,C", [(128, 1024), (32, 1200), (16, 8200)])
def test_encoder_assignment_in_the_band(mi, oracle, D, C):
    """(b) ix.encode and mmidx_assign_device: 300 near-tie rows (not a multiple of the 128-row tile), cells of encode_batch"""
    rng = np.random.default_rng(D + C)
    cent = rng.standard_normal((C, D))
    X = near_ties.midpoints(rng, cent, 300)
    ix, ref = _index(mi, oracle, D, C, 1)
    for scale in SWEEP:
        ix.loadCoarseQuantizer(cent * scale)
        ref.set_coarse(cent * scale)
        exp, _ = ref.encode_batch(X * scale)
        got, _ = ix.encode(X * scale)
        dev = _assign_cells(mi, ix, X * scale)
        print(f"assign D={D} C={C} scale={scale:.3g}: encode {int((got != exp).sum())}, assign_device {int((dev != exp).sum())} of {len(X)} differ")
        assert np.array_equal(got, exp), scale
        assert np.array_equal(dev, exp), scale
    ix.close()


def _image_sets(rng, cb, sizes):
    """images of near-tie midpoints of codebook rows, every third row an ordinary one"""
    sets = []
    for n in sizes:
        s = near_ties.midpoints(rng, cb, n) if n else np.zeros((0, cb.shape[1]))
        s[2::3] = rng.standard_normal(s[2::3].shape)
        sets.append(s)
    return sets


@pytest.mark.parametrize("nc,dl", [(128, 64), (100, 64), (17, 64), (3, 64), (2, 64), (20, 12)])
def test_vlad_ragged_vocabularies_and_magnitudes(mi, oracle, nc, dl):
    """(c) raw VLAD vectors.  dl = 64, nc <= 128: K8'' (k_vlad_fused) under (0, 0) -- vocabularies that are no multiple of 16 reach its
    padding rows, its index clamp and its output mask --, K8' under two_pass, the fp64 block under exact; (20, 12): K8'.  Scale 1, the
    band, and for the two large vocabularies the upper edge."""
    rng = np.random.default_rng(nc + dl)
    cb = rng.standard_normal((nc, dl))
    sets = _image_sets(rng, cb, (0, 1, 130, 513))
    for scale in [1.0] + near_ties.BAND + (UPPER if nc >= 100 else []):
        cbs, ss = cb * scale, [s * scale for s in sets]
        ref = [oracle.vlad_aggregate(cbs, s) for s in ss]
        agg = mi.VladAggregator(cbs)
        for exact, two in ((0, 0), (0, 1), (1, 0)):
            agg.set_option("exact", exact)
            agg.set_option("two_pass", two)
            out = agg.aggregate_batch(ss)
            assert out.shape == (len(ss), nc * dl)
            for i in range(len(ss)):
                assert np.array_equal(out[i], ref[i]), (scale, exact, two, i)
        agg.close()


@pytest.mark.parametrize("nc,dl,k", [(128, 64, 1), (128, 64, 3), (4096, 64, 1), (4096, 64, 3)])
def test_bow_in_the_band_and_at_the_upper_guard(mi, oracle, nc, dl, k):
    """(d) hard and soft histograms: near ties at ranks 1 / 2, and for soft at ranks k / k + 1 as well"""
    rng = np.random.default_rng(nc + dl + k)
    cb = rng.standard_normal((nc, dl))
    rows = near_ties.midpoints(rng, cb, 150)
    if k > 1:
        cb, extra = near_ties.tie_at_rank(rng, cb, cb[rng.integers(0, nc, 64)] + 0.7 * rng.standard_normal((64, dl)), k, 16)
        assert len(extra) == 16
        rows = np.concatenate([rows, extra])
    sets = [rows[:97], rows[97:], rows[:0]]
    for scale in near_ties.BAND + [1.5e18]:
        cbs, ss = cb * scale, [s * scale for s in sets]
        ref = BowTwin(oracle, cbs, k).aggregate_batch(ss)
        agg = mi.BowAggregator(cbs, k)
        out = agg.aggregate_batch(ss)
        agg.close()
        assert np.array_equal(out, ref), (scale, int((out != ref).sum()))


def test_kmeans_on_rows_scaled_into_the_band(mi):
    """(e) the learner's assignment (mmidx_assign_device through mmidx_learn.hip): the split_d4 fixture times 1e-22, against the twin"""
    X, kw = _case("split_d4")
    X = X * 1e-22
    k, it = kw.pop("k"), kw.pop("it")
    seed, twin = _twin(X, k, it, **kw)
    _check(_host(mi, X, k, it, seed=seed, **kw), twin)
