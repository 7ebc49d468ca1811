"""The front end (VLAD, bag of words, PCA, vectorize) at SIFT (128) and colour-SURF (192) descriptor lengths, at vocabularies of more
than one 128-centroid tile, and through its device entry points.

Which kernels serve a shape: dl = 64 and nc <= 128 -> K8'' (k_vlad_fused); dl = 64, nc > 128 -> the assignment over
several tiles + k_vlad_accum<64> (four per-wave centroid ranges); dl != 64 -> k_vlad_accum<0>, with the assignment's one-chunk FROMX
form at dl = 128 and k_split_bf16 + two k chunks at dl = 192; `exact` and a one-centroid vocabulary -> k_vlad.  Raw VLAD and bag of
words are compared with np.array_equal, normalised VLAD and PCA at the stated 1e-12, PCA without whitening also at the bound derived
in tests/frontend_cases.py.  Inputs are near ties (tests/near_ties.py) so that a wrong assignment shows."""
import importlib

import numpy as np
import pytest

import frontend_cases as fc
import near_ties
from bow_twin import BowTwin

pytestmark = pytest.mark.gpu
TOL = 1e-12
OPTS = ((0, 0), (0, 1), (1, 0))  # (exact, two_pass)
SIZES = (0, 1, 7, 130, 513, 130)


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


@pytest.fixture(scope="module")
def nat():
    return importlib.import_module("multimedia-indexing_amd._native")


# ---- 1. raw VLAD ----------------------------------------------------------------------------------------------------------------

def _check_raw(mi, nat, cb, sets, ref):
    """every option pair against the oracle's vectors; `exact` is refused where its block does not fit the LDS, and the handle
    serves the next call all the same"""
    nc, dl = cb.shape
    max_desc = max(len(s) for s in sets)
    agg = mi.VladAggregator(cb)
    for exact, two in OPTS:
        agg.set_option("exact", exact)
        agg.set_option("two_pass", two)
        if exact and fc.exact_lds_bytes(nc, dl, max_desc) > 160 * 1024:
            with pytest.raises(mi.MmidxError) as ei:
                agg.aggregate_batch(sets)
            assert ei.value.status == nat.ERR_UNSUPPORTED
            assert str(ei.value) == f"codebook {nc} x {dl} plus {max_desc} descriptors per image exceed the 160 KiB LDS"
            agg.set_option("exact", 0)
        out = agg.aggregate_batch(sets)
        assert out.shape == (len(sets), nc * dl)
        for i in range(len(sets)):
            assert np.array_equal(out[i], ref[i]), (exact, two, i, int((out[i] != ref[i]).sum()))
    agg.close()


@pytest.mark.parametrize("nc,dl", [(128, 128), (64, 128), (256, 128), (128, 192), (100, 192), (256, 64), (300, 64), (130, 64), (64, 32), (17, 32)])
def test_vlad_raw_bit_exact_at_sift_and_colour_surf_lengths(mi, nat, oracle, nc, dl):
    rng = np.random.default_rng(nc + dl)
    cb = rng.standard_normal((nc, dl))
    sets = fc.image_sets(rng, cb, SIZES)
    ref = [oracle.vlad_aggregate(cb, s) for s in sets]
    # (which shapes the `exact` block refuses at 513 descriptors is fixed here, not left to the formula alone)
    assert (fc.exact_lds_bytes(nc, dl, 513) > 160 * 1024) == ((nc, dl) in ((256, 128), (128, 192)))
    _check_raw(mi, nat, cb, sets, ref)


def test_vlad_exact_refusal_follows_the_stated_descriptor_count(mi, nat, oracle):
    """300 x 64 is 150 KiB of codebook: images of 513 descriptors fit beside it (the case above runs the fp64 block), a call that
    states 1200 does not.  Through the device entry point, where max_desc is the caller's statement."""
    import torch

    rng = np.random.default_rng(364)
    cb = rng.standard_normal((300, 64))
    sets = fc.image_sets(rng, cb, (7, 0, 130, 1))
    assert fc.exact_lds_bytes(300, 64, 513) <= 160 * 1024 < fc.exact_lds_bytes(300, 64, 1200)
    agg = mi.VladAggregator(cb)
    d_off, d_descs, mx = _upload(sets, 64)
    out = torch.full((len(sets), 300 * 64), np.nan, dtype=torch.float64, device="cuda")
    agg.set_option("exact", 1)
    st = mi.lib().mmidx_vlad_aggregate_device(agg._h, len(sets), d_off.data_ptr(), d_descs.data_ptr(), 1200, out.data_ptr(), None)
    assert st == nat.ERR_UNSUPPORTED
    assert mi.lib().mmidx_last_error() == b"codebook 300 x 64 plus 1200 descriptors per image exceed the 160 KiB LDS"
    nat.check(mi.lib().mmidx_vlad_aggregate_device(agg._h, len(sets), d_off.data_ptr(), d_descs.data_ptr(), mx, out.data_ptr(), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, s in enumerate(sets):
        assert np.array_equal(got[i], oracle.vlad_aggregate(cb, s)), i
    agg.close()


@pytest.mark.parametrize("nc,dl", [(256, 128), (256, 64)])
def test_vlad_ties_between_centroid_tiles_first_index_wins(mi, nat, oracle, nc, dl):
    """cb[200] = cb[3]: the equal pair sits in two different 128-centroid tiles of the assignment; cb[131] = cb[130]: inside the
    second tile.  computeNearestCentroid updates on `<` only (AFA:136-155): the first index wins."""
    rng = np.random.default_rng(7 * nc + dl)
    cb = rng.standard_normal((nc, dl))
    cb[200] = cb[3]
    cb[131] = cb[130]
    ties = np.concatenate([cb[[3, 200, 130, 131]], cb[[200, 131, 3]] + 1e-9])
    assert [oracle.nearest_centroid(cb, t) for t in ties] == [3, 3, 130, 130, 3, 130, 3]  # (the reference itself)
    rest = fc.image_sets(rng, cb, (0, 1, 123, 513))
    sets = [ties.copy(), rest[0], rest[1], np.concatenate([rest[2][:60], ties, rest[2][60:]]), rest[3]]
    assert [len(s) for s in sets] == [7, 0, 1, 130, 513]
    ref = [oracle.vlad_aggregate(cb, s) for s in sets]
    _check_raw(mi, nat, cb, sets, ref)


# ---- 2. normalised and multi-vocabulary VLAD at dl = 128 ------------------------------------------------------------------------

def test_vlad_multi_vocab_normalised_sift(mi, oracle):
    """[256, 128, 1]: two tiles, one tile, and a slot without an assignment handle (k_vlad<0>), power + L2 each and L2 over all"""
    rng = np.random.default_rng(128)
    dl = 128
    cbs = [rng.standard_normal((n, dl)) for n in (256, 128, 1)]
    sets = fc.image_sets(rng, cbs[0], (0, 7, 130, 513))
    agg = mi.VladAggregatorMultipleVocabularies(cbs)
    assert agg.getVectorLength() == (256 + 128 + 1) * dl
    out = agg.aggregate_batch(sets)
    for i, s in enumerate(sets):
        ref = oracle.vlad_aggregate_multi(cbs, s, True)
        assert np.max(np.abs(out[i] - ref)) <= TOL, (i, float(np.max(np.abs(out[i] - ref))))
    agg.close()
    # an empty image: every sub-vector has zero norm and becomes all ones (Normalization.java:29-30).  A single vocabulary gets no
    # second L2 (VladAggregatorMultipleVocabularies.java:97), so the ones are the output -- through k_vlad_accum<0> and k_vlad<0>;
    # with three vocabularies the L2 over the concatenation divides them by sqrt(length), which the oracle comparison above covers
    assert np.all(oracle.vlad_aggregate_multi(cbs[:1], sets[0], True) == 1.0)
    for one in ([cbs[0]], [cbs[2]]):
        a1 = mi.VladAggregatorMultipleVocabularies(one)
        o1 = a1.aggregate_batch(sets)
        assert np.all(o1[0] == 1.0)
        for i, s in enumerate(sets):
            assert np.max(np.abs(o1[i] - oracle.vlad_aggregate_multi(one, s, True))) <= TOL, i
        a1.close()


# ---- 3. bag of words at dl = 128 and 192 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nc", [128, 1000, 4096])
@pytest.mark.parametrize("dl", [128, 192])
def test_bow_bit_exact_at_sift_and_colour_surf_lengths(mi, oracle, dl, nc, k):
    rng = np.random.default_rng(nc + dl + k)
    cb = rng.standard_normal((nc, dl))
    rows = near_ties.midpoints(rng, cb, 150)
    if k > 1:  # sixteen of the rows at a near tie of ranks k / k + 1 instead of ranks 1 / 2
        cb, extra = near_ties.tie_at_rank(rng, cb, cb[rng.integers(0, nc, 64)] + 0.7 * rng.standard_normal((64, dl)), k, 16)
        assert len(extra) == 16
        rows[40:56] = extra
    sets = [rows[:97], rows[97:], rows[:0]]
    ref = BowTwin(oracle, cb, k).aggregate_batch(sets)
    agg = mi.BowAggregator(cb, k)
    out = agg.aggregate_batch(sets)
    agg.close()
    assert ref.sum() == 150 * (1 if k == 1 else k * dl)
    assert np.array_equal(out, ref), int((out != ref).sum())


# ---- 4. PCA projection ----------------------------------------------------------------------------------------------------------

def _pca(mi, nc, ss, whiten, mu, eig, Vt):
    """a loaded PCA.  The reference's constructor refuses more components than the sample is long (PCA.java:102-104); the kernel has
    no such limit and the case (300, 33) asks for it, so there the object is made at ss components and its count set before load"""
    pca = mi.PCA(min(nc, ss), 0, ss, whiten)
    pca.numComponents = nc
    pca.load(mu, eig if whiten else None, Vt)
    return pca


def _project_device(mi, nat, pca, X, stream):
    """mmidx_pca_project_device on torch buffers and the given stream"""
    import torch

    dX = torch.tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda")
    dY = torch.full((X.shape[0], pca.numComponents), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    nat.check(mi.lib().mmidx_pca_project_device(pca._h, X.shape[0], dX.data_ptr(), dY.data_ptr(), stream.cuda_stream))
    torch.cuda.synchronize()
    return dY.cpu().numpy()


@pytest.mark.parametrize("nc,ss,n,whiten", fc.PCA_SHAPES)
def test_pca_projection_beyond_one_column_block(mi, nat, oracle, nc, ss, n, whiten):
    import torch

    Vt, mu, eig, X = fc.pca_case(nc, ss, n, whiten)
    pca = _pca(mi, nc, ss, whiten, mu, eig, Vt)
    Y = pca.project(X)
    Vw = oracle.pca_whiten(Vt, eig) if whiten else Vt
    for i in range(n):
        ref = oracle.pca_project(Vw, mu, X[i], whiten)
        scale = max(1.0, float(np.linalg.norm(ref)))
        assert np.max(np.abs(Y[i] - ref)) <= TOL * scale, (i, np.max(np.abs(Y[i] - ref)))
    if whiten:
        assert np.all(Y[1] == 1.0)
    else:
        yhat, bound = fc.pca_exact_and_bound(Vt, mu, X)
        err = np.abs(Y.astype(np.longdouble) - yhat)
        print(f"K7 nc={nc} ss={ss}: max err / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
        assert np.all(err <= bound), float(np.max(err - bound))
    # the device entry point on a stream of the caller's: 1 row, one short of a 64-row block, one over, two blocks and a bit
    st = torch.cuda.Stream()
    for m in (1, 63, 65, 130):
        if m <= n:
            assert np.array_equal(_project_device(mi, nat, pca, X[:m], st), Y[:m]), m
    pca.close()


def test_pca_layout_identity_second_column_block(mi):
    """X = I-like rows against an asymmetric V_t with 160 components: Y = Vt.T exactly.  Columns 128 .. 159 come from the block with
    blockIdx.y = 1: a wrong col0 moves or repeats values, and no tolerance can absorb that."""
    nc, ss = 160, 48
    Vt = np.arange(nc * ss, dtype=np.float64).reshape(nc, ss) / 7.0
    pca = _pca(mi, nc, ss, False, np.zeros(ss), None, Vt)
    X = np.zeros((ss, ss))
    X[np.arange(ss), np.arange(ss)] = 1.0
    Y = pca.project(X)  # Y[i][c] = Vt[c][i]
    assert np.array_equal(Y, Vt.T)
    pca.close()


@pytest.mark.parametrize("m", [1, 63, 65, 130])
def test_pca_project_device_equals_host_form(mi, nat, m):
    """mmidx_pca_project_device, n = 1, 63, 65, 130 on a non-default stream, against mmidx_pca_project bit for bit (whitening on: the
    row normalisation runs on the same stream); 200 components: two column blocks"""
    import torch

    nc, ss, n, whiten = fc.PCA_SHAPES[1]
    Vt, mu, eig, X = fc.pca_case(nc, ss, n, whiten)
    rng = np.random.default_rng(m)
    Xm = np.concatenate([X, rng.standard_normal((130 - n, ss)) / np.sqrt(ss)])[:m]
    pca = _pca(mi, nc, ss, whiten, mu, eig, Vt)
    host = pca.project(Xm)
    assert np.array_equal(_project_device(mi, nat, pca, Xm, torch.cuda.Stream()), host)
    pca.close()


# ---- 5. fused vectorize ---------------------------------------------------------------------------------------------------------

def _vectorize_case(mi, nc, dl, ncomp, seed):
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((nc, dl)) / 4.0
    sets = fc.image_sets(rng, cb, (7, 0, 130, 513, 1, 130))
    ss = nc * dl
    mu = rng.standard_normal(ss) * 0.01
    eig = np.linspace(3.0, 0.4, ncomp)
    Vt = np.linalg.qr(rng.standard_normal((ss, ncomp)))[0].T.copy()
    agg = mi.VladAggregatorMultipleVocabularies([cb], normalizationsOn=True)
    pca = mi.PCA(ncomp, 0, ss, True)
    pca.load(mu, eig, Vt)
    return cb, sets, mu, eig, Vt, agg, pca


@pytest.mark.parametrize("nc,dl,ncomp", [(128, 128, 128), (64, 192, 96)])
def test_fused_vectorize_at_sift_and_colour_surf_lengths(mi, oracle, nc, dl, ncomp):
    cb, sets, mu, eig, Vt, agg, pca = _vectorize_case(mi, nc, dl, ncomp, nc + dl + ncomp)
    two = pca.project(agg.aggregate_batch(sets))
    one = mi.frontend.ImageVectorizer(agg, pca).transform_batch(sets)
    assert one.shape == (len(sets), ncomp) and np.array_equal(one, two)
    Vw = oracle.pca_whiten(Vt, eig)
    for i, s in enumerate(sets):
        ref = oracle.pca_project(Vw, mu, oracle.vlad_aggregate_multi([cb], s, True), True)
        assert np.max(np.abs(one[i] - ref)) <= TOL, (i, float(np.max(np.abs(one[i] - ref))))
    agg.close()
    pca.close()


# ---- 6. device entry points -----------------------------------------------------------------------------------------------------

def _upload(sets, dl, shift=0):
    """(d_off [nimg + 1] int64, d_descs [total][dl], true max_desc) as torch tensors; shift = 1 starts the descriptors one double
    into their allocation: 8-byte aligned, not 16"""
    import torch

    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    flat = np.concatenate([np.ascontiguousarray(s, np.float64).reshape(-1) for s in sets] + [np.zeros(dl)])  # (never empty)
    buf = torch.zeros(flat.size + shift, dtype=torch.float64, device="cuda")
    d_descs = buf[shift:]
    d_descs.copy_(torch.from_numpy(flat))
    assert d_descs.data_ptr() % 16 == 8 * shift
    return torch.from_numpy(off).cuda(), d_descs, max(len(s) for s in sets)


def _aggregate_device(mi, nat, agg, d_off, nimg, d_descs, max_desc, stream, i0=0):
    """mmidx_vlad_aggregate_device on images i0 .. i0 + nimg of d_off (absolute offsets: the pointer moves, nothing is rebased)"""
    import torch

    out = torch.full((nimg, agg.getVectorLength()), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    nat.check(mi.lib().mmidx_vlad_aggregate_device(agg._h, nimg, d_off.data_ptr() + 8 * i0, d_descs.data_ptr(), max_desc, out.data_ptr(),
                                                   stream.cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


FORMS = [(128, 64), (256, 64), (128, 128)]  # K8'' | K8' with k_vlad_accum<64> | K8' with k_vlad_accum<0>
DEV_SIZES = (7, 130, 0, 513, 1, 130, 7)  # offsets 0, 7, 137, 137, 650, 651, 781, 788: image 1 starts at an odd, non-zero offset


@pytest.mark.parametrize("nc,dl", FORMS)
@pytest.mark.parametrize("norms", [False, True])
def test_vlad_aggregate_device_contracts(mi, nat, oracle, nc, dl, norms):
    import torch

    rng = np.random.default_rng(nc + dl)
    cb = rng.standard_normal((nc, dl))
    sets = fc.image_sets(rng, cb, DEV_SIZES)
    nimg = len(sets)
    agg = mi.VladAggregatorMultipleVocabularies([cb], normalizationsOn=norms)
    full = agg.aggregate_batch(sets)
    if not norms:
        for i, s in enumerate(sets):
            assert np.array_equal(full[i], oracle.vlad_aggregate(cb, s)), i
    d_off, d_descs, mx = _upload(sets, dl)
    st = torch.cuda.Stream()
    i0, nb = 1, 3
    assert int(d_off[i0]) % 2 == 1
    # a short call first, then the whole batch, then short again: the assignment workspace grows and is reused
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, 2, d_descs, mx, st), full[:2])
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, nimg, d_descs, mx, st), full)
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, nimg - i0, d_descs, mx, st, i0), full[i0:])
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, nb, d_descs, mx, st, i0), full[i0:i0 + nb])
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, nimg, d_descs, 2 * mx, st), full)  # max_desc overstated
    agg.set_option("two_pass", 1)  # (its own host result: with normalisation the norm's reduction order differs between K8'' and K8')
    full2 = agg.aggregate_batch(sets)
    assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, nb, d_descs, mx, st, i0), full2[i0:i0 + nb])
    assert np.max(np.abs(full2 - full)) <= (TOL if norms else 0.0)
    agg.set_option("two_pass", 0)
    # every image empty, the descriptor pointer valid: zeros raw, ones with normalisation
    e_off = torch.zeros(5, dtype=torch.int64, device="cuda")
    empty = _aggregate_device(mi, nat, agg, e_off, 4, d_descs, 0, st)
    assert np.all(empty == (1.0 if norms else 0.0))
    agg.close()


@pytest.mark.parametrize("nc,dl,ncomp", [(128, 64, 96), (256, 64, 130), (128, 128, 128)])
def test_vectorize_device_equals_host_form(mi, nat, nc, dl, ncomp):
    import torch

    cb, _, mu, eig, Vt, agg, pca = _vectorize_case(mi, nc, dl, ncomp, nc + dl)
    sets = fc.image_sets(np.random.default_rng(ncomp), cb, DEV_SIZES)
    nimg = len(sets)
    host = mi.frontend.ImageVectorizer(agg, pca).transform_batch(sets)
    d_off, d_descs, mx = _upload(sets, dl)
    st = torch.cuda.Stream()

    def run(i0, n):
        out = torch.full((n, ncomp), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        nat.check(mi.lib().mmidx_vectorize_device(agg._h, pca._h, n, d_off.data_ptr() + 8 * i0, d_descs.data_ptr(), mx, out.data_ptr(),
                                                  st.cuda_stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    assert np.array_equal(run(0, nimg), host)
    assert np.array_equal(run(1, nimg - 1), host[1:])
    assert np.array_equal(run(1, 3), host[1:4])
    assert np.array_equal(run(0, nimg), host)
    agg.close()
    pca.close()


# ---- 7. a descriptor base that is 8-byte, not 16-byte aligned -------------------------------------------------------------------

@pytest.mark.parametrize("nc,dl", FORMS)
def test_vlad_aggregate_device_descriptors_at_an_odd_double(mi, nat, oracle, nc, dl):
    """include/mmidx.h: d_descs needs the alignment of a double and no more.  K8'' and the assignment's FROMX form load double2 and are
    gated on a 16-byte base; everything behind the gates (k_split_bf16, k_gather_rows, k_assign_coarse, k_vlad_accum, k_vlad) reads
    single doubles.  (128, 64) therefore runs K8' here, (128, 128) the k_split_bf16 form; the bits are the oracle's."""
    import torch

    rng = np.random.default_rng(nc + dl + 1)
    cb = rng.standard_normal((nc, dl))
    sets = fc.image_sets(rng, cb, DEV_SIZES)
    sets[1][:4] = cb[[5, 9, 5, 60]]  # (exact zeros of distance: flagged rows, gathered and redone in fp64)
    ref = np.stack([oracle.vlad_aggregate(cb, s) for s in sets])
    d_off, d_descs, mx = _upload(sets, dl, shift=1)
    st = torch.cuda.Stream()
    agg = mi.VladAggregator(cb)
    for exact, two in OPTS:
        agg.set_option("exact", exact)
        agg.set_option("two_pass", two)
        assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, len(sets), d_descs, mx, st), ref), (exact, two)
        assert np.array_equal(_aggregate_device(mi, nat, agg, d_off, 3, d_descs, mx, st, 1), ref[1:4]), (exact, two)
    agg.close()
