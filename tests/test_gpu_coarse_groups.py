"""K1e'' (k_coarse_gmin16_grp, option `coarse_groups`): the coarse stage's matrix kernel as two staggered wave groups of a
512-thread block, against the four-wave K1e' on the same handle and against the oracle, through mmidx_coarse_device.

The two kernels publish the same group minima bit for bit, so cells AND exact distances must be np.array_equal with the option on
and off, and the cells must be the oracle's nearest_coarse.  mmidx_get_dispatch names the form that ran.  The `groups` call is made
five times with identical bytes each time.

run_coarse splits the centroid tiles over ceil(CUs / ceil(nq / 256)) blocks, so how many tiles T a block walks depends on nq:

test_coarse_groups_equals_four_wave_kernel_and_oracle -- few queries, every block ONE tile (prologue DMA, one products phase, one
minima phase; no restage, no wait inside the loop).  D = 128 and 100 (both Dp = 128):
  C = 128   the certified coarse stage takes tables of 256 centroids and more (coarse_certified, csrc/mmidx_api.hip), so this
            table is answered by the exact path K1a + K1b with either setting and coarse_mm reads "-": the case pins that gate
            and that the option does not disturb it
  C = 384   three tile ranges;  C = 1000, 2049   padding centroids with infinite norms;  C = 8192  the headline table
  nq = 1, 129   group 1 wholly / partly past nq;  256, 257   a second block with one row;  600   three blocks

test_coarse_groups_tile_loop -- enough queries for the tile loop (on 256 CUs; the test works T out from the device's CU count by
run_coarse's formula and fails if no block would get two tiles):
  C = 8192,  nq = 1300   T = 2: tile 1 issued behind barrier 0, the counted wait of slot 2, the second norm row and store column
  C = 8192,  nq = 2049   T = 3 and a last range of 1: tile 2 refills the buffers of tile 0 (the ring wraps), an odd count,
                         the last query block holds one row (vmcnt(0) instead of vmcnt(8) in its waves)
  C = 16384, nq = 2049   T = 5 and 3: the ring wraps twice; the largest table the certified stage takes
Queries: near centroids, exact copies of centroids, far points; twenty centroids are duplicated (ties)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQS = (1, 129, 256, 257, 600)


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


def _problem(D, C, n=max(NQS)):
    rng = np.random.default_rng(D * 13 + C)
    centers = 4.0 * rng.standard_normal((C // 40 + 2, D))
    coarse = centers[rng.integers(0, len(centers), C)] + 0.7 * rng.standard_normal((C, D))
    coarse[C // 2:C // 2 + 20] = coarse[:20]  # duplicates -> equal distances
    Q = coarse[rng.integers(0, C, n)] + 0.05 * rng.standard_normal((n, D))
    Q[3::7] = coarse[rng.integers(0, C, len(Q[3::7]))]  # exact copies of centroids (some of them duplicated ones)
    Q[1::7][:6] = coarse[:6] + 1e-9
    Q[5::11] = 5.0 * rng.standard_normal((len(Q[5::11]), D))  # far points
    return coarse, Q


@pytest.mark.parametrize("C", [128, 384, 1000, 2049, 8192])
@pytest.mark.parametrize("D", [128, 100])
def test_coarse_groups_equals_four_wave_kernel_and_oracle(mi, oracle, D, C):
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    w = 3 if C == 128 else 8
    certified = C >= 256  # (coarse_certified: smaller tables go through the exact path)
    mm = {0: "dma", 1: "groups"} if certified else {0: "-", 1: "-"}
    coarse, Q = _problem(D, C)
    m = 2
    pq = np.random.default_rng(1).standard_normal((m, 16, D // m))
    ix = mi.IVFPQ(D, 10, False, "", m, 16, 0, C, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ref = oracle.OracleIndex(oracle.KIND_IVFPQ, D, m, 16, C)
    ref.set_coarse(coarse)
    ref.set_pq(pq)
    exp = np.stack([ref.nearest_coarse(q, w) for q in Q])
    dQ = torch.tensor(Q, dtype=torch.float64, device="cuda")

    def run(nq, groups):
        ix.set_option("coarse_groups", groups)
        cells = torch.full((nq, w), -1, dtype=torch.int32, device="cuda")
        cd = torch.full((nq, w), -1.0, dtype=torch.float64, device="cuda")
        nat.check(mi.lib().mmidx_coarse_device(ix._h, nq, dQ.data_ptr(), cells.data_ptr(), cd.data_ptr(), None))
        torch.cuda.synchronize()
        return cells.cpu().numpy(), cd.cpu().numpy(), ix.get_dispatch()

    try:
        for nq in NQS:
            c0, d0, disp0 = run(nq, 0)
            assert disp0["coarse_mm"] == mm[0] and disp0["coarse"].startswith("K1e'+K1f" if certified else "K1a+K1b"), (nq, disp0)
            assert np.array_equal(c0, exp[:nq]), nq
            for rep in range(5):
                c1, d1, disp1 = run(nq, 1)
                assert disp1["coarse_mm"] == mm[1] and disp1["coarse"] == disp0["coarse"], (nq, disp1)
                assert np.array_equal(c1, exp[:nq]), (nq, rep)
                assert np.array_equal(c1, c0) and np.array_equal(d1, d0), (nq, rep)
    finally:
        ix.close()


def _tiles_per_block(C, nq, cus):
    """run_coarse's split of K1e'': (tiles of a full range, tiles of the last range)"""
    ntiles = (C + 127) // 128
    qblocks = (nq + 255) // 256
    split = max(1, min(ntiles, (cus + qblocks - 1) // qblocks), (ntiles + 63) // 64)
    t_per = (ntiles + split - 1) // split
    return t_per, ntiles - (ntiles - 1) // t_per * t_per


@pytest.fixture(scope="module")
def loop_problems():
    """(coarse, Q, the oracle's cells of the rows in `rows`) per table size, computed once"""
    cache = {}

    def get(oracle, C):
        if C not in cache:
            D, w, n = 128, 8, 2049
            coarse, Q = _problem(D, C, n)
            pq = np.random.default_rng(1).standard_normal((2, 16, D // 2))
            ref = oracle.OracleIndex(oracle.KIND_IVFPQ, D, 2, 16, C)
            ref.set_coarse(coarse)
            ref.set_pq(pq)
            # (the oracle walks every centroid in scalar fp64: every row of the 8192 table, every fourth of the 16384 one;
            #  K1e' answers every row of both)
            rows = np.arange(n) if C <= 8192 else np.arange(0, n, 4)
            cache[C] = (coarse, pq, Q, rows, np.stack([ref.nearest_coarse(Q[i], w) for i in rows]))
        return cache[C]

    return get


@pytest.mark.parametrize("C,nq", [(8192, 1300), (8192, 2049), (16384, 2049)])
def test_coarse_groups_tile_loop(mi, oracle, loop_problems, C, nq):
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    D, w = 128, 8
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t_full, t_last = _tiles_per_block(C, nq, cus)
    print(f"C {C} nq {nq}: {cus} CUs, {t_full} tiles a block, {t_last} in the last range")
    assert t_full >= 2, "this device gives every block one tile: the loop is not reached"
    coarse, pq, Q, rows, exp = loop_problems(oracle, C)
    ix = mi.IVFPQ(D, 10, False, "", 2, 16, 0, C, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    dQ = torch.tensor(Q[:nq], dtype=torch.float64, device="cuda")

    def run(groups):
        ix.set_option("coarse_groups", groups)
        cells = torch.full((nq, w), -1, dtype=torch.int32, device="cuda")
        cd = torch.full((nq, w), -1.0, dtype=torch.float64, device="cuda")
        nat.check(mi.lib().mmidx_coarse_device(ix._h, nq, dQ.data_ptr(), cells.data_ptr(), cd.data_ptr(), None))
        torch.cuda.synchronize()
        return cells.cpu().numpy(), cd.cpu().numpy(), ix.get_dispatch()

    try:
        sel = rows[rows < nq]
        c0, d0, disp0 = run(0)
        assert disp0["coarse_mm"] == "dma" and disp0["coarse"].startswith("K1e'+K1f"), disp0
        assert np.array_equal(c0[sel], exp[:len(sel)])
        for rep in range(5):
            c1, d1, disp1 = run(1)
            assert disp1["coarse_mm"] == "groups" and disp1["coarse"] == disp0["coarse"], disp1
            assert np.array_equal(c1[sel], exp[:len(sel)]), rep
            assert np.array_equal(c1, c0) and np.array_equal(d1, d0), rep
    finally:
        ix.close()
