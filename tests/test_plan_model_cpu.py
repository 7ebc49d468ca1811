"""tests/plan_model.py, the host mirror of make_plan's sub-batch size for IVFPQ, pinned to figures worked out from the source, and
held to the source where the source can be read without a GPU (the constants)."""
import os
import re

import plan_model as pm
import sdc_cases as sc

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    return open(os.path.join(ROOT, "multimedia-indexing_amd", "csrc", name), errors="replace").read()


def test_constants_are_the_sources():
    k = _src("mmidx_kernels.h")

    def define(name):
        return int(re.search(r"^#define " + name + r" (\d+)", k, flags=re.M).group(1))

    assert (define("MMIDX_BLOCK"), define("MMIDX_CSEL_CAP"), define("MMIDX_CAND_CHUNK"), define("MMIDX_TERM_PAD"), define("MMIDX_HKEEP")) == \
        (pm.BLOCK, pm.CSEL_CAP, pm.CAND_CHUNK, pm.TERM_PAD, sc.HKEEP)
    api = _src("mmidx_api.hip")
    plan = api[api.index("int make_plan("):]
    plan = plan[:plan.index("\n}\n")]
    assert re.search(r"int64_t\s+chunk\s*=\s*%d\s*;" % pm.IVF_CHUNK, plan)
    # (what the option does to qb is held by the GPU tests of tests/test_gpu_sub_batches.py, which read the number of sub-batches
    #  and the dispatch from the library: no text of that line is pinned here)


def test_exact_coarse_stage_caps_at_2_gib():
    """C = 16390 cells is beyond the certified stage (64 x 256 = 16384): every row of the [nq][C] matrix is written, 2 GiB of it"""
    D, C, w, n, k = 16, 16390, 9, 20000, 10
    assert not pm.coarse_certified(D, C, w) and pm.coarse_certified(D, 16384, w)
    p = pm.ivf_plan(D, 2, 256, C, w, n, 8, k, 100000)
    assert p["qb"] == 2 ** 31 // (16390 * 8) == 16378 and not p["asks_free"] and not p["glut"]
    assert pm.sub_batches(16378 + 40, p["qb"]) == [(0, 16378), (16378, 40)]
    # handed the probe cells (mmidx_search_partial_device, the shard phases) the call has no coarse matrix: the pool alone caps it
    assert pm.ivf_plan(D, 2, 256, C, w, n, 8, k, 100000, need_coarse=False)["qb"] == 100000
    # the option "exact_coarse" puts a certifiable shape under the same cap
    assert pm.ivf_plan(128, 16, 256, 8192, 32, 10 ** 8, 20000, 100, 10 ** 6, exact_coarse=1)["qb"] == 2 ** 31 // (8192 * 8) == 32768


def test_table_slots_cap_at_2_gib():
    """m = 32, ks = 1024: 256 KiB of table per (query, probe) in global scratch; w = 6 probes of one chunk each"""
    D, C, m, ks, w, n, k = 64, 6, 32, 1024, 6, 4000, 10
    p = pm.ivf_plan(D, m, ks, C, w, n, 1000, k, 5000)
    assert p["glut"] and p["nitems"] == 6 and p["qb"] == 2 ** 31 // (2 ** 18 * 6) == 1365
    assert pm.sub_batches(1368, p["qb"]) == [(0, 1365), (1365, 3)]
    assert pm.ivf_plan(D, m, ks, C, 4, n, 1000, k, 5000)["qb"] == 2048
    # lists of two chunks double the slots
    assert pm.ivf_plan(D, m, ks, C, w, 40000, 16385, k, 5000)["qb"] == 682
    # the flat side (sdc_cases.plan): 128 x 256 with four chunks, the SDC case's shape
    assert sc.plan(128, 128, 256, 0, sc.N4, 10, 5000, sc.MIN_FLAT_CHUNK)["qb"] == 2048


def test_headline_shape_caps_at_16_gib_or_a_quarter_of_free_memory():
    D, m, ks, C, w, n, L, k = 128, 16, 256, 8192, 32, 10 ** 8, 15000, 100  # (12207 codes per list on average: one chunk)
    assert pm.coarse_certified(D, C, w)
    p = pm.ivf_plan(D, m, ks, C, w, n, L, k, 10 ** 6)
    assert p["certified"] and p["asks_free"] and p["qb"] == 16 * GIB // (8192 * 8) == 262144
    # the free figure is asked for from a matrix of 2 GiB on: 32768 queries do not ask, 32769 do
    assert not pm.ivf_plan(D, m, ks, C, w, n, L, k, 32768, free_bytes=GIB)["asks_free"]
    assert pm.ivf_plan(D, m, ks, C, w, n, L, k, 32768, free_bytes=GIB)["qb"] == 32768
    assert pm.ivf_plan(D, m, ks, C, w, n, L, k, 32769, free_bytes=GIB)["asks_free"]
    # a quarter of what is free, 2 GiB at least, 16 GiB at most
    for free, want in ((256 * GIB, 262144), (64 * GIB, 262144), (40 * GIB, 10 * GIB // 65536), (8 * GIB + 4096, 32768), (GIB, 32768), (0, 32768)):
        assert pm.ivf_plan(D, m, ks, C, w, n, L, k, 10 ** 6, free_bytes=free)["qb"] == want, free
    assert 10 * GIB // 65536 == 163840
    # the pool: w x chunks x (k + 1) + 256 entries of 16 bytes per query -- above the coarse cap with one chunk per list, below it
    # with two (a list beyond 16384 codes)
    assert p["poolq"] == 32 * 101 + 256 and 16 * GIB // (p["poolq"] * 16) == 307838
    assert pm.ivf_plan(D, m, ks, C, w, n, 20000, k, 10 ** 6)["qb"] == 16 * GIB // ((64 * 101 + 256) * 16) == 159783
    assert pm.ivf_plan(D, m, ks, C, 1024, n, 20000, 4095, 10 ** 6)["qb"] == 16 * GIB // ((2048 * 4096 + 256) * 16) == 127


def test_option_only_lowers():
    D, m, ks, C, w, n, L, k = 128, 16, 256, 6, 3, 22500, 4500, 100
    assert pm.ivf_plan(D, m, ks, C, w, n, L, k, 40)["qb"] == 40
    for sb, parts in ((17, [17, 17, 6]), (8, [8] * 5), (1, [1] * 40), (39, [39, 1]), (40, [40]), (41, [40])):
        p = pm.ivf_plan(D, m, ks, C, w, n, L, k, 40, sub_batch=sb)
        assert [nb for _, nb in pm.sub_batches(40, p["qb"])] == parts
    assert pm.ivf_plan(64, 32, 1024, 6, 6, 4000, 1000, 10, 5000, sub_batch=2000)["qb"] == 1365
    assert sc.plan(128, 8, 256, 0, 70000, 100, 100, 8192, sub_batch=37)["qb"] == 37
