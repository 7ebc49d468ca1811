"""The index build, record for record: assignment (K6a' from rows / from copies, K6a, exact), product quantisation (K6b' / K6b), the
CSR placement (k_move_old / k_place_new), the pending buffers across a reallocation, the device entry points and the 2^18-row chunk
edge of the host ones -- the path bench.py times as "index build".  Fixtures and expected values: tests/build_cases.py (the oracle;
a numpy twin above 2^18 rows); tests/test_build_cases_cpu.py shows on the CPU that the tie rule decides them and derives the window
`flagged` is held to.  Every comparison here is ==; which kernel ran comes from mmidx_get_dispatch (assign= / encode= / flagged=)."""
import importlib

import numpy as np
import pytest

import build_cases as bc

pytestmark = pytest.mark.gpu


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


def _index(mi, c, options=()):
    return bc.make_index(mi, c["kind"], c["D"], c["m"], c["ks"], c["C"], c["transform"], c["coarse"], c["pq"], c["rot"], options)


def _same_export(got, want, what):
    for g, w, part in zip(got, want, ("offsets", "ids", "codes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert len(bad) == 0, (what, part, len(bad), bad[:8])


# ---- 1. the encoder table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r[0] for r in bc.ENCODER])
def test_encoder_table(mi, name):
    """encode() equals the oracle in cells and codes for every vector, at 521 rows (a partial last block for both kernels) and at
    one; the reported kernels are the table's"""
    c = bc.encoder_case(name)
    ix = _index(mi, c)
    assert ix.get_dispatch()["assign"] == "-" and ix.get_dispatch()["encode"] == "-" and ix.get_dispatch()["flagged"] == "-"
    want_assign = bc.assign_gate(c["kind"], c["D"], c["C"])
    for n in (bc.ENC_N, 1):
        cells, codes = ix.encode(c["X"][:n])
        d = ix.get_dispatch()
        print(f"{name} n={n}: assign={d['assign']} encode={d['encode']} flagged={d['flagged']}")
        assert np.array_equal(cells, c["cells"][:n]), np.flatnonzero(cells != c["cells"][:n])[:8]
        want = bc.stored(c["codes"][:n], c["ks"])
        assert codes.dtype == want.dtype
        assert np.array_equal(codes, want), np.argwhere(codes != want)[:8]
        assert d["encode"] == c["expect"]
        assert d["assign"] == want_assign
        assert (d["flagged"] == "-") == (want_assign == "-")
    ix.close()


# ---- 2. the assignment table ----------------------------------------------------------------------------------------------------
def _assign_device(mi, nat, ix, X, shift):
    """mmidx_assign_device on a device buffer that starts `shift` doubles into its allocation (1: 8-byte aligned, not 16)"""
    import torch

    buf = torch.zeros(X.size + shift, dtype=torch.float64, device="cuda")
    dX = buf[shift:]
    dX.copy_(torch.from_numpy(np.ascontiguousarray(X).reshape(-1)))
    assert dX.data_ptr() % 16 == 8 * shift
    cells = torch.full((X.shape[0],), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nat.check(mi.lib().mmidx_assign_device(ix._h, X.shape[0], dX.data_ptr(), cells.data_ptr(), None))
    torch.cuda.synchronize()
    return cells.cpu().numpy()


@pytest.mark.parametrize("name", [r[0] for r in bc.ASSIGN])
def test_assignment_table(mi, nat, name):
    """cells equal the oracle's for every vector at 1, 127, 128, 129 rows and the full set; the reported kernel is the table's; at the
    full set the number of vectors sent to the exact redo lies in the window derived from the certificate (every exact tie must be
    flagged, nothing with a gap above 4.04 eps may be); the exact rows report no count.
    Measured on an MI355X, flagged [window] of 3853 rows: d128 297 [240, 351], d24_one_step 164 [84, 238], d64_pad127 829 [769, 858],
    d100 556 [498, 598], d130_two_chunks 828 [748, 852], d260_three_chunks 753 [661, 813], d128_misaligned 297 [240, 351] (the same
    count from copies as from rows), d32_v1 712 [686, 712]."""
    c = bc.assign_case(name)
    ix = bc.make_index(mi, bc.KIND_IVFPQ, c["D"], 2, 16, c["C"], bc.TR_NONE, c["coarse"], c["pq"], None, c["options"])
    for n in bc.ASSIGN_SIZES:
        X = c["X"] if n is None else c["X"][:n]
        if c["misaligned"]:
            cells = _assign_device(mi, nat, ix, X, 1)
        else:
            cells, _ = ix.encode(X)
        d = ix.get_dispatch()
        bad = np.flatnonzero(cells != c["cells"][:len(X)])
        assert len(bad) == 0, (n, len(bad), bad[:8])
        assert d["assign"] == c["expect"], n
        if c["expect"] in bc.CERTIFIED:
            flagged = int(d["flagged"])
            assert 0 <= flagged <= len(X)
            if n is None:
                print(f"{name}: D={c['D']} C={c['C']} n={len(X)} assign={d['assign']} flagged={flagged} window=[{c['lo']}, {c['hi']}]")
                assert c["lo"] <= flagged <= c["hi"]
        else:
            assert d["flagged"] == "-"
    if c["misaligned"]:  # the same rows on a 16-byte boundary take the other feed, and give the same cells
        cells = _assign_device(mi, nat, ix, c["X"], 0)
        assert ix.get_dispatch()["assign"] == "K6a'(rows)"
        assert np.array_equal(cells, c["cells"])
        assert c["lo"] <= int(ix.get_dispatch()["flagged"]) <= c["hi"]
    ix.close()


# ---- 3. placement ---------------------------------------------------------------------------------------------------------------
PLACE_CALLS = (1, 700, 1000)
PLACE_N = sum(PLACE_CALLS)


def _caller_ids(n):
    """neither ascending nor contiguous"""
    return (np.random.default_rng(n).permutation(n) * 3 + 5).astype(np.int32)


@pytest.mark.parametrize("caller_ids", [False, True], ids=["own_ids", "caller_ids"])
@pytest.mark.parametrize("ks", [256, 300])
def test_placement_after_every_add(mi, ks, caller_ids):
    """three adds of 1, 700 and 1000 rows with a search between them: after each, export() -- offsets, ids, stored codes -- is the
    stable sort of the oracle's records by cell (k_place_new for the new records, k_move_old for the ones already placed)"""
    c = bc.placement_case(ks, PLACE_N)
    ids = _caller_ids(PLACE_N) if caller_ids else np.arange(PLACE_N, dtype=np.int32)
    ix = _index(mi, c)
    ix.setW(4)
    done = 0
    for nb in PLACE_CALLS:
        if caller_ids:
            ix._add_vectors(c["X"][done:done + nb], ids[done:done + nb])
        else:
            assert ix.indexVectors([str(i) for i in range(done, done + nb)], c["X"][done:done + nb]) == nb
        done += nb
        got = ix.export()
        _same_export(got, bc.expected_export(c["cells"][:done], c["codes"][:done], ids[:done], c["C"], ks), (ks, done))
        assert (np.diff(got[0]) == 0).sum() >= 100  # many lists stay empty
        ix.search_batch(3, c["X"][:2])
    assert ix.get_dispatch()["encode"] == "K6b'"
    ix.close()


def test_pending_buffers_grow_with_records_pending(mi):
    """1000, 30, 1100 and 2200 rows with nothing between the adds that folds them into the lists: the pending buffers start at 1024
    rows and are reallocated twice with records in them (1030 -> 2130 -> 4330); one export at the end"""
    calls = (1000, 30, 1100, 2200)
    n = sum(calls)
    c = bc.placement_case(256, n)
    ix = _index(mi, c)
    done = 0
    for nb in calls:
        assert ix.indexVectors([str(i) for i in range(done, done + nb)], c["X"][done:done + nb]) == nb
        done += nb
    assert ix.size() == n
    _same_export(ix.export(), bc.expected_export(c["cells"], c["codes"], np.arange(n), c["C"], 256), "pending growth")
    ix.close()


# ---- 4. the device entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [256, 300])
def test_device_entry_points(mi, nat, ks):
    """(a) mmidx_add_vectors_device with device ids on a non-default stream, three calls, then mmidx_sync_index; (b)
    mmidx_encode_device then mmidx_add_codes_device, as bench.py builds a sharded index.  Both exports are byte-identical to the host
    route's (and to the oracle's records); calls with n = 0 return OK and change nothing."""
    import torch

    L = mi.lib()
    c = bc.placement_case(ks, PLACE_N)
    ids = _caller_ids(PLACE_N)
    want = bc.expected_export(c["cells"], c["codes"], ids, c["C"], ks)
    host = _index(mi, c)
    done = 0
    for nb in PLACE_CALLS:
        host._add_vectors(c["X"][done:done + nb], ids[done:done + nb])
        done += nb
    host_export = host.export()
    _same_export(host_export, want, "host route")
    host.close()

    s = torch.cuda.Stream()
    code_dtype = torch.int8 if ks <= 256 else torch.int16
    for route in ("add_vectors_device", "encode_device+add_codes_device"):
        ix = _index(mi, c)
        with torch.cuda.stream(s):  # the uploads are work of the caller's stream: the calls must order themselves behind it
            dX = torch.from_numpy(c["X"]).to("cuda", non_blocking=True)
            d_ids = torch.from_numpy(ids).to("cuda", non_blocking=True)
            # n = 0: OK, nothing changes (no pointer is looked at)
            before = ix.get_dispatch()
            assert L.mmidx_add_vectors_device(ix._h, 0, None, None, 0, s.cuda_stream) == 0
            assert L.mmidx_encode_device(ix._h, 0, None, None, None, s.cuda_stream) == 0
            assert L.mmidx_add_codes_device(ix._h, 0, None, None, None, s.cuda_stream) == 0
            assert L.mmidx_assign_device(ix._h, 0, None, None, s.cuda_stream) == 0
            assert ix.size() == 0 and ix.get_dispatch() == before
            done = 0
            for nb in PLACE_CALLS:
                x, i = dX[done:done + nb], d_ids[done:done + nb]
                if route == "add_vectors_device":
                    nat.check(L.mmidx_add_vectors_device(ix._h, nb, x.data_ptr(), i.data_ptr(), -1, s.cuda_stream))
                else:
                    cells = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
                    codes = torch.zeros((nb, c["m"]), dtype=code_dtype, device="cuda")
                    nat.check(L.mmidx_encode_device(ix._h, nb, x.data_ptr(), cells.data_ptr(), codes.data_ptr(), s.cuda_stream))
                    s.synchronize()
                    assert np.array_equal(cells.cpu().numpy(), c["cells"][done:done + nb])
                    assert np.array_equal(codes.cpu().numpy(), bc.stored(c["codes"][done:done + nb], ks))
                    nat.check(L.mmidx_add_codes_device(ix._h, nb, i.data_ptr(), cells.data_ptr(), codes.data_ptr(), s.cuda_stream))
                done += nb
                assert ix.size() == done
            assert L.mmidx_add_vectors_device(ix._h, 0, None, None, 0, s.cuda_stream) == 0
            assert L.mmidx_add_codes_device(ix._h, 0, None, None, None, s.cuda_stream) == 0
            assert ix.size() == PLACE_N
            nat.check(L.mmidx_sync_index(ix._h))
            nat.check(L.mmidx_sync_index(ix._h))  # (nothing pending: a no-op)
        s.synchronize()
        got = ix.export()
        _same_export(got, want, route)
        for g, h in zip(got, host_export):
            assert g.tobytes() == h.tobytes(), route
        d = ix.get_dispatch()
        assert d["assign"] == "K6a'(rows)" and d["encode"] == "K6b'" and int(d["flagged"]) >= 0
        ix.close()


# ---- 5. the chunk edge of the host entry points -----------------------------------------------------------------------------------
def test_chunk_edge_of_the_host_entry_points(mi):
    """2^18 + 3 rows: mmidx_encode and mmidx_add_vectors walk their input in chunks of 2^18, the second chunk holds three rows.  Cells,
    codes and the export equal the numpy twin's for every row, and `flagged` is the sum over both chunks."""
    c = bc.chunk_edge_case()
    n, B = len(c["X"]), 1 << 18
    ix = _index(mi, c)
    cells, codes = ix.encode(c["X"])
    whole = ix.get_dispatch()
    assert np.array_equal(cells, c["cells"]), np.flatnonzero(cells != c["cells"])[:8]
    assert np.array_equal(codes, bc.stored(c["codes"], c["ks"]))
    assert whole["assign"] == "K6a'(rows)" and whole["encode"] == "K6b'"
    parts = []
    for sl in (slice(0, B), slice(B, n)):
        pc, pk = ix.encode(c["X"][sl])
        assert np.array_equal(pc, c["cells"][sl]) and np.array_equal(pk, bc.stored(c["codes"][sl], c["ks"]))
        parts.append(int(ix.get_dispatch()["flagged"]))
    print(f"chunk edge: flagged {whole['flagged']} = {parts[0]} + {parts[1]}")
    assert int(whole["flagged"]) == sum(parts)
    assert ix.indexVectors([str(i) for i in range(n)], c["X"]) == n
    assert int(ix.get_dispatch()["flagged"]) == sum(parts)
    _same_export(ix.export(), bc.expected_export(c["cells"], c["codes"], np.arange(n), c["C"], c["ks"]), "chunk edge")
    ix.close()
