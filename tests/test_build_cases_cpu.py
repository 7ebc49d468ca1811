"""The build fixtures (tests/build_cases.py) have teeth, shown on the CPU: the tie rule decides codes and cells in them, the Python
mirrors of the two gates give the kernel names the tables expect, and the window the GPU test holds `flagged` to is derived from the
certificate, not measured."""
import numpy as np
import pytest

import build_cases as bc

ENC = [r[0] for r in bc.ENCODER]
ASG = [r[0] for r in bc.ASSIGN]


@pytest.mark.parametrize("name", ENC)
def test_encoder_fixture_ties(name):
    """the oracle's codes take the lower index of a duplicated pair at least 20 times (on the rows built for it: at least 60 of them),
    an encoder in which the last index wins disagrees on exactly those, and the first-wins twin is the oracle"""
    c = bc.encoder_case(name)
    coarse = c["coarse"]
    cells, codes = bc.twin_encode(c["X"], coarse, c["pq"], c["transform"], c["perm"], c["rot"])
    assert np.array_equal(cells, c["cells"]) and np.array_equal(codes, c["codes"])
    rows = np.arange(bc.TIE_ROWS)
    on_low = c["codes"][rows, c["tie_sub"]] == c["tie_low"]
    print(name, "rows built on a duplicated codebook row that encode to its lower index:", int(on_low.sum()), "of", bc.TIE_ROWS)
    assert on_low.sum() >= 60
    for s in range(c["m"]):  # the duplicated rows really are duplicates
        for j1, j2 in bc.dup_pairs(c["ks"], s):
            assert j1 < j2 and np.array_equal(c["pq"][s, j1], c["pq"][s, j2])
    lows = {(s, j1) for s in range(c["m"]) for j1, _ in bc.dup_pairs(c["ks"], s)}
    hits = sum(int((c["codes"][:, s] == j).sum()) for s, j in lows)
    assert hits >= 20
    _, wrong = bc.twin_encode(c["X"], coarse, c["pq"], c["transform"], c["perm"], c["rot"], last_wins=True)
    assert np.array_equal(wrong[rows[on_low], c["tie_sub"][on_low]], c["tie_high"][on_low])
    assert int((wrong != c["codes"]).any(1).sum()) >= 60
    # every other disagreement of the wrong encoder is a duplicated row too: the fixture holds no accidental ties
    d = np.argwhere(wrong != c["codes"])
    assert all((int(s), int(c["codes"][i, s])) in lows for i, s in d)


@pytest.mark.parametrize("name", [n for n in ASG if n != "d32_one_cell"])
def test_assignment_fixture_ties(name):
    """the same for the duplicated centroids: at least 20 rows take the lower index of a pair; last-index-wins moves them"""
    c = bc.assign_case(name)
    assert np.array_equal(c["coarse"][c["dup_low"]], c["coarse"][c["dup_high"]])
    assert np.array_equal(c["twin_first"], c["cells"])
    on_low = np.isin(c["cells"], c["dup_low"])
    print(name, "rows whose cell is the lower index of a duplicated centroid:", int(on_low.sum()))
    assert on_low.sum() >= 20
    assert np.array_equal(c["cells"][:25], np.arange(10, 35))
    wrong = c["twin_last"]
    assert np.all(wrong[on_low] == c["cells"][on_low] - 10 + c["C"] // 2)


def test_one_cell_fixture():
    c = bc.assign_case("d32_one_cell")
    assert c["C"] == 1 and not c["cells"].any() and c["lo"] is None


def test_gates_give_the_tables():
    for name, kind, D, m, ks, tr, expect in bc.ENCODER:
        assert bc.encode_gate(D, m, ks, tr) == expect, name
        assert D % m == 0
    for name, D, C, options, misaligned, expect in bc.ASSIGN:
        assert bc.assign_gate(bc.KIND_IVFPQ, D, C, options, aligned=not misaligned) == expect, name
    assert bc.assign_gate(bc.KIND_PQ, 32, 0) == "-"
    # the switch the two 16-dimension short-code rows straddle, to the byte
    assert 500 * 16 * 8 + 256 * 2 * 2 == 65024 and 512 * 16 * 8 + 256 * 2 * 2 == 66560
    assert bc.encode_gate(32, 2, 504, bc.TR_NONE) == "K6b'" and bc.encode_gate(32, 2, 505, bc.TR_NONE) == "K6b"
    # every branch of either gate is some row's
    assert {r[-1] for r in bc.ENCODER} == {"K6b'", "K6b"}
    assert {r[-1] for r in bc.ASSIGN} == {"K6a'(rows)", "K6a'(copies)", "K6a", "exact"}


@pytest.mark.parametrize("name", [r[0] for r in bc.ASSIGN if r[-1] in bc.CERTIFIED])
def test_flagged_window(name):
    """lo: rows with an exact fp64 tie (must be flagged); hi: rows with gap <= 4.04 eps (all that may be).  A window that pins
    something: at least 20 rows must be flagged, and no more than a quarter of the input can be."""
    c = bc.assign_case(name)
    n = len(c["X"])
    print(f"{name}: D={c['D']} C={c['C']} n={n} {c['expect']}: flagged must lie in [{c['lo']}, {c['hi']}]")
    assert c["lo"] >= 20
    assert c["hi"] <= n / 4
    assert c["lo"] <= c["hi"]


def test_expected_export_is_the_stable_sort():
    cells = np.array([2, 0, 2, 1, 0, 2])
    codes = np.arange(12).reshape(6, 2)
    off, ids, st = bc.expected_export(cells, codes, np.array([50, 40, 30, 20, 10, 0]), 4, 256)
    assert off.tolist() == [0, 2, 3, 6, 6]
    assert ids.tolist() == [40, 10, 20, 50, 30, 0]
    assert st.dtype == np.int8 and st[:, 0].tolist() == [2 - 128, 8 - 128, 6 - 128, 0 - 128, 4 - 128, 10 - 128]
    off, ids, st = bc.expected_export(None, codes, np.arange(6), 1, 300)
    assert off.tolist() == [0, 6] and ids.tolist() == list(range(6)) and st.dtype == np.int16 and np.array_equal(st, codes)


def test_chunk_edge_twin_is_the_oracle():
    c = bc.chunk_edge_case()  # (asserts its head and tail against the oracle)
    assert len(c["X"]) == (1 << 18) + 3
