"""GPU parity of a handle driven through every kernel switch of pass A, in every order, across an add.

The pass-A kernels share workspace with pass B (ws_pcount, ws_pstart, ws_gdesc, ws_gfb) and some of them rely on what the launch
before left there: K3q's k_q_scan_groups leaves the per-cell counters zeroed so that pass B skips its memset (SearchStep::pcount_zeroed:
set by stage_init, read by stage_pair_sort), K3ma does not (stage_pass_a withdraws it), k_pair_scan leaves at once on a zero total.  One handle of a long-list IVFPQ index (m = 16 x 256,
D = 128, six cells: five of >= 4096 codes and one that starts empty) serves a walk over eight dispatch states -- reached by options, k,
setW and the batch size -- in which every ordered pair of states follows each other at least once (an Eulerian circuit of the complete
directed graph with loops).  Which state a call was in is read back from mmidx_get_dispatch and the statistics, not assumed, and the
coverage is asserted on what was read.  Midway the empty cell is filled, which moves K3q's gate (4 nq >= 5 non-empty lists), and the
gate is checked on both sides of it.  Every call returns the oracle's ids and distance bits.  The walk runs through the host entry,
the device entry (mmidx_search_device on torch tensors) and a handle of two virtual shards on one device.
"""
import importlib

import numpy as np
import pytest

import synth
from test_gpu_parity import assert_same, mi, oracle_ivfpq  # noqa: F401  (mi: the module fixture; torch initialises first)

pytestmark = pytest.mark.gpu

D, M, KS, NC, W = 128, 16, 256, 6, 3
PER = 4500  # codes per cell (the sixth cell gets as many by the add: >= 4096 per non-empty list on average before and after)

# state -> options (unset ones at their defaults), k, w, which query set and how many of it.  (q_forced: 2 queries -- below the gate
# on the whole index and on a shard of three lists; k3ma: 64 >= 8 C queries, K3ma's own gate, but forced anyway)
STATES = {
    "q_gate": ({}, 100, W, "mid", 40),
    "q_forced": ({"passa_q": 1}, 100, W, "mid", 2),
    "k3h": ({"passa_q": 0}, 100, W, "mid", 40),
    "k3ma": ({"passa_mfma": 1}, 100, W, "mid", 64),
    "k3": ({"passa_q": 0, "passa_hist": 0}, 100, W, "mid", 40),
    "w1": ({}, 100, 1, "mid", 40),
    "empty_b": ({}, 10, W, "self", 40),
    "one": ({}, 100, W, "mid", 1),
}
NAMES = list(STATES)
DEFAULTS = {"passa_q": -1, "passa_mfma": -1, "passa_hist": -1}


def euler_walk(n):
    """a closed walk over the complete directed graph on n nodes with a loop at every node that uses each of its n^2 edges once
    (Hierholzer)"""
    out = {u: list(range(n)) for u in range(n)}
    stack, path = [0], []
    while stack:
        u = stack[-1]
        if out[u]:
            stack.append(out[u].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def classify(d, st, nq, nonempty):
    """the state a call was in, from what the library reports"""
    pa = d["pass_a"]
    if pa == "K3(single pass)":
        return "w1"
    if st["passb_items_last"] == 0:
        return "empty_b"
    if nq == 1:
        return "one"
    if pa == "K3q":
        return "q_gate" if 4 * nq >= 5 * nonempty else "q_forced"
    return {"K3h": "k3h", "K3ma": "k3ma", "K3": "k3"}.get(pa, pa)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2024)
    mu = 4.0 * rng.standard_normal((NC, D))  # (centroids ~64 apart, residuals ~11: a self-query's other probes fall to the bound)
    lab = np.repeat(np.arange(NC), PER)
    X = mu[lab] + rng.standard_normal((len(lab), D))
    ds = D // M
    tr = rng.choice(len(X), 3000, replace=False)
    pq = np.stack([synth.kmeans((X[tr] - mu[lab[tr]])[:, s * ds:(s + 1) * ds], KS, iters=2, seed=s) for s in range(M)])
    late = X[lab == NC - 1]  # the sixth cell's vectors arrive midway
    keep = rng.permutation(np.nonzero(lab < NC - 1)[0])
    base, blab = X[keep], lab[keep]
    # midpoints between vectors of two different cells (every query keeps pairs for pass B); two of the first 40 and the last eight
    # lie next to the sixth cell, whose list is empty before the add (queries whose nearest list is empty)
    a = rng.integers(0, len(base), 64)
    b = np.array([rng.choice(np.nonzero(blab != blab[i])[0]) for i in a])
    mid = 0.5 * (base[a] + base[b])
    j5 = [20, 21] + list(range(56, 64))
    mid[j5] = 0.65 * late[rng.integers(0, PER, len(j5))] + 0.35 * base[b[j5]]
    selfq = base[rng.integers(0, len(base), 40)] + 0.01 * rng.standard_normal((40, D))
    return dict(mu=mu, pq=pq, base=base, late=late, Q={"mid": mid, "self": selfq})


def _search(entry, ix, k, Q):
    if entry != "device":
        return ix.search_batch(k, Q)
    import torch

    nat = importlib.import_module("multimedia-indexing_amd._native")
    L = importlib.import_module("multimedia-indexing_amd").lib()
    dev = torch.device("cuda", 0)
    B = Q.shape[0]
    dQ = torch.tensor(Q, dtype=torch.float64, device=dev)
    iid = torch.empty(B, k, dtype=torch.int32, device=dev)
    dd = torch.empty(B, k, dtype=torch.float64, device=dev)
    cc = torch.empty(B, dtype=torch.int32, device=dev)
    nat.check(L.mmidx_search_device(ix._h, k, B, dQ.data_ptr(), iid.data_ptr(), dd.data_ptr(), cc.data_ptr(), None))
    torch.cuda.synchronize()
    return iid.cpu().numpy(), dd.cpu().numpy(), cc.cpu().numpy()


@pytest.mark.parametrize("entry", ["host", "device", "sharded"])
def test_kernel_switch_sequence(mi, oracle, data, entry):
    """The walk (65 calls + the gate checks) on one handle; see the module docstring.  The sharded handle reports its first shard's
    dispatch (cells 0, 2, 4: three non-empty lists on either side of the add), so its gate is classified against three lists and the
    boundary checks -- which count the whole index's non-empty lists -- run on the single-device handles only."""
    sharded = entry == "sharded"
    n0 = len(data["base"])
    ix = mi.IVFPQ(D, n0 + PER, False, "", M, KS, 0, NC, 512, devices=[0, 0] if sharded else None)
    ix.loadCoarseQuantizer(data["mu"])
    ix.loadProductQuantizer(data["pq"])
    ix.setW(W)
    ix.indexVectors([str(i) for i in range(n0)], data["base"])
    ref = oracle_ivfpq(oracle, {"coarse": data["mu"], "pq": data["pq"]}, D, M, KS, NC, W)
    ref.add_vectors(data["base"])
    expect = {}
    epoch = [0]

    def want(qset, nq, k, w):
        key = (epoch[0], qset, nq, k, w)
        if key not in expect:
            ref.set_w(w)
            expect[key] = ref.search_batch(data["Q"][qset][:nq], k)
        return expect[key]

    def call(opts, k, w, qset, nq):
        for o, v in dict(DEFAULTS, **opts).items():
            ix.set_option(o, v)
        ix.setW(w)
        ix.set_profiling(True)
        got = _search(entry, ix, k, data["Q"][qset][:nq])
        st = ix.get_stats()
        d = ix.get_dispatch()
        assert_same(got, want(qset, nq, k, w))
        return d, st

    seen = []

    def state(name):
        opts, k, w, qset, nq = STATES[name]
        d, st = call(opts, k, w, qset, nq)
        got = classify(d, st, nq, 3 if sharded else (5 if epoch[0] == 0 else 6))
        assert got == name, (name, got, d, st["passb_items_last"], len(seen))
        seen.append(got)

    def gate(nq, name):
        d, _ = call({}, 100, W, "mid", nq)
        assert d["pass_a"] == name, (epoch[0], nq, d)

    walk = [NAMES[i] for i in euler_walk(len(NAMES))]
    half = len(walk) // 2
    for s in walk[:half]:
        state(s)
    if not sharded:  # five non-empty lists: 4 x 7 >= 25 > 4 x 6
        gate(7, "K3q")
        gate(6, "K3h")
    ix.indexVectors([str(n0 + i) for i in range(PER)], data["late"])
    ref.add_vectors(data["late"])
    epoch[0] = 1
    if not sharded:  # six: 4 x 8 >= 30 > 4 x 7
        gate(7, "K3h")
        gate(8, "K3q")
    state(walk[half - 1])  # (the transition the checks above interrupted)
    for s in walk[half:]:
        state(s)
    ix.close()
    pairs = set(zip(seen[:-1], seen[1:]))
    missing = [(a, b) for a in NAMES for b in NAMES if (a, b) not in pairs]
    assert not missing, missing
