#!/usr/bin/env python3
"""Withdrawing and updating images in an IVFPQ index that lives in HBM.

The reference can only index: an image leaves a collection by a rebuilt BDB environment.  Here removeVector takes its record out of
the device index in place -- the survivors keep their list and their order inside it -- and replaceVector is remove + index again:

  python examples/remove_records.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def show(label, a):
    print(f"  {label:<22}", [(i, float(f"{d:.4g}")) for i, d in zip(a.getIds(), a.getDistances())])


def main():
    import synth

    mi = importlib.import_module("multimedia-indexing_amd")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("remove_records.py needs an MI355X: libmmidx_hip has no CPU fallback")
    D, C_, m, ks, n, k, w = 64, 32, 8, 256, 20000, 5, 8
    p = synth.make_ivfpq_problem(n=n, D=D, C=C_, m=m, ks=ks, nq=1, seed=3)
    ix = mi.IVFPQ(D, n + 16, False, "", m, ks, mi.TransformationType.None_, C_, 512)
    ix.loadCoarseQuantizer(p["coarse"])
    ix.loadProductQuantizer(p["pq"])
    ix.setW(w)
    assert ix.indexVectors([f"img{i}" for i in range(n)], p["base"]) == n
    q = p["base"][4242]

    first = ix.computeNearestNeighbors(k, q)
    show("before", first)
    top = first.getIds()[0]

    # the top hit is withdrawn
    assert ix.removeVector(top) and not ix.isIndexed(top) and ix.size() == n - 1
    second = ix.computeNearestNeighbors(k, q)
    show(f"without {top}", second)
    assert top not in second.getIds() and second.getIds()[:k - 1] == first.getIds()[1:]
    assert ix.removeVector(top) is False  # (prints: not indexed)

    # several at once; unknown ids are reported and skipped
    print("  removed", ix.removeVectors(second.getIds()[:2] + ["no such image"]), "of 3 ids;", ix.size(), "records left")

    # an image was re-extracted: its record is replaced (a fresh internal id; a removed record does not give its capacity back)
    id_ = "img17"
    old_iid = ix.getInternalId(id_)
    moved = p["base"][17] + 0.5 * np.random.default_rng(0).standard_normal(D)
    assert ix.replaceVector(id_, moved)
    print(f"  {id_}: internal id {old_iid} -> {ix.getInternalId(id_)}, loadCounter {ix.getLoadCounter()}")
    show(f"query = new {id_}", ix.computeNearestNeighbors(k, moved))
    show(f"query = old {id_}", ix.computeNearestNeighbors(k, p["base"][17]))
    ix.close()


if __name__ == "__main__":
    main()
