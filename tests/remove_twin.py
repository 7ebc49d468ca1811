"""The numpy twin of mmidx_remove: what an export looks like after a removal.

filter_export takes the three arrays of an export (list offsets, internal ids, codes -- list-major, arrival order inside every
list) and the requested ids, and returns the arrays of the index "as if the removed records had never been added": the survivors in
their lists, in their order.  tests/test_remove_cpu.py pins that reading against the CPU oracle; the GPU tests compare the library's
export with it array for array."""
import numpy as np


def filter_export(off, iids, codes, remove_ids):
    """-> (off_new [nlists + 1] int64, iids_new, codes_new, found [len(remove_ids)] int32, removed).
    Every record whose id occurs in remove_ids goes (all of them where an id is stored more than once); found[i] says whether
    remove_ids[i] was stored, so both occurrences of a repeated request get the same answer; removed counts records."""
    off = np.asarray(off, np.int64)
    iids = np.asarray(iids, np.int32)
    codes = np.asarray(codes)
    req = np.asarray(remove_ids, np.int64).reshape(-1)
    gone = np.isin(iids.astype(np.int64), req)
    found = np.isin(req, iids.astype(np.int64)).astype(np.int32)
    # a list's new start: the survivors in front of its old start
    kept_before = np.concatenate([[0], np.cumsum(~gone)]).astype(np.int64)
    off_new = kept_before[off]
    return off_new, iids[~gone].copy(), codes[~gone].copy(), found, int(gone.sum())


def list_of_position(off, n):
    """[n] the list every position of an export belongs to"""
    return (np.searchsorted(np.asarray(off, np.int64), np.arange(n), side="right") - 1).astype(np.int32)
