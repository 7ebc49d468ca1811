"""numpy restatement of the logic of Linear's certified scan, independent of the HIP code: seed, segments, the
survivor test d~ - eps <= T with a deliberately sloppy d~, pool reduction by (distance, index), falling thresholds, the tie
flag and the hand-back to a literal replay of the bounded queue.  It shows that the STRUCTURE returns the queue's answer for
any filter value within eps of the truth; the kernels' own eps is checked on the GPU against the oracle."""
import numpy as np

from np_twin import bpq_replay, sq_dists_rows


def scan_twin(X, q, k, segment=512, seed_rows=1024, eps=1e-3, sloppy="random", rng=None, record_cap=None):
    """-> (ids, distances, info).  sloppy: "random" perturbs the exact distance by up to +-eps, "worst" by +eps (the sign that
    makes a row look farthest), "none" not at all.  info: survivors, handed_back (None | "tie" | "overflow"), dropped."""
    rng = rng or np.random.default_rng(0)
    n = X.shape[0]
    d = sq_dists_rows(X, q)  # the exact values; the filter below sees only d~
    info = {"survivors": 0, "handed_back": None, "dropped": 0}

    def reduce_pool(idx):
        order = np.lexsort((idx, d[idx]))  # by (distance, row index)
        return idx[order][:k + 1]

    S = min(n, max(k + 1, seed_rows))
    pool = reduce_pool(np.arange(S))
    T = d[pool[k]] if len(pool) == k + 1 else np.inf
    done = S
    while done < n:
        rows = np.arange(done, min(n, done + segment))
        u = {"random": rng.uniform(-1, 1, len(rows)), "worst": np.ones(len(rows)), "none": np.zeros(len(rows))}[sloppy]
        d_tilde = d[rows] + u * eps
        surv = rows[d_tilde - eps <= T]
        info["dropped"] += len(rows) - len(surv)
        info["survivors"] += len(surv)
        if record_cap is not None and len(surv) > record_cap:
            info["handed_back"] = "overflow"
            break
        keep = surv[d[surv] <= T]  # verification: the exact distance
        pool = reduce_pool(np.concatenate([pool, keep]))
        if len(pool) == k + 1:
            assert d[pool[k]] <= T  # thresholds only fall
            T = d[pool[k]]
        done = rows[-1] + 1
    if info["handed_back"] is None and len(pool) == k + 1 and d[pool[k - 1]] == d[pool[k]]:
        info["handed_back"] = "tie"
    if info["handed_back"]:
        pos = bpq_replay(d, k)  # the exact path: the queue over all rows in index order
        return pos.astype(np.int32), d[pos], info
    head = pool[:k]
    out = []
    s = 0
    while s < len(head):  # nearest first; equal distances: later arrival first, as the queue empties
        e = s
        while e + 1 < len(head) and d[head[e + 1]] == d[head[s]]:
            e += 1
        out.extend(head[s:e + 1][::-1])
        s = e + 1
    out = np.array(out, dtype=np.int32)
    return out, d[out], info
