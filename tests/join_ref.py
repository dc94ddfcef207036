"""Plain numpy references for the join and the row-movement entry points,
shared by the CPU mock tier (test_mock_join_edges.py) and the GPU tier
(test_gpu_join_edges.py, test_gpu_entry_ownership.py).

The join reference is sort based: a stable argsort of the right keys, two
bound searches per left key, and an arithmetic expansion of each run.  It has
no histogram, no offset table and no per-slot state, so the device's CSR
build and two-pass probe are never compared with a copy of themselves.
Nothing here loops over rows in Python; the 4M-row cases run in well under a
second.  test_mock_join_edges.py checks inner_join_ref against pandas.merge.
"""

import numpy as np

I64 = np.dtype(np.int64)


def inner_join_ref(lkeys, rkeys, rvals):
    """(keys, lidx, ridx, [payload columns]) of the inner join in pandas'
    order: left row order, then original right row order within a key."""
    lkeys = np.asarray(lkeys, dtype=np.int64)
    rkeys = np.asarray(rkeys, dtype=np.int64)
    order = np.argsort(rkeys, kind="stable")
    srt = rkeys[order]
    lo = np.searchsorted(srt, lkeys, side="left")
    cnt = np.searchsorted(srt, lkeys, side="right") - lo
    lidx = np.repeat(np.arange(lkeys.size, dtype=np.int64), cnt)
    # output row r of left row i reads sorted position lo[i] + (r - start[i])
    start = np.cumsum(cnt) - cnt
    within = np.arange(lidx.size, dtype=np.int64) - np.repeat(start, cnt)
    ridx = order[np.repeat(lo, cnt) + within].astype(np.int64)
    return lkeys[lidx], lidx, ridx, [np.asarray(v)[ridx] for v in rvals]


def search_sorted_ref(keys, sorted_):
    """First position p with sorted_[p] == k per key, else -1."""
    keys, sorted_ = np.asarray(keys), np.asarray(sorted_)
    if sorted_.size == 0:
        return np.full(keys.size, -1, dtype=np.int64)
    p = np.searchsorted(sorted_, keys, side="left")
    hit = sorted_[np.minimum(p, sorted_.size - 1)] == keys
    return np.where((p < sorted_.size) & hit, p, -1).astype(np.int64)


def gather_ref(src, idx):
    return src[idx]


def gather_fill_ref(src, idx, fill):
    return np.where(idx < 0, np.asarray(fill, dtype=src.dtype),
                    src[np.maximum(idx, 0)])


def scatter_ref(src, perm):
    """out[perm[i]] = src[i], as a gather through the inverse permutation."""
    return src[np.argsort(perm, kind="stable")]


def cross_idx_ref(nl, nr):
    i = np.arange(nl * nr, dtype=np.int64)
    return i // max(nr, 1), i % max(nr, 1)


def bits(a):
    """int64 view of an 8-byte column: NaN payloads and -0.0 count."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 8, a.dtype
    return a.view(np.int64)
