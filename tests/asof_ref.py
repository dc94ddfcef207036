"""numpy restatements of hf_asof_idx and hf_gather_fill, written from their
header comments (include/hipframe.h) and shared by the CPU mock tier and the
GPU kernel tests.

The as-of restatement is a LINEAR SCAN of the right side per left row — the
candidates are picked by masks over every right row, not by a bound search —
so the device algorithm is never tested against itself.  Distances and
compares use Python ints / floats, so nothing wraps anywhere in the int64
range.
"""

import numpy as np

BACKWARD, FORWARD, NEAREST = 0, 1, 2


def asof_idx_arrays(lon, lby, ron, rby, direction, allow_exact=True,
                    tolerance=None):
    """int64 array: per left row the position in the (rby, ron)-sorted right
    side of its match, or -1."""
    lon, ron = np.asarray(lon), np.asarray(ron)
    assert lon.dtype == ron.dtype
    assert (lby is None) == (rby is None)
    assert direction in (BACKWARD, FORWARD, NEAREST)
    n, m = lon.size, ron.size
    out = np.full(n, -1, dtype=np.int64)
    is_int = lon.dtype == np.dtype(np.int64)

    def dist(hi, lo):
        return int(hi) - int(lo) if is_int else float(hi) - float(lo)

    for i in range(n):
        l = lon[i]
        group = (np.ones(m, dtype=bool) if lby is None
                 else np.asarray(rby) == lby[i])
        le = group & ((ron <= l) if allow_exact else (ron < l))
        ge = group & ((ron >= l) if allow_exact else (ron > l))
        pb = int(np.nonzero(le)[0][-1]) if le.any() else -1   # the LAST one
        pf = int(np.nonzero(ge)[0][0]) if ge.any() else -1    # the FIRST one
        db = dist(l, ron[pb]) if pb >= 0 else None
        df = dist(ron[pf], l) if pf >= 0 else None
        if tolerance is not None:
            if pb >= 0 and db > tolerance:
                pb = -1
            if pf >= 0 and df > tolerance:
                pf = -1
        if direction == BACKWARD:
            out[i] = pb
        elif direction == FORWARD:
            out[i] = pf
        elif pb >= 0 and pf >= 0:
            out[i] = pb if db <= df else pf
        else:
            out[i] = pb if pb >= 0 else pf
    return out


def gather_fill_arrays(col, idx, fill):
    col, idx = np.asarray(col), np.asarray(idx)
    out = np.full(idx.size, fill, dtype=col.dtype)
    hit = idx >= 0
    out[hit] = col[idx[hit]]
    return out
