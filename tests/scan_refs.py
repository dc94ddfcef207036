"""Plain numpy references for the scan and compaction kernels, written for
clarity rather than speed, plus a numpy restatement of the tiled f64 sum scan
(`hf_cumsum`, AGG_SUM) that lets the CPU tier check the scan's error bound
without a GPU.

Scan references return ``(values, absum)``.  For f64 SUM, `values` is a
``np.longdouble`` array and `absum` the running sum of |x| over the same
segment, also in longdouble: the scale every rounding-error bound of a sum is
stated in.  For f64 PROD `values` is longdouble and `absum` is None.  MIN/MAX
and every int64 op return the column's own dtype and `absum` None.
"""

import numpy as np

TILE = 4096     # rows per scan tile (FILT_TILE)
BLOCK = 256     # threads per block
PER = 16        # consecutive rows per thread (TILE / BLOCK)
SCAN = 1024     # tiles per iteration of the one-block tile scan
U = 2.0 ** -53  # unit roundoff of f64

# The longest chain of f64 additions behind one output of the tiled sum
# scan: 15 adds in the thread's serial run, 8 steps of the 256-thread
# Hillis-Steele scan, 10 steps of the 1024-tile scan, at most 3 carries
# between tile-scan iterations and 2 joins (tile base + thread base, base +
# run): about 38 roundings, each at most u times a partial sum of |x|.  48
# leaves slack for the fold order of the per-tile summaries.
SUM_BOUND = 48.0

OPS = ("sum", "min", "max", "prod")


def _segment_bounds(n, heads):
    """[start, end) of every segment; row 0 opens one with or without a
    head, as in the kernel."""
    if heads is None:
        starts = np.zeros(1, dtype=np.int64)
    else:
        heads = np.asarray(heads)
        assert heads.shape == (n,)
        starts = np.flatnonzero(heads != 0)
        if starts.size == 0 or starts[0] != 0:
            starts = np.r_[0, starts]
    return starts, np.r_[starts[1:], n]


def _scan_one(x, op):
    """One segment, sequentially."""
    if x.dtype == np.int64:
        with np.errstate(over="ignore"):
            if op == "sum":
                return np.cumsum(x, dtype=np.int64), None
            if op == "prod":
                return np.multiply.accumulate(x, dtype=np.int64), None
        acc = np.minimum if op == "min" else np.maximum
        return acc.accumulate(x), None
    assert x.dtype == np.float64
    nan = np.isnan(x)
    if op in ("min", "max"):
        # fmin/fmax skip NaN; a NaN row is emitted as NaN below
        acc = np.fmin if op == "min" else np.fmax
        out = acc.accumulate(x)
        out[nan] = np.nan
        return out, None
    xl = x.astype(np.longdouble)
    if op == "sum":
        xl[nan] = 0
        out = np.cumsum(xl)
        absum = np.cumsum(np.abs(xl))
    else:
        xl[nan] = 1
        out = np.cumprod(xl)
        absum = None
    out[nan] = np.nan
    return out, absum


def ref_seg_cumsum(x, heads, op):
    """Inclusive scan of `x` under `op`, restarting at rows whose `heads`
    entry is nonzero.  f64: NaN rows are skipped and emitted as NaN."""
    assert op in OPS
    x = np.asarray(x)
    n = x.size
    starts, ends = _segment_bounds(n, heads)
    is_f = x.dtype == np.float64
    wide = is_f and op in ("sum", "prod")
    out = np.empty(n, dtype=np.longdouble if wide else x.dtype)
    absum = np.empty(n, dtype=np.longdouble) if is_f and op == "sum" else None
    for s, e in zip(starts, ends):
        o, a = _scan_one(x[s:e], op)
        out[s:e] = o
        if absum is not None:
            absum[s:e] = a
    return out, absum


def ref_cumsum(x, op):
    return ref_seg_cumsum(x, None, op)


def ref_filter(mask, col):
    return np.asarray(col)[np.asarray(mask) != 0]


def ref_filter_iota(mask, base):
    return np.flatnonzero(np.asarray(mask) != 0).astype(np.int64) + \
        np.int64(base)


def _hillis_steele(a):
    """Inclusive scan along the last axis the way the kernels do it: log2
    steps, each adding the element `off` places to the left."""
    a = a.copy()
    off = 1
    while off < a.shape[-1]:
        nxt = a.copy()
        nxt[..., off:] = a[..., off:] + a[..., :-off]
        a = nxt
        off <<= 1
    return a


def tiled_sum_scan(x):
    """numpy restatement of hf_cumsum(f64, SUM), in f64 throughout and with
    the kernel's association order:

    1. tile summaries (k_cumsum_tiles): each of 256 threads folds its 16
       strided rows, a halving tree joins the 64 lanes of a wave, the four
       wave totals are added in order;
    2. one-block exclusive scan of the summaries (k_cumsum_scan_tiles):
       Hillis-Steele over 1024 tiles, a carry between iterations;
    3. apply (k_cumsum_apply): each thread scans its 16 consecutive rows
       serially, a Hillis-Steele scan over the 256 thread totals gives the
       thread's base, output = (tile base + thread base) + run.
    """
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    nan = np.isnan(x)
    ntiles = -(-n // TILE)
    v = np.zeros(ntiles * TILE)
    v[:n] = np.where(nan, 0.0, x)

    # 1. thread t of a tile folds rows t, t + 256, ...
    strided = v.reshape(ntiles, PER, BLOCK)
    local = np.zeros((ntiles, BLOCK))
    for j in range(PER):
        local = local + strided[:, j, :]
    lanes = local.reshape(ntiles, BLOCK // 64, 64)
    width = 32
    while width:
        lanes = lanes[..., :width] + lanes[..., width:2 * width]
        width >>= 1
    waves = lanes[..., 0]
    tile_sum = np.zeros(ntiles)
    for w in range(BLOCK // 64):
        tile_sum = tile_sum + waves[:, w]

    # 2. exclusive scan, 1024 tiles per iteration
    tile_base = np.empty(ntiles)
    carry = 0.0
    for base in range(0, ntiles, SCAN):
        chunk = np.zeros(SCAN)
        m = min(SCAN, ntiles - base)
        chunk[:m] = tile_sum[base:base + m]
        incl = _hillis_steele(chunk)
        excl = np.r_[0.0, incl[:-1]]
        tile_base[base:base + m] = (carry + excl)[:m]
        carry = carry + incl[-1]

    # 3. per-tile apply
    runs = v.reshape(ntiles, BLOCK, PER)
    loc = np.empty_like(runs)
    run = np.zeros((ntiles, BLOCK))
    for j in range(PER):
        run = run + runs[:, :, j]
        loc[:, :, j] = run
    incl = _hillis_steele(run)
    texcl = np.concatenate([np.zeros((ntiles, 1)), incl[:, :-1]], axis=1)
    tbase = tile_base[:, None] + texcl
    out = (tbase[:, :, None] + loc).reshape(-1)[:n]
    out[nan] = np.nan
    return out


def sum_error_ratio(got, ref, absum):
    """max over rows of |got - ref| / (u * cumsum|x|), the figure the bound
    SUM_BOUND caps; rows with a zero scale must match exactly."""
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok].astype(np.longdouble) - ref[ok])
    scale = absum[ok] * np.longdouble(U)
    zero = scale == 0
    assert not (err[zero] != 0).any(), "nonzero error where sum|x| is zero"
    if zero.all():
        return 0.0
    return float((err[~zero] / scale[~zero]).max())


def scan_datasets(rng, n):
    """The three f64 data sets the sum bound is checked on."""
    return {
        "normal": rng.normal(0.0, 1.0, n),
        "offset": 1e6 + rng.normal(0.0, 1.0, n),
        "mixed": rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n),
    }
