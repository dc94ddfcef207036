"""GPU tier: hf_cumsum and hf_seg_cumsum at the sizes and head placements
where a tiled scan goes wrong, against the plain references of
tests/scan_refs.py.

What is asserted, per case:
  * NaN positions identical to the reference;
  * int64 bit-exact (wrapping SUM/PROD; INT64_MIN/INT64_MAX, the scan
    identities, among the MIN/MAX data);
  * f64 MIN/MAX bit-exact;
  * f64 SUM within 48 * u * cumsum|x| of the longdouble reference, u = 2^-53.
    The bound is derived, not tuned on the kernel: the longest addition path
    is 15 adds in a thread's serial run, 8 block-scan steps, 10 tile-scan
    steps, at most 3 carries and 2 joins, about 38 roundings; 48 leaves slack
    for the fold order of the tile summaries (scan_refs.SUM_BOUND);
  * f64 PROD within 48 * u relative.  The path count alone would not give
    this for a product: a rounded product hands the relative errors of both
    operands on in full, so a plain f64 prefix of k factors carries all k - 1
    roundings of its tree (a plain-f64 state measured 91 u at 1023 rows,
    2.0e3 u at 2048 * TILE + 1 and 1.7e5 u = 1.9e-11 at 1024 * TILE + 4097
    rows with 10 % NaN on the MI355X).  The kernels therefore carry the f64
    product as hi + lo (double-double): a combine costs about u^2 and the
    output rounds once, which is what makes a bound of this size hold.  The
    longdouble reference itself drifts by about sqrt(k) * 2^-64, under 1 u
    at these sizes.
"""

import numpy as np
import pandas
import pytest

import modin_amd.pandas as mpd
from modin_amd.core import lib
from tests import scan_refs as sr
from tests.scan_refs import TILE, PER, U, SUM_BOUND

pytestmark = pytest.mark.gpu

AGG = {"sum": lib.AGG_SUM, "min": lib.AGG_MIN, "max": lib.AGG_MAX,
       "prod": lib.AGG_PROD}
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
ITER = 1024 * TILE      # rows per iteration of the one-block tile scan

# 16 rows is one thread's run, 256 the rows of one striped load, 1024 four of
# them, 4096 one tile; 1024 tiles fill one iteration of the tile scan, one
# more row opens the second, 2048 tiles and a row open the third, where the
# carry is itself built from a carry
SIZES = [1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
         3 * TILE + 5, ITER, ITER + 1, ITER + 4097, 2 * ITER + 1]


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _scan(x, heads, op):
    col = lib.put(x)
    if heads is None:
        out = lib.cumsum(col, AGG[op])
    else:
        out = lib.seg_cumsum(col, lib.put(heads), AGG[op])
    got = lib.get(out)
    assert got.dtype == x.dtype and got.shape == x.shape
    return got


def _check(x, heads, op, what):
    """One kernel call against the reference; returns the worst error in
    units of the bound's scale (0 for the exact ops)."""
    got = _scan(x, heads, op)
    ref, absum = sr.ref_seg_cumsum(x, heads, op)
    what = (what, op, str(x.dtype), x.size)
    if x.dtype == np.int64:
        assert np.array_equal(got, ref), what
        return 0.0
    assert np.array_equal(np.isnan(got), np.isnan(x)), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    if op in ("min", "max"):
        assert np.array_equal(got, ref, equal_nan=True), what
        return 0.0
    if op == "sum":
        ratio = sr.sum_error_ratio(got, ref, absum)
    else:
        ok = ~np.isnan(ref)
        rel = np.abs(got[ok].astype(np.longdouble) / ref[ok] - 1)
        ratio = float(rel.max() / U) if rel.size else 0.0
    assert ratio <= SUM_BOUND, (what, ratio)
    return ratio


def _nan_variants(rng, x):
    """NaN shares 0, 0.1 and 0.97, and a leading all-NaN tile plus 3 rows
    (the tile summary is the identity and the first valid row restarts)."""
    yield "nan 0", x
    for share in (0.1, 0.97):
        y = x.copy()
        y[rng.random(x.size) < share] = np.nan
        yield f"nan {share}", y
    y = x.copy()
    y[:TILE + 3] = np.nan
    yield "leading nan tile", y


def _prod_values(rng, valid):
    """Values in [0.5, 2) laid over the valid rows as reciprocal pairs
    v, 1/v, so no running product leaves [0.25, 4] wherever it starts."""
    x = np.full(valid.size, np.nan)
    idx = np.flatnonzero(valid)
    v = rng.uniform(0.5, 2.0, (idx.size + 1) // 2)
    x[idx[0::2]] = v
    x[idx[1::2]] = 1.0 / v[:idx.size // 2]
    return x


def _trend(rng, n, op, dtype):
    """Data whose running extreme keeps moving to the last row: a downward
    drift for min, upward for max, noise several steps wide."""
    step = np.arange(n, dtype=np.int64) * (-3 if op == "min" else 3)
    return (step + rng.integers(-50, 50, n)).astype(dtype)


# ---- hf_cumsum --------------------------------------------------------------

@pytest.mark.parametrize("data", ["normal", "offset", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_cumsum_f64_sum(n, data):
    rng = np.random.default_rng(n)
    x = sr.scan_datasets(rng, n)[data]
    worst = 0.0
    for what, y in _nan_variants(rng, x):
        worst = max(worst, _check(y, None, "sum", (data, what)))
    print(f"cumsum f64 sum n={n} {data}: worst {worst:.3g} u*cumsum|x|")


@pytest.mark.parametrize("n", SIZES)
def test_cumsum_f64_prod(n):
    rng = np.random.default_rng(n + 1)
    worst = 0.0
    for share in (0.0, 0.1, 0.97):
        x = _prod_values(rng, rng.random(n) >= share)
        worst = max(worst, _check(x, None, "prod", ("nan", share)))
    valid = np.ones(n, dtype=bool)
    valid[:TILE + 3] = False
    worst = max(worst, _check(_prod_values(rng, valid), None, "prod",
                              "leading nan tile"))
    print(f"cumsum f64 prod n={n}: worst {worst:.3g} u")


@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("n", SIZES)
def test_cumsum_f64_minmax(n, op):
    rng = np.random.default_rng(n + 2)
    x = _trend(rng, n, op, np.float64)
    for what, y in _nan_variants(rng, x):
        _check(y, None, op, what)


@pytest.mark.parametrize("n", SIZES)
def test_cumsum_int64(n):
    rng = np.random.default_rng(n + 3)
    # full-range values: the running sum wraps every few rows
    _check(rng.integers(I64_MIN, I64_MAX, n, endpoint=True), None, "sum",
           "wrapping")
    # odd factors: the wrapping product never collapses to zero
    _check(rng.integers(I64_MIN, I64_MAX, n, endpoint=True) | 1, None,
           "prod", "wrapping odd")
    for op in ("min", "max"):
        x = _trend(rng, n, op, np.int64)
        # the identity as data (first row and mid-column), and the opposite
        # extreme three quarters down, after which nothing may change
        ident, other = (I64_MAX, I64_MIN) if op == "min" else \
            (I64_MIN, I64_MAX)
        x[0] = x[n // 2] = ident
        if n > 4:
            x[3 * n // 4] = other
        _check(x, None, op, "identities as data")


# both infinities in one tile; in adjacent tiles; either side of the
# 1024-tile iteration boundary, where inf sits in the carry
@pytest.mark.parametrize("pos,neg", [(100, 3000), (TILE - 5, TILE + 5),
                                     (ITER - 3, ITER + 3)])
def test_cumsum_f64_sum_infinities(pos, neg):
    rng = np.random.default_rng(pos)
    n = ITER + 4097
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.1] = np.nan
    x[pos], x[neg] = np.inf, -np.inf
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        exp = np.cumsum(np.where(nan, 0.0, x))
    exp[nan] = np.nan
    assert np.isinf(exp[pos]) and np.isnan(exp[neg:]).all()
    got = _scan(x, None, "sum")
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(np.isinf(got), np.isinf(exp))
    inf = np.isinf(exp)
    assert np.array_equal(np.signbit(got[inf]), np.signbit(exp[inf]))


# ---- hf_seg_cumsum ----------------------------------------------------------

def _stepped(rng, heads, op, dtype):
    """MIN/MAX data for segments: every segment lies strictly above (min) or
    below (max) the one before, so the previous segment's extreme would win
    if a head were lost."""
    level = np.cumsum(heads != 0) * 1000 + rng.integers(0, 100, heads.size)
    return (level if op == "min" else -level).astype(dtype)


PARTS = ["f64_sum", "f64_prod", "f64_minmax", "int64"]


def _check_segments(rng, heads, what, part, nan_share=0.1):
    """One head layout under every op of one part."""
    assert heads.dtype == np.int64
    n = heads.size
    nan = rng.random(n) < nan_share
    if part == "f64_sum":
        x = 1e6 + rng.normal(0.0, 1.0, n)
        x[nan] = np.nan
        worst = _check(x, heads, "sum", what)
        print(f"seg_cumsum sum {what}: worst {worst:.3g} u*cumsum|x|")
    elif part == "f64_prod":
        worst = _check(_prod_values(rng, ~nan), heads, "prod", what)
        print(f"seg_cumsum prod {what}: worst {worst:.3g} u")
    elif part == "f64_minmax":
        for op in ("min", "max"):
            x = _stepped(rng, heads, op, np.float64)
            x[nan] = np.nan
            _check(x, heads, op, what)
    else:
        for op in ("min", "max"):
            _check(_stepped(rng, heads, op, np.int64), heads, op, what)
        _check(rng.integers(I64_MIN, I64_MAX, n, endpoint=True), heads,
               "sum", what)
        _check(rng.integers(I64_MIN, I64_MAX, n, endpoint=True) | 1, heads,
               "prod", what)


def _heads(n, rows):
    heads = np.zeros(n, dtype=np.int64)
    heads[rows] = 1
    return heads


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("n", [n for n in SIZES if n < ITER])
def test_seg_cumsum_sizes(n, part):
    """The small sizes with heads about every 700 rows (none at all below
    that), so each tail length also runs through the segmented kernels; the
    large sizes are test_seg_cumsum_heads_across_iterations."""
    rng = np.random.default_rng(n + 4)
    _check_segments(rng, (rng.random(n) < 1 / 700).astype(np.int64),
                    f"n={n}", part)


# row 0 with and without a head; the second row; the last row of a thread's
# run and the first of the next; the last row of a tile, the first of the
# next and the one after; all together; no head; every row
@pytest.mark.parametrize("rows", [
    [0], [1], [PER - 1], [PER], [TILE - 1], [TILE], [TILE + 1],
    [0, 1, PER - 1, PER, TILE - 1, TILE, TILE + 1], [], "all"], ids=str)
@pytest.mark.parametrize("part", PARTS)
def test_seg_cumsum_placed_heads(part, rows):
    rng = np.random.default_rng(21)
    n = 3 * TILE + 5
    heads = np.ones(n, dtype=np.int64) if rows == "all" else _heads(n, rows)
    _check_segments(rng, heads, f"heads {rows}", part)


# across the 1024-tile iteration of the one-block tile scan:
@pytest.mark.parametrize("rows,why", [
    ([], "the carry value flows across the iteration, no flag set"),
    ([1023 * TILE + 77], "carry_f set in iteration 0, no head in iteration 1"),
    ([ITER], "head on the first row of iteration 1: the carry is dropped"),
    ([ITER - 1], "head on the last row of iteration 0: the carry is one row"),
    ([ITER + 77], "only head inside the first tile of iteration 1"),
    ([1025 * TILE], "only head in tile 1025, whose single row is the last"),
], ids=["none", "tile1023", "first_of_iter1", "last_of_iter0", "tile1024",
        "tile1025"])
@pytest.mark.parametrize("part", PARTS)
def test_seg_cumsum_heads_across_iterations(part, rows, why):
    rng = np.random.default_rng(22)
    _check_segments(rng, _heads(ITER + 4097, rows), f"heads {rows}", part)


# runs far shorter than a thread's 16 rows, and runs longer than a tile
@pytest.mark.parametrize("run", [3, 5000])
@pytest.mark.parametrize("part", PARTS)
def test_seg_cumsum_random_heads(part, run):
    rng = np.random.default_rng(run)
    n = 12 * TILE + 9
    for nan_share in (0.1, 0.97):
        heads = (rng.random(n) < 1.0 / run).astype(np.int64)
        _check_segments(rng, heads, f"run {run} nan {nan_share}", part,
                        nan_share)


@pytest.mark.parametrize("op", sr.OPS)
def test_seg_cumsum_head_on_nan_row(op):
    """A head on a NaN row, more NaN rows behind it: NaN out there, and the
    segment's first valid row restarts from the identity."""
    rng = np.random.default_rng(23)
    n = 2 * TILE + 3
    rows = [5, 100, TILE, TILE + 40]
    heads = _heads(n, rows)
    nan_rows = rows + [101, 102, 103]
    valid = np.ones(n, dtype=bool)
    valid[nan_rows] = False
    if op == "prod":
        x = _prod_values(rng, valid)
    elif op == "sum":
        x = 1e6 + rng.normal(0.0, 1.0, n)
    else:
        x = _stepped(rng, heads, op, np.float64)
    x[nan_rows] = np.nan
    got = _scan(x, heads, op)
    assert np.isnan(got[nan_rows]).all()
    # restart from the identity: the first valid row gives itself back
    first = [6, 104, TILE + 1, TILE + 41]
    assert np.array_equal(got[first], x[first])
    _check(x, heads, op, "head on nan")


def test_argument_errors():
    col = lib.put(np.arange(10.0))
    with pytest.raises(lib.HfError, match=r"rc=2"):
        lib.seg_cumsum(col, lib.put(np.ones(9, dtype=np.int64)), lib.AGG_SUM)
    with pytest.raises(lib.HfError, match=r"rc=2"):
        lib.cumsum(col, 17)


# ---- rolling sum/mean: conditioned on the prefix, not the window ------------

@pytest.mark.parametrize("window", [3, 250])
def test_rolling_sum_mean_inherit_prefix_rounding(window):
    """rolling sum is cz[i] - cz[i - w] over the NaN-zero-filled prefix sums
    cz, each within 48 * u * cumsum|x| of exact, and the subtraction rounds
    once more: |got - ref| <= 2 * 48 * u * cumsum|x|[i] + 2 * u * |ref|.
    The error therefore scales with the prefix (5e10 at the last row here),
    not with the window (3e6 or 2.5e8); pandas' add/remove update with Kahan
    compensation does not inherit it.  Mean divides both by the count."""
    rng = np.random.default_rng(window)
    n = 50_000
    x = 1e6 + rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.1] = np.nan
    nan = np.isnan(x)
    xl = np.where(nan, 0.0, x).astype(np.longdouble)
    absum = np.cumsum(np.abs(xl))
    ref = np.zeros(n, dtype=np.longdouble)
    cnt = np.zeros(n, dtype=np.int64)
    for j in range(window):     # windowed sum, no prefix difference
        ref[j:] += xl[:n - j]
        cnt[j:] += ~nan[:n - j]
    df = mpd.DataFrame(pandas.DataFrame({"x": x}))
    roll = df.rolling(window, min_periods=1)
    bound = 2 * SUM_BOUND * U * absum + 2 * U * np.abs(ref)
    some = cnt > 0
    for name, got, r, b in (
            ("sum", roll.sum(), ref, bound),
            ("mean", roll.mean(), ref / np.maximum(cnt, 1),
             bound / np.maximum(cnt, 1))):
        got = got.to_pandas()["x"].to_numpy()
        assert np.array_equal(np.isnan(got), ~some), name
        err = np.abs(got[some].astype(np.longdouble) - r[some])
        print(f"rolling({window}).{name}: worst abs error "
              f"{float(err.max()):.3g}, worst error/bound "
              f"{float((err / b[some]).max()):.3g}")
        assert (err <= b[some]).all(), name
