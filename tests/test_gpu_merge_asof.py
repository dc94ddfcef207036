"""GPU tier: hf_asof_idx / hf_gather_fill against the numpy restatements of
their header comments (tests/asof_ref.py: a linear scan per left row), and
merge_asof above them against pandas.  Everything is a gather, so every
comparison is bit-exact.

hf_asof_idx runs calls without a by column on the sorted-left (window) form
and calls with one on the general form; HF_ASOF_FORM=1 keeps the former on
the general form too, which is how the two are compared on the same input.
"""

import ctypes as ct
import os

import numpy as np
import pandas
import pytest

import modin_amd.pandas as mpd
from modin_amd import config
from modin_amd.core import lib
from modin_amd.core.lib import HfError
from tests import asof_ref
from tests.test_mock_merge_asof import (DIRECTIONS, by_frames, dt_frames,
                                        fuzz_case, trades_quotes)

pytestmark = pytest.mark.gpu

TILE = 2048   # ASOF_TILE: left rows per workgroup of the sorted-left form
WIN = 2544    # ASOF_WIN: right keys the LDS window holds
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
COMBOS = [(d, e) for d in (0, 1, 2) for e in (True, False)]


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = config.NPartitions.get()
    config.NPartitions.put(request.param)
    yield request.param
    config.NPartitions.put(old)


def device_idx(lon, lby, ron, rby, direction, exact, tol, general=False):
    """hf_asof_idx on host arrays; general=True pins the general form."""
    old = os.environ.pop("HF_ASOF_FORM", None)
    if general:
        os.environ["HF_ASOF_FORM"] = "1"
    try:
        got = lib.get(lib.asof_idx(
            lib.put(lon), None if lby is None else lib.put(lby),
            lib.put(ron), None if rby is None else lib.put(rby),
            direction, exact, tol))
    finally:
        os.environ.pop("HF_ASOF_FORM", None)
        if old is not None:
            os.environ["HF_ASOF_FORM"] = old
    assert got.dtype == np.int64 and got.shape == lon.shape
    return got


def check_all_forms(lon, ron, direction, exact, tol, exp=None, what=""):
    """No-by input: the window form, the general form and the general form
    with an all-zero by column all give the restatement's positions."""
    if exp is None:
        exp = asof_ref.asof_idx_arrays(lon, None, ron, None, direction,
                                       exact, tol)
    zl = np.zeros(lon.size, dtype=np.int64)
    zr = np.zeros(ron.size, dtype=np.int64)
    for name, got in (
            ("window", device_idx(lon, None, ron, None, direction, exact,
                                  tol)),
            ("general", device_idx(lon, None, ron, None, direction, exact,
                                   tol, general=True)),
            ("general+by", device_idx(lon, zl, ron, zr, direction, exact,
                                      tol))):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (what, name, direction, exact, tol, bad[:5],
                               got[bad[:5]], exp[bad[:5]])
    return exp


LEFT_LENS = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1,
             3 * TILE + 17]


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
@pytest.mark.parametrize("nr", [0, 1, 2, 255, 256, 257, 5000])
def test_edge_lengths(nr, dtype):
    """Keys from a small range, so duplicates abound on both sides; each
    (left, right) length pair takes two of the six direction x exact
    combinations, rotating so that every combination meets every length."""
    rng = np.random.default_rng(nr + 7)
    span = max(4, nr // 3)
    ron = np.sort(rng.integers(0, span, nr)).astype(dtype)
    for a, nl in enumerate(LEFT_LENS):
        lon = np.sort(rng.integers(-2, span + 2, nl)).astype(dtype)
        for k in (0, 3):
            direction, exact = COMBOS[(a + k + nr) % 6]
            tol = None if (a + k) % 2 else dtype(2)
            check_all_forms(lon, ron, direction, exact, tol, what=(nl, nr))


def fence_case():
    """Adjacent right groups whose `on` ranges interleave: a search that
    leaks over a group fence lands on a plausible row of the neighbour."""
    right = {0: [10, 30, 30, 50],      # first group
             1: [20, 40, 60],
             2: [35],                  # groups of one row
             4: [5],
             5: [25, 45, 45, 65],
             7: [15, 55]}              # last group; 3 and 6 are absent
    rby = np.array([g for g, v in right.items() for _ in v], dtype=np.int64)
    ron = np.array([x for v in right.values() for x in v], dtype=np.int64)
    keys = [0, 5, 9, 10, 15, 20, 29, 30, 31, 35, 36, 45, 50, 55, 60, 65, 70]
    lby = np.repeat(np.arange(-1, 9, dtype=np.int64), len(keys))
    lon = np.tile(np.array(keys, dtype=np.int64), 10)
    order = np.random.default_rng(5).permutation(lon.size)  # any left order
    return lon[order], lby[order], ron, rby


@pytest.mark.parametrize("direction,exact", COMBOS)
def test_group_fences(direction, exact):
    lon, lby, ron, rby = fence_case()
    for tol in (None, 0, 4, 100):
        exp = asof_ref.asof_idx_arrays(lon, lby, ron, rby, direction, exact,
                                       tol)
        got = device_idx(lon, lby, ron, rby, direction, exact, tol)
        assert np.array_equal(got, exp), (tol, np.nonzero(got != exp)[0])
        # a match never leaves its group, absent groups match nothing
        hit = got >= 0
        assert np.array_equal(rby[got[hit]], lby[hit])
        assert not hit[np.isin(lby, [-1, 3, 6, 8])].any()
    got = device_idx(lon, lby, ron, rby, direction, exact, None)
    below = (lby == 1) & (lon < 20)    # under group 1's minimum
    above = (lby == 1) & (lon > 60)    # over group 1's maximum
    if direction == asof_ref.BACKWARD:
        assert (got[below] == -1).all()      # not group 0's last row
    if direction == asof_ref.FORWARD:
        assert (got[above] == -1).all()      # not group 2's first row


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
def test_by_random(dtype):
    rng = np.random.default_rng(11)
    nl, nr, groups = 3001, 1999, 40
    rby = rng.integers(0, groups, nr).astype(np.int64)
    ron = rng.integers(0, 300, nr).astype(dtype)
    order = np.lexsort((ron, rby))
    rby, ron = rby[order], ron[order]
    lby = rng.integers(-1, groups + 1, nl).astype(np.int64)
    lon = rng.integers(-5, 305, nl).astype(dtype)
    for direction, exact in COMBOS:
        tol = None if exact else dtype(7)
        exp = asof_ref.asof_idx_arrays(lon, lby, ron, rby, direction, exact,
                                       tol)
        got = device_idx(lon, lby, ron, rby, direction, exact, tol)
        assert np.array_equal(got, exp), (direction, exact)


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_window_over_lds_budget(direction):
    """Right ~60x denser than left: the first tile's window holds far more
    than WIN keys, so its lanes search the window in place."""
    rng = np.random.default_rng(12)
    nl = TILE + 100
    lon = np.sort(rng.integers(0, 200_000, nl)).astype(np.int64)
    ron = np.sort(rng.integers(0, 200_000, 60 * nl)).astype(np.int64)
    first = np.searchsorted(ron, lon[0]), np.searchsorted(ron, lon[TILE - 1])
    assert first[1] - first[0] > 10 * WIN
    # the restatement on a sample of rows (tile edges included), the general
    # form on all of them
    pick = np.unique(np.concatenate([np.arange(0, nl, 37),
                                     [0, TILE - 1, TILE, nl - 1]]))
    exp = asof_ref.asof_idx_arrays(lon[pick], None, ron, None, direction,
                                   True, None)
    for tol in (None, 1):
        win = device_idx(lon, None, ron, None, direction, True, tol)
        gen = device_idx(lon, None, ron, None, direction, True, tol,
                         general=True)
        assert np.array_equal(win, gen), tol
    assert np.array_equal(
        device_idx(lon, None, ron, None, direction, True, None)[pick], exp)


@pytest.mark.parametrize("direction,exact", COMBOS)
def test_window_empty_and_clamped(direction, exact):
    # the whole left tile falls into a gap of the right side
    ron = np.concatenate([np.arange(1000), 100_000 + np.arange(1000)]
                         ).astype(np.int64)
    lon = np.sort(np.random.default_rng(13).integers(5000, 6000, TILE + 9)
                  ).astype(np.int64)
    for tol in (None, 4500):
        check_all_forms(lon, ron, direction, exact, tol, what="gap")
    # the left tile overhangs the right side at both ends
    ron = np.repeat(np.arange(250), 2).astype(np.int64)
    lon = np.sort(np.random.default_rng(14).integers(-1000, 1250, TILE)
                  ).astype(np.int64)
    for tol in (None, 30):
        check_all_forms(lon, ron, direction, exact, tol, what="clamped")
    # a window exactly at, and one past, the LDS budget
    for wn in (WIN, WIN + 1):
        ron = np.arange(wn, dtype=np.int64)
        lon = np.sort(np.random.default_rng(wn).integers(0, wn, TILE)
                      ).astype(np.int64)
        lon[0], lon[-1] = 0, wn - 1
        check_all_forms(lon, ron, direction, exact, None, what=("win", wn))


@pytest.mark.parametrize("direction,exact", COMBOS)
def test_exact_datetime_scale(direction, exact):
    """Keys near 1.7e18, where one double ulp is 256 ns: neighbours 1 ns
    apart and a 1 ns tolerance.  Promoting a key to double fails this."""
    base = np.int64(1_700_000_000_000_000_000)
    ron = base + 2 * np.arange(300, dtype=np.int64)
    lon = base + np.arange(-3, 603, dtype=np.int64)
    for tol in (0, 1, None):
        exp = check_all_forms(lon, ron, direction, exact, tol, what="ns")
        if tol == 0:
            # only the even offsets inside the right side can match
            want = exact & ((lon - base) % 2 == 0) & (lon >= base) \
                & (lon <= ron[-1])
            assert np.array_equal(exp >= 0, want)


def test_exact_unsigned_distance():
    """Distances that overflow a signed subtraction: the restatement works
    in Python ints (pandas' own subtraction wraps here)."""
    hi = np.array([I64_MAX - 1], dtype=np.int64)
    lo = np.array([I64_MIN + 2], dtype=np.int64)
    for lon, ron, direction in ((hi, lo, 0), (lo, hi, 1), (hi, lo, 2),
                                (lo, hi, 2)):
        for tol, want in ((None, 0), (10, -1), (int(I64_MAX), -1)):
            exp = asof_ref.asof_idx_arrays(lon, None, ron, None, direction,
                                           True, tol)
            assert exp[0] == want
            check_all_forms(lon, ron, direction, True, tol, exp=exp)
    # nearest picks by the true distances: 2^63 + 1 back against 2^63 - 5
    # forward goes forward; a signed difference would see a negative one
    lon = np.array([3], dtype=np.int64)
    ron = np.array([I64_MIN + 2, I64_MAX - 1], dtype=np.int64)
    exp = asof_ref.asof_idx_arrays(lon, None, ron, None, 2, True, None)
    assert exp[0] == 1
    check_all_forms(lon, ron, 2, True, None, exp=exp)


def test_exact_signed_zero():
    ron = np.array([-1.0, -0.0, 0.0, 1.0])
    lon = np.array([-0.0, 0.0])
    for (direction, exact), want in zip(COMBOS, (2, 0, 1, 3, 2, 0)):
        exp = check_all_forms(lon, ron, direction, exact, 1.0)
        assert (exp == want).all(), (direction, exact, exp)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_gather_fill(n):
    rng = np.random.default_rng(n)
    for src, fill in ((rng.normal(size=97), np.nan),
                      (rng.integers(-9, 9, 97).astype(np.int64), -1),
                      (rng.integers(-9, 9, 97).astype(np.int64), I64_MIN)):
        for idx in (rng.integers(-1, 97, n).astype(np.int64),
                    np.full(n, -1, dtype=np.int64),
                    rng.integers(-5, 0, n).astype(np.int64)):
            got = lib.get(lib.gather_fill(lib.put(src), lib.put(idx), fill))
            exp = asof_ref.gather_fill_arrays(src, idx, fill)
            assert got.dtype == src.dtype
            assert np.array_equal(got, exp, equal_nan=src.dtype.kind == "f")
    # an empty source is fine while no index points into it
    got = lib.get(lib.gather_fill(lib.put(np.empty(0)),
                                  lib.put(np.full(n, -1, dtype=np.int64)),
                                  np.nan))
    assert got.shape == (n,) and np.isnan(got).all()


def test_err_arg():
    i8 = lib.put(np.arange(5, dtype=np.int64))
    f8 = lib.put(np.arange(5, dtype=np.float64))
    i8b = lib.put(np.arange(4, dtype=np.int64))
    for args in ((i8, None, f8, None, 0),            # mixed on dtypes
                 (i8, i8, i8, None, 0),              # by on one side
                 (i8, None, i8, i8, 0),
                 (i8, f8, i8, i8, 0),                # by dtype
                 (i8, i8, i8, f8, 0),
                 (i8, i8b, i8, i8, 0),               # by length
                 (i8, i8, i8, i8b, 0),
                 (i8, None, i8, None, 3),            # direction
                 (i8, None, i8, None, -1)):
        with pytest.raises(HfError, match="hf_asof_idx"):
            lib.asof_idx(*args)
    with pytest.raises(HfError, match="tolerance"):
        lib.asof_idx(i8, None, i8, None, 0, True, -1)
    with pytest.raises(HfError, match="tolerance"):
        lib.asof_idx(f8, None, f8, None, 0, True, -0.5)
    dll = lib.load()
    out = ct.c_void_p()
    for lon, ron, slot in ((None, i8.handle, ct.byref(out)),
                           (i8.handle, None, ct.byref(out)),
                           (i8.handle, i8.handle, None)):
        rc = dll.hf_asof_idx(lon, None, ron, None, 0, 1, 0, 0, 0.0, slot)
        assert rc != 0 and out.value is None
    with pytest.raises(HfError, match="hf_gather_fill"):
        lib.gather_fill(i8, f8, 0)                   # index must be int64
    for col, idx, slot in ((None, i8.handle, ct.byref(out)),
                           (i8.handle, None, ct.byref(out)),
                           (i8.handle, i8.handle, None)):
        assert dll.hf_gather_fill(col, idx, 0.0, 0, slot) != 0
    # nothing above left a column behind in a caller's slot
    assert out.value is None


def test_device_blocks_balance():
    """Each call hands out exactly its output column; a rejected call hands
    out nothing; dropping the outputs returns to the starting count."""
    import gc
    a = lib.put(np.arange(3000, dtype=np.int64))
    z = lib.put(np.zeros(3000, dtype=np.int64))
    f8 = lib.put(np.zeros(3000))
    gc.collect()
    base = lib.dev_live()
    pos = lib.asof_idx(a, None, a, None, 2, True, 1)
    assert lib.dev_live() == base + 1
    pos_by = lib.asof_idx(a, z, a, z, 0)
    out = lib.gather_fill(f8, pos, np.nan)
    assert lib.dev_live() == base + 3
    for bad in (lambda: lib.asof_idx(a, None, f8, None, 0),
                lambda: lib.asof_idx(a, None, a, None, 0, True, -1),
                lambda: lib.gather_fill(a, f8, 0)):
        with pytest.raises(HfError):
            bad()
        assert lib.dev_live() == base + 3
    del pos, pos_by, out
    gc.collect()
    assert lib.dev_live() == base


def test_kernel_stats_names():
    lib.profiling(True)
    try:
        lib.kernel_stats_reset()
        a = lib.put(np.arange(10, dtype=np.int64))
        lib.gather_fill(a, lib.asof_idx(a, None, a, None, 0), -1)
        assert lib.kernel_stats("asof_idx")[0] == 1
        assert lib.kernel_stats("gather_fill")[0] == 1
    finally:
        lib.profiling(False)


# ---- API level, against pandas ----

def check(left, right, **kw):
    exp = pandas.merge_asof(left, right, **kw)
    got = mpd.merge_asof(mpd.DataFrame(left), mpd.DataFrame(right),
                         **kw).to_pandas()
    pandas.testing.assert_frame_equal(got, exp, check_exact=True)
    assert isinstance(got.index, pandas.RangeIndex)
    return got


def test_api_scenarios(npartitions):
    rng = np.random.default_rng(21)
    left, right = trades_quotes(rng)
    for direction in DIRECTIONS:
        for exact in (True, False):
            check(left, right, on="t", direction=direction,
                  allow_exact_matches=exact)
    check(left, right, on="t", tolerance=0)
    check(left, right, on="t", tolerance=2, direction="nearest")
    check(left.iloc[:0], right, on="t")
    check(left, right.iloc[:0], on="t")
    check(left.assign(t=left["t"] - 1000), right, on="t")
    check(left.assign(t=left["t"] + 1000), right, on="t",
          direction="forward")
    for kind in ("int", "float", "str"):
        bl, br = by_frames(rng, kind)
        check(bl, br, on="t", by="k", direction="nearest")
    bl, br = by_frames(rng, "str")
    bl["j"] = rng.integers(0, 3, len(bl)).astype(np.int64)
    br["j"] = rng.integers(0, 3, len(br)).astype(np.int64)
    check(bl, br, on="t", by=["k", "j"])
    bl, br = by_frames(rng, "int")
    br = br.rename(columns={"t": "rt", "k": "rk"})
    br["rt"] += 2
    got = check(bl, br, left_on="t", right_on="rt", left_by="k",
                right_by="rk")
    assert got["rt"].dtype == np.float64 and got["rt"].isna().any()
    dl, dr = dt_frames(rng)
    check(dl, dr, on="time", tolerance=pandas.Timedelta("20ms"))
    dl["s"] = rng.choice(np.array(["p", "q", None], dtype=object), len(dl))
    dr["s"] = rng.choice(np.array(["q", "r", None], dtype=object), len(dr))
    dr["stamp"] = dr["time"] + pandas.Timedelta("1s")
    dr["time"] += pandas.Timedelta("1s")
    got = check(dl, dr, on="time", suffixes=("_l", "_r"))
    assert got["stamp"].isna().any() and got["s_r"].isna().any()
    fl = pandas.DataFrame({"x": np.sort(rng.normal(size=90))})
    fr = pandas.DataFrame({"x": np.sort(rng.normal(size=70)),
                           "b": np.arange(70, dtype=np.int64)})
    check(fl, fr, on="x", tolerance=0.05, direction="nearest")


def test_api_dtype_rule_and_rejections(npartitions):
    n = 60
    left = pandas.DataFrame({"t": np.arange(n, dtype=np.int64) + 5})
    right = pandas.DataFrame({"t": np.arange(0, n + 5, 3, dtype=np.int64),
                              "rv": np.arange(22, dtype=np.int64)})
    assert check(left, right, on="t")["rv"].dtype == np.int64
    left.loc[0, "t"] = -1
    assert check(left, right, on="t")["rv"].dtype == np.float64
    # unsorted and null keys are rejected before any search runs
    L, R = mpd.DataFrame(left.iloc[::-1]), mpd.DataFrame(right)
    with pytest.raises(ValueError, match="left keys must be sorted"):
        mpd.merge_asof(L, R, on="t")
    with pytest.raises(ValueError, match="right keys must be sorted"):
        mpd.merge_asof(mpd.DataFrame(left), mpd.DataFrame(right.iloc[::-1]),
                       on="t")
    lf = left.astype({"t": np.float64})
    rf = right.astype({"t": np.float64})
    lf.loc[9, "t"] = np.nan
    with pytest.raises(ValueError, match="null values on left side"):
        mpd.merge_asof(mpd.DataFrame(lf), mpd.DataFrame(rf), on="t")


@pytest.mark.parametrize("seed", range(20))
def test_api_fuzz(npartitions, seed):
    left, right, kw = fuzz_case(seed)
    check(left, right, **kw)


def test_api_trades_and_quotes(npartitions):
    """70 001 trades x 9 973 quotes, 37 tickers, datetime `on`: many tiles
    and partitions, every direction."""
    rng = np.random.default_rng(31)
    nl, nr = 70_001, 9_973
    tickers = np.array([f"T{i:02d}" for i in range(37)], dtype=object)
    base = np.datetime64("2024-06-03T13:30:00", "ns").astype(np.int64)
    day = 6 * 3600 * 10**9 + 30 * 60 * 10**9
    lt = np.sort(base + rng.integers(0, day, nl))
    rt = np.sort(base + rng.integers(0, day, nr))
    left = pandas.DataFrame({"time": lt.view("datetime64[ns]"),
                             "ticker": rng.choice(tickers, nl),
                             "qty": rng.integers(1, 500, nl)
                             .astype(np.int64)})
    right = pandas.DataFrame({"time": rt.view("datetime64[ns]"),
                              "ticker": rng.choice(tickers[:35], nr),
                              "bid": rng.normal(100, 5, nr),
                              "seq": np.arange(nr, dtype=np.int64)})
    for direction in DIRECTIONS:
        check(left, right, on="time", by="ticker", direction=direction)
    check(left, right, on="time", by="ticker",
          tolerance=pandas.Timedelta("30s"))
    check(left, right, on="time", direction="nearest")
