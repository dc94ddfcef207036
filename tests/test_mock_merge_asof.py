"""CPU tier: merge_asof through the REAL composition layer
(modin_amd/pandas, the query compiler, HipDataframe.asof_join) over the numpy
lib mock, at NPartitions 1 and 3, bit-exact against pandas.

tests/mocklib.py stands in for the existing kernels; the two new entry points
hf_asof_idx and hf_gather_fill are restated in tests/asof_ref.py from their
header comments — the as-of match as a linear scan per left row, not the
bound search the device runs.
"""

import numpy as np
import pandas
import pytest
from pandas.errors import MergeError

from tests import asof_ref, mocklib
from modin_amd import config
from modin_amd.core import lib as _lib
from modin_amd.core.lib import HfError


def np_asof_idx(lon, lby, ron, rby, direction, allow_exact=True,
                tolerance=None):
    if (lby is None) != (rby is None) or lon.arr.dtype != ron.arr.dtype \
            or direction not in (0, 1, 2) \
            or (tolerance is not None and tolerance < 0):
        raise HfError("hf_asof_idx failed: bad argument")
    return mocklib.MockCol(asof_ref.asof_idx_arrays(
        lon.arr, None if lby is None else lby.arr, ron.arr,
        None if rby is None else rby.arr, direction, allow_exact, tolerance))


def np_gather_fill(col, idx, fill):
    return mocklib.MockCol(asof_ref.gather_fill_arrays(col.arr, idx.arr,
                                                       fill))


@pytest.fixture(params=[1, 3])
def mpd(request, monkeypatch):
    mocklib.install(monkeypatch)
    monkeypatch.setattr(_lib, "asof_idx", np_asof_idx)
    monkeypatch.setattr(_lib, "gather_fill", np_gather_fill)
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(request.param)
    config.MinRowPartitionSize.put(4)
    import modin_amd.pandas as mpd_
    yield mpd_
    config.NPartitions.put(old[0])
    config.MinRowPartitionSize.put(old[1])


def check(mpd, left, right, **kw):
    exp = pandas.merge_asof(left, right, **kw)
    got = mpd.merge_asof(mpd.DataFrame(left), mpd.DataFrame(right),
                         **kw).to_pandas()
    pandas.testing.assert_frame_equal(got, exp, check_exact=True)
    assert isinstance(got.index, pandas.RangeIndex)
    return got


def trades_quotes(rng, nl=120, nr=90, hi=60):
    """int64 `on` with duplicates on both sides, an int64 payload each."""
    left = pandas.DataFrame({
        "t": np.sort(rng.integers(0, hi, nl)).astype(np.int64),
        "lv": rng.integers(-50, 50, nl).astype(np.int64)})
    right = pandas.DataFrame({
        "t": np.sort(rng.integers(0, hi, nr)).astype(np.int64),
        "rv": np.arange(nr, dtype=np.int64),
        "rf": rng.normal(size=nr)})
    return left, right


DIRECTIONS = ["backward", "forward", "nearest"]


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("exact", [True, False])
def test_directions_exact(mpd, direction, exact):
    left, right = trades_quotes(np.random.default_rng(1))
    check(mpd, left, right, on="t", direction=direction,
          allow_exact_matches=exact)


def by_frames(rng, kind, nl=150, nr=110):
    left, right = trades_quotes(rng, nl, nr)
    if kind == "int":
        lk = rng.integers(-3, 4, nl).astype(np.int64)
        rk = rng.integers(-2, 6, nr).astype(np.int64)
    elif kind == "float":
        lk = rng.integers(0, 5, nl).astype(np.float64) / 2
        rk = rng.integers(0, 6, nr).astype(np.float64) / 2
        lk[rng.random(nl) < 0.15] = np.nan
        rk[rng.random(nr) < 0.15] = np.nan
    else:
        lk = rng.choice(np.array(["aa", "b", "cc", None], dtype=object), nl)
        rk = rng.choice(np.array(["b", "cc", "zz", None], dtype=object), nr)
    left["k"], right["k"] = lk, rk
    return left, right


@pytest.mark.parametrize("kind", ["int", "float", "str"])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_by_kinds(mpd, kind, direction):
    left, right = by_frames(np.random.default_rng(2), kind)
    check(mpd, left, right, on="t", by="k", direction=direction)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_by_two_columns(mpd, direction):
    rng = np.random.default_rng(3)
    left, right = by_frames(rng, "str")
    left["j"] = rng.integers(0, 3, len(left)).astype(np.int64)
    right["j"] = rng.integers(0, 3, len(right)).astype(np.int64)
    check(mpd, left, right, on="t", by=["k", "j"], direction=direction)


def test_left_right_names_differ(mpd):
    rng = np.random.default_rng(4)
    left, right = by_frames(rng, "int")
    right = right.rename(columns={"t": "rt", "k": "rk"})
    right["rt"] += 2   # every left row before t=2 is unmatched
    got = check(mpd, left, right, left_on="t", right_on="rt", left_by="k",
                right_by="rk")
    # the kept right key columns are payload: NaN / float64 where unmatched
    assert got["rt"].dtype == np.float64 and got["rt"].isna().any()
    assert got["rk"].dtype == np.float64


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("tol", [0, 1, 3])
def test_tolerance_int(mpd, direction, tol):
    left, right = trades_quotes(np.random.default_rng(5), hi=200)
    check(mpd, left, right, on="t", tolerance=tol, direction=direction)
    check(mpd, left, right, on="t", tolerance=np.int64(tol),
          direction=direction, allow_exact_matches=False)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_tolerance_float(mpd, direction):
    rng = np.random.default_rng(6)
    left = pandas.DataFrame({"x": np.sort(rng.normal(size=90)),
                             "a": np.arange(90, dtype=np.int64)})
    right = pandas.DataFrame({"x": np.sort(rng.normal(size=70)),
                              "b": np.arange(70, dtype=np.int64)})
    right.loc[10:14, "x"] = left["x"].to_numpy()[20]   # exact hits, dups
    right = right.sort_values("x", ignore_index=True)
    check(mpd, left, right, on="x", tolerance=0.05, direction=direction)
    check(mpd, left, right, on="x", tolerance=1, direction=direction)
    check(mpd, left, right, on="x", direction=direction,
          allow_exact_matches=False)


def dt_frames(rng, nl=130, nr=100):
    base = np.datetime64("2024-03-01T09:30:00", "ns").astype(np.int64)
    lt = np.sort(base + rng.integers(0, 5_000, nl) * 1_000_000)
    rt = np.sort(base + rng.integers(0, 5_000, nr) * 1_000_000)
    left = pandas.DataFrame({"time": lt.view("datetime64[ns]"),
                             "px": rng.normal(size=nl)})
    right = pandas.DataFrame({"time": rt.view("datetime64[ns]"),
                              "bid": rng.normal(size=nr),
                              "n": np.arange(nr, dtype=np.int64)})
    return left, right


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_tolerance_timedelta(mpd, direction):
    left, right = dt_frames(np.random.default_rng(7))
    check(mpd, left, right, on="time", direction=direction,
          tolerance=pandas.Timedelta("20ms"))
    check(mpd, left, right, on="time", direction=direction)


def test_dtype_rule_across_partitions(mpd):
    n = 60
    left = pandas.DataFrame({"t": np.arange(n, dtype=np.int64) + 5})
    right = pandas.DataFrame({"t": np.arange(0, n + 5, 3, dtype=np.int64),
                              "rv": np.arange(22, dtype=np.int64)})
    got = check(mpd, left, right, on="t")
    assert got["rv"].dtype == np.int64          # all matched: stays int64
    # ONE unmatched row, the first — with 3 partitions the other two have
    # none, and the whole column is float64 all the same
    left2 = left.copy()
    left2.loc[0, "t"] = -1
    got = check(mpd, left2, right, on="t")
    assert got["rv"].dtype == np.float64 and got["rv"].isna().sum() == 1


def test_suffixes_and_payload_kinds(mpd):
    rng = np.random.default_rng(8)
    left, right = dt_frames(rng)
    left["v"] = rng.normal(size=len(left))
    left["s"] = rng.choice(np.array(["p", "q", None], dtype=object),
                           len(left))
    right["v"] = rng.normal(size=len(right))
    right["s"] = rng.choice(np.array(["q", "r", None], dtype=object),
                            len(right))
    right["stamp"] = right["time"] + pandas.Timedelta("1s")
    right["time"] += pandas.Timedelta("1s")   # early left rows: unmatched
    got = check(mpd, left, right, on="time", suffixes=("_l", "_r"))
    assert got["stamp"].isna().any() and got["s_r"].isna().any()
    check(mpd, left, right, on="time", suffixes=("", "_r"),
          direction="forward")


def test_empty_sides(mpd):
    left, right = trades_quotes(np.random.default_rng(9))
    for kw in (dict(on="t"), dict(on="t", direction="nearest")):
        check(mpd, left.iloc[:0], right, **kw)
        check(mpd, left, right.iloc[:0], **kw)
    left["k"] = np.int64(1)
    right["k"] = np.int64(1)
    check(mpd, left.iloc[:0], right, on="t", by="k")
    check(mpd, left, right.iloc[:0], on="t", by="k")


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_all_before_all_after(mpd, direction):
    left, right = trades_quotes(np.random.default_rng(10))
    before = left.assign(t=left["t"] - 1000)
    after = left.assign(t=left["t"] + 1000)
    check(mpd, before, right, on="t", direction=direction)
    check(mpd, after, right, on="t", direction=direction)


def test_non_range_left_index(mpd):
    left, right = trades_quotes(np.random.default_rng(11))
    left.index = pandas.Index(np.arange(len(left))[::-1] * 7, name="ix")
    got = check(mpd, left, right, on="t")
    assert got.index.equals(pandas.RangeIndex(len(left)))


# ---- errors: pandas' type and message ----

def raises_like_pandas(mpd, left, right, **kw):
    with pytest.raises(Exception) as exp:
        pandas.merge_asof(left, right, **kw)
    with pytest.raises(type(exp.value)) as got:
        mpd.merge_asof(mpd.DataFrame(left), mpd.DataFrame(right), **kw)
    assert type(got.value) is type(exp.value)
    assert str(got.value) == str(exp.value)
    return got.value


def test_errors_unsorted_and_null(mpd):
    left, right = trades_quotes(np.random.default_rng(12))
    e = raises_like_pandas(mpd, left.iloc[::-1], right, on="t")
    assert str(e) == "left keys must be sorted"
    e = raises_like_pandas(mpd, left, right.iloc[::-1], on="t")
    assert str(e) == "right keys must be sorted"
    # one descent right at a partition boundary
    bad = left.copy()
    bad.loc[len(bad) // 3, "t"] = -5
    raises_like_pandas(mpd, bad, right, on="t")
    lf = left.assign(t=left["t"].astype(np.float64))
    rf = right.assign(t=right["t"].astype(np.float64))
    ln, rn = lf.copy(), rf.copy()
    ln.loc[7, "t"] = np.nan
    rn.loc[len(rn) - 1, "t"] = np.nan
    e = raises_like_pandas(mpd, ln, rf, on="t")
    assert str(e) == "Merge keys contain null values on left side"
    e = raises_like_pandas(mpd, lf, rn, on="t")
    assert str(e) == "Merge keys contain null values on right side"
    dl, dr = dt_frames(np.random.default_rng(13))
    dl.loc[3, "time"] = pandas.NaT
    e = raises_like_pandas(mpd, dl, dr, on="time")
    assert str(e) == "Merge keys contain null values on left side"


def test_errors_arguments(mpd):
    left, right = trades_quotes(np.random.default_rng(14))
    e = raises_like_pandas(mpd, left, right, on="t", tolerance=-1)
    assert isinstance(e, MergeError)
    e = raises_like_pandas(mpd, left, right, on="t", tolerance=1.5)
    assert isinstance(e, MergeError)
    e = raises_like_pandas(mpd, left, right, on="t", direction="sideways")
    assert isinstance(e, MergeError)
    rf = right.assign(t=right["t"].astype(np.float64))
    e = raises_like_pandas(mpd, left, rf, on="t")
    assert isinstance(e, MergeError)
    l2, r2 = left.assign(u=left["t"]), right.assign(u=right["t"])
    e = raises_like_pandas(mpd, l2, r2, on=["t", "u"])
    assert isinstance(e, MergeError)
    dl, dr = dt_frames(np.random.default_rng(15))
    raises_like_pandas(mpd, dl, dr, on="time", tolerance=5)
    raises_like_pandas(mpd, dl, dr, on="time",
                       tolerance=pandas.Timedelta("-1ms"))
    ls = left.assign(t=left["t"].astype(str))
    rs = right.assign(t=right["t"].astype(str))
    with pytest.raises(MergeError):
        mpd.merge_asof(mpd.DataFrame(ls), mpd.DataFrame(rs), on="t")
    # argument combinations: ValueErrors of the public function itself,
    # raised before any pandas-shaped check is reached
    L, R = mpd.DataFrame(left), mpd.DataFrame(right)
    for kw, msg in (
            (dict(on="t", left_on="t"), "If 'on' is set"),
            (dict(on="t", right_on="t"), "If 'on' is set"),
            (dict(on="t", by="lv", left_by="lv"), "Can't have both 'by'"),
            (dict(on="t", by="lv", right_by="rv"), "Can't have both 'by'"),
            (dict(), "Must pass on, left_on, or left_index=True"),
            (dict(right_on="t"), "Must pass on, left_on, or left_index=True"),
            (dict(left_on="t"), "Must pass on, right_on, or right_index=True"),
            (dict(on="t", left_index=True), "Can't combine"),
            (dict(on="t", right_index=True), "Can't combine"),
            (dict(left_on="t", left_index=True, right_on="t"),
             "Can't combine"),
            (dict(left_on="t", right_on="t", right_index=True),
             "Can't combine")):
        with pytest.raises(ValueError, match=msg):
            mpd.merge_asof(L, R, **kw)
    with pytest.raises(ValueError, match="can not merge DataFrame"):
        mpd.merge_asof(L, right, on="t")
    # a collision the suffixes do not resolve
    lc = left.assign(rv=1, rv_x=2)
    raises_like_pandas(mpd, lc, right, on="t")


def test_errors_loud_hferror(mpd, monkeypatch):
    left, right = trades_quotes(np.random.default_rng(16))
    L, R = mpd.DataFrame(left), mpd.DataFrame(right)
    with pytest.raises(HfError, match="left_index"):
        mpd.merge_asof(L, R, left_index=True, right_on="t")
    with pytest.raises(HfError, match="right_index"):
        mpd.merge_asof(L, R, left_on="t", right_index=True)
    with pytest.raises(HfError, match="no column 'nope'"):
        mpd.merge_asof(L, R, left_on="nope", right_on="t")
    with pytest.raises(HfError, match="no column 'nope'"):
        mpd.merge_asof(L, R, on="t", left_by="nope", right_by="rv")
    from modin_amd import distributed
    monkeypatch.setattr(distributed, "is_active", lambda: True)
    with pytest.raises(HfError, match="world>1 is a later round"):
        mpd.merge_asof(L, R, on="t")


# ---- fuzz ----

def fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    nl, nr = int(rng.integers(0, 301)), int(rng.integers(0, 301))
    kind = ["int", "float", "dt"][seed % 3]
    hi = int(rng.integers(5, 400))
    lt = np.sort(rng.integers(0, hi, nl)).astype(np.int64)
    rt = np.sort(rng.integers(0, hi, nr)).astype(np.int64)
    tol = None
    if kind == "float":
        lt, rt = lt / 4.0, rt / 4.0
        if rng.random() < 0.6:
            tol = float(rng.integers(0, 12)) / 4.0
    elif kind == "dt":
        base = np.datetime64("2025-01-01", "ns").astype(np.int64)
        lt = (base + lt * 1000).view("datetime64[ns]")
        rt = (base + rt * 1000).view("datetime64[ns]")
        if rng.random() < 0.6:
            tol = pandas.Timedelta(int(rng.integers(0, 12)) * 1000, "ns")
    elif rng.random() < 0.6:
        tol = int(rng.integers(0, 12))
    left = pandas.DataFrame({"t": lt,
                             "lv": rng.integers(0, 9, nl).astype(np.int64)})
    right = pandas.DataFrame({"t": rt, "rv": np.arange(nr, dtype=np.int64),
                              "rs": rng.choice(np.array(["u", "v", None],
                                                        dtype=object), nr)})
    by = []
    for j in range(int(rng.integers(0, 4))):
        name = f"b{j}"
        bkind = int(rng.integers(0, 4))
        for frame, n in ((left, nl), (right, nr)):
            miss = rng.random(n) < 0.15
            if bkind == 0:
                col = rng.integers(-2, 3, n).astype(np.int64)
            elif bkind == 1:
                col = rng.integers(0, 4, n).astype(np.float64) * 0.5
                col[miss] = np.nan
            elif bkind == 2:
                col = rng.choice(np.array(["x", "yy", "z"], dtype=object), n)
                col[miss] = None
            else:
                col = (np.datetime64("2020-01-01", "ns")
                       + rng.integers(0, 3, n).astype("timedelta64[D]")
                       ).astype("datetime64[ns]")
                col[miss] = np.datetime64("NaT")
            frame[name] = col
        by.append(name)
    kw = dict(on="t", direction=DIRECTIONS[int(rng.integers(0, 3))],
              allow_exact_matches=bool(rng.integers(0, 2)))
    if tol is not None:
        kw["tolerance"] = tol
    if by:
        kw["by"] = by if len(by) > 1 or rng.random() < 0.5 else by[0]
    return left, right, kw


@pytest.mark.parametrize("seed", range(60))
def test_fuzz(mpd, seed):
    left, right, kw = fuzz_case(seed)
    check(mpd, left, right, **kw)
