"""GPU tier: hf_ewm_mean (the chained weight/mean recurrence scan) and the
ewm API above it, against pandas ewm(...).mean().

Tolerance: NaN positions identical; values within 1e-12 * max(1, max|x|).
The bound is not tuned on the kernel: a numpy restatement of the tiled
algorithm measured 9.6e-16 worst scaled error against pandas 2.3.3 over 400
random cases (3.5e-16 on the underflow-gap case), which leaves about three
decades for FMA contraction and the 4096-row tiles.
"""

import numpy as np
import pandas
import pytest

import modin_amd.pandas as mpd
from modin_amd import config
from modin_amd.core import lib
from modin_amd.core.lib import HfError

pytestmark = pytest.mark.gpu

TILE = 4096


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = config.NPartitions.get()
    config.NPartitions.put(request.param)
    yield request.param
    config.NPartitions.put(old)


def _close(got, exp, x, what):
    assert got.dtype == np.float64 and got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    mag = np.abs(x[np.isfinite(x)])
    scale = max(1.0, float(mag.max())) if mag.size else 1.0
    diff = np.abs(got - exp)
    diff = diff[~np.isnan(diff)]
    err = float(diff.max()) if diff.size else 0.0
    assert err <= 1e-12 * scale, (what, err, scale)
    return err / scale


def _values(rng, n, nan_share):
    x = rng.normal(3.0, 2.0, n)
    if nan_share:
        x[rng.random(n) < nan_share] = np.nan
    return x


FLAGS = [(alpha, adjust, ignore_na, minp)
         for alpha in (0.01, 0.3, 1.0)
         for adjust in (True, False)
         for ignore_na in (True, False)
         for minp in (0, 3)]


# 16 rows is one thread's run, 4096 one tile; 1024 * 4096 + 4097 is the
# smallest count that crosses the 1024-tile iteration of the one-block tile
# scan, where the carry between iterations can go wrong
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097,
                               3 * TILE + 5, 1024 * TILE + 4097])
def test_kernel_vs_pandas(n):
    rng = np.random.default_rng(n)
    worst = 0.0
    for nan_share in (0.0, 0.1, 0.97):
        x = _values(rng, n, nan_share)
        col = lib.put(x)
        s = pandas.Series(x)
        for alpha, adjust, ignore_na, minp in FLAGS:
            got = lib.get(lib.ewm_mean(col, None, alpha, adjust, ignore_na,
                                       minp))
            exp = s.ewm(alpha=alpha, adjust=adjust, ignore_na=ignore_na,
                        min_periods=minp).mean().to_numpy()
            worst = max(worst, _close(
                got, exp, x, (n, nan_share, alpha, adjust, ignore_na, minp)))
    print(f"ewm n={n}: worst scaled error {worst:.3g}")


def _both_adjust(x, col, heads=None, seg=None, alpha=0.3, minp=0, what=""):
    s = pandas.Series(x)
    for adjust in (True, False):
        for ignore_na in (True, False):
            kw = dict(alpha=alpha, adjust=adjust, ignore_na=ignore_na,
                      min_periods=minp)
            got = lib.get(lib.ewm_mean(col, heads, alpha, adjust, ignore_na,
                                       minp))
            if seg is None:
                exp = s.ewm(**kw).mean().to_numpy()
            else:
                exp = s.groupby(seg).ewm(**kw).mean().to_numpy()
            _close(got, exp, x.astype(np.float64), (what, kw))


def test_placed_nans():
    rng = np.random.default_rng(11)
    n = 3 * TILE + 5
    x = _values(rng, n, 0.0)
    x[[TILE - 1, TILE]] = np.nan
    _both_adjust(x, lib.put(x), what="nan at 4095/4096")
    x = _values(rng, n, 0.05)
    x[:TILE + 3] = np.nan
    for minp in (0, 3):
        _both_adjust(x, lib.put(x), minp=minp, what="leading nan tile")


def test_underflow_gap_carries_the_mean_forward():
    """alpha = 0.9 and a 2000-row NaN gap: 0.1**2000 underflows to zero, so
    a numerator/denominator scan divides 0 by 0 after the gap where pandas
    restarts from the next value."""
    rng = np.random.default_rng(12)
    n = 2 * TILE
    x = 1e6 + rng.normal(0.0, 1.0, n)
    x[3000:5000] = np.nan
    col = lib.put(x)
    s = pandas.Series(x)
    for adjust in (True, False):
        for ignore_na in (True, False):
            got = lib.get(lib.ewm_mean(col, None, 0.9, adjust, ignore_na, 0))
            exp = s.ewm(alpha=0.9, adjust=adjust,
                        ignore_na=ignore_na).mean().to_numpy()
            assert np.array_equal(np.isnan(got), np.isnan(exp))
            assert not np.isnan(got).any()
            err = _close(got, exp, x, ("underflow", adjust, ignore_na))
            print(f"underflow gap adjust={adjust} ignore_na={ignore_na}: "
                  f"scaled error {err:.3g}")


def test_int64_column():
    rng = np.random.default_rng(13)
    x = rng.integers(-1000, 1000, 2 * TILE + 77).astype(np.int64)
    col = lib.put(x)
    out = lib.ewm_mean(col, None, 0.3, True, False, 0)
    assert out.np_dtype == np.float64
    _both_adjust(x, col, minp=3, what="int64")
    seg = np.arange(x.size) // 1000
    heads = np.r_[1, np.diff(seg)].astype(np.int64)
    _both_adjust(x, col, lib.put(heads), seg, what="int64 segments")


def test_conditioning_small_alpha_large_offset():
    """Long memory over a large offset.  A numpy restatement of the tiled
    algorithm measured 5.1e-14 relative here; the MI355X measures 2.06e-14
    (DESIGN.md)."""
    rng = np.random.default_rng(14)
    x = 1e6 + rng.normal(0.0, 1.0, 100_000)
    got = lib.get(lib.ewm_mean(lib.put(x), None, 0.001, True, False, 0))
    exp = pandas.Series(x).ewm(alpha=0.001).mean().to_numpy()
    rel = float(np.max(np.abs(got - exp) / np.abs(exp)))
    print(f"ewm conditioning alpha=0.001 offset 1e6: relative {rel:.3g}")
    assert rel <= 1e-12


def _segment_case(x, heads, what):
    assert heads.dtype == np.int64
    # a head at row 0 or not, row 0 opens the first segment either way
    seg = np.cumsum(heads)
    _both_adjust(x, lib.put(x), lib.put(heads), seg, what=what)
    _both_adjust(x, lib.put(x), lib.put(heads), seg, alpha=1.0, minp=3,
                 what=what)


def test_segments_placed_heads():
    rng = np.random.default_rng(15)
    n = 3 * TILE + 5
    x = _values(rng, n, 0.1)
    for rows in ([0], [1], [TILE - 1], [TILE], [TILE + 1],
                 [0, 1, TILE - 1, TILE, TILE + 1]):
        heads = np.zeros(n, dtype=np.int64)
        heads[rows] = 1
        _segment_case(x, heads, ("heads at", rows))


@pytest.mark.parametrize("run,n", [(3, 3 * TILE + 5), (5000, 12 * TILE + 9)])
def test_segments_random_heads(run, n):
    rng = np.random.default_rng(run)
    for nan_share in (0.1, 0.97):
        x = _values(rng, n, nan_share)
        heads = (rng.random(n) < 1.0 / run).astype(np.int64)
        _segment_case(x, heads, ("random heads", run, nan_share))


def test_segment_head_on_nan_row():
    rng = np.random.default_rng(16)
    n = 2 * TILE + 3
    x = _values(rng, n, 0.0)
    heads = np.zeros(n, dtype=np.int64)
    for r in (5, 100, TILE, TILE + 40):
        heads[r] = 1
        x[r] = np.nan
    x[101:104] = np.nan   # the segment stays empty for three more rows
    _segment_case(x, heads, "head on nan")
    got = lib.get(lib.ewm_mean(lib.put(x), lib.put(heads), 0.3, True,
                               False, 0))
    assert np.isnan(got[[5, 100, 101, 102, 103, TILE, TILE + 40]]).all()
    assert not np.isnan(got[[4, 6, 99, 104, TILE - 1, TILE + 1]]).any()


def test_argument_errors():
    col = lib.put(np.arange(10.0))
    for alpha in (0.0, 1.5):
        with pytest.raises(HfError, match=r"rc=2"):
            lib.ewm_mean(col, None, alpha, True, False, 0)
    with pytest.raises(HfError, match=r"rc=2"):
        lib.ewm_mean(col, lib.put(np.ones(9, dtype=np.int64)), 0.5, True,
                     False, 0)
    empty = lib.ewm_mean(lib.put(np.empty(0)), None, 0.5, True, False, 0)
    assert empty.length == 0 and empty.np_dtype == np.float64


# ---- API level -------------------------------------------------------------

def _check_api(got, exp):
    assert type(got) is type(exp)
    if isinstance(exp, pandas.Series):
        assert got.name == exp.name
        got, exp = got.to_frame("x"), exp.to_frame("x")
    assert list(got.columns) == list(exp.columns)
    assert got.index.names == exp.index.names
    assert got.index.nlevels == exp.index.nlevels
    for lv in range(exp.index.nlevels):
        g, e = got.index.get_level_values(lv), exp.index.get_level_values(lv)
        assert g.dtype == e.dtype and g.equals(e), lv
    for c in exp.columns:
        assert got[c].dtype == exp[c].dtype == np.float64, c
        _close(got[c].to_numpy(), exp[c].to_numpy(), exp[c].to_numpy(), c)


@pytest.fixture(scope="module")
def api_frame():
    rng = np.random.default_rng(17)
    n = 10_000
    v = _values(rng, n, 0.1)
    w = rng.integers(-50, 50, n).astype(np.int64)
    gid = rng.integers(0, 37, n)
    fk = gid.astype(np.float64) / 4
    fk[rng.random(n) < 0.05] = np.nan
    return pandas.DataFrame({
        "k": gid.astype(np.int64), "fk": fk,
        "sk": np.array([f"g{i:02d}" for i in gid], dtype=object),
        "a": (gid % 5).astype(np.int64), "b": (gid // 5).astype(np.int64),
        "v": v, "w": w})


def test_api_frame_and_series(npartitions, api_frame):
    pdf = api_frame[["v", "w"]]
    df = mpd.DataFrame(pdf)
    _check_api(df.ewm(span=5).mean().to_pandas(), pdf.ewm(span=5).mean())
    kw = dict(halflife=2, adjust=False, ignore_na=True, min_periods=2)
    _check_api(df["v"].ewm(**kw).mean().to_pandas(),
               pdf["v"].ewm(**kw).mean())


@pytest.mark.parametrize("by", ["k", "fk", "sk", ["a", "b"]], ids=str)
def test_api_groupby(npartitions, api_frame, by):
    keys = [by] if isinstance(by, str) else by
    pdf = api_frame[[*keys, "v", "w"]]
    df = mpd.DataFrame(pdf)
    _check_api(df.groupby(by).ewm(alpha=.5).mean().to_pandas(),
               pdf.groupby(by).ewm(alpha=.5).mean())
    _check_api(df.groupby(by)["v"].ewm(alpha=.5).mean().to_pandas(),
               pdf.groupby(by)["v"].ewm(alpha=.5).mean())
