"""CPU tier: groupby skew/any/all and frame skew/kurt through the REAL
composition layer (modin_amd/core/dataframe.py) over the numpy lib mock.

tests/mocklib.py stands in for the existing kernels; the new
hf_group_moments entry point is restated here in numpy from its header
comment (include/hipframe.h): per row with gid >= 0 and a non-NaN value,
d = x - centre[gid] feeds the rows  Σd, Σd², Σd³, Σd⁴, min x, max x  of a
[6][n_groups] table that the caller initialised to 0,0,0,0,+inf,-inf; a
null gid means group 0; gid >= n_groups is an error.
"""

from fractions import Fraction

import numpy as np
import pandas
import pytest

from tests import mocklib
from modin_amd import config
from modin_amd.core import lib as _lib
from modin_amd.core.lib import HfError


def np_group_moments(gid, val, centre, n_groups, table):
    x = val.arr.astype(np.float64)
    g = (np.zeros(x.size, dtype=np.int64) if gid is None else gid.arr)
    assert centre.arr.size == n_groups and table.arr.size == 6 * n_groups
    if (g >= n_groups).any():
        raise HfError("hf_group_moments failed: gid >= n_groups")
    ok = (g >= 0) & ~np.isnan(x)
    g, x = g[ok], x[ok]
    d = x - centre.arr[g]
    t = table.arr.reshape(6, n_groups)
    for p in range(4):
        t[p] += np.bincount(g, weights=d ** (p + 1), minlength=n_groups)
    np.minimum.at(t[4], g, x)
    np.maximum.at(t[5], g, x)


def np_group_moments_table(n_groups):
    t = np.zeros((6, n_groups))
    t[4] = np.inf
    t[5] = -np.inf
    return mocklib.MockCol(t.reshape(-1))


@pytest.fixture(params=[1, 3])
def mpd(request, monkeypatch):
    mocklib.install(monkeypatch)
    monkeypatch.setattr(_lib, "group_moments", np_group_moments)
    monkeypatch.setattr(_lib, "group_moments_table", np_group_moments_table)
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(request.param)
    config.MinRowPartitionSize.put(4)
    import modin_amd.pandas as mpd_
    yield mpd_
    config.NPartitions.put(old[0])
    config.MinRowPartitionSize.put(old[1])


def _values(rng, n):
    v = rng.gamma(2.0, 1.0, n)
    v[rng.random(n) < 0.1] = np.nan
    w = rng.integers(-3, 4, n).astype(np.int64)
    return v, w


def _check(got, exp, rtol=1e-9):
    assert list(got.columns) == list(exp.columns)
    assert got.index.equals(exp.index) or np.array_equal(
        got.index.to_numpy(), exp.index.to_numpy(), equal_nan=True), \
        (got.index, exp.index)
    for c in exp.columns:
        assert got[c].dtype == exp[c].dtype, (c, got[c].dtype, exp[c].dtype)
        if exp[c].dtype == bool:
            np.testing.assert_array_equal(got[c].to_numpy(),
                                          exp[c].to_numpy(), err_msg=str(c))
        else:
            np.testing.assert_allclose(got[c].to_numpy(), exp[c].to_numpy(),
                                       rtol=rtol, atol=1e-12, equal_nan=True,
                                       err_msg=str(c))


def _keyed(rng, kind, n=600):
    v, w = _values(rng, n)
    if kind == "int":
        k = rng.integers(0, 13, n).astype(np.int64)
    elif kind == "float":
        k = rng.integers(0, 13, n).astype(np.float64) / 2
    else:
        k = np.array([f"s{i:02d}" for i in rng.integers(0, 13, n)],
                     dtype=object)
    return pandas.DataFrame({"k": k, "v": v, "w": w})


@pytest.mark.parametrize("kind", ["int", "float", "str"])
def test_groupby_skew_any_all_vs_pandas(mpd, kind):
    pdf = _keyed(np.random.default_rng(5), kind)
    df = mpd.DataFrame(pdf)
    for how in ("skew", "any", "all"):
        got = getattr(df.groupby("k"), how)().to_pandas()
        exp = getattr(pdf.groupby("k"), how)()
        _check(got, exp)


def test_two_keys(mpd):
    rng = np.random.default_rng(6)
    n = 900
    v, w = _values(rng, n)
    pdf = pandas.DataFrame({
        "a": rng.integers(0, 4, n).astype(np.int64),
        "b": np.array([f"x{i}" for i in rng.integers(0, 3, n)], dtype=object),
        "v": v, "w": w})
    df = mpd.DataFrame(pdf)
    for how in ("skew", "any", "all"):
        got = getattr(df.groupby(["a", "b"]), how)().to_pandas()
        exp = getattr(pdf.groupby(["a", "b"]), how)()
        _check(got, exp)


def test_dropna_false_nan_float_keys(mpd):
    rng = np.random.default_rng(7)
    pdf = _keyed(rng, "float")
    pdf.loc[rng.random(len(pdf)) < 0.1, "k"] = np.nan
    df = mpd.DataFrame(pdf)
    for dropna in (True, False):
        for how in ("skew", "any", "all"):
            got = getattr(df.groupby("k", dropna=dropna), how)().to_pandas()
            exp = getattr(pdf.groupby("k", dropna=dropna), how)()
            _check(got, exp)
    assert np.isnan(df.groupby("k", dropna=False).skew()
                    .to_pandas().index[-1])


def test_as_index_series_and_agg_forms(mpd):
    pdf = _keyed(np.random.default_rng(8), "int")
    df = mpd.DataFrame(pdf)
    got = df.groupby("k", as_index=False).skew().to_pandas()
    exp = pdf.groupby("k", as_index=False).skew()
    _check(got, exp)
    _check(df.groupby("k", as_index=False).all().to_pandas(),
           pdf.groupby("k", as_index=False).all())
    got_s = df.groupby("k")["v"].skew().to_pandas()
    exp_s = pdf.groupby("k")["v"].skew()
    assert got_s.name == "v"
    np.testing.assert_allclose(got_s.to_numpy(), exp_s.to_numpy(),
                               rtol=1e-9, equal_nan=True)
    got_a = df.groupby("k")["w"].any().to_pandas()
    exp_a = pdf.groupby("k")["w"].any()
    assert got_a.dtype == bool
    np.testing.assert_array_equal(got_a.to_numpy(), exp_a.to_numpy())
    got = df.groupby("k").agg(["sum", "skew"]).to_pandas()
    exp = pdf.groupby("k").agg(["sum", "skew"])
    _check(got, exp)
    got = df.groupby("k").agg({"v": "skew", "w": "any"}).to_pandas()
    exp = pdf.groupby("k").agg({"v": "skew", "w": "any"})
    _check(got, exp)
    got = df.groupby("k").agg("all").to_pandas()
    _check(got, pdf.groupby("k").agg("all"))
    got = df.groupby("k").agg(s=("v", "skew"), a=("w", "all")).to_pandas()
    _check(got, pdf.groupby("k").agg(s=("v", "skew"), a=("w", "all")))


def edge_frames():
    """Groups: constant 0.1 -> 0.0; [1,2] -> NaN; [1,NaN,NaN,3] -> NaN;
    all-NaN -> NaN; [1,2,4,NaN] -> 0.93522...; a tight group (spread 1e-3
    at mean 1e6) that must not be zeroed.  Plus a constant int64 column."""
    k = [0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5]
    nan = np.nan
    v = [0.1, 0.1, 0.1, 1, 2, 1, nan, nan, 3, nan, nan, nan, 1, 2, 4, nan,
         1e6, 1e6 + 1e-3, 1e6 + 3e-4, 1e6 - 2e-4]
    skew = pandas.DataFrame({"k": np.array(k, dtype=np.int64),
                             "v": np.array(v, dtype=np.float64),
                             "c": np.full(len(k), 7, dtype=np.int64)})
    anyall = pandas.DataFrame({
        "k": np.array([0, 0, 1, 1, 2, 2], dtype=np.int64),
        "a": np.array([0, nan, 0, 2, nan, nan]),
        "i": np.array([0, 0, 1, 0, 5, 5], dtype=np.int64)})
    return skew, anyall


def test_edge_frame(mpd):
    pdf, pany = edge_frames()
    got = mpd.DataFrame(pdf).groupby("k").skew().to_pandas()
    exp = pdf.groupby("k").skew()
    # the NaN / exact-0.0 pattern is pandas'; the tight group's value is
    # held to the exact rational result (pandas' running-mean update is
    # itself ~1e-7 off there: eps * mean/std)
    for c in ("v", "c"):
        gc, ec = got[c].to_numpy(), exp[c].to_numpy()
        assert np.array_equal(np.isnan(gc), np.isnan(ec)), c
        assert np.array_equal(gc == 0.0, ec == 0.0), c
    g = got["v"].to_numpy()
    assert g[0] == 0.0 and np.isnan(g[1:4]).all()
    assert abs(g[4] - 0.9352195295828246) < 1e-12
    tight = [Fraction(x) for x in pdf["v"].to_numpy()[-4:]]
    mean = sum(tight) / 4
    m2 = float(sum((x - mean) ** 2 for x in tight))
    m3 = float(sum((x - mean) ** 3 for x in tight))
    truth = 4 * np.sqrt(3.0) / 2 * m3 / m2 ** 1.5
    assert abs(g[5] - truth) <= 1e-9 * abs(truth)
    assert abs(g[5] - exp["v"].to_numpy()[5]) <= 1e-5 * abs(truth)
    df = mpd.DataFrame(pany)
    ga, gl = df.groupby("k").any().to_pandas(), \
        df.groupby("k").all().to_pandas()
    assert ga["a"].tolist() == [False, True, False]
    assert ga["i"].tolist() == [False, True, True]
    assert gl["a"].tolist() == [False, False, True]
    assert gl["i"].tolist() == [False, False, True]
    assert all(dt == bool for dt in list(ga.dtypes) + list(gl.dtypes))
    _check(ga, pany.groupby("k").any())
    _check(gl, pany.groupby("k").all())


def test_frame_skew_kurt(mpd):
    rng = np.random.default_rng(9)
    n = 500
    v, w = _values(rng, n)
    pdf = pandas.DataFrame({"v": v, "w": w, "big": 1e6 + rng.gamma(2, 1, n),
                            "allnan": np.full(n, np.nan),
                            "const": np.full(n, 3, dtype=np.int64)})
    df = mpd.DataFrame(pdf)
    for how in ("skew", "kurt", "kurtosis"):
        got = getattr(df, how)()
        exp = getattr(pdf, how)()
        assert list(got.index) == list(exp.index)
        np.testing.assert_allclose(got.to_numpy(), exp.to_numpy(),
                                   rtol=1e-9, equal_nan=True, err_msg=how)
    assert np.isclose(df["v"].skew(), pdf["v"].skew(), rtol=1e-9)
    assert np.isclose(df["big"].kurtosis(), pdf["big"].kurtosis(), rtol=1e-9)
    short = mpd.DataFrame(pandas.DataFrame({"v": [1.0, 2.0, 4.0]}))
    assert np.isclose(short.skew()["v"], 0.9352195295828246)
    assert np.isnan(short.kurt()["v"])


def test_loud_errors(mpd, monkeypatch):
    pdf = _keyed(np.random.default_rng(10), "int", n=60)
    df = mpd.DataFrame(pdf)
    with pytest.raises(HfError):
        df.skew(skipna=False)
    with pytest.raises(HfError):
        df.kurt(axis=1)
    sdf = mpd.DataFrame(pandas.DataFrame(
        {"k": np.arange(6, dtype=np.int64) % 2,
         "s": np.array(list("abcdef"), dtype=object)}))
    with pytest.raises(HfError, match="string"):
        sdf.groupby("k").skew()
    with pytest.raises(HfError):
        sdf.groupby("k").any()
    # world>1 is loud for every new op
    import modin_amd.distributed as dist
    monkeypatch.setattr(dist, "is_active", lambda: True)
    for call in (lambda: df.groupby("k").skew(),
                 lambda: df.groupby("k").any(),
                 lambda: df.groupby("k").all(),
                 lambda: df.skew(), lambda: df.kurt()):
        with pytest.raises(HfError, match="world>1 is a later round"):
            call()
