"""GPU tier: hf_group_moments and what is built on it — groupby
skew/any/all and frame skew/kurt.

1. kernel contract against a numpy bincount / minimum.at restatement, at
   the sizes where it can break: n in {0, 1, 2, 255, 100003} (odd tail,
   multi-block grid) x group counts {1 null gid, 1, 3, GM_LDS_MAX,
   GM_LDS_MAX + 1, 5000} (both sides of the LDS/global switch);
2. conditioning: exact rational truth, pandas as the yardstick;
3. the edge frame's exact NaN / 0.0 / bool pattern;
4. L1 parity vs pandas at 1 and 3 partitions;
5. golden fixture from the reference (PandasOnPython, NPartitions=3);
6. loud errors.
"""

from fractions import Fraction

import numpy as np
import pandas
import pytest

import modin_amd.pandas as mpd
from modin_amd import config
from modin_amd.core import lib
from tests.conftest import load_golden
from tests.test_mock_skew import edge_frames

pytestmark = pytest.mark.gpu

LDS_MAX = lib.GM_LDS_MAX


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = config.NPartitions.get()
    config.NPartitions.put(request.param)
    yield request.param
    config.NPartitions.put(old)


# ---- 1. kernel contract ---------------------------------------------------

def _np_moments(gid, x, centre, ng, table=None, absd=False):
    t = np.zeros((6, ng)) if table is None else table
    if table is None:
        t[4], t[5] = np.inf, -np.inf
    g = np.zeros(x.size, dtype=np.int64) if gid is None else gid
    ok = (g >= 0) & ~np.isnan(x)
    g, x = g[ok], x[ok]
    d = x - centre[g]
    if absd:
        d = np.abs(d)
    for p in range(4):
        t[p] += np.bincount(g, weights=d ** (p + 1), minlength=ng)
    np.minimum.at(t[4], g, x)
    np.maximum.at(t[5], g, x)
    return t


def _inputs(rng, n, ng, null_gid):
    x = 100.0 + rng.gamma(2.0, 1.0, n)
    x[rng.random(n) < 0.05] = np.nan
    if null_gid:
        gid = None
    else:
        gid = rng.integers(0, ng, n).astype(np.int64)
        gid[rng.random(n) < 0.05] = -1
    centre = 100.0 + 2.0 + rng.standard_normal(ng) * 0.01
    return gid, x, centre


def _run(gid, x, centre, ng, table=None):
    table = lib.group_moments_table(ng) if table is None else table
    lib.group_moments(None if gid is None else lib.put(gid), lib.put(x),
                      lib.put(centre), ng, table)
    return table


def _assert_table(got, exp, absd):
    got = got.reshape(6, -1)
    np.testing.assert_array_equal(got[4], exp[4])
    np.testing.assert_array_equal(got[5], exp[5])
    for p in range(4):
        err = np.abs(got[p] - exp[p])
        bound = 1e-12 * np.abs(exp[p]) + 1e-12 * absd[p]
        assert (err <= bound).all(), (p, err.max(), bound[err.argmax()])


GROUPS = [("null", 1), ("one", 1), ("three", 3), ("lds_last", LDS_MAX),
          ("global_first", LDS_MAX + 1), ("global", 5000)]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 100003])
@pytest.mark.parametrize("label,ng", GROUPS, ids=[g[0] for g in GROUPS])
def test_kernel_contract(label, ng, n):
    rng = np.random.default_rng(1000 + 7 * n + ng)
    gid, x, centre = _inputs(rng, n, ng, label == "null")
    got = lib.get(_run(gid, x, centre, ng))
    exp = _np_moments(gid, x, centre, ng)
    absd = _np_moments(gid, x, centre, ng, absd=True)
    _assert_table(got, exp, absd)
    # groups no row reached still hold the identities
    empty = exp[5] == -np.inf
    g6 = got.reshape(6, -1)
    assert (g6[:4, empty] == 0.0).all()
    assert (g6[4, empty] == np.inf).all() and (g6[5, empty] == -np.inf).all()


@pytest.mark.parametrize("ng,null_gid", [(1, True), (3, False),
                                         (LDS_MAX + 1, False)])
def test_two_calls_equal_one_on_concatenation(ng, null_gid):
    rng = np.random.default_rng(77 + ng)
    g1, x1, centre = _inputs(rng, 4097, ng, null_gid)
    g2, x2, _ = _inputs(rng, 2500, ng, null_gid)
    table = _run(g1, x1, centre, ng)
    got = lib.get(_run(g2, x2, centre, ng, table))
    gcat = None if null_gid else np.concatenate([g1, g2])
    xcat = np.concatenate([x1, x2])
    exp = _np_moments(gcat, xcat, centre, ng)
    _assert_table(got, exp, _np_moments(gcat, xcat, centre, ng, absd=True))


@pytest.mark.parametrize("ng", [3, LDS_MAX + 1])
def test_gid_out_of_range_is_an_error(ng):
    rng = np.random.default_rng(5)
    gid, x, centre = _inputs(rng, 1001, ng, False)
    gid[500] = ng
    with pytest.raises(lib.HfError, match="n_groups"):
        _run(gid, x, centre, ng)
    with pytest.raises(lib.HfError):
        lib.group_moments(None, lib.put(x), lib.put(centre), ng,
                          lib.group_moments_table(ng))


# ---- 2. conditioning ------------------------------------------------------

def _exact_shape(x):
    """(skew, kurt) of the non-NaN values: exact rational central moments,
    then one float formula."""
    fx = [Fraction(float(v)) for v in x[~np.isnan(x)]]
    n = len(fx)
    mean = sum(fx) / n
    d = [v - mean for v in fx]
    m2 = float(sum(v * v for v in d))
    m3 = float(sum(v ** 3 for v in d))
    m4 = float(sum(v ** 4 for v in d))
    skew = n * np.sqrt(n - 1.0) / (n - 2.0) * m3 / m2 ** 1.5
    den = (n - 2.0) * (n - 3.0)
    kurt = (n * (n + 1.0) * (n - 1.0) * m4 / (den * m2 * m2)
            - 3.0 * (n - 1.0) ** 2 / den)
    return skew, kurt


@pytest.mark.parametrize("mu", [0.0, 1e4, 1e6])
def test_conditioning(mu, npartitions):
    rng = np.random.default_rng(314)
    n, ng = 4000, 7
    k = rng.integers(0, ng, n).astype(np.int64)
    x = mu + rng.gamma(2.0, 1.0, n)
    x[rng.random(n) < 0.05] = np.nan
    pdf = pandas.DataFrame({"k": k, "x": x})
    df = mpd.DataFrame(pdf)
    truth = np.array([_exact_shape(x[k == g])[0] for g in range(ng)])
    ours = df.groupby("k").skew().to_pandas()["x"].to_numpy()
    theirs = pdf.groupby("k").skew()["x"].to_numpy()
    err_ours = np.max(np.abs(ours - truth) / np.abs(truth))
    err_pandas = np.max(np.abs(theirs - truth) / np.abs(truth))
    print(f"group skew mu={mu}: ours {err_ours:.3g} pandas {err_pandas:.3g}")
    assert err_ours <= max(10 * err_pandas, 1e-12)
    t_skew, t_kurt = _exact_shape(x)
    for how, t in (("skew", t_skew), ("kurt", t_kurt)):
        e_ours = abs(getattr(df, how)()["x"] - t) / abs(t)
        e_pandas = abs(getattr(pdf, how)()["x"] - t) / abs(t)
        print(f"frame {how} mu={mu}: ours {e_ours:.3g} pandas {e_pandas:.3g}")
        assert e_ours <= max(10 * e_pandas, 1e-12)


# ---- 3. edge frame --------------------------------------------------------

def test_edge_frame(npartitions):
    old = config.MinRowPartitionSize.get()
    config.MinRowPartitionSize.put(4)
    try:
        pdf, pany = edge_frames()
        got = mpd.DataFrame(pdf).groupby("k").skew().to_pandas()
        exp = pdf.groupby("k").skew()
        for c in ("v", "c"):
            gc, ec = got[c].to_numpy(), exp[c].to_numpy()
            assert np.array_equal(np.isnan(gc), np.isnan(ec)), c
            assert np.array_equal(gc == 0.0, ec == 0.0), c
        g = got["v"].to_numpy()
        assert g[0] == 0.0 and np.isnan(g[1:4]).all()
        assert abs(g[4] - 0.9352195295828246) < 1e-12
        truth = _exact_shape(pdf["v"].to_numpy()[-4:])[0]
        assert g[5] != 0.0 and abs(g[5] - truth) <= 1e-9 * abs(truth)
        df = mpd.DataFrame(pany)
        ga = df.groupby("k").any().to_pandas()
        gl = df.groupby("k").all().to_pandas()
    finally:
        config.MinRowPartitionSize.put(old)
    assert ga["a"].tolist() == [False, True, False]
    assert ga["i"].tolist() == [False, True, True]
    assert gl["a"].tolist() == [False, False, True]
    assert gl["i"].tolist() == [False, False, True]
    assert all(dt == bool for dt in list(ga.dtypes) + list(gl.dtypes))


# ---- 4. L1 parity vs pandas -----------------------------------------------

def _same(got, exp, rtol=1e-9):
    if isinstance(exp, pandas.Series):
        got, exp = got.to_frame("x"), exp.to_frame("x")
    assert list(got.columns) == list(exp.columns)
    gi, ei = got.index, exp.index
    assert gi.equals(ei) or np.array_equal(gi.to_numpy(), ei.to_numpy(),
                                           equal_nan=True), (gi, ei)
    for c in exp.columns:
        assert got[c].dtype == exp[c].dtype, (c, got[c].dtype)
        if exp[c].dtype == bool or exp[c].dtype == object:
            assert got[c].tolist() == exp[c].tolist(), c
        else:
            np.testing.assert_allclose(
                got[c].to_numpy().astype(float),
                exp[c].to_numpy().astype(float), rtol=rtol, atol=1e-12,
                equal_nan=True, err_msg=str(c))


def _vals(rng, n):
    v = rng.gamma(2.0, 1.0, n)
    v[rng.random(n) < 0.1] = np.nan
    u = rng.standard_normal(n)
    u[rng.random(n) < 0.4] = 0.0
    u[rng.random(n) < 0.1] = np.nan
    return {"v": v, "u": u, "w": rng.integers(-2, 3, n).astype(np.int64)}


def _all_three(df, pdf, by, **kw):
    for how in ("skew", "any", "all"):
        got = getattr(df.groupby(by, **kw), how)().to_pandas()
        _same(got, getattr(pdf.groupby(by, **kw), how)())


def test_l1_int_dense_keys(npartitions):
    rng = np.random.default_rng(21)
    n = 5000
    pdf = pandas.DataFrame({"k": rng.integers(0, 50, n).astype(np.int64),
                            **_vals(rng, n)})
    _all_three(mpd.DataFrame(pdf), pdf, "k")


def test_l1_hash_route(npartitions):
    rng = np.random.default_rng(22)
    n = 20000
    pool = np.unique(rng.integers(-10**12, 10**12, 2000)).astype(np.int64)
    pdf = pandas.DataFrame({"k": rng.choice(pool, n), **_vals(rng, n)})
    old = config.MaxGroupbySlots.get()
    config.MaxGroupbySlots.put(1000)
    try:
        _all_three(mpd.DataFrame(pdf), pdf, "k")
    finally:
        config.MaxGroupbySlots.put(old)


@pytest.mark.parametrize("dropna", [True, False])
def test_l1_float_keys_with_nan(npartitions, dropna):
    rng = np.random.default_rng(23)
    n = 3000
    k = rng.integers(-5, 20, n).astype(np.float64) / 4
    k[rng.random(n) < 0.08] = np.nan
    pdf = pandas.DataFrame({"k": k, **_vals(rng, n)})
    _all_three(mpd.DataFrame(pdf), pdf, "k", dropna=dropna)


def test_l1_string_keys(npartitions):
    rng = np.random.default_rng(24)
    n = 3000
    k = np.array([f"key{i:02d}" for i in rng.integers(0, 17, n)],
                 dtype=object)
    k[rng.random(n) < 0.05] = None
    pdf = pandas.DataFrame({"k": k, **_vals(rng, n)})
    _all_three(mpd.DataFrame(pdf), pdf, "k")


def test_l1_datetime_keys(npartitions):
    rng = np.random.default_rng(25)
    n = 3000
    days = rng.integers(0, 11, n)
    k = (np.datetime64("2024-01-01", "ns")
         + days.astype("timedelta64[D]").astype("timedelta64[ns]"))
    pdf = pandas.DataFrame({"k": k, **_vals(rng, n)})
    _all_three(mpd.DataFrame(pdf), pdf, "k")


def test_l1_two_keys(npartitions):
    rng = np.random.default_rng(26)
    n = 4000
    pdf = pandas.DataFrame({
        "a": rng.integers(0, 6, n).astype(np.int64),
        "b": np.array([f"s{i}" for i in rng.integers(0, 4, n)], dtype=object),
        **_vals(rng, n)})
    _all_three(mpd.DataFrame(pdf), pdf, ["a", "b"])


def test_l1_forms(npartitions):
    rng = np.random.default_rng(27)
    n = 3000
    pdf = pandas.DataFrame({"k": rng.integers(0, 9, n).astype(np.int64),
                            **_vals(rng, n)})
    df = mpd.DataFrame(pdf)
    _same(df.groupby("k", as_index=False).skew().to_pandas(),
          pdf.groupby("k", as_index=False).skew())
    _same(df.groupby("k", as_index=False).any().to_pandas(),
          pdf.groupby("k", as_index=False).any())
    for how in ("skew", "any", "all"):
        got = getattr(df.groupby("k")["u"], how)().to_pandas()
        exp = getattr(pdf.groupby("k")["u"], how)()
        assert got.name == "u"
        _same(got, exp)
    _same(df.groupby("k").agg(["sum", "skew"]).to_pandas(),
          pdf.groupby("k").agg(["sum", "skew"]))
    _same(df.groupby("k").agg({"v": "skew", "w": "any"}).to_pandas(),
          pdf.groupby("k").agg({"v": "skew", "w": "any"}))
    _same(df.groupby("k").agg("all").to_pandas(),
          pdf.groupby("k").agg("all"))
    _same(df.groupby("k").agg(s=("v", "skew"), a=("u", "all")).to_pandas(),
          pdf.groupby("k").agg(s=("v", "skew"), a=("u", "all")))


def test_l1_frame_skew_kurt(npartitions):
    rng = np.random.default_rng(28)
    n = 5001
    pdf = pandas.DataFrame({**_vals(rng, n),
                            "allnan": np.full(n, np.nan)})
    df = mpd.DataFrame(pdf)
    for how in ("skew", "kurt"):
        got, exp = getattr(df, how)(), getattr(pdf, how)()
        assert list(got.index) == list(exp.index)
        np.testing.assert_allclose(got.to_numpy(), exp.to_numpy(),
                                   rtol=1e-9, equal_nan=True, err_msg=how)
    assert np.isclose(df["v"].kurtosis(), pdf["v"].kurtosis(), rtol=1e-9)
    assert np.isclose(df["w"].skew(), pdf["w"].skew(), rtol=1e-9)
    assert np.isnan(df["allnan"].skew())


def test_l1_global_path_from_l1():
    """300 000 rows, 1 025 groups: one past the LDS switch."""
    rng = np.random.default_rng(29)
    n = 300_000
    k = rng.integers(0, LDS_MAX + 1, n).astype(np.int64)
    k[:LDS_MAX + 1] = np.arange(LDS_MAX + 1)
    v = 50.0 + rng.gamma(2.0, 1.0, n)
    v[rng.random(n) < 0.05] = np.nan
    pdf = pandas.DataFrame({"k": k, "v": v})
    got = mpd.DataFrame(pdf).groupby("k").skew().to_pandas()
    assert len(got) == LDS_MAX + 1
    _same(got, pdf.groupby("k").skew())


# ---- 5. golden ------------------------------------------------------------

def test_golden_reference(npartitions):
    g = load_golden("gbs_skew")
    pdf = pandas.DataFrame({"k": g["in_k"], "v": g["in_v"], "u": g["in_u"],
                            "w": g["in_w"]})
    df = mpd.DataFrame(pdf)
    for how in ("skew", "any", "all"):
        got = getattr(df.groupby("k"), how)().to_pandas()
        np.testing.assert_array_equal(got.index.to_numpy(),
                                      g[f"{how}_index"])
        for c in ("v", "u", "w"):
            exp = g[f"{how}_{c}"]
            assert got[c].dtype == exp.dtype, (how, c)
            if how == "skew":
                np.testing.assert_allclose(got[c].to_numpy(), exp,
                                           rtol=1e-9, equal_nan=True)
            else:
                np.testing.assert_array_equal(got[c].to_numpy(), exp)


# ---- 6. loud errors -------------------------------------------------------

def test_loud_errors():
    df = mpd.DataFrame(pandas.DataFrame(
        {"k": np.arange(8, dtype=np.int64) % 2,
         "v": np.arange(8, dtype=np.float64),
         "s": np.array(list("abcdefgh"), dtype=object)}))
    with pytest.raises(lib.HfError):
        df[["k", "v"]].skew(skipna=False)
    with pytest.raises(lib.HfError):
        df[["k", "v"]].kurt(axis=1)
    with pytest.raises(lib.HfError, match="string"):
        df.groupby("k").skew()
    with pytest.raises(lib.HfError):
        df.groupby("k").all()
