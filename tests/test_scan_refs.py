"""CPU tier: the references of tests/scan_refs.py against pandas at small
sizes, and the error bound of the tiled f64 sum scan on the numpy restatement
of the algorithm (no GPU)."""

import numpy as np
import pandas
import pytest

from tests import scan_refs as sr
from tests.scan_refs import TILE

PANDAS_CUM = {"sum": "cumsum", "min": "cummin", "max": "cummax",
              "prod": "cumprod"}


def _f64(rng, n, nan_share):
    x = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    x[rng.random(n) < nan_share] = np.nan
    return x


def _same(got, exp, op, absum):
    """min/max pick an input value: exact.  pandas' own sequential f64
    sum is within n * u * cumsum|x| of the exact one, its product within
    n * u relative."""
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    got = got[ok].astype(np.float64)
    exp = exp[ok]
    if op in ("min", "max"):
        assert np.array_equal(got, exp)
    elif op == "sum":
        tol = exp.size * sr.U * absum[ok].astype(np.float64)
        assert (np.abs(got - exp) <= tol).all()
    else:
        assert (np.abs(got / exp - 1) <= exp.size * sr.U).all()


@pytest.mark.parametrize("op", sr.OPS)
@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_ref_cumsum_vs_pandas(op, n):
    rng = np.random.default_rng(n)
    for nan_share in (0.0, 0.3):
        x = _f64(rng, n, nan_share)
        got, absum = sr.ref_cumsum(x, op)
        exp = getattr(pandas.Series(x), PANDAS_CUM[op])().to_numpy()
        _same(got, exp, op, absum)
        assert (absum is not None) == (op == "sum")
    k = rng.integers(-2**62, 2**62, n).astype(np.int64) | 1
    got, absum = sr.ref_cumsum(k, op)
    exp = getattr(pandas.Series(k), PANDAS_CUM[op])().to_numpy()
    assert got.dtype == np.int64 and absum is None
    assert np.array_equal(got, exp)     # wrapping included


@pytest.mark.parametrize("op", sr.OPS)
def test_ref_seg_cumsum_vs_pandas_groupby(op):
    rng = np.random.default_rng(5)
    n = 500
    for first_head in (0, 1):
        heads = (rng.random(n) < 0.1).astype(np.int64)
        heads[0] = first_head       # row 0 opens a segment either way
        seg = np.cumsum(heads)
        x = _f64(rng, n, 0.2)
        got, absum = sr.ref_seg_cumsum(x, heads, op)
        exp = getattr(pandas.Series(x).groupby(seg), PANDAS_CUM[op])()
        _same(got, exp.to_numpy(), op, absum)
        k = rng.integers(-2**62, 2**62, n).astype(np.int64) | 1
        got, _ = sr.ref_seg_cumsum(k, heads, op)
        exp = getattr(pandas.Series(k).groupby(seg), PANDAS_CUM[op])()
        assert np.array_equal(got, exp.to_numpy())


def test_ref_seg_cumsum_absum_restarts():
    x = np.array([1.0, -2.0, np.nan, 4.0, -8.0])
    heads = np.array([0, 0, 0, 1, 0], dtype=np.int64)
    out, absum = sr.ref_seg_cumsum(x, heads, "sum")
    assert out.dtype == np.longdouble
    assert np.array_equal(np.nan_to_num(out.astype(np.float64), nan=99.0),
                          [1.0, -1.0, 99.0, 4.0, -4.0])
    assert np.array_equal(absum.astype(np.float64), [1, 3, 3, 4, 12])


def test_ref_filter_vs_boolean_indexing():
    rng = np.random.default_rng(6)
    mask = (rng.random(1000) < 0.3).astype(np.int64) * 7   # nonzero = kept
    col = rng.normal(size=1000)
    exp = pandas.Series(col)[pandas.Series(mask != 0)]
    assert np.array_equal(sr.ref_filter(mask, col), exp.to_numpy())
    assert np.array_equal(sr.ref_filter_iota(mask, 2**40 + 3),
                          exp.index.to_numpy() + (2**40 + 3))
    assert sr.ref_filter_iota(np.zeros(4, np.int64), 0).dtype == np.int64


def test_restatement_is_a_cumsum():
    """On integers small enough that every partial sum is exact, any
    association order gives the same answer: the restatement must equal
    numpy's cumsum bit for bit, NaN rows aside."""
    rng = np.random.default_rng(7)
    for n in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        x = rng.integers(-1000, 1000, n).astype(np.float64)
        assert np.array_equal(sr.tiled_sum_scan(x), np.cumsum(x)), n
    x[::7] = np.nan
    exp = np.cumsum(np.where(np.isnan(x), 0.0, x))
    exp[np.isnan(x)] = np.nan
    assert np.array_equal(sr.tiled_sum_scan(x), exp, equal_nan=True)


# 3 tiles and a tail; and the smallest count at which the one-block tile
# scan takes a second iteration with a full tile and a tail behind it
@pytest.mark.parametrize("n", [3 * TILE + 5, 1024 * TILE + 4097])
def test_restatement_within_sum_bound(n):
    rng = np.random.default_rng(n)
    for name, x in sr.scan_datasets(rng, n).items():
        ref, absum = sr.ref_cumsum(x, "sum")
        ratio = sr.sum_error_ratio(sr.tiled_sum_scan(x), ref, absum)
        print(f"tiled scan n={n} {name}: {ratio:.3g} u*cumsum|x|")
        assert ratio <= sr.SUM_BOUND, (name, ratio)


def test_sequential_f64_cumsum_is_no_reference():
    """Why the reference is longdouble: a sequential f64 cumsum (numpy,
    pandas) is itself hundreds of u*cumsum|x| off on offset data, far
    outside the bound asserted on the kernel."""
    rng = np.random.default_rng(8)
    x = 1e6 + rng.normal(0.0, 1.0, 1024 * TILE + 4097)
    ref, absum = sr.ref_cumsum(x, "sum")
    ratio = sr.sum_error_ratio(np.cumsum(x), ref, absum)
    print(f"sequential f64 cumsum: {ratio:.3g} u*cumsum|x|")
    assert ratio > sr.SUM_BOUND
