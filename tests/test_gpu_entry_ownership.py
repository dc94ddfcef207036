"""GPU tier: the C-ABI entry points own their outputs and temporaries.

Balance: ``lib.dev_live()`` counts the device blocks the engine's allocator
has handed out and not got back.  Every scenario runs from putting its inputs
to reading its results inside a function, so that all its references die with
the function's frame; the counter is then back at its baseline.  While a
scenario holds only columns, the counter is baseline + the columns it holds.
A block released twice (or never) shows as a counter off by one.

Reachable error paths: the call raises HfError, leaves the counter where it
was, and a following valid call on the same inputs is correct.

sort_perm is compared with ``oracle.sort_perm`` exactly, both directions, with
duplicate keys so that stability is part of the comparison.
"""

import gc

import numpy as np
import pytest

import oracle
from modin_amd.core import lib
from tests.join_ref import inner_join_ref

pytestmark = pytest.mark.gpu

N = 4097          # one FILT_TILE / JOIN_TILE plus one row
I64 = np.iinfo(np.int64)


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _balanced(scenario):
    """Run scenario(base); every reference it made dies with its frame."""
    gc.collect()
    base = lib.dev_live()
    scenario(base)
    gc.collect()
    assert lib.dev_live() == base, "device blocks leaked or freed twice"


def _held(base, k):
    assert lib.dev_live() == base + k


def _fails_clean(call, match=None):
    """call() raises HfError and leaves the live-block count unchanged."""
    gc.collect()
    before = lib.dev_live()
    with pytest.raises(lib.HfError, match=match):
        call()
    gc.collect()
    assert lib.dev_live() == before


# ---- balance -------------------------------------------------------------

_SCAN_NP = {
    lib.AGG_SUM: np.cumsum, lib.AGG_MIN: np.minimum.accumulate,
    lib.AGG_MAX: np.maximum.accumulate, lib.AGG_PROD: np.cumprod,
}


def _scan_input(op, dtype, n=N, seed=0):
    """Values whose running sum / product is exact in both dtypes."""
    rng = np.random.default_rng(seed)
    if op == lib.AGG_PROD:
        pool = [1, -1] if dtype == np.int64 else [1.0, -1.0, 2.0, 0.5]
        return rng.choice(pool, n).astype(dtype)
    return rng.integers(-50, 50, n).astype(dtype)


def _seg_scan_np(x, heads, op):
    out = np.empty_like(x)
    starts = np.flatnonzero(heads)
    for a, b in zip(starts, np.r_[starts[1:], x.size]):
        out[a:b] = _SCAN_NP[op](x[a:b])
    return out


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
@pytest.mark.parametrize("op", [lib.AGG_SUM, lib.AGG_MIN, lib.AGG_MAX,
                                lib.AGG_PROD])
def test_balance_cumsum(op, dtype):
    x = _scan_input(op, dtype)

    def scenario(base):
        col = lib.put(x)
        out = lib.cumsum(col, op)
        _held(base, 2)
        np.testing.assert_array_equal(lib.get(out), _SCAN_NP[op](x))
        empty = lib.cumsum(lib.put(x[:0]), op)
        assert lib.get(empty).size == 0
    _balanced(scenario)


def test_balance_seg_cumsum():
    rng = np.random.default_rng(1)
    x = _scan_input(lib.AGG_SUM, np.float64, seed=1)
    heads = (rng.random(N) < 0.01).astype(np.int64)
    heads[0] = 1

    def scenario(base):
        col, hd = lib.put(x), lib.put(heads)
        out = lib.seg_cumsum(col, hd, lib.AGG_SUM)
        _held(base, 3)
        np.testing.assert_array_equal(
            lib.get(out), _seg_scan_np(x, heads, lib.AGG_SUM))
    _balanced(scenario)


@pytest.mark.parametrize("with_heads", [False, True])
def test_balance_ewm_mean(with_heads):
    rng = np.random.default_rng(2)
    x = rng.normal(size=N)
    heads = np.zeros(N, dtype=np.int64)
    heads[::1000] = 1

    def scenario(base):
        col = lib.put(x)
        hd = lib.put(heads) if with_heads else None
        out = lib.ewm_mean(col, hd, 0.3)
        _held(base, 2 + with_heads)
        got = lib.get(out)
        assert got.size == N and got[0] == x[0]
        if with_heads:
            assert got[1000] == x[1000]    # a head row restarts the mean
    _balanced(scenario)


@pytest.mark.parametrize("span", [1000, 1 << 40], ids=["narrow", "wide"])
def test_balance_sort_perm(span):
    rng = np.random.default_rng(3)
    k = rng.integers(-span // 2, span // 2, N).astype(np.int64)

    def scenario(base):
        col = lib.put(k)
        for asc in (True, False):
            perm = lib.sort_perm(col, asc)
            _held(base, 2)
            np.testing.assert_array_equal(lib.get(perm),
                                          oracle.sort_perm(k, asc))
    _balanced(scenario)


def test_balance_gather_scatter_cross_shuffle():
    rng = np.random.default_rng(4)
    x = rng.random(N)
    k = rng.integers(-1000, 1000, N).astype(np.int64)
    perm = rng.permutation(N).astype(np.int64)
    splitters = np.array([-500, 0, 0, 700], dtype=np.int64)

    def scenario(base):
        xc, kc, pc = lib.put(x), lib.put(k), lib.put(perm)
        g = lib.gather(xc, pc)
        gi = lib.gather(kc, pc)
        s = lib.scatter(g, pc)
        _held(base, 6)
        np.testing.assert_array_equal(lib.get(g), x[perm])
        np.testing.assert_array_equal(lib.get(gi), k[perm])
        np.testing.assert_array_equal(lib.get(s), x)
        li, ri = lib.cross_idx(17, 241)     # 4097 pairs
        _held(base, 8)
        np.testing.assert_array_equal(lib.get(li), np.repeat(np.arange(17), 241))
        np.testing.assert_array_equal(lib.get(ri), np.tile(np.arange(241), 17))
        dest = lib.shuffle_dest(kc, splitters)
        none = lib.shuffle_dest(kc, [])
        _held(base, 10)
        np.testing.assert_array_equal(
            lib.get(dest), np.searchsorted(splitters, k, side="right"))
        assert not lib.get(none).any()
    _balanced(scenario)


def test_balance_filter():
    rng = np.random.default_rng(5)
    x = rng.random(N)
    k = rng.integers(0, 100, N).astype(np.int64)
    mask = (rng.random(N) < 0.4).astype(np.int64)

    def scenario(base):
        xc, kc, mc = lib.put(x), lib.put(k), lib.put(mask)
        plan = lib.filter_plan(mc)
        _held(base, 4)                      # the plan owns one block
        fx, fk = lib.filter_apply(plan, xc), lib.filter_apply(plan, kc)
        rows = lib.filter_iota(plan, 10)
        _held(base, 7)
        keep = mask.astype(bool)
        assert plan.n_kept == keep.sum()
        np.testing.assert_array_equal(lib.get(fx), x[keep])
        np.testing.assert_array_equal(lib.get(fk), k[keep])
        np.testing.assert_array_equal(lib.get(rows), np.flatnonzero(keep) + 10)
        none = lib.filter_plan(lib.put(np.zeros(N, dtype=np.int64)))
        assert lib.get(lib.filter_apply(none, xc)).size == 0
    _balanced(scenario)


def _group_sums(keys, vals):
    uniq, inv = np.unique(keys, return_inverse=True)
    return uniq, [np.bincount(inv, weights=v) for v in vals], np.bincount(inv)


@pytest.mark.parametrize("nvals", [1, 8])
@pytest.mark.parametrize("counts", [False, True])
def test_balance_groupby_dense(counts, nvals):
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 300, N).astype(np.int64) * 3 - 100
    vals = [rng.integers(-9, 9, N).astype(np.float64) for _ in range(nvals)]
    kmin, n_slots = int(keys.min()), int(keys.max() - keys.min()) + 1

    def scenario(base):
        kc, vc = lib.put(keys), [lib.put(v) for v in vals]
        tabs = [lib.alloc_raw(8 * nvals * n_slots), lib.alloc_raw(8 * n_slots),
                lib.alloc_raw(8 * nvals * n_slots) if counts else 0]
        try:
            for t, b in zip(tabs, (nvals, 1, nvals)):
                if t:
                    lib.memset_raw(t, 0, 8 * b * n_slots)
            lib.groupby_accum(kc, vc, lib.AGG_SUM, kmin, n_slots, *tabs)
            ok, osums, ocnts, n = lib.groupby_compact(*tabs, nvals, kmin,
                                                      n_slots)
            uniq, sums, cnt = _group_sums(keys, vals)
            assert n == uniq.size
            np.testing.assert_array_equal(lib.get(ok), uniq)
            for c in range(nvals):
                np.testing.assert_array_equal(lib.get(osums[c]), sums[c])
                if counts:
                    np.testing.assert_array_equal(lib.get(ocnts[c]), cnt)
        finally:
            for t in tabs:
                lib.free_raw(t)
    _balanced(scenario)


def test_balance_groupby_hash():
    rng = np.random.default_rng(7)
    keys = rng.choice(rng.integers(I64.min, I64.max, 500), N).astype(np.int64)
    vals = [rng.integers(-9, 9, N).astype(np.float64) for _ in range(2)]
    H = 1 << 13
    L = H + 1

    def scenario(base):
        kc, vc = lib.put(keys), [lib.put(v) for v in vals]
        tkey, sums = lib.alloc_raw(8 * L), lib.alloc_raw(8 * 2 * L)
        rowcnt, counts = lib.alloc_raw(8 * L), lib.alloc_raw(8 * 2 * L)
        try:
            lib.fill_i64(tkey, int(I64.min), L)
            lib.memset_raw(sums, 0, 8 * 2 * L)
            lib.memset_raw(rowcnt, 0, 8 * L)
            lib.memset_raw(counts, 0, 8 * 2 * L)
            lib.groupby_hash_accum(kc, vc, lib.AGG_SUM, H, tkey, sums, rowcnt,
                                   counts)
            ok, osums, ocnts, n = lib.groupby_hash_compact(tkey, sums, rowcnt,
                                                           counts, 2, H)
            uniq, exp, cnt = _group_sums(keys, vals)
            assert n == uniq.size
            np.testing.assert_array_equal(lib.get(ok), uniq)
            for c in range(2):
                np.testing.assert_array_equal(lib.get(osums[c]), exp[c])
                np.testing.assert_array_equal(lib.get(ocnts[c]), cnt)
        finally:
            for t in (tkey, sums, rowcnt, counts):
                lib.free_raw(t)
    _balanced(scenario)


def _join_np(lkeys, rkeys, rvals):
    """Inner join, left order then right order within a key."""
    keys, lidx, _ridx, cols = inner_join_ref(lkeys, rkeys, rvals)
    return keys, lidx, cols


def _join_scenario(lkeys, rkeys, rvals, key_min, n_slots):
    def scenario(base):
        rk, rv = lib.put(rkeys), [lib.put(v) for v in rvals]
        lk = lib.put(lkeys)
        j = lib.join_build(rk, rv, key_min, n_slots)
        _held(base, 2 + len(rvals) + 2 + len(rvals))   # csr, jidx, payloads
        keys, lidx, rcols, n = lib.join_probe(j, lk)
        _held(base, 2 * (2 + len(rvals)) + 2 + len(rvals))
        ek, el, er = _join_np(lkeys, rkeys, rvals)
        assert n == ek.size
        np.testing.assert_array_equal(lib.get(keys), ek)
        np.testing.assert_array_equal(lib.get(lidx), el)
        for got, exp in zip(rcols, er):
            np.testing.assert_array_equal(lib.get(got), exp)
    return scenario


def _right_side(rng, nr, n=N, nkeys=1500):
    rkeys = rng.integers(0, nkeys, n).astype(np.int64) + 40
    rvals = [rng.random(n) if c % 2 else rng.integers(0, 99, n).astype(np.int64)
             for c in range(nr)]
    return rkeys, rvals


@pytest.mark.parametrize("nr", [0, 1, 8])
def test_balance_join(nr):
    rng = np.random.default_rng(8)
    rkeys, rvals = _right_side(rng, nr)
    lkeys = rng.integers(0, 1700, N).astype(np.int64)     # some miss
    _balanced(_join_scenario(lkeys, rkeys, rvals, 40, 1500))


def test_balance_join_sorted_fill_fallback():
    rng = np.random.default_rng(9)
    rkeys, rvals = _right_side(rng, 2)
    rkeys = np.r_[rkeys, np.full(5000, 77, dtype=np.int64)]   # > 4096 dups
    rng.shuffle(rkeys)
    rvals = [rng.random(rkeys.size), np.arange(rkeys.size, dtype=np.int64)]
    lkeys = np.array([77, 41, 77, 9999], dtype=np.int64)
    _balanced(_join_scenario(lkeys, rkeys, rvals, 40, 1500))


def test_balance_join_empty_left_and_no_match():
    rng = np.random.default_rng(10)
    rkeys, rvals = _right_side(rng, 1)
    _balanced(_join_scenario(np.empty(0, dtype=np.int64), rkeys, rvals,
                             40, 1500))
    lkeys = rng.integers(5000, 9000, N).astype(np.int64)
    _balanced(_join_scenario(lkeys, rkeys, rvals, 40, 1500))


# ---- reachable error paths -------------------------------------------------

def test_error_join_build_key_outside_range():
    rng = np.random.default_rng(11)
    rkeys, rvals = _right_side(rng, 2)
    lkeys = rng.integers(0, 1700, N).astype(np.int64)
    bad = rkeys.copy()
    bad[1234] = 40 + 1500          # first key past [key_min, key_min+n_slots)

    def scenario(base):
        bk, rv = lib.put(bad), [lib.put(v) for v in rvals]
        _fails_clean(lambda: lib.join_build(bk, rv, 40, 1500), "outside")
    _balanced(scenario)
    _balanced(_join_scenario(lkeys, rkeys, rvals, 40, 1500))


def test_error_map_and_binary():
    rng = np.random.default_rng(12)
    xi = rng.integers(-99, 99, N).astype(np.int64)
    xf = rng.random(N)

    def scenario(base):
        ci, cf = lib.put(xi), lib.put(xf)
        _fails_clean(lambda: lib.map_scalar(lib.MAP_IDIV, ci, 0), "floordiv")
        _fails_clean(lambda: lib.map_scalar(lib.MAP_IMOD, ci, 0), "mod by zero")
        _fails_clean(lambda: lib.map_scalar(99, cf, 1.0), "unknown op")
        _fails_clean(lambda: lib.map_scalar(99, ci, 1), "not defined")
        _fails_clean(lambda: lib.binary(99, cf, cf), "unknown op")
        _fails_clean(lambda: lib.binary(99, ci, ci), "unknown op")
        np.testing.assert_array_equal(
            lib.get(lib.map_scalar(lib.MAP_IDIV, ci, 7)), xi // 7)
        np.testing.assert_array_equal(
            lib.get(lib.map_scalar(lib.MAP_IMOD, ci, 7)), xi % 7)
        np.testing.assert_array_equal(
            lib.get(lib.map_scalar(lib.MAP_ADD, cf, 1.0)), xf + 1.0)
        np.testing.assert_array_equal(
            lib.get(lib.binary(lib.BIN_ADD, cf, cf)), xf + xf)
        np.testing.assert_array_equal(
            lib.get(lib.binary(lib.BIN_MUL, ci, ci)), xi * xi)
    _balanced(scenario)


def test_error_scans():
    rng = np.random.default_rng(13)
    x = _scan_input(lib.AGG_SUM, np.int64, seed=13)
    xf = x.astype(np.float64)
    heads = (rng.random(N) < 0.01).astype(np.int64)
    heads[0] = 1

    def scenario(base):
        col, cf, hd = lib.put(x), lib.put(xf), lib.put(heads)
        short = lib.put(heads[:-1])
        _fails_clean(lambda: lib.cumsum(col, 7), "bad agg_op")
        _fails_clean(lambda: lib.seg_cumsum(col, hd, 7), "bad agg_op")
        _fails_clean(lambda: lib.seg_cumsum(col, short, lib.AGG_SUM),
                     "same length")
        _fails_clean(lambda: lib.ewm_mean(cf, short, 0.5), "same length")
        np.testing.assert_array_equal(lib.get(lib.cumsum(col, lib.AGG_SUM)),
                                      np.cumsum(x))
        np.testing.assert_array_equal(
            lib.get(lib.seg_cumsum(col, hd, lib.AGG_SUM)),
            _seg_scan_np(x, heads, lib.AGG_SUM))
        # alpha = 1: the mean is the row itself (exact), heads or not
        np.testing.assert_array_equal(lib.get(lib.ewm_mean(cf, hd, 1.0)), xf)
    _balanced(scenario)


def test_error_filter_apply_length_mismatch():
    rng = np.random.default_rng(14)
    x = rng.random(N)
    mask = (rng.random(N) < 0.5).astype(np.int64)

    def scenario(base):
        xc, mc, short = lib.put(x), lib.put(mask), lib.put(x[:-1])
        plan = lib.filter_plan(mc)
        _fails_clean(lambda: lib.filter_apply(plan, short), "length mismatch")
        np.testing.assert_array_equal(lib.get(lib.filter_apply(plan, xc)),
                                      x[mask.astype(bool)])
    _balanced(scenario)


# ---- sort_perm at the C ABI ------------------------------------------------

def _sort_keys(n, span, seed):
    """n int64 keys covering exactly [lo, lo + span], with duplicates."""
    rng = np.random.default_rng(seed)
    if span == "extremes":
        pool = np.array([I64.min, I64.max, I64.min + 1, I64.max - 1, -1, 0, 1],
                        dtype=np.int64)
        k = rng.choice(pool, n)
        if n >= 2:
            k[0], k[-1] = I64.max, I64.min
        return k
    lo = -(span // 2) if span == 1 << 40 else 1000
    # few distinct values, so equal keys repeat at every n
    pool = lo + np.unique(np.r_[0, span, rng.integers(0, span + 1, 30)])
    k = rng.choice(pool, n).astype(np.int64)
    if n >= 2:
        k[0], k[-1] = lo + span, lo     # the span is exact
    return k


_SPANS = [0, 255, 256, (1 << 27) - 1, 1 << 27, 1 << 40, "extremes"]


@pytest.mark.parametrize("span", _SPANS, ids=lambda s: f"span{s}")
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 8193])
def test_sort_perm_matches_oracle(n, span):
    k = _sort_keys(n, span, seed=n)
    if n > 1:
        assert np.unique(k).size < n        # duplicates: stability is checked
    if n >= 2 and span != "extremes":
        assert int(k.max()) - int(k.min()) == span
    if n >= 2 and span == "extremes":
        assert k.min() == I64.min and k.max() == I64.max
    col = lib.put(k)
    for asc in (True, False):
        np.testing.assert_array_equal(lib.get(lib.sort_perm(col, asc)),
                                      oracle.sort_perm(k, asc),
                                      err_msg=f"ascending={asc}")
