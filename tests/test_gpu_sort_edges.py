"""GPU tier: hf_sort_perm (stable LSD radix sort) at the sizes and key spans
where it changes path, and the float-key transform hf_ordered_i64.  The whole
permutation must equal the oracle's stable argsort, in both directions: equal
sorted keys alone would not show an unstable pass."""

import numpy as np
import pytest

import oracle
from modin_amd.core import lib

pytestmark = pytest.mark.gpu

SORT_TILE = 2048    # rows per wave-tile
SORT_WPB = 4        # wave-tiles per block
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
FULL = 2**64 - 1

# a wave's 64 lanes; one wave-tile; one block of four wave-tiles; 37 tiles and
# a tail, so the last block is part-filled and the last tile part-valid
MID = 37 * SORT_TILE + 11
SIZES = [1, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1,
         SORT_WPB * SORT_TILE - 1, SORT_WPB * SORT_TILE,
         SORT_WPB * SORT_TILE + 1, MID]

# span -> the path it exists for (passes = ceil(bits(span) / 8))
SPANS_ALL_SIZES = {
    255: "narrow, last span with 1 pass",
    2**27 - 1: "last narrow span (origin packed under the key), 4 passes",
    2**27: "first wide span (separate key and origin arrays), 4 passes",
}
SPANS_MID_SIZE = {
    0: "zero passes: pack and unpack only",
    1: "one pass over a single bit",
    256: "first span with 2 passes",
    2**16 - 1: "last span with 2 passes",
    2**16: "first span with 3 passes",
    2**24 - 1: "last span with 3 passes",
    2**24: "first span with 4 passes",
    2**32: "wide, 5 passes; the shifted key no longer fits 32 bits",
    2**56: "wide, 8 passes",
    FULL: "INT64_MIN..INT64_MAX: span 2^64-1, descending key is span - k",
}


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _check(k, what):
    col = lib.put(k)
    for ascending in (True, False):
        got = lib.sort_perm(col, ascending)
        assert got.np_dtype == np.int64 and got.length == k.size
        exp = oracle.sort_perm(k, ascending)
        assert np.array_equal(lib.get(got), exp), (what, ascending)


def _keys(rng, n, lo, span):
    """Uniform over [lo, lo + span], both endpoints forced present (from two
    rows on), so the kernel sees exactly this span."""
    k = rng.integers(lo, lo + span, n, endpoint=True, dtype=np.int64)
    k[n // 3] = lo
    if n > 1:
        k[(2 * n) // 3] = lo + span
    return k


def _span_case(n, span):
    rng = np.random.default_rng([n, span % 2**63])
    # minimum at zero, negative, and with the maximum at INT64_MAX (the
    # shifted key k - lo must not overflow); the full span has one placement
    los = [I64_MIN] if span == FULL else [0, -(span // 2), I64_MAX - span]
    for lo in los:
        _check(_keys(rng, n, lo, span), (n, span, lo))


@pytest.mark.parametrize("span", SPANS_ALL_SIZES, ids=lambda s: f"span{s}")
@pytest.mark.parametrize("n", SIZES)
def test_sort_perm_sizes(n, span):
    _span_case(n, span)


@pytest.mark.parametrize("span", SPANS_MID_SIZE, ids=lambda s: f"span{s}")
def test_sort_perm_spans(span):
    _span_case(MID, span)


def test_sort_perm_stable_under_heavy_duplication():
    rng = np.random.default_rng(31)
    # every 64-row step has many lanes per digit: the ballot rank and the
    # leader's base advance carry the whole order; narrow path
    _check(rng.integers(0, 3, MID), "3 keys narrow")
    # the same on the wide path; all but two digits of every pass are empty
    _check(rng.choice(np.array([0, 2**39, 2**40]), MID), "3 keys wide")
    _check(rng.choice(np.array([0, 2**40]), MID), "2 keys wide")
    # one distinct key: span 0, the permutation is the identity both ways
    _check(np.full(SORT_TILE + 1, -7, dtype=np.int64), "1 key")
    _check(np.full(SORT_TILE + 1, I64_MIN, dtype=np.int64), "1 key, minimum")


# 8192 wave-tiles fill the 2048-block grid cap; one more row gives block 0 a
# second tile in the grid-stride loops of k_sort_count / k_sort_scatter.
# 16384 tiles and 2049 rows make 16386 * 256 digit counts, the first count
# above 1024 scan tiles in sort_digit_offsets' k_compact_scan.
@pytest.mark.parametrize("n", [8192 * SORT_TILE + 1,
                               16384 * SORT_TILE + 2049])
def test_sort_perm_large_one_pass(n):
    rng = np.random.default_rng(n)
    k8 = rng.integers(0, 256, n, dtype=np.uint8)
    k8[n // 3], k8[(2 * n) // 3] = 0, 255
    got = lib.get(lib.sort_perm(lib.put(k8.astype(np.int64)), True))
    assert np.array_equal(got, np.argsort(k8, kind="stable"))


def test_sort_perm_large_wide_mostly_empty_digits():
    """Wide path, 6 passes, above 1024 scan tiles: five of the passes see a
    single digit, so every tile's whole count sits in one column of the
    transposed table."""
    n = 16384 * SORT_TILE + 2049
    rng = np.random.default_rng(n + 1)
    b = rng.integers(0, 2, n, dtype=np.uint8)
    b[n // 3], b[(2 * n) // 3] = 0, 1
    got = lib.get(lib.sort_perm(lib.put(b.astype(np.int64) << 40), True))
    assert np.array_equal(got, np.argsort(b, kind="stable"))


# ---- hf_ordered_i64 ---------------------------------------------------------

def _bits(*patterns):
    return np.array(patterns, dtype=np.uint64).view(np.float64)


def test_ordered_i64_transform():
    rng = np.random.default_rng(32)
    fi = np.finfo(np.float64)
    denorm = float(np.nextafter(0.0, 1.0))
    nans = _bits(0xFFF8000000000000, 0xFFF8000000000001, 0xFFFFFFFFFFFFFFFF,
                 0xFFF0000000000001, 0x7FF8000000000000, 0x7FF8000000000001,
                 0x7FFFFFFFFFFFFFFF, 0x7FF0000000000001)
    named = np.array([-np.inf, -fi.max, -1.0, -fi.tiny, -denorm, -0.0, 0.0,
                      denorm, fi.tiny, 1.0, np.nextafter(1.0, 2.0), fi.max,
                      np.inf])
    x = np.concatenate([nans, named,
                        rng.integers(0, 2**64, 10_000, dtype=np.uint64)
                        .view(np.float64)])
    x = x[rng.permutation(x.size)]
    col = lib.put(x)
    img_col = lib.ordered_i64(col)
    assert img_col.np_dtype == np.int64
    img = lib.get(img_col)
    nan = np.isnan(x)

    # the images are ordered exactly as the doubles; -0.0 == +0.0 share one
    order = np.argsort(img, kind="stable")
    xs, ims = x[order][~nan[order]], img[order][~nan[order]]
    assert np.array_equal(xs[:-1] < xs[1:], ims[:-1] < ims[1:])
    assert np.array_equal(xs[:-1] == xs[1:], ims[:-1] == ims[1:])
    assert (xs[:-1] <= xs[1:]).all()
    zero_img = img[x == 0.0]
    assert zero_img.size >= 2 and (zero_img == zero_img[0]).all()
    # every NaN, either sign, any payload: one value strictly above +inf's
    assert np.unique(img[nan]).size == 1
    assert img[nan][0] > img[x == np.inf][0] == img[~nan].max()

    # the inverse gives the canonical double back, bit for bit
    canon = x.copy()
    canon[x == 0.0] = 0.0
    canon[nan] = _bits(0x7FF8000000000000)[0]
    back_col = lib.ordered_i64(img_col, inverse=True)
    assert back_col.np_dtype == np.float64
    back = lib.get(back_col)
    assert np.array_equal(back.view(np.int64), canon.view(np.int64))
    assert np.array_equal(lib.ordered_to_f64_np(img).view(np.int64),
                          back.view(np.int64))

    # float keys on the int64 sort: stable, NaN last
    got = lib.get(lib.sort_perm(img_col, True))
    assert np.array_equal(got, np.argsort(x, kind="stable"))
