"""GPU tier: boundary shapes of the three groupby paths a key range takes when
it does not fit the radix path:

  atomic  hf_groupby_accum -> k_gb_accum (global atomics on a dense table),
          then hf_groupby_compact
  hash    hf_groupby_hash_accum -> k_gb_hash_accum, hf_groupby_hash_compact,
          and the grow-and-retry loop of _groupby_hash
  sorted  hf_groupby_sorted -> k_head_flags, the filter plan, k_segagg, and
          the concat + sort + gather of _groupby_sorted in front of it

The cases, the reference (groupby_ref) and the checkers live in
tests/groupby_fallback_cases.py and ran on the CPU mock first
(test_mock_groupby_fallbacks.py), where the preconditions of the hash cases
are asserted on a serial model of the table.  Keys, counts, presence, min and
max are bit-exact; sums are bit-exact on integer-valued f64 and, in one
random case per path, within gamma(c - 1) * sum|x| of the exact sum.  Sizes:

  W = 64, B = 256, T = FILT_TILE = 4096, G = GRID_CAP * BLOCK = 1 048 576,
  R = 1024 << 13 = 8 388 608, PROBE = 4096.

Where each boundary is (test ids):
  atomic route[*]            n_slots = R still takes the radix path (gb_accum
                             launches 0 times), R + 1 the atomic one (once)
  atomic rows[0 .. 4G+1]     tail only, one pair, pair + tail, the grid-stride
                             wrap at G row pairs; an odd last row is the only
                             row of its group
  atomic kmin[*]             negative, INT64_MIN, range ending at INT64_MAX;
                             slot 0 and slot n_slots - 1 are always used
  atomic parts[odd+even]     two accumulate calls into one table
  atomic vals[*], inst[*]    NaN rows, an all-NaN group, +-inf; every
                             k_gb_accum instantiation the entry can select
  atomic out_of_range        one key on each side, pair loop and tail
  hash special[*]            INT64_MIN, the key of the extra slot H
  hash full[2 .. 4096]       H ordinary keys + INT64_MIN fill the table;
                             overflow[H] is one key more
  hash wrap                  a chain from slot H - 2 through slot 0
  hash probe[4096]           4096 keys on one home of an 8192-slot table fit,
                             4097 report "full" (probe_bound_overflow)
  hash retry                 _groupby_hash at H = 16384, then 65536
  hash rows[1 .. 2G+1]       the grid-stride wrap at G rows
  sorted shapes[0 .. 3T+1]   one run, every row a run, runs of 2, and one or
                             two extra heads at lanes 62..65, rows 127..257
                             and the tile edges T - 1, T, T + 1, 2T - 1, 2T
No case feeds an entry a key or index it does not guard: a dense slot is
written under ok0 / ok1 (and the tail's range test) only, and the hash probe
loop is bounded and skips the row it could not place.
"""

import gc

import numpy as np
import pytest

import modin_amd.pandas as mpd
from modin_amd import config
from modin_amd.core import lib
from tests import groupby_fallback_cases as fc

pytestmark = pytest.mark.gpu

T, G, R, PROBE = fc.T, fc.G, fc.R, fc.PROBE
assert (R, R + 1, 2 * G + 1, 4 * G + 1) == (8388608, 8388609, 2097153, 4194305)
assert (3 * T + 1, PROBE + 1, fc.BOUND_H, fc.RETRY_H, 4 * fc.RETRY_H) == \
    (12289, 4097, 8192, 16384, 65536)
assert fc.ATOMIC_SLOTS == R + 1 and fc.SORTED_INST_N == 2 * T + 1


@pytest.fixture(scope="module")
def live_at_start(gpu_ready):
    gc.collect()
    return lib.dev_live()


@pytest.fixture(autouse=True)
def _ready(gpu_ready, live_at_start):
    yield


@pytest.fixture()
def profiled():
    lib.profiling(True)
    lib.kernel_stats_reset()
    try:
        yield
    finally:
        lib.profiling(False)


def _launches(name):
    return lib.kernel_stats(name)[0]


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(request.param)
    config.MinRowPartitionSize.put(4)
    yield request.param
    config.NPartitions.put(old[0])
    config.MinRowPartitionSize.put(old[1])


def _calls(case):
    """Accumulate calls check_case makes: a keys-only case runs twice."""
    return len(case.parts) * (2 if case.nvals == 0 else 1)


# ---- 1. the global-atomic path ---------------------------------------------------

def test_radix_rl_gives_up_above_R():
    for wc in (False, True):
        assert lib.groupby_radix_rl(R, wc) != 0
        assert lib.groupby_radix_rl(R + 1, wc) == 0


@pytest.mark.parametrize("want_counts", [False, True],
                         ids=["nocounts", "counts"])
def test_atomic_route(profiled, want_counts):
    """n_slots = R is the last range of the radix path, R + 1 the first of
    k_gb_accum."""
    for n_slots, launches in ((R, 0), (R + 1, 1)):
        lib.kernel_stats_reset()
        case = fc.atomic_case(257, nvals=1, want_counts=want_counts,
                              n_slots=n_slots)
        fc.check_case(lib, case, fc.run_atomic, f"n_slots={n_slots}")
        assert _launches("gb_accum") == launches, n_slots


@pytest.mark.parametrize("name", list(fc.ATOMIC_CASES))
def test_atomic_case(profiled, name):
    case = fc.ATOMIC_CASES[name]()
    assert case.n_slots == R + 1
    fc.check_case(lib, case, fc.run_atomic, name)
    assert _launches("gb_accum") == _calls(case) >= 1


def test_atomic_reassociation(profiled):
    fc.check_reassoc(lib, fc.atomic_reassoc_case(), fc.run_atomic, "atomic")
    assert _launches("gb_accum") == 1


def test_atomic_out_of_range_keys_are_counted(profiled):
    """key_min - 1 in the pair loop and key_min + n_slots as the odd tail.
    k_gb_accum writes a slot under ok0 / ok1 (the tail under its own range
    test) and nowhere else, so the two rows are counted, not written; the
    compaction names the count and clears the error word."""
    case = fc.atomic_out_of_range_case()
    gc.collect()
    before = lib.dev_live()
    with pytest.raises(lib.HfError, match=r"\b2 keys fell outside"):
        fc.run_atomic(lib, case)
    gc.collect()
    assert lib.dev_live() == before
    fc.check_case(lib, fc.atomic_case(257, seed=9), fc.run_atomic)
    assert _launches("gb_accum") == 2


def test_atomic_end_to_end(profiled, npartitions):
    """A key span of R + 5 under the default MaxGroupbySlots."""
    pdf = fc.e2e_frame()
    assert pdf["k"].max() - pdf["k"].min() + 1 == R + 5
    assert R + 5 <= config.MaxGroupbySlots.get()
    fc.check_frame(mpd, pdf)
    assert _launches("gb_accum") >= 1
    assert _launches("gb_hash_accum") == 0


# ---- 2. the hash path ------------------------------------------------------------

@pytest.mark.parametrize("name", list(fc.HASH_CASES))
def test_hash_case(profiled, name):
    case = fc.HASH_CASES[name]()
    got = fc.check_case(lib, case, fc.run_hash, name)
    assert _launches("gb_hash_accum") == _calls(case)
    if name == "empty":
        assert got.n == 0 and _launches("gb_hash_accum") == 0
        assert all(a.size == 0 for a in got.aggs + got.counts)
    if name.startswith("full["):
        assert got.n == case.H + 1


def test_hash_reassociation(profiled):
    fc.check_reassoc(lib, fc.hash_reassoc_case(), fc.run_hash, "hash")
    assert _launches("gb_hash_accum") == 1


def _full_then_clean(case):
    """The probe loop of k_gb_hash_accum is bounded by min(H, 4096) and a row
    it cannot place is counted and skipped, never written.  The compaction
    raises and clears the flag: the next table must not see it."""
    gc.collect()
    before = lib.dev_live()
    with pytest.raises(lib.HfError, match="hash table full"):
        fc.run_hash(lib, case)
    gc.collect()
    assert lib.dev_live() == before
    fc.check_case(lib, fc.hash_rows_case(257), fc.run_hash)


@pytest.mark.parametrize("H", fc.FULL_H)
def test_hash_overflow(H):
    """H + 1 distinct ordinary keys in H slots."""
    _full_then_clean(fc.hash_full_case(H, extra=1))


def test_hash_probe_bound_overflow():
    """4097 keys on one home of an 8192-slot table: "full" while half empty."""
    _full_then_clean(fc._keyed_case(fc.bound_keys(PROBE + 1), fc.BOUND_H,
                                    nvals=1))


def test_hash_retry_grows_fourfold(profiled, npartitions):
    """_groupby_hash starts at H = 16384 for this frame, where 4097 of its
    keys share a home; the attempt reports a full table and the next one, at
    H = 65536, succeeds: every non-empty partition is accumulated twice."""
    pdf = fc.retry_frame()
    old = config.MaxGroupbySlots.get()
    config.MaxGroupbySlots.put(10)
    try:
        fc.check_frame(mpd, pdf, aggs=("sum",))
    finally:
        config.MaxGroupbySlots.put(old)
    assert _launches("gb_hash_accum") == 2 * npartitions
    assert _launches("gb_accum") == 0


# ---- 3. the sorted path -----------------------------------------------------------

@pytest.mark.parametrize("label", list(fc.ROWS_SORTED))
def test_sorted_shapes(profiled, label):
    n = fc.ROWS_SORTED[label]
    if n == 0:
        for nv in (0, 2):
            for wc in (False, True):
                got = fc.run_sorted(lib, fc.sorted_empty_case(nv, wc))
                assert got.n == 0 and got.keys.size == 0
                assert all(a.size == 0 and a.dtype == np.float64
                           for a in got.aggs)
        assert _launches("gb_segagg") == 0
        return
    shapes = fc.sorted_shapes(n)
    for what, heads in shapes:
        fc.check_case(lib, fc.sorted_shape_case(n, heads), fc.run_sorted,
                      f"n={n} {what}")
    assert _launches("gb_segagg") == 2 * len(shapes)


@pytest.mark.parametrize("name", list(fc.SORTED_CASES))
def test_sorted_case(profiled, name):
    case = fc.SORTED_CASES[name]()
    fc.check_case(lib, case, fc.run_sorted, name)
    # one launch per value column; keys only: one, and one for the ones
    assert _launches("gb_segagg") == (case.nvals or 2)


def test_sorted_reassociation(profiled):
    fc.check_reassoc(lib, fc.sorted_reassoc_case(), fc.run_sorted, "sorted")
    assert _launches("gb_segagg") == 1


def test_groupby_sorted_over_partitions(profiled):
    """Unsorted keys in partitions of 257, 0 and T + 43 rows through
    _groupby_sorted."""
    from modin_amd.core.partition_manager import \
        HipDataframePartitionManager as PM
    case = fc.unsorted_parts_case()
    assert [k.size for k, _ in case.parts] == [257, 0, T + 43]
    kcols = [lib.put(k) for k, _ in case.parts]
    vcols = [[lib.put(v) for v in vs] for _, vs in case.parts]
    k, s, c, n = PM._groupby_sorted(kcols, vcols, True, case.agg_op)
    got = fc.Got(lib.get(k), [lib.get(x) for x in s],
                 [lib.get(x) for x in c], n)
    fc.check_exact(got, fc.case_ref(case))
    assert _launches("gb_segagg") == 2


# ---- last: everything above gave its device blocks back --------------------------

def test_zz_dev_live_back_at_start(live_at_start):
    gc.collect()
    assert lib.dev_live() == live_at_start
