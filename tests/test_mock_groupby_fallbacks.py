"""CPU tier of the fallback-groupby boundary tests (atomic, hash, sorted).

1. The tools earn their authority: groupby_ref against pandas on seeded
   random cases, unmix against oracle.ops._mix64, the serial table model and
   the serial k_segagg model against groupby_ref.
2. Each hash case's precondition is asserted on the serial table model: which
   cases fit, which overflow, that the wrap case wraps and that the probe
   bound is met exactly.  The mock does not model table fullness, so the
   overflow, probe-bound and retry cases themselves run on the GPU tier only.
3. Every case of tests/groupby_fallback_cases.py runs through the same
   drivers and checkers as on the GPU, over tests/mocklib.py.  Left to the GPU
   tier: the launch counts, the error words, and the empty sorted input with
   value columns (the mock returns no columns for it).
4. The checkers are sensitive: a lost odd tail row, a probe step without the
   mask, a result without the INT64_MIN slot and an exclusive run-number mask
   each make the check of the named case fail.
"""

import numpy as np
import pandas
import pytest

from modin_amd import config
from modin_amd.core import lib
from oracle.ops import _mix64
from tests import groupby_fallback_cases as fc
from tests import mocklib

T, G, R = fc.T, fc.G, fc.R
I64MIN, I64MAX = fc.I64MIN, fc.I64MAX


@pytest.fixture()
def mlib(monkeypatch):
    mocklib.install(monkeypatch)
    yield lib


# ---- 1. the tools -------------------------------------------------------------

def test_sizes():
    assert (fc.W, fc.B, T, G, R) == (64, 256, 4096, 1048576, 8388608)
    assert fc.ATOMIC_SLOTS == R + 1 and fc.PROBE == 4096


def test_unmix_round_trip():
    rng = np.random.default_rng(1)
    x = np.r_[rng.integers(0, 2**64, 10000, dtype=np.uint64),
              np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 1], dtype=np.uint64)]
    np.testing.assert_array_equal(_mix64(fc.unmix(x)), x)
    np.testing.assert_array_equal(fc.unmix(_mix64(x)), x)
    for H, home in [(2, 1), (64, 63), (8192, 5), (1 << 14, 77)]:
        k = fc.keys_with_home(home, 100, H)
        assert (fc.homes(k, H) == home).all()


def test_groupby_ref_matches_pandas():
    for seed in range(60):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(0, 400))
        keys = rng.integers(-20, 20, n).astype(np.int64)
        v = rng.integers(-50, 51, n).astype(np.float64)
        v[rng.random(n) < 0.3] = np.nan
        gb = pandas.DataFrame({"k": keys, "v": v}).groupby("k")["v"]
        for op, exp in ((fc.AGG_SUM, gb.sum()), (fc.AGG_MIN, gb.min()),
                        (fc.AGG_MAX, gb.max())):
            ref = fc.groupby_ref(keys, [v], op, True)
            np.testing.assert_array_equal(ref.keys, exp.index.to_numpy())
            np.testing.assert_array_equal(ref.counts[0],
                                          gb.count().to_numpy())
            np.testing.assert_array_equal(ref.rows, gb.size().to_numpy())
            want = exp.to_numpy().copy()
            want[ref.counts[0] == 0] = fc.IDENT[op]
            np.testing.assert_array_equal(ref.aggs[0], want)
    assert fc.groupby_ref(keys, [v], 0, False).counts is None


def test_groupby_ref_sums_are_fsum():
    keys = np.zeros(4, dtype=np.int64)
    v = np.array([1e100, 1.0, -1e100, np.nan])
    assert fc.groupby_ref(keys, [v], fc.AGG_SUM, True).aggs[0][0] == 1.0


# ---- 2. hash preconditions on the serial table model ----------------------------

def _fits(keys, H):
    m = fc.table_model(keys, H)
    return m.failed == 0, m


def test_model_special_slot_and_duplicates():
    m = fc.table_model(np.array([I64MIN, 5, 5, I64MIN, 7], np.int64), 4)
    assert m.special and m.failed == 0 and m.occupied == 2
    assert m.slot_of[I64MIN] == 4


@pytest.mark.parametrize("H", fc.FULL_H)
def test_full_cases_fit_and_one_more_key_does_not(H):
    ok, m = _fits(fc.full_keys(H), H)
    assert ok and m.occupied == H and m.special
    ok, m = _fits(fc.full_keys(H, extra=1), H)
    assert not ok and m.failed == 1 and m.occupied == H


def test_wrap_case_wraps(table_model=fc.table_model):
    keys = fc.wrap_keys()
    m = table_model(keys, fc.WRAP_H)
    assert m.failed == 0 and m.wrapped and m.max_probes >= 5
    used = sorted(m.slot_of.values())
    assert used == [0, 1, 2, 3, 4, 5, 62, 63]


def test_probe_bound_cases():
    H = fc.BOUND_H
    ok, m = _fits(fc.bound_keys(4096), H)
    assert ok and m.max_probes == 4096 and not m.wrapped
    ok, m = _fits(fc.bound_keys(4097), H)
    assert not ok and m.failed == 1 and m.occupied == 4096 < H // 2 + 1


def test_retry_frame_overflows_once():
    pdf = fc.retry_frame()
    keys = pdf["k"].to_numpy()
    assert 4097 <= keys.size <= 8192 and np.unique(keys).size == 4097
    # where _groupby_hash starts for this row count
    assert 1 << max(12, min(27, (2 * keys.size - 1).bit_length())) \
        == fc.RETRY_H
    assert not _fits(keys, fc.RETRY_H)[0]
    assert _fits(keys, 4 * fc.RETRY_H)[0]


@pytest.mark.parametrize("name", list(fc.HASH_CASES))
def test_every_hash_case_fits(name):
    case = fc.HASH_CASES[name]()
    keys, _ = fc.all_rows(case)
    ok, m = _fits(keys, case.H)
    assert ok
    if name.startswith(("rows[", "special[")) and keys.size >= 3:
        assert m.special and keys.min() == I64MIN


# ---- 3. the cases on the mock ---------------------------------------------------

@pytest.mark.parametrize("name", list(fc.ATOMIC_CASES))
def test_mock_atomic_case(mlib, name):
    case = fc.ATOMIC_CASES[name]()
    keys, _ = fc.all_rows(case)
    slot = keys.view(np.uint64) - np.uint64(case.key_min % 2**64)
    assert (slot < np.uint64(case.n_slots)).all()
    if keys.size >= 2:
        assert slot.min() == 0 and slot.max() == case.n_slots - 1
    if keys.size % 2:       # the odd tail is the only row of its group
        assert (keys == keys[-1]).sum() == 1
    fc.check_case(mlib, case, fc.run_atomic, name)


def test_mock_atomic_out_of_range_rows_are_not_written(mlib):
    """The mock drops rows outside the range as the kernel does (it does not
    count them); the case has exactly two, one in the pair loop and one as
    the odd tail."""
    case = fc.atomic_out_of_range_case()
    (keys, vals), = case.parts
    slot = keys.view(np.uint64) - np.uint64(case.key_min % 2**64)
    bad = np.nonzero(slot >= np.uint64(case.n_slots))[0]
    assert bad.tolist() == [10, 256] and keys.size == 257
    inside = case._replace(parts=[(np.delete(keys, bad),
                                   [np.delete(v, bad) for v in vals])])
    fc.check_exact(fc.run_atomic(mlib, case), fc.case_ref(inside))


@pytest.mark.parametrize("name", list(fc.HASH_CASES))
def test_mock_hash_case(mlib, name):
    fc.check_case(mlib, fc.HASH_CASES[name](), fc.run_hash, name)


@pytest.mark.parametrize("label", list(fc.ROWS_SORTED))
def test_mock_sorted_shapes(mlib, label):
    n = fc.ROWS_SORTED[label]
    if n == 0:
        for wc in (False, True):
            got = fc.run_sorted(mlib, fc.sorted_empty_case(0, wc))
            assert got.n == 0 and got.keys.size == 0
        return
    for what, heads in fc.sorted_shapes(n):
        case = fc.sorted_shape_case(n, heads)
        assert fc.case_ref(case).keys.size == len(np.unique(heads))
        fc.check_case(mlib, case, fc.run_sorted, f"n={n} {what}")


@pytest.mark.parametrize("name", list(fc.SORTED_CASES))
def test_mock_sorted_case(mlib, name):
    fc.check_case(mlib, fc.SORTED_CASES[name](), fc.run_sorted, name)


@pytest.mark.parametrize("path", ["atomic", "hash", "sorted"])
def test_mock_reassociation_case(mlib, path):
    case, run = {"atomic": (fc.atomic_reassoc_case, fc.run_atomic),
                 "hash": (fc.hash_reassoc_case, fc.run_hash),
                 "sorted": (fc.sorted_reassoc_case, fc.run_sorted)}[path]
    fc.check_reassoc(mlib, case(), run, path)


def test_mock_groupby_sorted_over_partitions(mlib):
    from modin_amd.core.partition_manager import \
        HipDataframePartitionManager as PM
    case = fc.unsorted_parts_case()
    assert [k.size for k, _ in case.parts] == [257, 0, T + 43]
    kcols = [mlib.put(k) for k, _ in case.parts]
    vcols = [[mlib.put(v) for v in vs] for _, vs in case.parts]
    k, s, c, n = PM._groupby_sorted(kcols, vcols, True, case.agg_op)
    got = fc.Got(mlib.get(k), [mlib.get(x) for x in s],
                 [mlib.get(x) for x in c], n)
    fc.check_exact(got, fc.case_ref(case))


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(request.param)
    config.MinRowPartitionSize.put(4)
    yield request.param
    config.NPartitions.put(old[0])
    config.MinRowPartitionSize.put(old[1])


def test_mock_end_to_end_wide_range(mlib, npartitions):
    import modin_amd.pandas as mpd
    pdf = fc.e2e_frame()
    assert pdf["k"].max() - pdf["k"].min() + 1 == R + 5
    assert R + 5 <= config.MaxGroupbySlots.get()
    fc.check_frame(mpd, pdf, aggs=("sum", "mean"))


def test_mock_retry_frame(mlib, npartitions):
    import modin_amd.pandas as mpd
    old = config.MaxGroupbySlots.get()
    config.MaxGroupbySlots.put(10)
    try:
        fc.check_frame(mpd, fc.retry_frame(), aggs=("sum", "count"))
    finally:
        config.MaxGroupbySlots.put(old)


# ---- 4. sensitivity --------------------------------------------------------------

def test_lost_tail_row_is_noticed(mlib, monkeypatch):
    """k_gb_accum without its odd-row tail."""
    plain = lib.groupby_accum

    def no_tail(keys, vals, *rest):
        n = keys.length & ~1
        plain(mocklib.MockCol(keys.arr[:n]),
              [mocklib.MockCol(v.arr[:n]) for v in vals], *rest)

    for name in ("rows[1]", "rows[257]", "rows[2G+1]", "inst[sum-nv0-nocounts]"):
        case = fc.ATOMIC_CASES[name]()
        monkeypatch.setattr(lib, "groupby_accum", no_tail)
        with pytest.raises(AssertionError):
            fc.check_case(mlib, case, fc.run_atomic, name)
        monkeypatch.setattr(lib, "groupby_accum", plain)


def test_doubled_tail_row_is_noticed(mlib, monkeypatch):
    plain = lib.groupby_accum

    def twice(keys, vals, *rest):
        plain(keys, vals, *rest)
        if keys.length & 1:
            plain(mocklib.MockCol(keys.arr[-1:]),
                  [mocklib.MockCol(v.arr[-1:]) for v in vals], *rest)

    monkeypatch.setattr(lib, "groupby_accum", twice)
    with pytest.raises(AssertionError):
        fc.check_case(mlib, fc.ATOMIC_CASES["rows[257]"](), fc.run_atomic)


def test_probe_step_without_mask_is_noticed():
    def no_mask(keys, H):
        return fc.table_model(keys, H, wrap=False)

    with pytest.raises(AssertionError):
        test_wrap_case_wraps(table_model=no_mask)


def test_forgotten_special_slot_is_noticed(mlib, monkeypatch):
    plain = lib.groupby_hash_compact

    def without_slot_h(*a):
        k, s, c, n = plain(*a)
        keep = k.arr != I64MIN
        cut = lambda col: mocklib.MockCol(col.arr[keep])
        return (cut(k), [cut(x) for x in s],
                [cut(x) for x in c] if c is not None else None,
                int(keep.sum()))

    monkeypatch.setattr(lib, "groupby_hash_compact", without_slot_h)
    for name in ("special[only]", "special[mixed]", "full[4]", "rows[257]"):
        with pytest.raises(AssertionError):
            fc.check_case(mlib, fc.HASH_CASES[name](), fc.run_hash, name)
    fc.check_case(mlib, fc.HASH_CASES["wrap"](), fc.run_hash)


def _segagg_against_ref(n, heads, inclusive):
    case = fc.sorted_shape_case(n, heads)
    (keys, vals), = case.parts
    head = np.r_[True, keys[1:] != keys[:-1]]
    sums, counts = fc.segagg_model(head, vals[1], inclusive)
    ref = fc.case_ref(case)
    np.testing.assert_array_equal(sums, ref.aggs[1])
    np.testing.assert_array_equal(counts, ref.counts[1])


@pytest.mark.parametrize("n", [65, 257, T + 1])
def test_exclusive_run_mask_is_noticed(n):
    """k_segagg with (1 << lane) - 1 in place of (2 << lane) - 1: a head row
    goes to the run in front of its own (row 0 to none), so every shape
    notices."""
    for what, heads in fc.sorted_shapes(n):
        _segagg_against_ref(n, heads, inclusive=True)
        with pytest.raises(AssertionError):
            _segagg_against_ref(n, heads, inclusive=False)
