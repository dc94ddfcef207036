"""GPU tier: boundary shapes of the dense-range CSR join (hf_join_build /
hf_join_probe: k_hist_u32, k_tile_sums_u32, k_compact_scan, k_scan_apply_u32,
k_join_fill, k_join_fixup, the sorted refill, k_probe_count, k_probe_emit)
and of the row-movement entries (hf_search_sorted, hf_gather, hf_gather_fill,
hf_scatter, hf_cross_idx, hf_col_concat, hf_col_slice).

The cases and checkers live in tests/join_cases.py and ran on the CPU mock
first (test_mock_join_edges.py); the reference is tests/join_ref.py.  Every
comparison is bit-exact.  Sizes, as in join_cases:

  W = 64, B = 256, T = JOIN_TILE = 4096, G = GRID_CAP * BLOCK = 1 048 576,
  S = 1024 * T = 4 194 304.

Where each boundary of the join is (test_join_case ids):
  slots[1 .. S + 1]        n_slots around a wave, a block, a tile, two tiles
                           and the 1024 tiles of one k_compact_scan pass
  occupancy[*-2T+1|S+1]    which slots hold rows
  nright[0 .. G + 1]       right rows around the grid-stride wrap
  key_min[*]               negative, INT64_MIN, range ending at INT64_MAX
  dup[2 .. 4097-first|last]  order within a key: 4096 is the last in-thread
                           fixup, 4097 the first sorted refill
  refill[nr0|nr2|nr8]      a 4097-duplicate key next to keys of 2 to 4096
  payload[nr0 .. nr8]      every k_join_fill / k_probe_emit instantiation
  nleft[0 .. S + 1]        probe rows; S + 1 rows are 1025 probe tiles
  match[*], multi[*]       where in a wave, chunk and tile the matches sit
  cap[1<<27]               the largest dense build, 1 << 27 slots
No case passes an index outside its source column: the entries do not check
bounds, so the checkers assert the range on the host before every call.
"""

import gc

import numpy as np
import pandas
import pytest

import modin_amd.pandas as mpd
from modin_amd import config
from modin_amd.core import lib
from tests import join_cases as jc

pytestmark = pytest.mark.gpu

T, G, S, DUP, CAP = jc.T, jc.G, jc.S, jc.DUP, jc.CAP
assert (S + 1, DUP + 1, CAP, G + 1) == (4194305, 4097, 1 << 27, 1048577)
ROW_SIZES = {"0": 0, "1": 1, "255": 255, "256": 256, "257": 257,
             "G-1": G - 1, "G": G, "G+1": G + 1}


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


# ---- the join ----------------------------------------------------------------

@pytest.mark.parametrize("name", list(jc.CASES))
def test_join_case(profiled, name):
    """Build + two probes against inner_join_ref, and the order path taken:
    join_sortfill launches once where a key has more than 4096 right rows
    (4097 is the first) and not at all otherwise."""
    case = jc.CASES[name]()
    mult = np.unique(case.rkeys, return_counts=True)[1]
    refill = bool(mult.size) and int(mult.max()) > DUP
    jc.check_join(lib, case)
    assert _launches("join_sortfill") == (1 if refill else 0)
    assert _launches("join_fixup") == 1


def test_dup_cases_take_both_paths():
    """The multiplicities of the dup[] ids straddle the cap as intended."""
    assert jc.DUP_MULTS[-3:] == (4095, 4096, 4097)
    for m in jc.DUP_MULTS[:3]:
        c = jc.dup_case(m, "last")
        assert np.unique(c.rkeys, return_counts=True)[1].max() == m
        assert c.rkeys.size >= m * 4 * jc.B


def test_error_words_are_clean_after_a_failed_build(profiled):
    """A right side with an out-of-range key AND a 4097-duplicate key sets
    both device error words; the build raises "outside".  The next build,
    small and valid, must not see a stale fixup word: it would launch the
    sorted refill."""
    rng = np.random.default_rng(20)
    rkeys = np.r_[np.full(DUP + 1, 77), rng.integers(40, 1540, 3000),
                  [40 + 1500]].astype(np.int64)
    rng.shuffle(rkeys)
    rv = [lib.put(np.arange(rkeys.size, dtype=np.int64))]
    gc.collect()
    before = lib.dev_live()
    with pytest.raises(lib.HfError, match="outside"):
        lib.join_build(lib.put(rkeys), rv, 40, 1500)
    gc.collect()
    assert lib.dev_live() == before
    lib.kernel_stats_reset()
    jc.check_join(lib, jc.nleft_case(257))
    assert _launches("join_fixup") == 1
    assert _launches("join_sortfill") == 0
    # and a hist word left behind would fail this one
    jc.check_join(lib, jc.refill_case(1))
    assert _launches("join_sortfill") == 1


def test_no_match_output_is_empty_with_dtypes():
    case = jc.match_case("none")
    rk, rv = lib.put(case.rkeys), [lib.put(v) for v in case.rvals]
    j = lib.join_build(rk, rv, case.key_min, case.n_slots)
    keys, lidx, rcols, n = lib.join_probe(j, lib.put(case.lkeys))
    assert case.lkeys.size > 0 and n == 0
    assert lib.get(keys).dtype == np.int64 and lib.get(keys).size == 0
    assert lib.get(lidx).dtype == np.int64 and lib.get(lidx).size == 0
    assert [lib.get(c).dtype for c in rcols] == [v.dtype for v in case.rvals]
    assert all(lib.get(c).size == 0 for c in rcols)


def test_payload_dtypes_follow_inputs():
    case = jc.nr_case(8)
    assert {v.dtype for v in case.rvals} == {np.dtype(np.int64),
                                             np.dtype(np.float64)}
    j = lib.join_build(lib.put(case.rkeys), [lib.put(v) for v in case.rvals],
                       case.key_min, case.n_slots)
    _k, _l, rcols, _n = lib.join_probe(j, lib.put(case.lkeys[:300]))
    assert [c.np_dtype for c in rcols] == [v.dtype for v in case.rvals]


# ---- the slot cap --------------------------------------------------------------

def test_cap_plus_one_fails_clean():
    """n_slots = (1 << 27) + 1 is refused at the entry, before anything is
    allocated."""
    case = jc.cap_case(n_slots=CAP + 1)
    rk, rv = lib.put(case.rkeys), [lib.put(v) for v in case.rvals]
    gc.collect()
    before = lib.dev_live()
    with pytest.raises(lib.HfError, match="range too large"):
        lib.join_build(rk, rv, case.key_min, CAP + 1)
    gc.collect()
    assert lib.dev_live() == before


@pytest.fixture(params=[1, 3])
def npartitions(request):
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(request.param)
    config.MinRowPartitionSize.put(4)
    yield request.param
    config.NPartitions.put(old[0])
    config.MinRowPartitionSize.put(old[1])


@pytest.mark.parametrize("top,code_space", [(CAP - 1, False), (CAP, True)],
                         ids=["dense-2^27-slots", "code-space-2^27+1"])
def test_merge_at_the_slot_cap(profiled, npartitions, top, code_space):
    """Right keys {0, 2^27 - 1} span exactly 2^27 slots and build densely;
    {0, 2^27} span one more, and _merge joins in search_sorted code space."""
    pl, pr = jc.cap_frames(top)
    got = mpd.DataFrame(pl).merge(mpd.DataFrame(pr), on="k",
                                  how="inner").to_pandas()
    pandas.testing.assert_frame_equal(got, pl.merge(pr, on="k", how="inner"))
    if code_space:
        assert _launches("search_sorted") >= 1
    else:
        assert _launches("search_sorted") == 0


# ---- row movement --------------------------------------------------------------

@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 2**16 - 1, 2**16,
                               2**16 + 1])
def test_search_sorted_m(m):
    jc.check_search_sorted(lib, *jc.search_sorted_m_case(m))


@pytest.mark.parametrize("n", [0, 1, G - 1, G, G + 1])
def test_search_sorted_n(n):
    jc.check_search_sorted(lib, *jc.search_sorted_n_case(n))


def test_search_sorted_int64_ends_and_repeats():
    jc.check_search_sorted(lib, *jc.search_sorted_ends_case())
    jc.check_search_sorted(lib, *jc.search_sorted_repeats_case())


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", list(ROW_SIZES.values()), ids=list(ROW_SIZES))
def test_gather(n, dtype):
    src = jc.column(max(n // 2, 1) + 3, dtype)
    jc.check_gather(lib, src, jc.gather_idx(n, src.size))


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", list(ROW_SIZES.values()), ids=list(ROW_SIZES))
def test_gather_fill(n, dtype):
    src = jc.column(max(n // 2, 1) + 3, dtype)
    idx = jc.gather_fill_idx(n, src.size)
    all_missing = np.full(n, -1, dtype=np.int64)
    for fill in jc.fills_for(dtype):
        jc.check_gather_fill(lib, src, idx, fill)
        jc.check_gather_fill(lib, src[:1], all_missing, fill)


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", list(ROW_SIZES.values()), ids=list(ROW_SIZES))
def test_scatter(n, dtype):
    perm = np.random.default_rng(n).permutation(n).astype(np.int64)
    jc.check_scatter(lib, jc.column(n, dtype), perm)


@pytest.mark.parametrize("nl,nr", jc.CROSS_SHAPES)
def test_cross_idx(nl, nr):
    jc.check_cross_idx(lib, nl, nr)


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", [0, 1, T, T + 1])
def test_concat_slice(n, dtype):
    jc.check_concat_slice(lib, jc.column(n, dtype))


# ---- last: everything above gave its device blocks back ------------------------

def test_zz_dev_live_back_at_start(live_at_start):
    gc.collect()
    assert lib.dev_live() == live_at_start
