"""CPU tier of the join / row-movement boundary tests.

1. tests/join_ref.py earns its authority: inner_join_ref against
   pandas.merge(how="inner") on 200 seeded random cases with many duplicates.
2. Every case of tests/join_cases.py that is small enough runs through the
   same checkers as on the GPU, over tests/mocklib.py, so the cases are known
   to be consistent before a GPU run is spent.  Left out (join_cases.GPU_ONLY,
   the S- and 2^27-sized ones): slots[S], slots[S+1], occupancy[*-S+1],
   nleft[S+1], dup[4095-*], dup[4096-*], dup[4097-*], cap[1<<27].
3. The checkers are sensitive: six perturbations of the mock's output, each
   of which a comparison of lengths, sorted keys, sums or allclose would let
   through, make the checker of the named case raise AssertionError.
"""

import numpy as np
import pandas
import pytest

from modin_amd.core import lib
from tests import join_cases as jc
from tests import join_ref as ref
from tests import mocklib

T, G = jc.T, jc.G
ROW_SIZES = {"0": 0, "1": 1, "255": 255, "256": 256, "257": 257,
             "G-1": G - 1, "G": G, "G+1": G + 1}


@pytest.fixture()
def mlib(monkeypatch):
    mocklib.install(monkeypatch)
    yield lib


# ---- 1. the reference against pandas ----------------------------------------

def test_inner_join_ref_matches_pandas():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        nl, nr = rng.integers(0, 301, 2)
        span = int(rng.integers(1, 41))
        lkeys = rng.integers(0, span, nl).astype(np.int64)
        rkeys = rng.integers(0, span, nr).astype(np.int64)
        rv = rng.random(nr)
        m = pandas.DataFrame({"k": lkeys, "li": np.arange(nl)}).merge(
            pandas.DataFrame({"k": rkeys, "ri": np.arange(nr), "v": rv}),
            on="k", how="inner", sort=False)
        keys, lidx, ridx, (v,) = ref.inner_join_ref(lkeys, rkeys, [rv])
        for got, col in ((keys, "k"), (lidx, "li"), (ridx, "ri"), (v, "v")):
            np.testing.assert_array_equal(got, m[col].to_numpy(),
                                          err_msg=f"seed {seed}: {col}")


def test_search_sorted_ref_first_of_equals():
    s = np.array([1, 1, 1, 4, 4, 9], dtype=np.int64)
    k = np.array([0, 1, 2, 4, 9, 10], dtype=np.int64)
    np.testing.assert_array_equal(ref.search_sorted_ref(k, s),
                                  [-1, 0, -1, 3, 5, -1])
    assert ref.search_sorted_ref(k, s[:0]).tolist() == [-1] * 6


# ---- 2. the cases on the mock -----------------------------------------------

@pytest.mark.parametrize("name", jc.MOCK_CASES)
def test_mock_join_case(mlib, name):
    jc.check_join(mlib, jc.CASES[name]())


def test_every_case_is_in_one_tier():
    assert set(jc.MOCK_CASES) | set(jc.GPU_ONLY) == set(jc.CASES)
    assert not set(jc.MOCK_CASES) & set(jc.GPU_ONLY)


def test_mock_join_build_contract(mlib):
    """The mock refuses what hf_join_build refuses, in its words."""
    case = jc.nleft_case(10)
    rv = [mlib.put(v) for v in case.rvals]
    for bad in (case.key_min - 1, case.key_min + case.n_slots):
        rk = case.rkeys.copy()
        rk[3] = bad
        with pytest.raises(lib.HfError, match="outside"):
            mlib.join_build(mlib.put(rk), rv, case.key_min, case.n_slots)
    with pytest.raises(lib.HfError, match="range too large"):
        mlib.join_build(mlib.put(case.rkeys), rv, case.key_min,
                        (1 << 27) + 1)
    jc.check_join(mlib, jc.kmin_case("int64_min"))     # wraps, stays inside


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("top", [(1 << 27) - 1, 1 << 27],
                         ids=["dense-2^27-slots", "code-space-2^27+1"])
def test_mock_merge_at_the_slot_cap(mlib, top, nparts):
    """The frames of the GPU tier's cap test, against pandas; with 2^27 + 1
    slots _merge must go to code space, or the mock's join_build raises."""
    from modin_amd import config
    import modin_amd.pandas as mpd
    old = (config.NPartitions.get(), config.MinRowPartitionSize.get())
    config.NPartitions.put(nparts)
    config.MinRowPartitionSize.put(4)
    try:
        pl, pr = jc.cap_frames(top)
        got = mpd.DataFrame(pl).merge(mpd.DataFrame(pr), on="k",
                                      how="inner").to_pandas()
        pandas.testing.assert_frame_equal(got,
                                          pl.merge(pr, on="k", how="inner"))
    finally:
        config.NPartitions.put(old[0])
        config.MinRowPartitionSize.put(old[1])


@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 2**16 - 1, 2**16,
                               2**16 + 1])
def test_mock_search_sorted_m(mlib, m):
    jc.check_search_sorted(mlib, *jc.search_sorted_m_case(m))


@pytest.mark.parametrize("n", [0, 1, G - 1, G, G + 1])
def test_mock_search_sorted_n(mlib, n):
    jc.check_search_sorted(mlib, *jc.search_sorted_n_case(n))


def test_mock_search_sorted_ends_and_repeats(mlib):
    jc.check_search_sorted(mlib, *jc.search_sorted_ends_case())
    jc.check_search_sorted(mlib, *jc.search_sorted_repeats_case())


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", list(ROW_SIZES.values()), ids=list(ROW_SIZES))
def test_mock_gather_scatter(mlib, n, dtype):
    src = jc.column(max(n // 2, 1) + 3, dtype)
    jc.check_gather(mlib, src, jc.gather_idx(n, src.size))
    for fill in jc.fills_for(dtype):
        jc.check_gather_fill(mlib, src, jc.gather_fill_idx(n, src.size),
                             fill)
        jc.check_gather_fill(mlib, src[:1], np.full(n, -1, dtype=np.int64),
                             fill)
    jc.check_scatter(mlib, jc.column(n, dtype),
                     np.random.default_rng(n).permutation(n).astype(np.int64))


@pytest.mark.parametrize("nl,nr", jc.CROSS_SHAPES)
def test_mock_cross_idx(mlib, nl, nr):
    jc.check_cross_idx(mlib, nl, nr)


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("n", [0, 1, T, T + 1])
def test_mock_concat_slice(mlib, n, dtype):
    jc.check_concat_slice(mlib, jc.column(n, dtype))


# ---- 3. sensitivity ----------------------------------------------------------

def _perturbed_probe(monkeypatch, edit):
    """lib.join_probe's host arrays go through edit(cols) -> cols; cols is
    [keys, lidx, payload 0, ...].  Only the FIRST probe is edited, so the
    second-probe comparison also has something to find."""
    plain = lib.join_probe
    state = {"applied": False}

    def probe(j, lkeys):
        keys, lidx, rcols, n = plain(j, lkeys)
        cols = [c.arr.copy() for c in [keys, lidx] + rcols]
        if not state["applied"]:
            cols = edit(cols)
            state["applied"] = True
        cols = [mocklib.MockCol(c) for c in cols]
        return cols[0], cols[1], cols[2:], n

    monkeypatch.setattr(lib, "join_probe", probe)
    return state


def _first_pair_of_one_left_row(cols):
    lidx = cols[1]
    r = np.nonzero(lidx[1:] == lidx[:-1])[0]
    assert r.size, "the case has no multi-match row"
    return int(r[0])


def _swap_within_key(cols):
    r = _first_pair_of_one_left_row(cols)
    for c in cols[2:]:
        c[[r, r + 1]] = c[[r + 1, r]]
    return cols


def _tile_handoff(cols):
    lidx = cols[1]
    a = np.nonzero(lidx == T - 1)[0]
    b = np.nonzero(lidx == T)[0]
    assert a.size and b.size and a[-1] + 1 == b[0]
    order = np.arange(lidx.size)
    order[a[0]:b[-1] + 1] = np.concatenate([b, a])
    return [c[order] for c in cols]


def _other_nan(cols):
    f = next(c for c in cols[2:] if c.dtype == np.float64)
    at = np.nonzero(np.isnan(f))[0]
    assert at.size, "the case has no NaN payload"
    f.view(np.uint64)[at[0]] ^= np.uint64(1)
    assert np.isnan(f[at[0]])
    return cols


def _other_duplicate(cols):
    r = _first_pair_of_one_left_row(cols)
    cols[2][r] = cols[2][r + 1]         # the right row number alone
    return cols


JOIN_PERTURBATIONS = {
    "order_within_key": ("dup[64-first]", _swap_within_key),
    "tile_handoff": ("multi[3-tile_last]", _tile_handoff),
    "nan_payload_bits": ("payload[nr3]", _other_nan),
    "other_duplicate": ("match[all]", _other_duplicate),
}


@pytest.mark.parametrize("which", list(JOIN_PERTURBATIONS))
def test_join_checker_is_sensitive(mlib, monkeypatch, which):
    name, edit = JOIN_PERTURBATIONS[which]
    case = jc.CASES[name]()
    jc.check_join(mlib, case)                      # passes untouched
    state = _perturbed_probe(monkeypatch, edit)
    with pytest.raises(AssertionError):
        jc.check_join(mlib, case)
    assert state["applied"]


def _last_of_equals(keys, sorted_):
    p = np.searchsorted(sorted_.arr, keys.arr, side="right") - 1
    hit = (p >= 0) & (sorted_.arr[np.maximum(p, 0)] == keys.arr)
    return mocklib.MockCol(np.where(hit, p, -1).astype(np.int64))


def _last_for_above(plain):
    def search(keys, sorted_):
        out = plain(keys, sorted_).arr.copy()
        out[keys.arr > sorted_.arr[-1]] = sorted_.arr.size - 1
        return mocklib.MockCol(out)
    return search


@pytest.mark.parametrize("which", ["last_of_equals", "last_for_above"])
def test_search_sorted_checker_is_sensitive(mlib, monkeypatch, which):
    if which == "last_of_equals":
        case, wrong = jc.search_sorted_repeats_case(), _last_of_equals
    else:
        case = jc.search_sorted_m_case(65)
        wrong = _last_for_above(lib.search_sorted)
    jc.check_search_sorted(mlib, *case)            # passes untouched
    monkeypatch.setattr(lib, "search_sorted", wrong)
    with pytest.raises(AssertionError):
        jc.check_search_sorted(mlib, *case)
