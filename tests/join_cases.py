"""Boundary cases and checkers for hf_join_build / hf_join_probe and the
row-movement entries, shared by the CPU mock tier (test_mock_join_edges.py)
and the GPU tier (test_gpu_join_edges.py).

Every case is built on demand from a name, so importing this module allocates
nothing, and a test holds one case at a time.  The checkers take the library
module as an argument: `modin_amd.core.lib` itself on the GPU, the same
module with tests/mocklib.py installed on the CPU.  All comparisons are
bit-exact (int64 views), against tests/join_ref.py.

Sizes the kernels switch on:
  W  wave, B block, T = JOIN_TILE (slots per build-scan tile, left rows per
  probe tile), G = GRID_CAP * BLOCK (first row a grid-stride kernel reaches
  on its second trip), S = 1024 * T (tiles one k_compact_scan pass folds),
  DUP = JOIN_MAX_DUP (in-thread order fixup up to here, sorted refill above),
  CAP = the largest dense slot range.
"""

import functools
from collections import namedtuple

import numpy as np

from tests import join_ref as ref

W, B, T = 64, 256, 4096
G = 4096 * B                  # 1 048 576
S = 1024 * T                  # 4 194 304
DUP = 4096
CAP = 1 << 27
I64MIN, I64MAX = -2**63, 2**63 - 1

JoinCase = namedtuple("JoinCase", "lkeys rkeys rvals key_min n_slots")

# quiet NaNs (plain, with payload, negative), signalling NaNs, -0.0, +-inf,
# the smallest denormal, 1.0
F64_BITS = np.array([0x7FF8000000000000, 0x7FF8000000000123,
                     0xFFF8000000000000, 0x7FF0000000000001,
                     0xFFF4000000000BAD, 0x8000000000000000,
                     0x7FF0000000000000, 0xFFF0000000000000,
                     0x0000000000000001, 0x3FF0000000000000],
                    dtype=np.uint64)
I64_EDGES = np.array([I64MIN, I64MAX, -1, 0, I64MIN + 1], dtype=np.int64)


def f64_specials(n, seed):
    u = np.random.default_rng(seed).random(n).view(np.uint64).copy()
    k = u[::3].size
    u[::3] = F64_BITS[(np.arange(k) + seed) % F64_BITS.size]
    return u.view(np.float64)


def i64_specials(n, seed):
    v = np.random.default_rng(seed).integers(-99, 99, n).astype(np.int64)
    k = v[::4].size
    v[::4] = I64_EDGES[(np.arange(k) + seed) % I64_EDGES.size]
    return v


def payloads(n, nr, seed=0):
    """nr columns of n rows: the right row number first, then float64 and
    int64 columns of special bit patterns in turn."""
    cols = []
    for c in range(nr):
        if c == 0:
            cols.append(np.arange(n, dtype=np.int64))
        elif c % 2:
            cols.append(f64_specials(n, seed + c))
        else:
            cols.append(i64_specials(n, seed + c))
    return cols


def _i64(vals):
    return np.array(list(vals), dtype=np.int64)


def misses(key_min, n_slots):
    """Keys next to the slot range and at the ends of int64 (those that
    exist).  An end of int64 that lies inside the range is a hit there, and
    the reference says so."""
    cand = [key_min - 1, key_min + n_slots, I64MIN, I64MAX]
    return _i64(k for k in cand if I64MIN <= k <= I64MAX)


def left_all_slots(key_min, n_slots):
    """Every slot's key in order, with the misses in front, in the middle
    and at the end."""
    keys = np.int64(key_min) + np.arange(n_slots, dtype=np.int64)
    m = misses(key_min, n_slots)
    h = n_slots // 2
    return np.concatenate([m, keys[:h], m, keys[h:], m])


def right_from_slots(slots, key_min, nr, seed, shuffle=True):
    slots = np.asarray(slots, dtype=np.int64)
    if shuffle:
        slots = np.random.default_rng(seed).permutation(slots)
    return np.int64(key_min) + slots, payloads(slots.size, nr, seed)


def ntiles(n):
    return (n + T - 1) // T


# ---- build: CSR scan -------------------------------------------------------

def occupancy_slots(n_slots, pattern):
    nt = ntiles(n_slots)
    if pattern == "every":
        return np.arange(n_slots, dtype=np.int64)
    if pattern == "slot0":
        return _i64([0])
    if pattern == "last":
        return _i64([n_slots - 1])
    if pattern == "tile_edges":     # last slot of a tile, first of the next
        t = np.arange(1, nt, dtype=np.int64) * T
        return np.sort(np.concatenate([t - 1, t]))
    if pattern == "tile_gap":       # full, (empty ...), full, EMPTY, full
        full = sorted({0, max(nt - 3, 0), nt - 1})
        return np.concatenate([np.arange(t * T, min((t + 1) * T, n_slots),
                                         dtype=np.int64) for t in full])
    if pattern == "single":         # DUP rows in the first slot of the last tile
        return np.full(DUP, (nt - 1) * T, dtype=np.int64)
    raise KeyError(pattern)


def build_case(n_slots, pattern="every", key_min=-17, nr=2, seed=1):
    rkeys, rvals = right_from_slots(occupancy_slots(n_slots, pattern),
                                    key_min, nr, seed)
    return JoinCase(left_all_slots(key_min, n_slots), rkeys, rvals, key_min,
                    n_slots)


def nright_case(n_right, seed=2):
    """Round-robin keys: multiplicity n_right / n_slots, far below DUP."""
    n_slots = 300 if n_right <= 257 else 2 * T + 1
    key_min = 1000
    slots = np.arange(n_right, dtype=np.int64) % n_slots
    rkeys, rvals = right_from_slots(slots, key_min, 2, seed, shuffle=False)
    return JoinCase(left_all_slots(key_min, n_slots), rkeys, rvals, key_min,
                    n_slots)


def kmin_case(which, n_slots=T + 1):
    key_min = {"neg": -(10**12), "int64_min": I64MIN,
               "to_int64_max": I64MAX - n_slots + 1}[which]
    return build_case(n_slots, "every", key_min=key_min, seed=3)


# ---- order within a key ----------------------------------------------------

def dup_case(mult, where, nr=2, seed=4):
    """One key held by `mult` right rows spread over the whole right column,
    4 blocks apart on average; every other right row has a key of its own."""
    n_right = mult * 4 * B
    n_slots = n_right - mult + 1
    key_min = -5
    rng = np.random.default_rng(seed + mult)
    slot = 0 if where == "first" else n_slots - 1
    others = np.arange(n_slots, dtype=np.int64)
    others = rng.permutation(others[others != slot])
    slots = np.empty(n_right, dtype=np.int64)
    at = np.sort(rng.choice(n_right, mult, replace=False))
    mask = np.zeros(n_right, dtype=bool)
    mask[at] = True
    slots[mask] = slot
    slots[~mask] = others
    rkeys, rvals = right_from_slots(slots, key_min, nr, seed, shuffle=False)
    k = key_min + slot
    lkeys = np.concatenate([misses(key_min, n_slots),
                            _i64([k, key_min + n_slots // 2, k,
                                  key_min + (0 if slot else n_slots - 1)])])
    return JoinCase(lkeys, rkeys, rvals, key_min, n_slots)


REFILL_MULTS = (DUP + 1, DUP, DUP - 1, 257, 65, 64, 3, 2)
REFILL_MULTS_LIGHT = (DUP + 1, 1025, 513, 257, 65, 64, 3, 2)


def refill_case(nr, seed=5):
    """A key past the cap next to keys of 2 to DUP duplicates and single
    ones, all shuffled: the refill overwrites what the fixup sorted.  The
    in-thread sort of a DUP-row run moves every payload column about DUP^2/4
    times, so only the two-column case carries the DUP and DUP - 1 runs; the
    other column counts stop at 1025."""
    n_slots = 500
    key_min = 40
    mult = np.ones(n_slots, dtype=np.int64)
    mult[[7, 8, 100, 101, 250, 251, 498, 499]] = \
        REFILL_MULTS if nr == 2 else REFILL_MULTS_LIGHT
    mult[[3, 300]] = 0
    slots = np.repeat(np.arange(n_slots, dtype=np.int64), mult)
    rkeys, rvals = right_from_slots(slots, key_min, nr, seed)
    rng = np.random.default_rng(seed)
    lkeys = np.concatenate([left_all_slots(key_min, n_slots),
                            key_min + rng.integers(-3, n_slots + 3, 700)])
    return JoinCase(lkeys, rkeys, rvals, key_min, n_slots)


# ---- payload columns -------------------------------------------------------

def nr_case(nr, seed=6):
    n_slots = T + 1
    key_min = -100
    mult = np.random.default_rng(seed).integers(0, 4, n_slots)
    mult[[0, T - 1, T]] = (2, 3, 2)
    slots = np.repeat(np.arange(n_slots, dtype=np.int64), mult)
    rkeys, rvals = right_from_slots(slots, key_min, nr, seed + nr)
    return JoinCase(left_all_slots(key_min, n_slots), rkeys, rvals, key_min,
                    n_slots)


# ---- probe -----------------------------------------------------------------

def nleft_case(n_left, seed=7):
    n_slots = 300
    key_min = -150
    rng = np.random.default_rng(seed)
    mult = rng.integers(0, 3, n_slots)
    slots = np.repeat(np.arange(n_slots, dtype=np.int64), mult)
    rkeys, rvals = right_from_slots(slots, key_min, 2, seed)
    lkeys = key_min + rng.integers(-10, n_slots + 10, n_left)
    return JoinCase(lkeys.astype(np.int64), rkeys, rvals, key_min, n_slots)


MATCH_PATTERNS = {
    "lane0": lambda i: i % W == 0,
    "lane63": lambda i: i % W == W - 1,
    "chunk_last": lambda i: i % B == B - 1,
    "wave1_misses": lambda i: (i % B) // W != 1,
    "mid_tile_misses": lambda i: (i < T) | (i >= 2 * T),
    "none": lambda i: np.zeros(i.size, dtype=bool),
    "all": lambda i: np.ones(i.size, dtype=bool),
}


def match_case(pattern, n_left=2 * T + 1, seed=8):
    """Right keys 0..99 with 1 to 3 rows each; a left row holds one of them
    where the pattern says so and a miss elsewhere."""
    n_slots = 100
    slots = np.repeat(np.arange(n_slots, dtype=np.int64),
                      np.arange(n_slots) % 3 + 1)
    rkeys, rvals = right_from_slots(slots, 0, 3, seed)
    i = np.arange(n_left, dtype=np.int64)
    miss = np.where(i % 2 == 0, -5, n_slots + 900)
    lkeys = np.where(MATCH_PATTERNS[pattern](i), (i * 7) % n_slots, miss)
    return JoinCase(lkeys.astype(np.int64), rkeys, rvals, 0, n_slots)


MULTI_ROWS = {"lane63": W + W - 1, "chunk_last": 3 * B + B - 1,
              "tile_last": T - 1, "tile_first": T}


def multi_case(mult, where, n_left=2 * T + 1, seed=9):
    """Key 7 has `mult` right rows and one left row; all other left rows
    match one right row each."""
    n_slots = 1000
    m = np.ones(n_slots, dtype=np.int64)
    m[7] = mult
    slots = np.repeat(np.arange(n_slots, dtype=np.int64), m)
    rkeys, rvals = right_from_slots(slots, 0, 2, seed)
    lkeys = (np.arange(n_left, dtype=np.int64) * 11) % n_slots
    lkeys[lkeys == 7] = 8
    lkeys[MULTI_ROWS[where]] = 7
    return JoinCase(lkeys, rkeys, rvals, 0, n_slots)


# ---- cap -------------------------------------------------------------------

def cap_case(n_slots=CAP, key_min=-3):
    rkeys = _i64([key_min + n_slots - 1, key_min])
    lkeys = _i64([key_min, key_min + 12345, key_min + n_slots - 1,
                  key_min - 1, key_min + n_slots, key_min])
    return JoinCase(lkeys, rkeys, payloads(2, 2, 10), key_min, n_slots)


def cap_frames(top):
    """pandas frames for a merge whose right keys are {0, top}."""
    import pandas
    lk = _i64([0, top, 5, top, 0, top - 1, 1, top] * 5)
    left = pandas.DataFrame({"k": lk, "a": np.arange(lk.size) * 0.5})
    right = pandas.DataFrame({"k": _i64([top, 0]), "b": [1.5, -2.5],
                              "c": _i64([7, I64MIN])})
    return left, right


# ---- registry --------------------------------------------------------------

SLOT_SIZES = {"1": 1, "63": 63, "64": 64, "65": 65, "255": 255, "256": 256,
              "257": 257, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T,
              "2T+1": 2 * T + 1, "S": S, "S+1": S + 1}
OCC_PATTERNS = ("every", "slot0", "last", "tile_edges", "tile_gap", "single")
OCC_SIZES = {"2T+1": 2 * T + 1, "S+1": S + 1}
NRIGHT_SIZES = {"0": 0, "1": 1, "255": 255, "256": 256, "257": 257,
                "G-1": G - 1, "G": G, "G+1": G + 1}
DUP_MULTS = (2, 3, 64, 65, 257, DUP - 1, DUP, DUP + 1)   # 4095, 4096, 4097
NLEFT_SIZES = {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "255": 255,
               "256": 256, "257": 257, "T-1": T - 1, "T": T, "T+1": T + 1,
               "2T+1": 2 * T + 1, "S+1": S + 1}

CASES = {}
for _tag, _n in SLOT_SIZES.items():
    CASES[f"slots[{_tag}]"] = functools.partial(build_case, _n)
for _tag, _n in OCC_SIZES.items():
    for _p in OCC_PATTERNS:
        CASES[f"occupancy[{_p}-{_tag}]"] = functools.partial(build_case, _n,
                                                             _p)
for _tag, _n in NRIGHT_SIZES.items():
    CASES[f"nright[{_tag}]"] = functools.partial(nright_case, _n)
for _w in ("neg", "int64_min", "to_int64_max"):
    CASES[f"key_min[{_w}]"] = functools.partial(kmin_case, _w)
for _m in DUP_MULTS:
    for _w in ("first", "last"):
        CASES[f"dup[{_m}-{_w}]"] = functools.partial(dup_case, _m, _w)
for _nr in (0, 2, 8):
    CASES[f"refill[nr{_nr}]"] = functools.partial(refill_case, _nr)
for _nr in range(9):
    CASES[f"payload[nr{_nr}]"] = functools.partial(nr_case, _nr)
for _tag, _n in NLEFT_SIZES.items():
    CASES[f"nleft[{_tag}]"] = functools.partial(nleft_case, _n)
for _p in MATCH_PATTERNS:
    CASES[f"match[{_p}]"] = functools.partial(match_case, _p)
for _m in (3, 300):
    for _w in MULTI_ROWS:
        CASES[f"multi[{_m}-{_w}]"] = functools.partial(multi_case, _m, _w)
CASES["cap[1<<27]"] = cap_case

# The S- and 2^27-sized cases: millions of rows through the mock's pandas
# merge would take minutes, so they run on the GPU tier only.
#   slots[S], slots[S+1], occupancy[*-S+1], nleft[S+1]: S or more slots/rows
#   dup[4095-*], dup[4096-*], dup[4097-*]: about S right rows (4 blocks per
#     duplicate)
#   cap[1<<27]: 2^27 slots
GPU_ONLY = (["slots[S]", "slots[S+1]", "nleft[S+1]", "cap[1<<27]"]
            + [f"occupancy[{p}-S+1]" for p in OCC_PATTERNS]
            + [f"dup[{m}-{w}]" for m in (DUP - 1, DUP, DUP + 1)
               for w in ("first", "last")])
assert set(GPU_ONLY) <= set(CASES)
MOCK_CASES = [n for n in CASES if n not in GPU_ONLY]


# ---- join checker ----------------------------------------------------------

def _assert_bits(got, exp, what):
    assert got.dtype == exp.dtype, f"{what}: dtype {got.dtype} != {exp.dtype}"
    assert got.shape == exp.shape, f"{what}: {got.shape} != {exp.shape}"
    np.testing.assert_array_equal(ref.bits(got), ref.bits(exp), err_msg=what)


def _probe_host(libmod, j, lk):
    keys, lidx, rcols, n = libmod.join_probe(j, lk)
    out = [libmod.get(keys), libmod.get(lidx)] + [libmod.get(c)
                                                  for c in rcols]
    assert all(a.size == n for a in out), "n_out differs from column length"
    return out


def check_join(libmod, case):
    """Build, probe, compare keys, lidx and every payload column bit for bit
    with inner_join_ref; then probe the same build again (the right frame
    caches its build) and require the same output."""
    lkeys, rkeys, rvals, key_min, n_slots = case
    assert rkeys.size == 0 or (
        int(rkeys.min()) >= key_min
        and int(rkeys.max()) - key_min < n_slots), "case keys out of range"
    ek, el, _er, ev = ref.inner_join_ref(lkeys, rkeys, rvals)
    expect = [ek, el] + ev
    names = ["keys", "lidx"] + [f"payload {c}" for c in range(len(rvals))]
    rk = libmod.put(rkeys)
    rv = [libmod.put(v) for v in rvals]
    lk = libmod.put(lkeys)
    j = libmod.join_build(rk, rv, key_min, n_slots)
    first = _probe_host(libmod, j, lk)
    assert len(first) == len(expect)
    for got, exp, name in zip(first, expect, names):
        _assert_bits(got, exp, name)
    second = _probe_host(libmod, j, lk)
    for got, exp, name in zip(second, first, names):
        _assert_bits(got, exp, f"second probe, {name}")


# ---- row-movement cases and checkers ---------------------------------------

def column(n, dtype, seed=11):
    return f64_specials(n, seed) if dtype == "f64" else i64_specials(n, seed)


def _in_range(idx, length, low=0):
    """No entry takes an index outside its source: checked on the host."""
    assert idx.dtype == ref.I64
    assert idx.size == 0 or (int(idx.min()) >= low
                             and int(idx.max()) < length), "index out of range"


def check_search_sorted(libmod, keys, sorted_):
    assert np.all(sorted_[1:] >= sorted_[:-1])
    got = libmod.get(libmod.search_sorted(libmod.put(keys),
                                          libmod.put(sorted_)))
    _assert_bits(got, ref.search_sorted_ref(keys, sorted_), "search_sorted")


def search_sorted_m_case(m, seed=12):
    """A sorted column of m distinct keys; probes below the first, above the
    last, equal to each end and to inner entries, and between neighbours."""
    rng = np.random.default_rng(seed)
    sorted_ = -7 + 3 * np.arange(m, dtype=np.int64)
    pick = sorted_[rng.integers(0, m, 500)] if m else _i64([])
    keys = np.concatenate([pick, pick + 1, pick - 1, sorted_[:3],
                           sorted_[-3:], _i64([-8, -9, 3 * m - 7, 3 * m - 6,
                                               I64MIN, I64MAX])])
    return keys, sorted_


def search_sorted_ends_case():
    """INT64_MIN and INT64_MAX in both columns."""
    sorted_ = _i64([I64MIN, I64MIN + 1, -1, 0, 5, I64MAX - 1, I64MAX])
    keys = _i64([I64MAX, I64MIN, I64MIN + 2, I64MAX - 2, 0, 5, 6, -1,
                 I64MIN + 1, I64MAX - 1])
    return keys, sorted_


def search_sorted_repeats_case(seed=13):
    """Repeated values in `sorted`: the first position wins."""
    rng = np.random.default_rng(seed)
    vals = np.sort(rng.integers(-50, 50, 40).astype(np.int64))
    sorted_ = np.repeat(vals, rng.integers(1, 70, vals.size))
    sorted_ = np.concatenate([np.full(65, I64MIN), sorted_,
                              np.full(64, I64MAX)])
    keys = np.concatenate([np.arange(-60, 60, dtype=np.int64),
                           _i64([I64MIN, I64MAX])])
    return keys, sorted_


def search_sorted_n_case(n, seed=14):
    rng = np.random.default_rng(seed)
    sorted_ = np.sort(rng.integers(-2000, 2000, 1000).astype(np.int64))
    keys = rng.integers(-2100, 2100, n).astype(np.int64)
    return keys, sorted_


def gather_idx(n, length, seed=15):
    """n indices into a column of `length` rows: 0 and length - 1 at both
    ends of the index column, repeats in between."""
    idx = np.random.default_rng(seed).integers(0, length, n).astype(np.int64)
    if n >= 2:
        idx[0], idx[-1] = 0, length - 1
    if n >= 4:
        idx[1], idx[-2] = length - 1, 0
    return idx


def check_gather(libmod, src, idx):
    _in_range(idx, src.size)
    got = libmod.get(libmod.gather(libmod.put(src), libmod.put(idx)))
    _assert_bits(got, ref.gather_ref(src, idx), "gather")


def gather_fill_idx(n, length, seed=16):
    """-1 and valid indices mixed, with both kinds at the ends of the
    256-row chunks and of the column."""
    idx = gather_idx(n, length, seed)
    idx[np.random.default_rng(seed).random(n) < 0.3] = -1
    for e in range(B - 1, n - 1, 2 * B):
        idx[e], idx[e + 1] = -1, length - 1
    for e in range(2 * B - 1, n - 1, 2 * B):
        idx[e], idx[e + 1] = 0, -1
    if n:
        idx[-1] = -1
    return idx


def fills_for(dtype):
    return [float("nan"), -1, float(I64MIN)] if dtype == "f64" \
        else [-1, I64MIN]


def check_gather_fill(libmod, src, idx, fill):
    _in_range(idx, src.size, low=-1)
    got = libmod.get(libmod.gather_fill(libmod.put(src), libmod.put(idx),
                                        fill))
    _assert_bits(got, ref.gather_fill_ref(src, idx, fill), "gather_fill")


def check_scatter(libmod, src, perm):
    """scatter against the inverse-permutation reference, and
    scatter(gather(x, p), p) == x."""
    _in_range(perm, src.size)
    assert perm.size == src.size
    assert np.array_equal(np.sort(perm), np.arange(src.size))
    s, p = libmod.put(src), libmod.put(perm)
    _assert_bits(libmod.get(libmod.scatter(s, p)),
                 ref.scatter_ref(src, perm), "scatter")
    back = libmod.get(libmod.scatter(libmod.gather(s, p), p))
    _assert_bits(back, src, "scatter(gather(x, p), p)")


CROSS_SHAPES = [(0, 5), (1, 1), (1, G + 1), (G + 1, 1), (1025, 1023)]


def check_cross_idx(libmod, nl, nr):
    li, ri = libmod.cross_idx(nl, nr)
    el, er = ref.cross_idx_ref(nl, nr)
    _assert_bits(libmod.get(li), el, "cross lidx")
    _assert_bits(libmod.get(ri), er, "cross ridx")


def check_concat_slice(libmod, x):
    n = x.size
    col = libmod.put(x)
    empty = libmod.put(x[:0])
    cat = lambda parts: libmod.get(libmod.concat(parts))      # noqa: E731
    _assert_bits(cat([col]), x, "concat of a single part")
    _assert_bits(cat([empty, col]), x, "concat, empty part first")
    _assert_bits(cat([col, empty]), x, "concat, empty part last")
    _assert_bits(cat([empty, col, empty, col]), np.concatenate([x, x]),
                 "concat, empty parts between")
    _assert_bits(cat([empty]), x[:0], "concat of one empty part")
    _assert_bits(libmod.get(libmod.col_slice(col, n, 0)), x[:0],
                 "slice at start = len")
    for k in sorted({0, 1, T, n} & set(range(n + 1))):
        head = libmod.col_slice(col, 0, k)
        tail = libmod.col_slice(col, k, n - k)
        _assert_bits(libmod.get(head), x[:k], f"slice [0, {k})")
        _assert_bits(libmod.get(tail), x[k:], f"slice [{k}, n)")
        _assert_bits(cat([head, tail]), x, f"concat of the slices at {k}")
