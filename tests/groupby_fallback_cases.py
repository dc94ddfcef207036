"""Boundary cases, reference and checkers for the three groupby paths a key
range takes when it does not fit the radix path, shared by the CPU mock tier
(test_mock_groupby_fallbacks.py) and the GPU tier
(test_gpu_groupby_fallbacks.py):

  atomic  hf_groupby_accum -> k_gb_accum, then hf_groupby_compact
  hash    hf_groupby_hash_accum -> k_gb_hash_accum, hf_groupby_hash_compact
  sorted  hf_groupby_sorted -> k_head_flags, the filter plan, k_segagg

Every case is built on demand from a name, so importing this module allocates
nothing.  The drivers take the library module as an argument:
`modin_amd.core.lib` itself on the GPU, the same module with tests/mocklib.py
installed on the CPU.

The reference is groupby_ref, plain numpy with math.fsum for the sums.  Keys,
counts, presence, min and max compare bit-exactly.  Sums compare bit-exactly
too wherever the values are integers stored as f64 whose partial sums stay far
below 2^53 (every order of adds is then exact); one case per path has random
f64 values and is held to the bound of a sum in any order,
|got - exact| <= gamma(c - 1) * sum|x|, gamma(k) = k u / (1 - k u), u = 2^-53,
c the group's non-NaN count, evaluated in rational arithmetic.

Sizes the kernels switch on:
  W wave, B block, T = FILT_TILE (rows per k_segagg tile), G = GRID_CAP * BLOCK
  (first row, or row pair, a grid-stride kernel reaches on its second trip),
  R = 1024 << 13 (the widest range the radix path takes), PROBE = 4096 (the
  longest probe chain k_gb_hash_accum walks before it reports a full table).
"""

import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle.ops import _mix64

W, B, T = 64, 256, 4096
G = 4096 * B                  # 1 048 576
R = 1024 << 13                # 8 388 608
PROBE = 4096
I64MIN, I64MAX = -2**63, 2**63 - 1
AGG_SUM, AGG_MIN, AGG_MAX = 0, 1, 2
OPS = {"sum": AGG_SUM, "min": AGG_MIN, "max": AGG_MAX}
IDENT = {AGG_SUM: 0.0, AGG_MIN: np.inf, AGG_MAX: -np.inf}
U = 2.0 ** -53

# parts: [(keys, [value columns])], one entry per accumulate call (sorted: one)
GbCase = namedtuple("GbCase", "parts nvals agg_op want_counts key_min n_slots H")
Ref = namedtuple("Ref", "keys aggs counts rows")
Got = namedtuple("Got", "keys aggs counts n")


def _case(parts, nvals, agg_op=AGG_SUM, want_counts=True, key_min=0,
          n_slots=0, H=0):
    parts = [(np.ascontiguousarray(k, dtype=np.int64),
              [np.ascontiguousarray(v, dtype=np.float64) for v in vs])
             for k, vs in parts]
    assert all(len(vs) == nvals and all(v.size == k.size for v in vs)
               for k, vs in parts)
    return GbCase(parts, nvals, agg_op, want_counts, key_min, n_slots, H)


def all_rows(case):
    """The case's partitions as one (keys, [columns])."""
    if not case.parts:
        return (np.empty(0, np.int64),
                [np.empty(0, np.float64) for _ in range(case.nvals)])
    keys = np.concatenate([k for k, _ in case.parts])
    vals = [np.concatenate([vs[c] for _, vs in case.parts])
            for c in range(case.nvals)]
    return keys, vals


# ---- the reference ------------------------------------------------------------

def groupby_ref(keys, vals, agg_op, want_counts):
    """Ascending unique keys; per column the aggregate over the non-NaN rows
    of each group (the op's identity for a group with none) and the non-NaN
    counts; the row count per group.  Sums are math.fsum per group."""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    ukeys, start, rows = np.unique(keys[order], return_index=True,
                                   return_counts=True)
    ng = ukeys.size
    aggs, counts = [], []
    for v in vals:
        sv = np.asarray(v, dtype=np.float64)[order]
        ok = ~np.isnan(sv)
        out = np.full(ng, IDENT[agg_op])
        cnt = np.zeros(ng, dtype=np.int64)
        if ng:
            cnt = np.add.reduceat(ok.astype(np.int64), start)
            if agg_op == AGG_SUM:
                z = np.where(ok, sv, 0.0)
                for g in range(ng):
                    out[g] = math.fsum(z[start[g]:start[g] + rows[g]].tolist())
            else:
                fn = np.minimum if agg_op == AGG_MIN else np.maximum
                out = fn.reduceat(np.where(ok, sv, IDENT[agg_op]), start)
        aggs.append(out)
        counts.append(cnt)
    return Ref(ukeys, aggs, counts if want_counts else None,
               rows.astype(np.int64))


def case_ref(case):
    keys, vals = all_rows(case)
    return groupby_ref(keys, vals, case.agg_op, case.want_counts)


# ---- drivers ------------------------------------------------------------------

def _host(lib, k, s, c, n, nvals, want_counts):
    assert k.length == n
    assert len(s) == nvals and all(x.length == n for x in s)
    if want_counts:
        assert len(c) == nvals and all(x.length == n for x in c)
    else:
        assert c is None
    return Got(lib.get(k), [lib.get(x) for x in s],
               [lib.get(x) for x in c] if want_counts else None, n)


def run_atomic(lib, case):
    """hf_groupby_accum per partition into caller-owned dense tables, then
    hf_groupby_compact."""
    nv, ns = case.nvals, case.n_slots
    cols = max(nv, 1)
    sums = lib.alloc_raw(8 * cols * ns)
    rowcnt = lib.alloc_raw(8 * ns)
    counts = lib.alloc_raw(8 * cols * ns) if case.want_counts else 0
    try:
        lib.fill_f64(sums, IDENT[case.agg_op], cols * ns)
        lib.memset_raw(rowcnt, 0, 8 * ns)
        if counts:
            lib.memset_raw(counts, 0, 8 * cols * ns)
        for keys, vals in case.parts:
            lib.groupby_accum(lib.put(keys), [lib.put(v) for v in vals],
                              case.agg_op, case.key_min, ns, sums, rowcnt,
                              counts)
        k, s, c, n = lib.groupby_compact(sums, rowcnt, counts, nv,
                                         case.key_min, ns)
        return _host(lib, k, s, c, n, nv, case.want_counts)
    finally:
        lib.free_raw(sums)
        lib.free_raw(rowcnt)
        if counts:
            lib.free_raw(counts)


def run_hash(lib, case):
    """hf_groupby_hash_accum per partition into tables initialised as
    _groupby_hash does (tkey INT64_MIN, sums the identity, the rest zero),
    then hf_groupby_hash_compact."""
    nv, L = case.nvals, case.H + 1
    cols = max(nv, 1)
    tkey = lib.alloc_raw(8 * L)
    sums = lib.alloc_raw(8 * cols * L)
    rowcnt = lib.alloc_raw(8 * L)
    counts = lib.alloc_raw(8 * cols * L) if case.want_counts else 0
    try:
        lib.fill_i64(tkey, I64MIN, L)
        lib.fill_f64(sums, IDENT[case.agg_op], cols * L)
        lib.memset_raw(rowcnt, 0, 8 * L)
        if counts:
            lib.memset_raw(counts, 0, 8 * cols * L)
        for keys, vals in case.parts:
            lib.groupby_hash_accum(lib.put(keys), [lib.put(v) for v in vals],
                                   case.agg_op, case.H, tkey, sums, rowcnt,
                                   counts)
        k, s, c, n = lib.groupby_hash_compact(tkey, sums, rowcnt, counts, nv,
                                              case.H)
        return _host(lib, k, s, c, n, nv, case.want_counts)
    finally:
        lib.free_raw(tkey)
        lib.free_raw(sums)
        lib.free_raw(rowcnt)
        if counts:
            lib.free_raw(counts)


def run_sorted(lib, case):
    (keys, vals), = case.parts
    assert (keys[1:] >= keys[:-1]).all()
    k, s, c, n = lib.groupby_sorted(lib.put(keys), [lib.put(v) for v in vals],
                                    case.agg_op, case.want_counts)
    return _host(lib, k, s, c, n, case.nvals, case.want_counts)


# ---- checkers -----------------------------------------------------------------

def check_exact(got, ref, what=""):
    assert got.n == ref.keys.size, what
    assert got.keys.dtype == np.int64
    np.testing.assert_array_equal(got.keys, ref.keys, err_msg=f"{what} keys")
    assert len(got.aggs) == len(ref.aggs)
    for c, (g, r) in enumerate(zip(got.aggs, ref.aggs)):
        assert g.dtype == np.float64
        np.testing.assert_array_equal(g, r, err_msg=f"{what} column {c}")
    if ref.counts is None:
        assert got.counts is None
    else:
        for c, (g, r) in enumerate(zip(got.counts, ref.counts)):
            assert g.dtype == np.int64
            np.testing.assert_array_equal(g, r, err_msg=f"{what} counts {c}")


def check_case(lib, case, run, what=""):
    """One exact case through `run`.  A keys-only case (nvals = 0) returns no
    row counts, so the same keys go through a second call under a column of
    ones, whose sum and count per group are the group's rows."""
    ref = case_ref(case)
    got = run(lib, case)
    check_exact(got, ref, what)
    if case.nvals == 0:
        ones = case._replace(
            parts=[(k, [np.ones(k.size)]) for k, _ in case.parts], nvals=1,
            agg_op=AGG_SUM, want_counts=True)
        got1 = run(lib, ones)
        np.testing.assert_array_equal(got1.keys, ref.keys)
        np.testing.assert_array_equal(got1.counts[0], ref.rows)
        np.testing.assert_array_equal(got1.aggs[0], ref.rows.astype(float))
    return got


def check_reassoc(lib, case, run, what=""):
    """The random-values case of a path: keys and counts exact, each sum
    within gamma(c - 1) * sum|x| of the exact sum.  Returns the worst
    |error| / bound (0 where every group was exact)."""
    keys, vals = all_rows(case)
    ref = case_ref(case)
    got = run(lib, case)
    np.testing.assert_array_equal(got.keys, ref.keys)
    worst = 0.0
    for c in range(case.nvals):
        np.testing.assert_array_equal(got.counts[c], ref.counts[c])
        order = np.argsort(keys, kind="stable")
        sv = vals[c][order]
        edges = np.r_[0, np.cumsum(ref.rows)]
        for g in range(ref.keys.size):
            x = [Fraction(float(t)) for t in sv[edges[g]:edges[g + 1]]
                 if t == t]
            cnt = len(x)
            assert cnt == ref.counts[c][g]
            exact = sum(x, Fraction(0))
            err = abs(Fraction(float(got.aggs[c][g])) - exact)
            k = max(cnt - 1, 0)
            bound = Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U)) \
                * sum((abs(t) for t in x), Fraction(0))
            assert err <= bound, (what, c, g, float(err), float(bound))
            if bound:
                worst = max(worst, float(err / bound))
    print(f"{what}: worst |err| / (gamma(c-1) * sum|x|) = {worst:.3e}")
    return worst


# ---- values -------------------------------------------------------------------

def int_vals(n, nvals, agg_op, seed):
    """Integer-valued f64 columns.  Under sum column 0 is all ones (its sum
    and count are the group's rows) and the others are in [-1000, 1000] with a
    tenth of the rows NaN; under min/max every column has NaN rows and a wide
    range.  Partial sums stay below 2^33."""
    rng = np.random.default_rng(seed)
    cols = []
    for c in range(nvals):
        if agg_op == AGG_SUM and c == 0:
            cols.append(np.ones(n))
            continue
        lim = 1000 if agg_op == AGG_SUM else 10**6
        v = rng.integers(-lim, lim + 1, n).astype(np.float64)
        v[rng.random(n) < 0.1] = np.nan
        cols.append(v)
    return cols


def special_vals(keys, agg_op, seed):
    """Two columns over `keys`: NaN rows, one group (the second smallest key)
    NaN in every row of both columns, and under min/max +-inf rows, with one
    group (the third smallest) holding nothing but the op's identity."""
    n = keys.size
    cols = int_vals(n, 2, agg_op, seed)
    cols[0] = cols[1][::-1].copy()
    uk = np.unique(keys)
    assert uk.size >= 4
    if agg_op != AGG_SUM:
        rng = np.random.default_rng(seed + 1)
        at = rng.choice(n, max(n // 16, 2), replace=False)
        cols[0][at[::2]] = np.inf
        cols[0][at[1::2]] = -np.inf
        cols[1][at[::2]] = -np.inf
        for col in cols:
            col[keys == uk[2]] = IDENT[agg_op]
    for col in cols:
        col[keys == uk[1]] = np.nan
    return cols


def reassoc_vals(n, seed):
    """Random f64 of mixed sign over twelve decades."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    v[rng.random(n) < 0.05] = np.nan
    return v


# ---- 1. the global-atomic path ------------------------------------------------

ATOMIC_SLOTS = R + 1
ROWS_ATOMIC = {"0": 0, "1": 1, "2": 2, "3": 3, "255": 255, "256": 256,
               "257": 257, "2G-1": 2 * G - 1, "2G": 2 * G, "2G+1": 2 * G + 1,
               "2G+2": 2 * G + 2, "4G+1": 4 * G + 1}


def spread_slots(n, n_slots, seed, ngroups=300):
    """A slot per row: up to `ngroups` distinct slots, slot 0 and slot
    n_slots - 1 among them (n >= 2), every one of them used, and the last row
    alone in its slot."""
    if n == 0:
        return np.empty(0, dtype=np.int64)
    rng = np.random.default_rng(seed)
    g = min(ngroups, n)
    inner = rng.permutation(np.unique(rng.integers(1, n_slots - 1, 4 * g + 8)))
    pool = np.r_[[0, n_slots - 1][2 - min(g, 2):], inner[:max(g - 2, 0)]]
    pool = pool.astype(np.int64)
    assert pool.size == g and np.unique(pool).size == g
    shared = pool[:-1]
    out = np.empty(n, dtype=np.int64)
    out[-1] = pool[-1]
    if n > 1:
        body = np.r_[shared, shared[rng.integers(0, shared.size,
                                                 n - 1 - shared.size)]]
        out[:-1] = rng.permutation(body)
    return out


def atomic_case(n, nvals=2, op="sum", want_counts=True, key_min=-17,
                n_slots=ATOMIC_SLOTS, seed=0, nparts=1):
    slots = spread_slots(n, n_slots, seed + n)
    keys = np.int64(key_min) + slots
    vals = int_vals(n, nvals, OPS[op], seed + n + 1)
    cut = [0, n] if nparts == 1 else [0, n // 2 - (n // 2 + 1) % 2, n]
    parts = [(keys[a:b], [v[a:b] for v in vals])
             for a, b in zip(cut[:-1], cut[1:])]
    return _case(parts, nvals, OPS[op], want_counts, key_min, n_slots)


def atomic_vals_case(op):
    n = 513
    keys = np.int64(-17) + spread_slots(n, ATOMIC_SLOTS, 7, ngroups=40)
    return _case([(keys, special_vals(keys, OPS[op], 70))], 2, OPS[op], True,
                 -17, ATOMIC_SLOTS)


def atomic_reassoc_case():
    n = 20001
    keys = np.int64(-17) + spread_slots(n, ATOMIC_SLOTS, 8, ngroups=40)
    return _case([(keys, [reassoc_vals(n, 80)])], 1, AGG_SUM, True, -17,
                 ATOMIC_SLOTS)


def atomic_out_of_range_case():
    """257 rows with two keys outside the range: key_min - 1 in the pair loop
    (row 10) and key_min + n_slots as the odd tail (row 256)."""
    case = atomic_case(257, seed=9)
    (keys, vals), = case.parts
    keys = keys.copy()
    keys[10] = case.key_min - 1
    keys[256] = case.key_min + case.n_slots
    return case._replace(parts=[(keys, vals)])


INST = ([("sum", nv, wc) for nv in range(9) for wc in (False, True)] +
        [(op, nv, wc) for op in ("min", "max") for nv in (1, 8)
         for wc in (False, True)])


def _inst_name(op, nv, wc):
    return f"inst[{op}-nv{nv}-{'counts' if wc else 'nocounts'}]"


ATOMIC_CASES = {}
for _lab, _n in ROWS_ATOMIC.items():
    ATOMIC_CASES[f"rows[{_lab}]"] = functools.partial(atomic_case, _n)
ATOMIC_CASES["kmin[negative]"] = functools.partial(
    atomic_case, 257, key_min=-10**12)
ATOMIC_CASES["kmin[int64_min]"] = functools.partial(
    atomic_case, 257, key_min=I64MIN)
ATOMIC_CASES["kmin[to_int64_max]"] = functools.partial(
    atomic_case, 257, key_min=I64MAX - (ATOMIC_SLOTS - 1))
ATOMIC_CASES["parts[odd+even]"] = functools.partial(atomic_case, 513,
                                                    nparts=2)
for _op in OPS:
    ATOMIC_CASES[f"vals[{_op}]"] = functools.partial(atomic_vals_case, _op)
for _op, _nv, _wc in INST:
    ATOMIC_CASES[_inst_name(_op, _nv, _wc)] = functools.partial(
        atomic_case, 257, nvals=_nv, op=_op, want_counts=_wc, seed=_nv)


def e2e_frame(span=R + 5, n=300, seed=11):
    """A pandas frame whose int64 key column spans `span` slots."""
    import pandas
    rng = np.random.default_rng(seed)
    k = rng.integers(0, span, 40).astype(np.int64)
    k[0], k[1] = 0, span - 1
    keys = np.r_[k, k[rng.integers(0, 40, n - 40)]] - 1000
    a = rng.integers(-1000, 1001, n).astype(np.float64)
    a[rng.random(n) < 0.1] = np.nan
    return pandas.DataFrame({"k": rng.permutation(keys),
                             "a": a, "b": np.arange(n, dtype=np.float64)})


def check_frame(mpd, pdf, aggs=("sum", "count", "mean", "min", "max")):
    """groupby("k").<agg>() of the frame against pandas: integer data, so
    everything but the mean's division is exact."""
    df = mpd.DataFrame(pdf)
    for agg in aggs:
        got = getattr(df.groupby("k"), agg)().to_pandas()
        exp = getattr(pdf.groupby("k"), agg)()
        np.testing.assert_array_equal(got.index.to_numpy(),
                                      exp.index.to_numpy())
        assert list(got.columns) == list(exp.columns)
        for c in exp.columns:
            if agg == "mean":
                np.testing.assert_allclose(got[c].to_numpy(),
                                           exp[c].to_numpy(), rtol=1e-14)
            else:
                np.testing.assert_array_equal(got[c].to_numpy(),
                                              exp[c].to_numpy(), err_msg=agg)


# ---- 2. the hash path ---------------------------------------------------------

_M64 = (1 << 64) - 1
_C0 = 0x9E3779B97F4A7C15
_INV1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV2 = pow(0x94D049BB133111EB, -1, 1 << 64)


def _unxorshift(y, s):
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> np.uint64(s))
    return x


def unmix(h):
    """The inverse of oracle.ops._mix64 (the splitmix64 finalizer, a
    bijection on 64 bits): the uint64 x with _mix64(x) == h."""
    x = np.asarray(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = _unxorshift(x, 31) * np.uint64(_INV2)
        x = _unxorshift(x, 27) * np.uint64(_INV1)
        return _unxorshift(x, 30) - np.uint64(_C0)


def keys_with_home(home, count, H, first=0):
    """`count` distinct int64 keys whose home slot in a table of H slots is
    `home`: key j is unmix(home + (first + j) * H)."""
    j = np.arange(first, first + count, dtype=np.uint64)
    keys = unmix(np.uint64(home) + j * np.uint64(H)).view(np.int64)
    assert (homes(keys, H) == home).all() and np.unique(keys).size == count
    assert (keys != I64MIN).all()
    return keys


def homes(keys, H):
    return (_mix64(np.asarray(keys, np.int64).view(np.uint64))
            & np.uint64(H - 1)).astype(np.int64)


TableModel = namedtuple("TableModel", "failed max_probes wrapped occupied "
                        "special slot_of")


def table_model(keys, H, wrap=True):
    """Serial model of k_gb_hash_accum's table: open addressing with linear
    probing from hash_mix64(k) & (H - 1), at most min(H, 4096) probes, and
    INT64_MIN in the extra slot H.  Distinct keys are inserted in order of
    first appearance.  wrap=False is the wrong step `h + 1` without the mask
    (a probe that leaves the table finds nothing), kept for the CPU tier's
    sensitivity check."""
    keys = np.asarray(keys, dtype=np.int64)
    _, first = np.unique(keys, return_index=True)
    distinct = keys[np.sort(first)]
    occ = np.zeros(H, dtype=bool)
    maxprobe = min(H, PROBE)
    step = np.arange(maxprobe, dtype=np.int64)
    failed, most, wrapped, special, slot_of = 0, 0, False, False, {}
    for k, h in zip(distinct.tolist(), homes(distinct, H).tolist()):
        if k == I64MIN:
            special = True
            slot_of[k] = H
            continue
        window = h + step
        inside = window < H
        window = window & (H - 1)
        free = ~occ[window]
        if not wrap:
            free &= inside
        if not free.any():
            failed += 1
            continue
        p = int(np.argmax(free))
        occ[window[p]] = True
        slot_of[k] = int(window[p])
        most = max(most, p + 1)
        wrapped |= h + p >= H
    return TableModel(failed, most, wrapped, int(occ.sum()), special, slot_of)


def _keyed_case(keys, H, nvals=2, op="sum", want_counts=True, seed=0,
                nparts=1):
    n = keys.size
    vals = int_vals(n, nvals, OPS[op], seed + 1)
    cut = [0, n] if nparts == 1 else [0, n // 2 - (n // 2 + 1) % 2, n]
    parts = [(keys[a:b], [v[a:b] for v in vals])
             for a, b in zip(cut[:-1], cut[1:])]
    return _case(parts, nvals, OPS[op], want_counts, H=H)


def repeat_shuffled(distinct, times, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(np.repeat(np.asarray(distinct, np.int64), times))


def span_keys(n, seed, ngroups=300):
    """n rows over up to `ngroups` keys spread over all of int64, INT64_MIN
    and INT64_MAX among them (n >= 3); the last row alone in its group."""
    rng = np.random.default_rng(seed)
    g = min(ngroups, n)
    pool = np.unique(rng.integers(I64MIN + 1, I64MAX, 2 * g + 8,
                                  dtype=np.int64))
    pool = rng.permutation(pool)[:g]
    if g >= 3:
        pool[0], pool[1] = I64MIN, I64MAX
    shared = pool[:-1]
    out = np.empty(n, dtype=np.int64)
    out[-1] = pool[-1]
    if n > 1:
        body = np.r_[shared, shared[rng.integers(0, shared.size,
                                                 n - 1 - shared.size)]]
        out[:-1] = rng.permutation(body)
    return out


ROWS_HASH = {"1": 1, "255": 255, "256": 256, "257": 257, "G-1": G - 1,
             "G": G, "G+1": G + 1, "2G+1": 2 * G + 1}
ROOMY_H = 1024
FULL_H = (2, 4, 64, 4096)
WRAP_H = 64
BOUND_H = 8192
RETRY_H = 1 << 14


def hash_rows_case(n, **kw):
    return _keyed_case(span_keys(n, 100 + n), ROOMY_H, seed=n, **kw)


def hash_empty_case():
    return _case([], 2, H=64)


def hash_special_case(kind):
    if kind == "only":
        return _keyed_case(np.full(5, I64MIN, dtype=np.int64), 64)
    mixed = repeat_shuffled([I64MIN, I64MAX, 0, -1], 3, 21)
    return _keyed_case(mixed, 64, nparts=2 if kind == "two_parts" else 1)


def full_keys(H, extra=0):
    """H + extra distinct ordinary keys and INT64_MIN, three rows each.  With
    extra = 0 they fit in any insertion order: a sweep of min(H, 4096) = H
    probes that finds no slot has met H other ordinary keys."""
    assert H <= PROBE
    rng = np.random.default_rng(300 + H)
    pool = np.unique(rng.integers(I64MIN + 1, I64MAX, 2 * H + 8,
                                  dtype=np.int64))
    distinct = np.r_[rng.permutation(pool)[:H + extra], I64MIN]
    return repeat_shuffled(distinct, 3, H)


def hash_full_case(H, extra=0):
    return _keyed_case(full_keys(H, extra), H, seed=H)


def wrap_keys():
    """Five keys at home H - 1 and three at home H - 2 of a 64-slot table:
    eight slots from H - 2 on, so the chain runs through slot 0."""
    k = np.r_[keys_with_home(WRAP_H - 1, 5, WRAP_H),
              keys_with_home(WRAP_H - 2, 3, WRAP_H)]
    return repeat_shuffled(k, 4, 31)


def hash_wrap_case():
    return _keyed_case(wrap_keys(), WRAP_H, seed=31)


def bound_keys(count, H=BOUND_H, home=5):
    """`count` distinct keys sharing one home.  Whatever the insertion order,
    the claimed slots are a prefix of the chain from `home`, so 4096 of them
    fit (the last one claimed needs exactly 4096 probes) and of 4097 at least
    one finds its whole sweep taken."""
    return keys_with_home(home, count, H)


def hash_bound_case(count=PROBE):
    return _keyed_case(bound_keys(count), BOUND_H, nvals=1, seed=41)


def retry_frame(n=5000, seed=51):
    """4097 distinct keys sharing one home at H = 16384 (where _groupby_hash
    starts for 4097..8192 rows) in a frame of n rows."""
    import pandas
    assert PROBE + 1 <= n <= 2 * PROBE
    rng = np.random.default_rng(seed)
    k = keys_with_home(77, PROBE + 1, RETRY_H)
    keys = rng.permutation(np.r_[k, k[rng.integers(0, k.size, n - k.size)]])
    return pandas.DataFrame({"k": keys,
                             "v": rng.integers(-1000, 1001, n).astype(float)})


def hash_vals_case(op):
    keys = span_keys(513, 61, ngroups=40)
    return _case([(keys, special_vals(keys, OPS[op], 62))], 2, OPS[op], True,
                 H=ROOMY_H)


def hash_reassoc_case():
    keys = span_keys(20001, 63, ngroups=40)
    return _case([(keys, [reassoc_vals(keys.size, 64)])], 1, AGG_SUM, True,
                 H=ROOMY_H)


def hash_inst_case(op, nvals, want_counts):
    """257 rows over 40 keys in a 64-slot table."""
    return _keyed_case(span_keys(257, 65, ngroups=40), 64, nvals=nvals, op=op,
                       want_counts=want_counts, seed=nvals)


HASH_CASES = {"empty": hash_empty_case}
for _kind in ("only", "mixed", "two_parts"):
    HASH_CASES[f"special[{_kind}]"] = functools.partial(hash_special_case,
                                                        _kind)
for _H in FULL_H:
    HASH_CASES[f"full[{_H}]"] = functools.partial(hash_full_case, _H)
HASH_CASES["wrap"] = hash_wrap_case
HASH_CASES["probe[4096]"] = hash_bound_case
for _lab, _n in ROWS_HASH.items():
    HASH_CASES[f"rows[{_lab}]"] = functools.partial(hash_rows_case, _n)
HASH_CASES["parts[odd+even]"] = functools.partial(hash_rows_case, 513,
                                                  nparts=2)
for _op in OPS:
    HASH_CASES[f"vals[{_op}]"] = functools.partial(hash_vals_case, _op)
for _op, _nv, _wc in INST:
    HASH_CASES[_inst_name(_op, _nv, _wc)] = functools.partial(
        hash_inst_case, _op, _nv, _wc)


# ---- 3. the sorted path -------------------------------------------------------

ROWS_SORTED = {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "255": 255,
               "256": 256, "257": 257, "T-1": T - 1, "T": T, "T+1": T + 1,
               "2T": 2 * T, "3T+1": 3 * T + 1}
PLACED = (1, 62, 63, 64, 65, 127, 128, 255, 256, 257, T - 1, T, T + 1,
          2 * T - 1, 2 * T)
PLACED_PAIRS = ((63, 64), (255, 256), (T - 1, T))


def keys_from_heads(n, heads):
    """Sorted keys of n rows whose runs start at `heads` (row 0 is always a
    head): the first run is INT64_MIN, the last of several INT64_MAX, those
    between negative and positive."""
    flag = np.zeros(n, dtype=np.int64)
    flag[np.asarray(heads, dtype=np.int64)] = 1
    if n:
        flag[0] = 1
    r = int(flag.sum())
    kv = (np.arange(r, dtype=np.int64) - r // 2) * 3
    if r:
        kv[0] = I64MIN
    if r > 1:
        kv[-1] = I64MAX
    return kv[np.cumsum(flag) - 1] if n else np.empty(0, dtype=np.int64)


def sorted_shapes(n):
    """(label, heads) of every run shape at n rows."""
    if n == 0:
        return [("empty", [])]
    out = [("one-run", [0]), ("each-row", np.arange(n)),
           ("runs-of-2", np.arange(0, n, 2))]
    out += [(f"head@{p}", [0, p]) for p in PLACED if p < n]
    out += [(f"heads@{a},{b}", [0, a, b]) for a, b in PLACED_PAIRS if b < n]
    return out


def sorted_shape_case(n, heads):
    """Column 0 all ones, column 1 the row number: count and sum of column 0
    are the run's length, the sum of column 1 names the run's rows."""
    keys = keys_from_heads(n, heads)
    return _case([(keys, [np.ones(n), np.arange(n, dtype=np.float64)])], 2,
                 AGG_SUM, True)


def sorted_empty_case(nvals, want_counts):
    return _case([(np.empty(0, np.int64), [np.empty(0)] * nvals)], nvals,
                 AGG_SUM, want_counts)


def mixed_runs(n, seed):
    """Heads of runs 1 to 600 rows long."""
    rng = np.random.default_rng(seed)
    lens = np.r_[rng.integers(1, 9, 40), rng.integers(1, 601, 200)]
    heads = np.r_[0, np.cumsum(rng.permutation(lens))]
    return heads[heads < n]


SORTED_INST_N = 2 * T + 1


def sorted_inst_case(op, nvals, want_counts):
    n = SORTED_INST_N
    keys = keys_from_heads(n, mixed_runs(n, 71))
    return _case([(keys, int_vals(n, nvals, OPS[op], 72 + nvals))], nvals,
                 OPS[op], want_counts)


def sorted_vals_case(op):
    """NaN on every head row of column 1, an all-NaN run, +-inf rows."""
    n = SORTED_INST_N
    heads = mixed_runs(n, 73)
    keys = keys_from_heads(n, heads)
    cols = special_vals(keys, OPS[op], 74)
    cols[1][heads] = np.nan
    return _case([(keys, cols)], 2, OPS[op], True)


def sorted_reassoc_case():
    n = 20001
    keys = keys_from_heads(n, mixed_runs(n, 75))
    return _case([(keys, [reassoc_vals(n, 76)])], 1, AGG_SUM, True)


def unsorted_parts_case():
    """Unsorted keys in 3 partitions of uneven length, one of them empty, for
    _groupby_sorted's concat + sort + gather."""
    n = T + 300
    keys = span_keys(n, 77, ngroups=200)
    vals = int_vals(n, 2, AGG_SUM, 78)
    cut = [0, 257, 257, n]
    parts = [(keys[a:b], [v[a:b] for v in vals])
             for a, b in zip(cut[:-1], cut[1:])]
    return _case(parts, 2, AGG_SUM, True)


SORTED_INST = [(op, nv, wc) for op in OPS for nv in (0, 1, 2, 8)
               for wc in (False, True)]
SORTED_CASES = {}
for _op, _nv, _wc in SORTED_INST:
    SORTED_CASES[_inst_name(_op, _nv, _wc)] = functools.partial(
        sorted_inst_case, _op, _nv, _wc)
for _op in OPS:
    SORTED_CASES[f"vals[{_op}]"] = functools.partial(sorted_vals_case, _op)


def segagg_model(head, vals, inclusive=True):
    """Serial restatement of k_segagg's run numbering for one column under
    sum: per 4096-row tile the base is the heads before the tile; per 256-row
    chunk and 64-row wave the run of lane l is base + heads of earlier waves
    + popcount(ballot & mask(l)) - 1, mask(l) = (2 << l) - 1 with lane 63
    taking every bit.  inclusive=False is the wrong mask (1 << l) - 1, kept
    for the CPU tier's sensitivity check; a run number below 0 is dropped
    there (on the device it would be a write in front of the table, which is
    why that mutant is never run on one).  Returns (sums, counts) per run."""
    head = np.asarray(head, dtype=bool)
    n = head.size
    runs = int(head.sum())
    sums, counts = np.zeros(runs), np.zeros(runs, dtype=np.int64)
    for t0 in range(0, n, T):
        base = int(head[:t0].sum())
        for c0 in range(t0, min(t0 + T, n), B):
            wave_base = 0
            for w0 in range(c0, c0 + B, W):
                lanes = head[w0:min(w0 + W, n, t0 + T)]
                for l in range(lanes.size):
                    upto = l + 1 if inclusive or l == W - 1 else l
                    run = base + wave_base + int(lanes[:upto].sum()) - 1
                    v = vals[w0 + l]
                    if run >= 0 and v == v:
                        sums[run] += v
                        counts[run] += 1
                wave_base += int(lanes.sum())
            base += wave_base
    return sums, counts
