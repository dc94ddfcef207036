// hipframe.hip — gfx950 (MI355X, CDNA4) implementation of the hipframe C-ABI.
//
// Every op here is the device form of one Modin operator template (the
// reference executes these as pandas calls inside each partition — see the
// per-function citations in include/hipframe.h).  All paths are
// HBM-bandwidth-bound (no MFMA anywhere on this path), so the
// kernels are built around the CDNA4 streaming rules:
//   - 16 B/lane vectorized loads (double2 / longlong2) — the coalescing sweet
//     spot on gfx950,
//   - grid-stride loops capped at a few thousand 256-thread workgroups
//     (≫256 so all 8 XCDs fill),
//   - wave64 shuffle reductions + LDS block reductions, one atomic per block,
//   - dense-key groupby via hardware global_atomic_add_f64 into an
//     HBM/L3-resident key-indexed table (the table for the north-star config,
//     1e6 keys, is 8–24 MB: Infinity-Cache resident).
//
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see Makefile).

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/hipframe.h"

// ---------------------------------------------------------------------------
// module state & error plumbing
// ---------------------------------------------------------------------------

// Everything the radix groupby path caches on a key column.  Derivation
// chain: histogram -> layout (cursor-init + work items) -> scatter plan;
// d_k32 hangs off key_min alone.  The member functions at the end are the
// only places that list the fields to free.
struct GbKeyCache {
  // cached per-bucket histogram for the radix groupby path (host copy, one
  // entry per bucket; empty = none).  Valid when hist_kmin/hist_nb/
  // hist_nslots match the current query.  The column is immutable, so this
  // is the device analog of the reference's lazy-metadata caches
  // (modin/core/dataframe/pandas/metadata/) — a repeated groupby on the same
  // key column skips the histogram pass.
  std::vector<int64_t> hist;
  int64_t hist_kmin = 0;
  int64_t hist_nb = 0;
  int64_t hist_nslots = 0;       // exact n_slots the histogram was cut for
  // cached u32 shifted copy of an int64 key column (key - key_min), the
  // narrow-key fast path for the radix scatter (12 B/row instead of 16).
  // Same immutable-column caching rationale as hist.
  void*   d_k32 = nullptr;
  int64_t k32_min = 0;
  // cached radix-scatter layout derived from hist: device cursor-init
  // array (region starts) + device work items — steady-state groupby
  // launches copy cursors D2D and never touch the host (no H2D, no sync)
  void*   d_curinit = nullptr;   // u32[nb]
  void*   d_work = nullptr;      // GbWorkItem[work_n]
  void*   d_item0 = nullptr;     // u32[nb + 1]: bucket -> its first work item
                                 // (a bucket's items are contiguous)
  int64_t work_n = 0;
  int64_t radix_rows = 0;        // payload rows (64-aligned region total)
  int     radix_rl = 0;          // validity: matches (hist_kmin, hist_nb)
  // cached scatter plan: every decision the radix scatter takes depends on
  // the (immutable) key column alone, so the first radix call records them
  // and later calls replay a pure value permutation that never reads keys
  // (k_gb_replay).  One plan per column, valid for exactly
  // (plan_kmin, plan_nslots, plan_rl) at GB_PLAN_TILE rows per tile; another
  // geometry re-records.  Invalidated with hist (same derivation chain).
  // The plan's payload is tile-major: tile t's bucket-sorted staging lies at
  // [t * TILE, (t + 1) * TILE) of the value buffer and of plan_rk, and P2
  // fetches a bucket's run out of each tile through plan_runs.
  void*   d_plan_dst = nullptr;  // u16[n]: row -> slot in its tile's bucket-
                                 // sorted LDS staging; 0xFFFF = key out of range
  void*   d_plan_rk = nullptr;   // u16[ntiles * TILE]: low key of staged slot p
                                 // of tile t at [t * TILE + p]
  void*   d_plan_runs = nullptr; // u32[nb][ntiles], bucket-major: the bucket's
                                 // run in the tile, start | length << 16
  void*   d_plan_items = nullptr;  // GbTileItem[plan_items_n]: P2 work items,
                                   // a bucket's items contiguous, in tile order
  void*   d_plan_item0 = nullptr;  // u32[nb + 1]: bucket -> its first item
  void*   d_plan_order = nullptr;  // u32[plan_items_n]: P2 block -> item,
                                   // costliest item first
  void*   d_plan_meta = nullptr; // u64: out-of-range rows recorded
  int64_t plan_items_n = 0;
  int64_t plan_kmin = 0;
  int64_t plan_nslots = 0;
  int     plan_rl = 0;           // 0 = no plan
  // cached group map: which slots are present, and the compacted keys, are
  // functions of the key column and (key_min, n_slots) alone.  Valid for
  // exactly the plan's (plan_kmin, plan_nslots, plan_rl) and dropped with it;
  // armed (d_gidx != null) only by a call that compacted with a valid plan
  // and a zero error word, so a column with out-of-range keys never has one.
  // hf_groupby_reduce then skips the dense tables and the compaction.
  void*   d_gidx = nullptr;      // u32[plan_nslots]: slot -> output row,
                                 // 0xFFFFFFFF = absent
  void*   d_gkeys = nullptr;     // i64[n_groups]: compacted ascending keys
  int64_t n_groups = 0;

  void drop_plan();     // free the plan and group-map buffers, plan_rl = 0
  void drop_derived();  // the histogram changed: drop the layout and the plan
  void release();       // the column dies: give every device block back
};

struct hf_col {
  void*   dptr;
  int64_t len;
  int     dtype;
  int     gpu;
  GbKeyCache gb;
};

namespace {

thread_local std::string g_err;

struct TimedPair { hipEvent_t a, b; std::string name; };

struct State {
  bool        inited = false;
  int         gpu = -1;
  hipStream_t stream = nullptr;
  // small persistent device scratch: reduce accumulators + error word +
  // compact bookkeeping
  void*       d_scratch = nullptr;   // see layout below
  // profiling
  bool        profiling = false;
  std::vector<TimedPair> pending;
  std::unordered_map<std::string, std::pair<int64_t, double>> stats;
};
State g;

// d_scratch layout (bytes):
//   [0..128)    reduce accumulator block (hf_reduce)
//   [128..136)  groupby error word (u64: count of out-of-range keys)
//   [136..144)  compact total (i64 n_groups)
constexpr int64_t SCRATCH_BYTES = 4096;
constexpr int64_t SCRATCH_GB_ERR = 128;
constexpr int64_t SCRATCH_NGROUPS = 136;
constexpr int64_t SCRATCH_JOIN_HIST_ERR = 144;
constexpr int64_t SCRATCH_JOIN_FIXUP_ERR = 152;
constexpr int64_t SCRATCH_HASH_FULL = 160;
constexpr int64_t SCRATCH_GM_ERR = 168;
template <typename T = unsigned long long>
T* scratch_at(int64_t off) { return (T*)((char*)g.d_scratch + off); }

int set_err(int code, const char* where, const char* what) {
  g_err = std::string(where) + ": " + what;
  return code;
}

int set_hip_err(const char* where, hipError_t e) {
  return set_err(HF_ERR_HIP, where, hipGetErrorString(e));
}

#define HF_HIP(where, call)                                   \
  do {                                                        \
    hipError_t _e = (call);                                   \
    if (_e != hipSuccess) return set_hip_err(where, _e);      \
  } while (0)

#define HF_NEED_INIT(where)                                   \
  if (!g.inited) return set_err(HF_ERR_NOINIT, where, "hf_init not called")

int64_t dtype_size(int dt) {
  switch (dt) {
    case HF_INT64:   return 8;
    case HF_FLOAT64: return 8;
    default:         return 0;
  }
}

// resolve pending profiling events into stats (syncs the stream)
int resolve_stats(const char* where) {
  if (g.pending.empty()) return HF_OK;
  HF_HIP(where, hipStreamSynchronize(g.stream));
  for (auto& p : g.pending) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, p.a, p.b);
    auto& s = g.stats[p.name];
    s.first += 1;
    s.second += ms;
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  g.pending.clear();
  return HF_OK;
}

// launch helper with optional event bracketing on the module stream
template <typename F>
int timed_launch(const char* name, F&& launch) {
  if (!g.profiling) {
    launch();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_hip_err(name, e);
    return HF_OK;
  }
  TimedPair p;
  p.name = name;
  HF_HIP(name, hipEventCreate(&p.a));
  HF_HIP(name, hipEventCreate(&p.b));
  HF_HIP(name, hipEventRecord(p.a, g.stream));
  launch();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_hip_err(name, e);
  HF_HIP(name, hipEventRecord(p.b, g.stream));
  g.pending.push_back(p);
  if (g.pending.size() > 4096) return resolve_stats(name);
  return HF_OK;
}

// Runtime value -> compile-time tag for a generic lambda: f receives a
// std::integral_constant and the caller reads decltype(tag)::value.  Callers
// validate agg_op / nvals first.  Only the combinations a caller actually
// nests are instantiated.
template <int V>
using int_tag = std::integral_constant<int, V>;
template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
int with_aop(int agg_op, F&& f) {
  return agg_op == HF_AGG_SUM   ? f(int_tag<HF_AGG_SUM>{})
         : agg_op == HF_AGG_MIN ? f(int_tag<HF_AGG_MIN>{})
                                : f(int_tag<HF_AGG_MAX>{});
}
template <int MAX, int N = 0, typename F>
int with_nvals(int nv, F&& f) {  // nv in [0, MAX]
  if (nv == N) return f(int_tag<N>{});
  if constexpr (N < MAX)
    return with_nvals<MAX, N + 1>(nv, std::forward<F>(f));
  else
    return set_err(HF_ERR_ARG, "with_nvals", "column count out of range");
}
// Radix bucket width (log2): what gb_radix_rl returns when it is not 0.
template <typename F>
int with_rl(int rl, F&& f) {
  return rl == 14 ? f(int_tag<14>{})
         : rl == 13 ? f(int_tag<13>{}) : f(int_tag<12>{});
}
// The scan ops are with_aop's plus PROD.  Kept apart from with_aop, whose
// groupby callers would otherwise instantiate PROD kernels they never launch.
template <typename F>
int with_scan_op(int agg_op, F&& f) {
  return agg_op == HF_AGG_PROD ? f(int_tag<HF_AGG_PROD>{})
                               : with_aop(agg_op, std::forward<F>(f));
}
// column dtype -> a value of its element type (double{} or int64_t{})
template <typename F>
int with_dtype(int dtype, F&& f) {
  return dtype == HF_FLOAT64 ? f(double{}) : f(int64_t{});
}

constexpr int BLOCK = 256;
// memory-bound grid cap: ≫256 workgroups to fill 8 XCDs, grid-stride the rest
// (cdna_hip_programming.md §6 Guideline 11)
constexpr int64_t GRID_CAP = 4096;

int64_t grid_for(int64_t work_items) {
  int64_t b = (work_items + BLOCK - 1) / BLOCK;
  if (b < 1) b = 1;
  return b < GRID_CAP ? b : GRID_CAP;
}

}  // namespace


// Device allocator: a size-bucketed cache over hipMalloc.  All compute runs
// on ONE module stream, so reusing a cached block is ordered-correct by
// construction (every prior user's work precedes the next user's on the
// stream).  ROCm 7.2's hipMallocAsync default pool showed reuse corruption
// under the join's varied alloc/free pattern (partial histograms + "write
// access to a read-only page" faults, joinbench vs joindbg bisect) — this
// cache replaces it.  Steady-state workloads allocate nothing.
// HF_SYNC_ALLOC=1 bypasses the cache (plain hipMalloc/hipFree, debug).
namespace {
inline bool sync_alloc() {
  static int v = -1;
  if (v < 0) v = getenv("HF_SYNC_ALLOC") ? 1 : 0;
  return v == 1;
}

struct DevCache {
  std::unordered_map<int64_t, std::vector<void*>> free_by_size;
  std::unordered_map<void*, int64_t> size_of;
  int64_t cached_bytes = 0;

  hipError_t alloc(void** p, int64_t bytes) {
    bytes = (bytes + 255) & ~255LL;
    auto it = free_by_size.find(bytes);
    if (it != free_by_size.end() && !it->second.empty()) {
      *p = it->second.back();
      it->second.pop_back();
      cached_bytes -= bytes;
      return hipSuccess;
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
      trim();
      e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) size_of[*p] = bytes;
    return e;
  }
  void free(void* p) {
    auto it = size_of.find(p);
    if (it == size_of.end()) { hipFree(p); return; }
    free_by_size[it->second].push_back(p);
    cached_bytes += it->second;
  }
  void trim() {  // OOM fallback: release every cached block after draining
                 // outstanding users
    hipDeviceSynchronize();
    for (auto& kv : free_by_size)
      for (void* p : kv.second) { size_of.erase(p); hipFree(p); }
    free_by_size.clear();
    cached_bytes = 0;
  }
};
DevCache g_cache;
// blocks handed out by dev_alloc and not yet given back through dev_free
// (hf_dev_live): the balance the ownership tests assert
int64_t g_dev_live = 0;

inline hipError_t dev_alloc(void** p, int64_t bytes, hipStream_t s) {
  if (sync_alloc()) hipStreamSynchronize(s);
  const hipError_t e = sync_alloc() ? hipMalloc(p, bytes)
                                    : g_cache.alloc(p, bytes);
  if (e == hipSuccess) ++g_dev_live;
  return e;
}
inline hipError_t dev_free(void* p, hipStream_t s) {
  --g_dev_live;
  if (sync_alloc()) { hipStreamSynchronize(s); return hipFree(p); }
  g_cache.free(p);
  return hipSuccess;
}

// Scoped device block on the module stream: goes back to the allocator on
// scope exit (so every early return is leak-free) unless release() hands it
// to a longer-lived owner.  Move-only.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.release()) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p_) (void)dev_free(p_, g.stream); }
  hipError_t alloc(int64_t bytes) {  // call once per holder
    hipError_t e = dev_alloc(&p_, bytes, g.stream);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void* release() { void* p = p_; p_ = nullptr; return p; }
  // allocate straight into a field of a handle whose owner frees it
  // (hf_join_free, hf_filter_plan_free); null on failure
  template <typename T>
  static hipError_t alloc_into(T*& field, int64_t bytes) {
    DevBuf b;
    const hipError_t e = b.alloc(bytes);
    field = static_cast<T*>(b.release());
    return e;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
};

// give a cached device block back and forget it (a column freed after
// hf_shutdown only forgets: the stream and allocator are gone)
void drop_dev(void*& p) {
  if (p && g.inited) (void)dev_free(p, g.stream);
  p = nullptr;
}

// An hf_col that is allocated but not yet the caller's: freed on scope exit
// unless commit() hands it out.  Entry points commit their outputs as the
// last thing before returning HF_OK, so a failed call leaves no column behind
// and no pointer to one in the caller's slot.  Move-only.
class ColOut {
 public:
  ColOut() = default;
  ColOut(ColOut&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
  ColOut(const ColOut&) = delete;
  ColOut& operator=(const ColOut&) = delete;
  ~ColOut() { hf_col_free(c_); }
  int alloc(int64_t len, int dtype) {  // call once per holder
    return hf_col_alloc(len, dtype, &c_);
  }
  hf_col** slot() { return &c_; }  // to receive another entry point's output
  hf_col* get() const { return c_; }
  template <typename T>
  T* data() const { return static_cast<T*>(c_->dptr); }
  void commit(hf_col** out) { *out = c_; c_ = nullptr; }
  // tail of an entry point whose last step returned rc: commit on success,
  // leave a null in the caller's slot otherwise
  int commit_if(int rc, hf_col** out) {
    if (rc == HF_OK) commit(out); else *out = nullptr;
    return rc;
  }

 private:
  hf_col* c_ = nullptr;
};

// The output triple of the groupby entry points: keys, one sum column per
// value and, when wanted, one count column per value; committed together.
struct GroupOut {
  ColOut keys;
  std::vector<ColOut> sums, cnts;
  GroupOut(int nvals, bool counts) : sums(nvals), cnts(counts ? nvals : 0) {}
  void commit(hf_col** out_keys, hf_col** out_sums, hf_col** out_counts) {
    keys.commit(out_keys);
    for (size_t c = 0; c < sums.size(); ++c) sums[c].commit(&out_sums[c]);
    for (size_t c = 0; c < cnts.size(); ++c) cnts[c].commit(&out_counts[c]);
  }
};

// owners for the two handle types while an entry point builds or borrows one
using JoinOwner = std::unique_ptr<hf_join, int (*)(hf_join*)>;
using PlanOwner = std::unique_ptr<hf_filterplan, int (*)(hf_filterplan*)>;
}  // namespace

void GbKeyCache::drop_plan() {
  drop_dev(d_plan_dst);
  drop_dev(d_plan_rk);
  drop_dev(d_plan_runs);
  drop_dev(d_plan_items);
  drop_dev(d_plan_item0);
  drop_dev(d_plan_order);
  drop_dev(d_plan_meta);
  plan_items_n = 0;
  plan_rl = 0;
  drop_dev(d_gidx);
  drop_dev(d_gkeys);
  n_groups = 0;
}

void GbKeyCache::drop_derived() {
  drop_dev(d_curinit);
  drop_dev(d_work);
  drop_dev(d_item0);
  work_n = radix_rows = 0;
  radix_rl = 0;
  drop_plan();
}

void GbKeyCache::release() {
  drop_derived();
  drop_dev(d_k32);
}

// ---------------------------------------------------------------------------
// kernels: Map (elementwise scalar) — algebra/map.py:28 device form
// ---------------------------------------------------------------------------

namespace {

template <int OP>
__device__ __forceinline__ double map1_f64(double x, double s) {
  switch (OP) {
    case HF_MAP_ADD:    return x + s;
    case HF_MAP_SUB:    return x - s;
    case HF_MAP_RSUB:   return s - x;
    case HF_MAP_MUL:    return x * s;
    case HF_MAP_DIV:    return x / s;
    case HF_MAP_RDIV:   return s / x;
    case HF_MAP_FILLNA: return (x != x) ? s : x;
    case HF_MAP_ABS:    return fabs(x);
    case HF_MAP_NEG:    return -x;
    case HF_MAP_SQRT:   return sqrt(x);
    // NaN-PROPAGATING (pandas clip leaves NaN alone; fmin/fmax would
    // replace NaN with the bound)
    case HF_MAP_ROUND:  return rint(x * s) / s;
    case HF_MAP_MIN:    return (x != x) ? x : fmin(x, s);
    case HF_MAP_MAX:    return (x != x) ? x : fmax(x, s);
  }
  return x;
}

template <int OP>
__global__ void __launch_bounds__(BLOCK) k_map_f64(const double* __restrict__ in,
                                                   double* __restrict__ out,
                                                   double s, int64_t n) {
  // 16 B/lane double2 stream; tail element handled by thread 0 of block 0.
  const int64_t npair = n >> 1;
  const double2* in2 = reinterpret_cast<const double2*>(in);
  double2* out2 = reinterpret_cast<double2*>(out);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    double2 v = in2[i];
    v.x = map1_f64<OP>(v.x, s);
    v.y = map1_f64<OP>(v.y, s);
    out2[i] = v;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    out[n - 1] = map1_f64<OP>(in[n - 1], s);
}

template <int OP>
__device__ __forceinline__ int64_t map1_i64(int64_t x, int64_t s) {
  switch (OP) {
    case HF_MAP_ADD:  return x + s;
    case HF_MAP_SUB:  return x - s;
    case HF_MAP_RSUB: return s - x;
    case HF_MAP_MUL:  return x * s;
    case HF_MAP_ABS:  return x < 0 ? -x : x;
    case HF_MAP_MIN:  return x < s ? x : s;
    case HF_MAP_MAX:  return x > s ? x : s;
    case HF_MAP_NEG:  return -x;
    case HF_MAP_IDIV: {  // Python floordiv: round toward -inf
      int64_t q = x / s, r = x % s;
      return (r != 0 && ((r < 0) != (s < 0))) ? q - 1 : q;
    }
    case HF_MAP_IMOD: {  // Python mod: result takes s's sign
      int64_t r = x % s;
      return (r != 0 && ((r < 0) != (s < 0))) ? r + s : r;
    }
  }
  return x;
}

template <int OP>
__global__ void __launch_bounds__(BLOCK) k_map_i64(const int64_t* __restrict__ in,
                                                   int64_t* __restrict__ out,
                                                   int64_t s, int64_t n) {
  const int64_t npair = n >> 1;
  const longlong2* in2 = reinterpret_cast<const longlong2*>(in);
  longlong2* out2 = reinterpret_cast<longlong2*>(out);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    longlong2 v = in2[i];
    v.x = map1_i64<OP>(v.x, s);
    v.y = map1_i64<OP>(v.y, s);
    out2[i] = v;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    out[n - 1] = map1_i64<OP>(in[n - 1], s);
}

__global__ void __launch_bounds__(BLOCK) k_cast_i64_f64(const int64_t* __restrict__ in,
                                                        double* __restrict__ out,
                                                        int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (double)in[i];
}

__global__ void __launch_bounds__(BLOCK) k_cast_f64_i64(const double* __restrict__ in,
                                                        int64_t* __restrict__ out,
                                                        int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (int64_t)in[i];
}

// ---------------------------------------------------------------------------
// kernels: Binary (elementwise column op column) — algebra/binary.py device form
// ---------------------------------------------------------------------------

__device__ __forceinline__ double hf_minv(double a, double b) {
  return fmin(a, b);  // NaN-skipping: pandas axis=1 min/max fold
}
__device__ __forceinline__ int64_t hf_minv(int64_t a, int64_t b) {
  return a < b ? a : b;
}
__device__ __forceinline__ double hf_maxv(double a, double b) {
  return fmax(a, b);
}
__device__ __forceinline__ int64_t hf_maxv(int64_t a, int64_t b) {
  return a > b ? a : b;
}

template <int OP, typename T>
__device__ __forceinline__ T bin1(T a, T b) {
  switch (OP) {
    case HF_BIN_ADD: return a + b;
    case HF_BIN_SUB: return a - b;
    case HF_BIN_MUL: return a * b;
    case HF_BIN_DIV: return a / b;
    case HF_BIN_MIN: return hf_minv(a, b);
    case HF_BIN_MAX: return hf_maxv(a, b);
  }
  return a;
}

template <int OP, typename T, typename T2>
__global__ void __launch_bounds__(BLOCK) k_bin(const T* __restrict__ a,
                                               const T* __restrict__ b,
                                               T* __restrict__ out, int64_t n) {
  const int64_t npair = n >> 1;
  const T2* a2 = reinterpret_cast<const T2*>(a);
  const T2* b2 = reinterpret_cast<const T2*>(b);
  T2* o2 = reinterpret_cast<T2*>(out);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    T2 va = a2[i], vb = b2[i];
    va.x = bin1<OP, T>(va.x, vb.x);
    va.y = bin1<OP, T>(va.y, vb.y);
    o2[i] = va;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    out[n - 1] = bin1<OP, T>(a[n - 1], b[n - 1]);
}

// ---------------------------------------------------------------------------
// kernels: TreeReduce — algebra/tree_reduce.py device form
// pandas nan-skipping sum/count/min/max in one pass.
// Wave64 shuffle reduce -> LDS across waves -> one CAS/atomic per block
// (cdna_hip_programming.md Appendix B "Reduction").
// ---------------------------------------------------------------------------

struct ReduceAccF64 {  // lives in d_scratch[0..128)
  double sum;
  unsigned long long count;
  double mn, mx;
};
struct ReduceAccI64 {
  long long sum;
  unsigned long long count;
  long long mn, mx;
};

__device__ void atomic_min_f64(double* addr, double v) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = *p, assumed;
  while (v < __longlong_as_double(old)) {
    assumed = old;
    old = atomicCAS(p, assumed, __double_as_longlong(v));
    if (old == assumed) break;
  }
}
__device__ void atomic_max_f64(double* addr, double v) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = *p, assumed;
  while (v > __longlong_as_double(old)) {
    assumed = old;
    old = atomicCAS(p, assumed, __double_as_longlong(v));
    if (old == assumed) break;
  }
}
__device__ void atomic_min_i64(long long* addr, long long v) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = *p, assumed;
  while (v < (long long)old) {
    assumed = old;
    old = atomicCAS(p, assumed, (unsigned long long)v);
    if (old == assumed) break;
  }
}
__device__ void atomic_max_i64(long long* addr, long long v) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(addr);
  unsigned long long old = *p, assumed;
  while (v > (long long)old) {
    assumed = old;
    old = atomicCAS(p, assumed, (unsigned long long)v);
    if (old == assumed) break;
  }
}

__global__ void k_reduce_init(ReduceAccF64* f, ReduceAccI64* i64a) {
  f->sum = 0.0; f->count = 0;
  f->mn = __longlong_as_double(0x7FF0000000000000LL);   // +inf
  f->mx = __longlong_as_double(0xFFF0000000000000LL);   // -inf
  i64a->sum = 0; i64a->count = 0;
  i64a->mn = 0x7FFFFFFFFFFFFFFFLL;
  i64a->mx = 0x8000000000000000LL;
}

__global__ void __launch_bounds__(BLOCK) k_reduce_f64(const double* __restrict__ in,
                                                      int64_t n, ReduceAccF64* acc) {
  double sum = 0.0, mn = __longlong_as_double(0x7FF0000000000000LL),
         mx = __longlong_as_double(0xFFF0000000000000LL);
  unsigned long long cnt = 0;
  const int64_t npair = n >> 1;
  const double2* in2 = reinterpret_cast<const double2*>(in);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    double2 v = in2[i];
    if (v.x == v.x) { sum += v.x; ++cnt; mn = fmin(mn, v.x); mx = fmax(mx, v.x); }
    if (v.y == v.y) { sum += v.y; ++cnt; mn = fmin(mn, v.y); mx = fmax(mx, v.y); }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double v = in[n - 1];
    if (v == v) { sum += v; ++cnt; mn = fmin(mn, v); mx = fmax(mx, v); }
  }
  // wave64 shuffle reduce
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    cnt += __shfl_down(cnt, off);
    mn = fmin(mn, __shfl_down(mn, off));
    mx = fmax(mx, __shfl_down(mx, off));
  }
  __shared__ double s_sum[BLOCK / 64], s_mn[BLOCK / 64], s_mx[BLOCK / 64];
  __shared__ unsigned long long s_cnt[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; s_mn[wave] = mn; s_mx[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
      sum += s_sum[w]; cnt += s_cnt[w];
      mn = fmin(mn, s_mn[w]); mx = fmax(mx, s_mx[w]);
    }
    if (cnt) {
      unsafeAtomicAdd(&acc->sum, sum);
      atomicAdd(&acc->count, cnt);
      atomic_min_f64(&acc->mn, mn);
      atomic_max_f64(&acc->mx, mx);
    }
  }
}

__device__ __forceinline__ long long llmin(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long llmax(long long a, long long b) { return a > b ? a : b; }

__global__ void __launch_bounds__(BLOCK) k_reduce_i64(const int64_t* __restrict__ in,
                                                      int64_t n, ReduceAccI64* acc) {
  long long sum = 0, mn = 0x7FFFFFFFFFFFFFFFLL, mx = 0x8000000000000000LL;
  unsigned long long cnt = 0;
  const int64_t npair = n >> 1;
  const longlong2* in2 = reinterpret_cast<const longlong2*>(in);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    longlong2 v = in2[i];
    sum += v.x + v.y; cnt += 2;
    mn = llmin(mn, llmin(v.x, v.y));
    mx = llmax(mx, llmax(v.x, v.y));
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    long long v = in[n - 1];
    sum += v; ++cnt; mn = llmin(mn, v); mx = llmax(mx, v);
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    cnt += __shfl_down(cnt, off);
    mn = llmin(mn, (long long)__shfl_down(mn, off));
    mx = llmax(mx, (long long)__shfl_down(mx, off));
  }
  __shared__ long long s_sum[BLOCK / 64], s_mn[BLOCK / 64], s_mx[BLOCK / 64];
  __shared__ unsigned long long s_cnt[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; s_mn[wave] = mn; s_mx[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
      sum += s_sum[w]; cnt += s_cnt[w];
      mn = llmin(mn, s_mn[w]); mx = llmax(mx, s_mx[w]);
    }
    if (cnt) {
      atomicAdd((unsigned long long*)&acc->sum, (unsigned long long)sum);
      atomicAdd(&acc->count, cnt);
      atomic_min_i64(&acc->mn, mn);
      atomic_max_i64(&acc->mx, mx);
    }
  }
}

// ---------------------------------------------------------------------------
// kernels: GroupByReduce — algebra/groupby.py:124/:211 device form.
// Dense key-indexed table accumulation: keys in [key_min, key_min+n_slots).
// One u32-slot rowcnt atomic per row + one hardware f64 atomic add per
// non-NaN value.  The 1e6-key north-star table (8 MB sums + 8 MB rowcnt)
// is Infinity-Cache resident; atomics execute memory-side so the per-XCD L2
// incoherence is not in play.
// ---------------------------------------------------------------------------

constexpr int GB_MAX_VALS = 8;

// per-slot combine for the value table (HF_AGG_*); LDS and global forms use
// hardware ds_*_f64 / global_atomic_*_f64
template <int AOP>
__device__ __forceinline__ void lds_slot_agg(double* a, double v) {
  if (AOP == HF_AGG_SUM)
    unsafeAtomicAdd(a, v);
  else if (AOP == HF_AGG_MIN)
    __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_fetch_max(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int AOP>
__device__ __forceinline__ void glob_slot_agg(double* a, double v) {
  if (AOP == HF_AGG_SUM)
    unsafeAtomicAdd(a, v);
  else if (AOP == HF_AGG_MIN)
    __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    __hip_atomic_fetch_max(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int AOP>
__device__ __forceinline__ double agg_identity() {
  return AOP == HF_AGG_SUM ? 0.0
         : AOP == HF_AGG_MIN ? __longlong_as_double(0x7FF0000000000000LL)
                             : __longlong_as_double(0xFFF0000000000000LL);
}

struct GbPtrs {
  const double* vals[GB_MAX_VALS];
};

template <int NVALS, bool COUNTS, int AOP>
__global__ void __launch_bounds__(BLOCK) k_gb_accum(
    const int64_t* __restrict__ keys, GbPtrs ptrs, int64_t n,
    int64_t key_min, int64_t n_slots,
    double* __restrict__ sums,            // [NVALS][n_slots]
    unsigned long long* __restrict__ rowcnt,  // [n_slots]
    unsigned long long* __restrict__ counts,  // [NVALS][n_slots] or null
    unsigned long long* __restrict__ err) {
  const int64_t npair = n >> 1;
  const longlong2* keys2 = reinterpret_cast<const longlong2*>(keys);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    longlong2 kk = keys2[i];
    const int64_t k0 = kk.x - key_min, k1 = kk.y - key_min;
    const bool ok0 = (uint64_t)k0 < (uint64_t)n_slots;
    const bool ok1 = (uint64_t)k1 < (uint64_t)n_slots;
    if (!ok0 || !ok1) atomicAdd(err, (unsigned long long)(!ok0 + !ok1));
    if (ok0) atomicAdd(&rowcnt[k0], 1ULL);
    if (ok1) atomicAdd(&rowcnt[k1], 1ULL);
#pragma unroll
    for (int c = 0; c < NVALS; ++c) {
      const double2 v = reinterpret_cast<const double2*>(ptrs.vals[c])[i];
      if (ok0 && v.x == v.x) {
        glob_slot_agg<AOP>(&sums[(int64_t)c * n_slots + k0], v.x);
        if (COUNTS) atomicAdd(&counts[(int64_t)c * n_slots + k0], 1ULL);
      }
      if (ok1 && v.y == v.y) {
        glob_slot_agg<AOP>(&sums[(int64_t)c * n_slots + k1], v.y);
        if (COUNTS) atomicAdd(&counts[(int64_t)c * n_slots + k1], 1ULL);
      }
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t k = keys[n - 1] - key_min;
    if ((uint64_t)k < (uint64_t)n_slots) {
      atomicAdd(&rowcnt[k], 1ULL);
      for (int c = 0; c < NVALS; ++c) {
        const double v = ptrs.vals[c][n - 1];
        if (v == v) {
          glob_slot_agg<AOP>(&sums[(int64_t)c * n_slots + k], v);
          if (COUNTS) atomicAdd(&counts[(int64_t)c * n_slots + k], 1ULL);
        }
      }
    } else {
      atomicAdd(err, 1ULL);
    }
  }
}

// ---------------------------------------------------------------------------
// Radix groupby path (the north-star kernel set).
//
// Global f64/u64 atomics saturate at ~23-27 G ops/s on gfx950 (measured,
// tools/atomic_probe.hip; privatizing tables per XCD changes nothing), while
// LDS ds_add_f64 aggregation runs within 14% of the streaming ceiling.  So
// for key ranges beyond LDS capacity the kernel radix-partitions rows into
// buckets of GB_RANGE=8192 keys (u16 local key + f64 value, packed SoA),
// then aggregates each bucket in an LDS-resident dense table:
//   P0 k_gb_hist       : per-bucket row counts (8 B/row read; cached per key
//                        column — immutable columns make this the device
//                        analog of the reference's lazy metadata caches)
//   P1 k_gb_scatter    : read 12 B/row (cached u32 key + f64 val), write
//                        8 B val + 2 B lowkey into exact per-bucket regions
//                        (LDS ranks, one global cursor atomic per
//                        block-tile per bucket); software-pipelined across
//                        tiles (round 2).  Its decisions depend on the keys
//                        alone, so by default the first call RECORDS them as
//                        a plan on the key column and later calls run
//      k_gb_replay     : the recorded value permutation — read 2 B dst +
//                        8 B val, write 8 B val per row; no key reads, no
//                        atomics (P2 reads the low keys from the plan).  The
//                        plan's payload is tile-major: record and replay
//                        write each tile's bucket-sorted staging verbatim
//                        as whole lines, and P2 fetches a bucket's run out
//                        of each tile (TILED)
//   P2 k_gb_bucket_agg : stream each bucket chunk into an LDS table
//                        (ds_add_f64 behind a register run-accumulator for
//                        skewed keys), merge non-empty slots into the
//                        global dense table (atomics only per slot) — or,
//                        for hf_groupby_reduce on a cached group map, store
//                        the whole table as one partial row (PART), which
//      k_gb_combine    : folds per slot, in work-item order, straight into
//                        the compacted output (no dense table, no atomics)
// n_slots <= GB_RANGE skips P0/P1 entirely (k_gb_dense: one 16 B/row pass).
// ---------------------------------------------------------------------------

constexpr int GB_RANGE_LOG = 12;               // 4096 keys per bucket: the
                                               // P2 LDS table is 48 KB -> 3
                                               // blocks/CU (probe: RL12 agg
                                               // 5.0 ms vs RL13 7.2)
constexpr int GB_RANGE = 1 << GB_RANGE_LOG;
constexpr int64_t GB_MAX_BUCKETS = 1024;       // radix path: n_slots <= 4.2M
constexpr int64_t GB_DENSE_MAX = 8192;         // direct-LDS path bound
constexpr int64_t AGG_CHUNK = 1 << 21;         // rows per P2 work item
// Row pairs a lane has in flight in the two streaming aggregates, chosen by
// A/B from {2, 4, 8} (profiles/r08): P2 runs 1.71 -> 1.61 ms at 2 and within
// 0.02 ms of the one-pair loop at 4 and 8; k_gb_dense 4.29 -> 3.03 / 2.87 /
// 2.87 ms at 2 / 4 / 8 (8 costs 117 VGPRs for nothing measurable).
constexpr int GB_P2_U = 2;                     // k_gb_bucket_agg
constexpr int GB_DENSE_U = 4;                  // k_gb_dense

struct GbWorkItem {
  int64_t start;   // absolute row in the scatter regions
  int32_t bucket;
  int32_t len;
};

__global__ void __launch_bounds__(BLOCK) k_gb_hist(
    const int64_t* __restrict__ keys, int64_t n, int64_t key_min,
    int64_t n_slots, int nb, int range_log,
    unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  unsigned* lhist = reinterpret_cast<unsigned*>(smem_raw);
  for (int t = threadIdx.x; t < nb; t += blockDim.x) lhist[t] = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i] - key_min;
    if ((uint64_t)k < (uint64_t)n_slots)
      atomicAdd(&lhist[k >> range_log], 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += blockDim.x)
    if (lhist[t]) atomicAdd(&hist[t], (unsigned long long)lhist[t]);
}

__global__ void __launch_bounds__(BLOCK) k_conv_keys32(
    const int64_t* __restrict__ keys, int64_t n, int64_t key_min,
    unsigned* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i] - key_min;
    out[i] = ((uint64_t)k < 0xFFFFFFFFull) ? (unsigned)k : 0xFFFFFFFFu;
  }
}

struct GbPlanRec {
  unsigned short* dst;
  unsigned* runs;            // [nb][ntiles]
  unsigned long long* meta;  // out-of-range rows
};

// P2 work item on a plan: the runs of one bucket in tiles [tile_begin,
// tile_end), at most AGG_CHUNK rows.
struct GbTileItem {
  int32_t bucket;
  int32_t tile_begin;
  int32_t tile_end;
  uint32_t row0;  // rows of the bucket before tile_begin
};

// P1: LDS-staged bucket-sorted tiles.  Row pairs load 16 B-vectorized
// (longlong2/double2), are ranked into a per-tile LDS histogram (`ds_add`),
// prefix-scanned wave-parallel, staged bucket-SORTED in LDS, and written out
// coalesced — each tile emits one contiguous chunk per bucket stream
// (probe: 2.6x the register-staged direct scatter).  RPT rows/thread
// (even); NV value columns; odd tail row handled by block 0 up front.
// Software-pipelined tile loop (round-2 probe winner, tools/ring_probe.hip:
// P1 6.69 -> 5.52 ms on the 1e9-row north star).  Raw global loads for tile
// t+1 are issued right after tile t's LDS staging — the registers are dead at
// that point — so their ~700-cycle latency hides under t's writeout + barrier
// instead of serializing at the top of the next iteration (the 81%
// wave-parked stall of the round-1 kernel, profiles/r01b/sq_scatter.txt).
// REC: the plan-recording variant (first radix call on a key column).  It
// ranks and stages the same way but does not partition across tiles: the
// tile's bucket-sorted staging goes out verbatim at tile * TILE (values to
// r0, low keys to rk), so it takes no global cursor, and the odd last row is
// one more row of the last tile.  It keeps what a replay and P2 need: each
// row's staging slot (`dst`, one coalesced ushort2 per row pair), the tile's
// run of every bucket (`runs`, bucket-major) and the out-of-range count.  It
// reads the int64 keys; the plan-less variant (!REC) reads the cached u32
// copy.
template <int NV, int RPT, int BLK, int RL, bool REC>
__global__ void __launch_bounds__(BLK) k_gb_scatter(
    const int64_t* __restrict__ keys, const unsigned* __restrict__ keys32,
    const double* __restrict__ v0,
    const double* __restrict__ v1, int64_t n,
    int64_t key_min, int64_t n_slots,
    int nb, unsigned* __restrict__ cursors,
    double* __restrict__ r0, double* __restrict__ r1,
    unsigned short* __restrict__ rk, unsigned long long* __restrict__ err,
    GbPlanRec rec) {
  constexpr bool K32 = !REC;
  constexpr int TILE = BLK * RPT;
  constexpr int PAIRS = RPT / 2;
  static_assert(!REC || TILE < 0xFFFF, "plan dst is u16 with 0xFFFF reserved");
  if (!REC && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    // odd tail row: direct single-row reservation + write
    const int64_t k = (int64_t)keys32[n - 1];
    if ((uint64_t)k < (uint64_t)n_slots) {
      const int b = (int)(k >> RL);
      const int64_t pos = (int64_t)atomicAdd(&cursors[b], 1u);
      rk[pos] = (unsigned short)(k & ((1 << RL) - 1));
      if (NV > 0) r0[pos] = v0[n - 1];
      if (NV > 1) r1[pos] = v1[n - 1];
    } else {
      atomicAdd(err, 1ULL);
    }
  }
  const int64_t npair_total = n >> 1;
  // REC: the odd last row is the x half of pair npair_total
  const int64_t half_pair = (REC && (n & 1)) ? npair_total : -1;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sval0 = reinterpret_cast<double*>(smem_raw);            // [TILE]
  double* sval1 = sval0 + (NV > 1 ? TILE : 0);
  unsigned* skey = reinterpret_cast<unsigned*>(
      sval0 + (NV > 1 ? 2 * (int64_t)TILE : (NV > 0 ? TILE : 0)));  // [TILE]
  unsigned* it_cnt = skey + TILE;                                 // [nb]
  unsigned* it_off = it_cnt + nb;                                 // [nb]
  unsigned* it_gbase = it_off + nb;                               // [nb]
  unsigned* s_total = it_gbase + nb;  // scalar; keep ALL LDS in the dynamic
                                      // region (a static __shared__ would
                                      // shift the base off 16B — G17)
  const int64_t ntiles = ((REC ? n : npair_total * 2) + TILE - 1) / TILE;

  // only the K32-selected key array and the first NV value arrays are ever
  // touched; the others constant-fold away (template params) and cost no
  // registers
  uint2 kraw[PAIRS];
  longlong2 kraw64[PAIRS];
  double2 vraw0[PAIRS];
  double2 vraw1[PAIRS];
  auto issue_loads = [&](int64_t tile) {
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int64_t pj = tile * (TILE / 2) + (int64_t)j * BLK + threadIdx.x;
      if (pj < npair_total) {
        if (K32)
          kraw[j] = reinterpret_cast<const uint2*>(keys32)[pj];
        else
          kraw64[j] = reinterpret_cast<const longlong2*>(keys)[pj];
        if (NV > 0) vraw0[j] = reinterpret_cast<const double2*>(v0)[pj];
        if (NV > 1) vraw1[j] = reinterpret_cast<const double2*>(v1)[pj];
      } else if (REC && pj == half_pair) {
        kraw64[j].x = keys[n - 1];
        if (NV > 0) vraw0[j].x = v0[n - 1];
      }
    }
  };

  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue_loads(tile);
  for (int t = threadIdx.x; t < nb; t += blockDim.x) it_cnt[t] = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    int lb[RPT];
    unsigned lk[RPT];
    unsigned lr[RPT];
    __syncthreads();  // it_cnt cleared (prologue or previous iteration)
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int64_t pj = tile * (TILE / 2) + (int64_t)j * BLK + threadIdx.x;
      const int a = 2 * j, bslot = 2 * j + 1;
      lb[a] = lb[bslot] = -1;
      if (pj < npair_total) {
        const int64_t ka = K32 ? (int64_t)kraw[j].x : kraw64[j].x - key_min;
        const int64_t kb = K32 ? (int64_t)kraw[j].y : kraw64[j].y - key_min;
        if ((uint64_t)ka < (uint64_t)n_slots) {
          lb[a] = (int)(ka >> RL);
          lk[a] = (unsigned)(ka & ((1 << RL) - 1));
        } else {
          atomicAdd(err, 1ULL);
          if (REC) atomicAdd(rec.meta, 1ULL);
        }
        if ((uint64_t)kb < (uint64_t)n_slots) {
          lb[bslot] = (int)(kb >> RL);
          lk[bslot] = (unsigned)(kb & ((1 << RL) - 1));
        } else {
          atomicAdd(err, 1ULL);
          if (REC) atomicAdd(rec.meta, 1ULL);
        }
      } else if (REC && pj == half_pair) {
        const int64_t ka = kraw64[j].x - key_min;
        if ((uint64_t)ka < (uint64_t)n_slots) {
          lb[a] = (int)(ka >> RL);
          lk[a] = (unsigned)(ka & ((1 << RL) - 1));
        } else {
          atomicAdd(err, 1ULL);
          atomicAdd(rec.meta, 1ULL);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < RPT; ++j)
      if (lb[j] >= 0) lr[j] = atomicAdd(&it_cnt[lb[j]], 1u);
    __syncthreads();
    // wave 0: parallel exclusive scan over the nb tile counters
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      unsigned carry = 0;
      for (int base = 0; base < nb; base += 64) {
        const int t = base + lane;
        unsigned v = (t < nb) ? it_cnt[t] : 0;
        unsigned incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          unsigned up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        if (t < nb) it_off[t] = carry + incl - v;
        carry += __shfl(incl, 63);
      }
      if (lane == 0) *s_total = carry;
    }
    __syncthreads();
    if (!REC) {
      for (int t = threadIdx.x; t < nb; t += blockDim.x) {
        const unsigned c = it_cnt[t];
        if (c) it_gbase[t] = atomicAdd(&cursors[t], c);
      }
    }
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      if (lb[j] >= 0) {
        const unsigned p = it_off[lb[j]] + lr[j];
        skey[p] = ((unsigned)lb[j] << 16) | lk[j];
        if (NV > 0) sval0[p] = (j & 1) ? vraw0[j >> 1].y : vraw0[j >> 1].x;
        if (NV > 1) sval1[p] = (j & 1) ? vraw1[j >> 1].y : vraw1[j >> 1].x;
      }
    }
    if (REC) {
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) {
        const int64_t pj = tile * (TILE / 2) + (int64_t)j * BLK + threadIdx.x;
        const int a = 2 * j, bslot = 2 * j + 1;
        if (pj < npair_total) {
          ushort2 d;
          d.x = lb[a] >= 0 ? (unsigned short)(it_off[lb[a]] + lr[a]) : 0xFFFF;
          d.y = lb[bslot] >= 0
                    ? (unsigned short)(it_off[lb[bslot]] + lr[bslot])
                    : 0xFFFF;
          reinterpret_cast<ushort2*>(rec.dst)[pj] = d;
        } else if (pj == half_pair) {
          rec.dst[n - 1] =
              lb[a] >= 0 ? (unsigned short)(it_off[lb[a]] + lr[a]) : 0xFFFF;
        }
      }
      // the tile's run of every bucket (before the loop-bottom clear of it_cnt)
      for (int t = threadIdx.x; t < nb; t += blockDim.x)
        rec.runs[(int64_t)t * ntiles + tile] = it_off[t] | (it_cnt[t] << 16);
    }
    __syncthreads();  // staging visible; it_cnt reads (scan, runs) done
    // registers are dead — issue the NEXT tile's loads so they fly during
    // this tile's writeout, and clear it_cnt for the next rank phase
    const int64_t nxt = tile + gridDim.x;
    if (nxt < ntiles) issue_loads(nxt);
    for (int t = threadIdx.x; t < nb; t += blockDim.x) it_cnt[t] = 0;
    const int staged = (int)*s_total;
    for (int p = threadIdx.x; p < staged; p += blockDim.x) {
      const unsigned b = skey[p] >> 16;
      const int64_t pos = REC ? tile * (int64_t)TILE + p
                              : (int64_t)it_gbase[b] + (p - it_off[b]);
      rk[pos] = (unsigned short)(skey[p] & 0xFFFF);
      if (NV > 0) r0[pos] = sval0[p];
      if (NV > 1) r1[pos] = sval1[p];
    }
    // loop-top barrier orders the writeout's LDS reads against the next
    // tile's staging writes
  }
}

// Plan geometry: the 1024x12 tile of the single-column scatter, for every
// nvals (one plan serves all value-column counts).
constexpr int GB_PLAN_BLK = 1024;
constexpr int GB_PLAN_RPT = 12;
constexpr int GB_PLAN_TILE = GB_PLAN_BLK * GB_PLAN_RPT;
// replay writeout flavour when HF_GB_NT_STORE is unset (profiles/r11)
constexpr bool GB_REPLAY_NT_DEFAULT = true;

// P1 steady state: replay a recorded plan as a pure value permutation, one
// value column per launch.  Reads 2 B dst + 8 B value per row, writes 8 B;
// no key reads, no LDS atomics, no scan, no global atomics, no table.  A
// tile's staging goes out verbatim at tile * TILE, as whole aligned 16-byte
// stores per lane; slots past the tile's staged count (a tile with
// out-of-range keys, the end of the last tile) carry stale LDS and are never
// read by P2, which follows the recorded runs.  Same software pipelining as
// k_gb_scatter: the next tile's loads are issued right after this tile's
// staging.  NT: non-temporal stores for the writeout.
template <int RPT, int BLK, bool NT>
__global__ void __launch_bounds__(BLK) k_gb_replay(
    const unsigned short* __restrict__ dst, const double* __restrict__ v,
    int64_t n, const unsigned long long* __restrict__ meta,
    double* __restrict__ r0, unsigned long long* __restrict__ err,
    int add_err) {
  constexpr int TILE = BLK * RPT;
  constexpr int PAIRS = RPT / 2;
  typedef double nd2 __attribute__((ext_vector_type(2)));
  if (add_err && blockIdx.x == 0 && threadIdx.x == 0) {
    // out-of-range keys were counted while recording; every call reports them
    const unsigned long long oor = meta[0];
    if (oor) atomicAdd(err, oor);
  }
  const int64_t npair_total = n >> 1;
  const int64_t half_pair = (n & 1) ? npair_total : -1;  // the odd last row
  const int64_t ntiles = (n + TILE - 1) / TILE;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sval = reinterpret_cast<double*>(smem_raw);         // [TILE]

  unsigned draw[PAIRS];
  double2 vraw[PAIRS];
  auto issue_loads = [&](int64_t tile) {
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int64_t pj = tile * (TILE / 2) + (int64_t)j * BLK + threadIdx.x;
      if (pj < npair_total) {
        draw[j] = reinterpret_cast<const unsigned*>(dst)[pj];
        vraw[j] = reinterpret_cast<const double2*>(v)[pj];
      } else if (pj == half_pair) {
        draw[j] = dst[n - 1] | 0xFFFF0000u;
        vraw[j].x = v[n - 1];
      }
    }
  };

  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue_loads(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // previous tile's writeout is done with sval
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int64_t pj = tile * (TILE / 2) + (int64_t)j * BLK + threadIdx.x;
      if (pj < npair_total || pj == half_pair) {
        const unsigned pa = draw[j] & 0xFFFFu, pb = draw[j] >> 16;
        if (pa < (unsigned)TILE) sval[pa] = vraw[j].x;
        if (pb < (unsigned)TILE) sval[pb] = vraw[j].y;
      }
    }
    __syncthreads();  // staging visible
    const int64_t nxt = tile + gridDim.x;
    if (nxt < ntiles) issue_loads(nxt);
    // rows of this tile, rounded up to a pair (r0 holds ntiles * TILE rows)
    const int64_t left = n - tile * (int64_t)TILE;
    const int pairs = left >= TILE ? TILE / 2 : (int)((left + 1) >> 1);
    nd2* out = reinterpret_cast<nd2*>(r0 + tile * (int64_t)TILE);
    const nd2* in = reinterpret_cast<const nd2*>(sval);
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int q = j * BLK + threadIdx.x;
      if (q < pairs) {
        if (NT)
          __builtin_nontemporal_store(in[q], out + q);
        else
          out[q] = in[q];
      }
    }
  }
}

// The P2 work items of a freshly recorded plan, from the per-(bucket, tile)
// run lengths; one wave per bucket.  Tile t of a bucket belongs to item
// (cost of the bucket before t) / cut, where a tile costs its rows of the
// bucket, but GB_TILE_COST at the least: the items are row-balanced where the
// runs are long, and where a bucket has a few rows in each of very many tiles
// (a zipf tail) an item is bounded in tiles, since such an item is bound by
// its chain of round trips, not by its rows.  A tile costs less than the cut,
// so the
// item index grows by at most one per tile, and an item holds fewer
// than cut + TILE <= AGG_CHUNK rows.
// Two passes of the same walk: FILL = false counts the bucket's items into
// nitems[b]; FILL = true writes them and item0.
// The cut (gb_item_cut) aims at GB_ITEMS_MIN items or more: a frame of 1e8
// rows in 62 buckets would otherwise keep 62 of 256 CUs busy, and P2 on a
// plan is bound by what one CU gathers (profiles/r11).  Not below 2^18 rows,
// so that the table an item flushes or merges stays small beside its rows.
constexpr int64_t GB_ITEM_CUT_MAX = AGG_CHUNK - GB_PLAN_TILE;
constexpr int64_t GB_ITEM_CUT_MIN = 1 << 18;
constexpr int64_t GB_ITEMS_MIN = 256;
constexpr int64_t GB_TILE_COST = 128;  // rows a tile of an item counts for

template <bool FILL>
__global__ void __launch_bounds__(64) k_gb_plan_items(
    const unsigned* __restrict__ runs, int64_t ntiles, int nb, int64_t cut,
    unsigned* __restrict__ nitems, unsigned* __restrict__ item0,
    GbTileItem* __restrict__ items) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const unsigned* row = runs + (int64_t)b * ntiles;
  unsigned first = 0, mine = 0;
  if (FILL) {
    // this bucket's first item: the items of the buckets before it
    unsigned acc = 0;
    for (int t = lane; t < nb; t += 64) acc += t < b ? nitems[t] : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    first = acc;
    mine = nitems[b];
    if (lane == 0) {
      item0[b] = first;
      if (b == nb - 1) item0[nb] = first + mine;
    }
    if (mine == 0) return;
  }
  int64_t carry = 0;      // rows of the bucket before this stride of tiles
  int64_t ccarry = 0;     // their cost
  int64_t last_excl = -1; // cost before the last non-empty tile
  int prev_item = -1;     // item of the tile before this stride
  for (int64_t t0 = 0; t0 < ntiles; t0 += 64) {
    const int64_t t = t0 + lane;
    const unsigned len = t < ntiles ? row[t] >> 16 : 0u;
    const unsigned cost =
        t < ntiles ? max(len, (unsigned)GB_TILE_COST) : 0u;
    unsigned incl = len, cincl = cost;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d);
      const unsigned cup = __shfl_up(cincl, d);
      if (lane >= d) incl += up;
      if (lane >= d) cincl += cup;
    }
    const int64_t excl = carry + incl - len;      // rows before t
    const int64_t cexcl = ccarry + cincl - cost;  // cost before t
    if (!FILL) {
      int64_t e = len ? cexcl : -1;
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(e, d);
        e = o > e ? o : e;
      }
      if (e > last_excl) last_excl = e;
    } else {
      // trailing empty tiles stay in the last item
      const int it = (int)min((int64_t)(cexcl / cut), (int64_t)mine - 1);
      int before = __shfl_up(it, 1);
      if (lane == 0) before = prev_item;
      if (t < ntiles && it != before) {
        items[first + it].bucket = b;
        items[first + it].tile_begin = (int)t;
        items[first + it].row0 = (unsigned)excl;
        if (it > 0) items[first + it - 1].tile_end = (int)t;
      }
      prev_item = __shfl(it, 63);
    }
    carry += __shfl(incl, 63);
    ccarry += __shfl(cincl, 63);
  }
  if (!FILL) {
    if (lane == 0)
      nitems[b] = last_excl < 0 ? 0u : (unsigned)(last_excl / cut) + 1u;
  } else if (lane == 0) {
    items[first + mine - 1].tile_end = (int)ntiles;
  }
}

// nvals == 0 on a recorded plan runs no P1 at all; this carries the recorded
// out-of-range count to the shared error word so compaction still raises.
__global__ void k_gb_plan_err(const unsigned long long* __restrict__ meta,
                              unsigned long long* __restrict__ err) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && meta[0]) atomicAdd(err, meta[0]);
}

// P2: one work item per (bucket, chunk), one block per item; one value
// column per launch.
// ROWCNT: also mark group presence (first column / keys-only pass).  The
// global rowcnt table is PRESENCE-ONLY everywhere (compaction tests >0;
// per-column counts live in the counts table), so the per-row mark is a
// plain LDS byte store (last-writer-wins, LDS is CU-local) — no atomic.
// CNT: also merge per-slot non-NaN counts for this column.
// 2 rows/lane vectorized.  INVARIANT: every item start is even — a start is
// region base + k * AGG_CHUNK, regions are 64-row aligned and AGG_CHUNK is
// even (ensure_radix_layout) — so the ushort2/double2 streams are aligned
// from the first row; only the last chunk of a bucket can have an odd tail.
// PART (hf_groupby_reduce on a cached group map): presence is already known,
// so no touch bytes and no ROWCNT, and instead of the atomic merge the block
// stores its whole table — identity in untouched slots — as its item's row of
// part_sums / part_cnt with plain 16-byte stores; k_gb_combine folds the rows
// of a bucket.
// A 16384-slot table (RL = 14, sums without counts) is 128 KB, so one block
// fits a CU: it runs 1024 threads, the same 16 waves per CU as two 512-thread
// blocks at RL = 13.  The loops stride by blockDim.x.
// Two row iterations feed the same accumulate / flush code:
//  * !TILED, the plan-less path: the item is a contiguous chunk of a bucket
//    region (GbWorkItem), streamed as row pairs;
//  * TILED, on a plan: the item is the bucket's runs in a range of tiles
//    (GbTileItem) of the tile-major payload.  Each wave takes chunks of up to
//    64 consecutive tiles: one coalesced load brings the chunk's run
//    descriptors, one per lane (the next chunk's are fetched before this
//    chunk's rows), and a wave scan turns the lengths into row offsets.  Then
//    either the wave sweeps the chunk's rows as one flat stream, 64 rows per
//    step and GB_P2_TU steps in flight, each lane keeping a cursor into the
//    chunk's offsets in LDS that only ever moves forward (about one 8-byte LDS
//    read per run a lane enters — no per-row search); or, when no run of the
//    chunk is longer than GB_P2_SPARSE rows (a zipf tail bucket), every lane
//    reads its own run, so 64 runs share one round trip.  Rows are loaded one
//    per lane (8 B + 2 B): runs start at any row, so there are no pair loads
//    and no pad rows.  No barrier inside the walk: the waves run apart until
//    the flush.
constexpr int gb_p2_block(int rl) { return rl >= 14 ? 1024 : 512; }
constexpr int GB_P2_TU = 8;       // 64-row steps in flight per wave (TILED)
constexpr int GB_P2_SPARSE = 8;   // longest run of a lane-per-run chunk

template <bool ROWCNT, bool CNT, bool HAVE_VAL, int RL, int AOP,
          bool PART = false, bool TILED = false>
__global__ void __launch_bounds__(gb_p2_block(RL)) k_gb_bucket_agg(
    const double* __restrict__ vals, const unsigned short* __restrict__ lowkeys,
    const void* __restrict__ work, int64_t n_slots,
    double* __restrict__ gsums, unsigned long long* __restrict__ growcnt,
    unsigned long long* __restrict__ gcounts,
    double* __restrict__ part_sums = nullptr,   // [gridDim.x][RANGE] (PART)
    unsigned* __restrict__ part_cnt = nullptr,  // likewise, with CNT
    const unsigned* __restrict__ runs = nullptr,  // [nb][ntiles] (TILED)
    int64_t ntiles = 0,
    const unsigned* __restrict__ order = nullptr) {  // block -> item (TILED)
  static_assert(!PART || (HAVE_VAL && !ROWCNT), "PART flushes value tables");
  static_assert(RL <= 16, "low keys are u16");
  static_assert(RL <= 13 || !CNT, "no LDS for a counts table beside 16384 sums");
  constexpr int RANGE = 1 << RL;
  __shared__ __attribute__((aligned(16))) double lsums[HAVE_VAL ? RANGE : 1];
  __shared__ __attribute__((aligned(16))) unsigned lcnt[CNT ? RANGE : 1];
  __shared__ unsigned char ltouch[PART ? 1 : RANGE];
  // TILED: per wave, a chunk's {end row, payload offset - start row} per run
  __shared__ uint2 lruns[TILED ? gb_p2_block(RL) : 1];
  // TILED: the blocks take the items in the plan's dispatch order
  const unsigned item = TILED ? order[blockIdx.x] : blockIdx.x;
  const int bucket = TILED
      ? reinterpret_cast<const GbTileItem*>(work)[item].bucket
      : reinterpret_cast<const GbWorkItem*>(work)[item].bucket;
  for (int s = threadIdx.x; s < RANGE; s += blockDim.x) {
    if (HAVE_VAL) lsums[s] = agg_identity<AOP>();
    if (!PART) ltouch[s] = 0;
    if (CNT) lcnt[s] = 0;
  }
  __syncthreads();
  // register run-accumulation: consecutive rows of a lane's stream that
  // share a slot combine in a register before ONE LDS op — on skewed
  // keys the head slot dominates its bucket and the per-slot ds_add
  // would serialize (zipf P2 was 3.8x the uniform cost); on uniform the
  // run length is ~1 and this is a predictable branch
  int rslot = -1;
  double racc = 0.0;
  unsigned rcnt = 0;
  auto flush = [&]() {
    if (rslot >= 0) {
      lds_slot_agg<AOP>(&lsums[rslot], racc);
      if (CNT) atomicAdd(&lcnt[rslot], rcnt);
    }
    rslot = -1;
    rcnt = 0;
  };
  auto feed = [&](int slot, double v) {
    if (!PART) ltouch[slot] = 1;
    if (HAVE_VAL && v == v) {
      if (slot == rslot) {
        racc = AOP == HF_AGG_SUM ? racc + v
               : AOP == HF_AGG_MIN ? fmin(racc, v) : fmax(racc, v);
        ++rcnt;
      } else {
        flush();
        rslot = slot;
        racc = v;
        rcnt = 1;
      }
    }
  };
  if constexpr (!TILED) {
    const GbWorkItem w =
        reinterpret_cast<const GbWorkItem*>(work)[blockIdx.x];
    const int64_t end = w.start + w.len;
    const int64_t a0 = w.start;  // even (see above)
    const int64_t npair = (end - a0) >> 1;
    const ushort2* k2 = reinterpret_cast<const ushort2*>(lowkeys + a0);
    const double2* v2 = reinterpret_cast<const double2*>(vals + a0);
    // both streams are read once: non-temporal loads (the builtin takes
    // native scalars and vectors, hence the u32 / ext_vector views of a
    // pair); P2 1.70 -> 1.56 ms on top of the two-pair loop (profiles/r08)
    auto ld_k = [&](int64_t i) {
      const unsigned r = __builtin_nontemporal_load(
          reinterpret_cast<const unsigned*>(k2) + i);
      return make_ushort2((unsigned short)(r & 0xFFFFu),
                          (unsigned short)(r >> 16));
    };
    auto ld_v = [&](int64_t i) {
      typedef double nd2 __attribute__((ext_vector_type(2)));
      const nd2 r = __builtin_nontemporal_load(
          reinterpret_cast<const nd2*>(v2) + i);
      return make_double2(r.x, r.y);
    };
    auto feed_pair = [&](ushort2 kk, double2 vv) {
      if (HAVE_VAL) {
        feed(kk.x, vv.x);
        feed(kk.y, vv.y);
      } else {
        ltouch[kk.x] = 1;
        ltouch[kk.y] = 1;
      }
    };
    // GB_P2_U pairs in flight per lane: a body trip issues the loads of U
    // block-strides, then feeds them in stride order, so a lane sees the rows
    // it would see one stride at a time, in that order.  The trip condition
    // is block-uniform; the last < U * blockDim.x pairs go one stride at a
    // time.
    constexpr int U = GB_P2_U;
    const int64_t bstep = (int64_t)U * blockDim.x;
    int64_t base = 0;
    for (; base + bstep <= npair; base += bstep) {
      ushort2 kk[U];
      double2 vv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * blockDim.x + threadIdx.x;
        kk[u] = ld_k(i);
        if (HAVE_VAL) vv[u] = ld_v(i);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) feed_pair(kk[u], vv[u]);
    }
    for (int64_t i = base + threadIdx.x; i < npair; i += blockDim.x) {
      const ushort2 kk = ld_k(i);
      double2 vv = make_double2(0.0, 0.0);
      if (HAVE_VAL) vv = ld_v(i);
      feed_pair(kk, vv);
    }
    flush();
    if (((end - a0) & 1) && threadIdx.x == 0) {
      const int slot = lowkeys[end - 1];
      if (!PART) ltouch[slot] = 1;
      if (HAVE_VAL) {
        const double v = vals[end - 1];
        if (v == v) {
          lds_slot_agg<AOP>(&lsums[slot], v);
          if (CNT) atomicAdd(&lcnt[slot], 1u);
        }
      }
    }
  } else {
    constexpr int TILE = GB_PLAN_TILE;
    constexpr int U = GB_P2_TU;
    const GbTileItem w = reinterpret_cast<const GbTileItem*>(work)[item];
    const int lane = threadIdx.x & 63;
    const int nw = blockDim.x >> 6;
    // tiles per chunk: every wave gets the same number of chunks, of at most
    // 64 tiles and of equal size (a block is as slow as its slowest wave; an
    // item of few tiles — sorted keys — still gives every wave a share)
    const int nt = w.tile_end - w.tile_begin;
    const int per_wave = (nt + nw * 64 - 1) / (nw * 64);  // chunks per wave
    const int cs = (nt + nw * per_wave - 1) / (nw * per_wave);
    const int64_t cstep = (int64_t)nw * cs;
    const unsigned* row = runs + (int64_t)w.bucket * ntiles;
    uint2* we = lruns + (threadIdx.x & ~63);
    auto ld_desc = [&](int64_t c) {
      const int64_t t = c + lane;
      return (lane < cs && t < w.tile_end) ? row[t] : 0u;
    };
    auto row_in = [&](const unsigned short* kb, const double* vb, unsigned at,
                      unsigned& k, double& v) {
      k = __builtin_nontemporal_load(kb + at);
      if (HAVE_VAL) v = __builtin_nontemporal_load(vb + at);
    };
    int64_t c = w.tile_begin + (int64_t)(threadIdx.x >> 6) * cs;
    unsigned d = c < w.tile_end ? ld_desc(c) : 0u;
    for (; c < w.tile_end; c += cstep) {  // wave-uniform trips
      const unsigned len = d >> 16, st = d & 0xFFFFu;
      d = c + cstep < w.tile_end ? ld_desc(c + cstep) : 0u;
      unsigned incl = len, longest = len;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const unsigned up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
        longest = max(longest, (unsigned)__shfl_xor(longest, s));
      }
      const unsigned total = __shfl(incl, 63);
      const unsigned short* kb = lowkeys + c * TILE;
      const double* vb = vals + c * TILE;
      if (longest <= (unsigned)GB_P2_SPARSE) {
        // a lane per run
        const unsigned at = (unsigned)lane * TILE + st;
        for (unsigned k0 = 0; k0 < longest; k0 += U) {
          unsigned kk[U];
          double vv[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            vv[u] = 0.0;
            if (k0 + u < len) row_in(kb, vb, at + k0 + u, kk[u], vv[u]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (k0 + u < len) feed(kk[u], vv[u]);
        }
      } else {
        // the chunk's rows as one stream; run j ends at row we[j].x and its
        // row r lies at payload offset we[j].y + r (mod 2^32)
        we[lane] = make_uint2(incl, (unsigned)lane * TILE + st - (incl - len));
        __builtin_amdgcn_wave_barrier();
        int j = 0;
        uint2 e = we[0];
        for (unsigned r0 = 0; r0 < total; r0 += 64 * U) {
          unsigned kk[U];
          double vv[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const unsigned r = r0 + u * 64 + lane;
            vv[u] = 0.0;
            if (r < total) {
              while (r >= e.x) e = we[++j];  // r < total = the last end
              row_in(kb, vb, e.y + r, kk[u], vv[u]);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (r0 + u * 64 + lane < total) feed(kk[u], vv[u]);
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  flush();
  __syncthreads();
  if (PART) {
    double2* ps = reinterpret_cast<double2*>(part_sums +
                                             (int64_t)item * RANGE);
    const double2* ls = reinterpret_cast<const double2*>(lsums);
    for (int s = threadIdx.x; s < RANGE / 2; s += blockDim.x) ps[s] = ls[s];
    if (CNT) {
      uint4* pc = reinterpret_cast<uint4*>(part_cnt +
                                           (int64_t)item * RANGE);
      const uint4* lc = reinterpret_cast<const uint4*>(lcnt);
      for (int s = threadIdx.x; s < RANGE / 4; s += blockDim.x) pc[s] = lc[s];
    }
    return;
  }
  const int64_t gbase = (int64_t)bucket << RL;
  for (int s = threadIdx.x; s < RANGE; s += blockDim.x) {
    if (!ltouch[s] || gbase + s >= n_slots) continue;
    if (HAVE_VAL) glob_slot_agg<AOP>(&gsums[gbase + s], lsums[s]);
    if (ROWCNT) atomicAdd(&growcnt[gbase + s], 1ULL);
    if (CNT) atomicAdd(&gcounts[gbase + s], (unsigned long long)lcnt[s]);
  }
}

// Merge + compaction of the PART flush, one thread per slot: fold the partial
// tables of the slot's bucket in work-item order (so the chunk merge is
// deterministic) and write the result at the slot's cached output row.
// Absent slots are skipped; a present slot's bucket has at least one item.
template <int RL, int AOP, bool CNT>
__global__ void __launch_bounds__(BLOCK) k_gb_combine(
    const unsigned* __restrict__ gidx, const unsigned* __restrict__ item0,
    const double* __restrict__ part_sums, const unsigned* __restrict__ part_cnt,
    int64_t n_slots, double* __restrict__ out_sums,
    int64_t* __restrict__ out_counts) {
  constexpr int RANGE = 1 << RL;
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const unsigned gi = gidx[s];
  if (gi == 0xFFFFFFFFu) return;
  const int64_t b = s >> RL;
  const int64_t lo = s & (RANGE - 1);
  double acc = agg_identity<AOP>();
  int64_t cnt = 0;
  auto fold = [&](double p) {
    acc = AOP == HF_AGG_SUM ? acc + p
          : AOP == HF_AGG_MIN ? fmin(acc, p) : fmax(acc, p);
  };
  const unsigned i1 = item0[b + 1];
  unsigned i = item0[b];
  // a skewed head bucket has hundreds of items and only RANGE threads to fold
  // them: load U tables' values at once, then fold them in item order
  constexpr unsigned U = 8;
  for (; i + U <= i1; i += U) {
    double p[U];
    unsigned c[U];
#pragma unroll
    for (unsigned u = 0; u < U; ++u) {
      p[u] = part_sums[(int64_t)(i + u) * RANGE + lo];
      if (CNT) c[u] = part_cnt[(int64_t)(i + u) * RANGE + lo];
    }
#pragma unroll
    for (unsigned u = 0; u < U; ++u) {
      fold(p[u]);
      if (CNT) cnt += c[u];
    }
  }
  for (; i < i1; ++i) {
    fold(part_sums[(int64_t)i * RANGE + lo]);
    if (CNT) cnt += part_cnt[(int64_t)i * RANGE + lo];
  }
  out_sums[gi] = acc;
  if (CNT) out_counts[gi] = cnt;
}

// Dense direct path: n_slots <= GB_RANGE, one 16 B/row pass per column.
template <bool ROWCNT, bool CNT, bool HAVE_VAL, int AOP>
__global__ void __launch_bounds__(512) k_gb_dense(
    const int64_t* __restrict__ keys, const double* __restrict__ vals,
    int64_t n, int64_t key_min, int64_t n_slots,
    double* __restrict__ gsums, unsigned long long* __restrict__ growcnt,
    unsigned long long* __restrict__ gcounts,
    unsigned long long* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* lsums = reinterpret_cast<double*>(smem_raw);       // [n_slots]
  unsigned* lcnt = reinterpret_cast<unsigned*>(
      lsums + (HAVE_VAL ? n_slots : 0));                     // when CNT
  unsigned char* ltouch = reinterpret_cast<unsigned char*>(
      lcnt + (CNT ? n_slots : 0));                           // presence bytes
  for (int64_t s = threadIdx.x; s < n_slots; s += blockDim.x) {
    if (HAVE_VAL) lsums[s] = agg_identity<AOP>();
    ltouch[s] = 0;
    if (CNT) lcnt[s] = 0;
  }
  __syncthreads();
  auto row = [&](int64_t key, double v) {
    const int64_t k = key - key_min;
    if ((uint64_t)k >= (uint64_t)n_slots) {
      atomicAdd(err, 1ULL);
      return;
    }
    ltouch[k] = 1;  // presence-only (plain LDS byte store, CU-local)
    if (HAVE_VAL && v == v) {
      lds_slot_agg<AOP>(&lsums[k], v);
      if (CNT) atomicAdd(&lcnt[k], 1u);
    }
  };
  // 2 rows/lane vectorized, block-strided over row pairs.  INVARIANT: keys
  // and vals are column buffers straight from the device allocator (hipMalloc
  // blocks, 256-byte aligned; a column never points into another's block), so
  // the longlong2/double2 casts are 16-byte aligned from row 0.
  const longlong2* k2 = reinterpret_cast<const longlong2*>(keys);
  const double2* v2 = reinterpret_cast<const double2*>(vals);
  const int64_t npair = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // GB_DENSE_U pairs in flight per lane: a body trip issues the loads of U
  // grid-strides before it consumes the first; the trip condition is
  // block-uniform, the rest goes one stride at a time.
  constexpr int U = GB_DENSE_U;
  int64_t p0 = (int64_t)blockIdx.x * blockDim.x;
  for (; p0 + (U - 1) * stride + blockDim.x <= npair; p0 += U * stride) {
    longlong2 kk[U];
    double2 vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t p = p0 + u * stride + threadIdx.x;
      kk[u] = k2[p];
      if (HAVE_VAL) vv[u] = v2[p];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row(kk[u].x, HAVE_VAL ? vv[u].x : 0.0);
      row(kk[u].y, HAVE_VAL ? vv[u].y : 0.0);
    }
  }
  for (int64_t p = p0 + threadIdx.x; p < npair; p += stride) {
    const longlong2 kk = k2[p];
    double2 vv = make_double2(0.0, 0.0);
    if (HAVE_VAL) vv = v2[p];
    row(kk.x, vv.x);
    row(kk.y, vv.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    row(keys[n - 1], HAVE_VAL ? vals[n - 1] : 0.0);
  __syncthreads();
  for (int64_t s = threadIdx.x; s < n_slots; s += blockDim.x) {
    if (!ltouch[s]) continue;
    if (HAVE_VAL) glob_slot_agg<AOP>(&gsums[s], lsums[s]);
    if (ROWCNT) atomicAdd(&growcnt[s], 1ULL);
    if (CNT) atomicAdd(&gcounts[s], (unsigned long long)lcnt[s]);
  }
}

// ---------------------------------------------------------------------------
// Fused group moments (hf_group_moments): Σd, Σd², Σd³, Σd⁴, min x, max x per
// group with d = x − centre[group] — the centred second pass behind groupby
// skew and frame skew/kurt (storage_formats/pandas/groupby.py:116 sums raw
// powers; centring first keeps the moments conditioned at large mean/std).
// Table rows are [6][n_groups] in LDS and in global memory alike.
// ---------------------------------------------------------------------------

constexpr int GM_ROWS = 6;
constexpr int64_t GM_LDS_MAX = 1024;  // 7 x 8 B x 1024 = 56 KB: 2 blocks / CU

template <bool LDS>
__device__ __forceinline__ void gm_update(double* tab, int64_t ng, int64_t g,
                                          double x, double c) {
  const double d = x - c, d2 = d * d;
  if (LDS) {
    lds_slot_agg<HF_AGG_SUM>(&tab[g], d);
    lds_slot_agg<HF_AGG_SUM>(&tab[ng + g], d2);
    lds_slot_agg<HF_AGG_SUM>(&tab[2 * ng + g], d2 * d);
    lds_slot_agg<HF_AGG_SUM>(&tab[3 * ng + g], d2 * d2);
    lds_slot_agg<HF_AGG_MIN>(&tab[4 * ng + g], x);
    lds_slot_agg<HF_AGG_MAX>(&tab[5 * ng + g], x);
  } else {
    glob_slot_agg<HF_AGG_SUM>(&tab[g], d);
    glob_slot_agg<HF_AGG_SUM>(&tab[ng + g], d2);
    glob_slot_agg<HF_AGG_SUM>(&tab[2 * ng + g], d2 * d);
    glob_slot_agg<HF_AGG_SUM>(&tab[3 * ng + g], d2 * d2);
    glob_slot_agg<HF_AGG_MIN>(&tab[4 * ng + g], x);
    glob_slot_agg<HF_AGG_MAX>(&tab[5 * ng + g], x);
  }
}

// LDS path: block-private copy of the six rows + centre, touched slots only
// are flushed.  gid < 0 rows are skipped, gid >= n_groups rows are counted.
__global__ void __launch_bounds__(512) k_gm_lds(
    const int64_t* __restrict__ gid, const double* __restrict__ val, int64_t n,
    const double* __restrict__ centre, int64_t ng, double* __restrict__ gtab,
    unsigned long long* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* ltab = reinterpret_cast<double*>(smem_raw);       // [6][ng]
  double* lc = ltab + GM_ROWS * ng;                         // [ng]
  unsigned char* ltouch = reinterpret_cast<unsigned char*>(lc + ng);
  for (int64_t s = threadIdx.x; s < ng; s += blockDim.x) {
    ltab[s] = ltab[ng + s] = ltab[2 * ng + s] = ltab[3 * ng + s] = 0.0;
    ltab[4 * ng + s] = agg_identity<HF_AGG_MIN>();
    ltab[5 * ng + s] = agg_identity<HF_AGG_MAX>();
    lc[s] = centre[s];
    ltouch[s] = 0;
  }
  __syncthreads();
  auto row = [&](int64_t g, double x) {
    if (g < 0) return;
    if (g >= ng) { atomicAdd(err, 1ULL); return; }
    if (x != x) return;
    ltouch[g] = 1;
    gm_update<true>(ltab, ng, g, x, lc[g]);
  };
  const int64_t npair = n >> 1;
  const longlong2* gid2 = reinterpret_cast<const longlong2*>(gid);
  const double2* val2 = reinterpret_cast<const double2*>(val);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    const longlong2 gg = gid2[i];
    const double2 v = val2[i];
    row(gg.x, v.x);
    row(gg.y, v.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) row(gid[n - 1], val[n - 1]);
  __syncthreads();
  for (int64_t s = threadIdx.x; s < ng; s += blockDim.x) {
    if (!ltouch[s]) continue;
    glob_slot_agg<HF_AGG_SUM>(&gtab[s], ltab[s]);
    glob_slot_agg<HF_AGG_SUM>(&gtab[ng + s], ltab[ng + s]);
    glob_slot_agg<HF_AGG_SUM>(&gtab[2 * ng + s], ltab[2 * ng + s]);
    glob_slot_agg<HF_AGG_SUM>(&gtab[3 * ng + s], ltab[3 * ng + s]);
    glob_slot_agg<HF_AGG_MIN>(&gtab[4 * ng + s], ltab[4 * ng + s]);
    glob_slot_agg<HF_AGG_MAX>(&gtab[5 * ng + s], ltab[5 * ng + s]);
  }
}

// Global path: the same arithmetic with agent-scope atomics straight into
// the table; centre is read through the cache.
__global__ void __launch_bounds__(BLOCK) k_gm_global(
    const int64_t* __restrict__ gid, const double* __restrict__ val, int64_t n,
    const double* __restrict__ centre, int64_t ng, double* __restrict__ gtab,
    unsigned long long* __restrict__ err) {
  auto row = [&](int64_t g, double x) {
    if (g < 0) return;
    if (g >= ng) { atomicAdd(err, 1ULL); return; }
    if (x != x) return;
    gm_update<false>(gtab, ng, g, x, centre[g]);
  };
  const int64_t npair = n >> 1;
  const longlong2* gid2 = reinterpret_cast<const longlong2*>(gid);
  const double2* val2 = reinterpret_cast<const double2*>(val);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    const longlong2 gg = gid2[i];
    const double2 v = val2[i];
    row(gg.x, v.x);
    row(gg.y, v.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) row(gid[n - 1], val[n - 1]);
}

// Null-gid form (every row is group 0: frame skew/kurt): register partials,
// wave shuffle + block combine, six atomics per block.
__global__ void __launch_bounds__(BLOCK) k_gm_one(
    const double* __restrict__ val, int64_t n,
    const double* __restrict__ centre, double* __restrict__ gtab) {
  const double c = centre[0];
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  double mn = agg_identity<HF_AGG_MIN>(), mx = agg_identity<HF_AGG_MAX>();
  auto row = [&](double x) {
    if (x != x) return;
    const double d = x - c, d2 = d * d;
    s1 += d; s2 += d2; s3 += d2 * d; s4 += d2 * d2;
    mn = fmin(mn, x); mx = fmax(mx, x);
  };
  const int64_t npair = n >> 1;
  const double2* val2 = reinterpret_cast<const double2*>(val);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < npair; i += stride) {
    const double2 v = val2[i];
    row(v.x);
    row(v.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) row(val[n - 1]);
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
    s3 += __shfl_down(s3, off);
    s4 += __shfl_down(s4, off);
    mn = fmin(mn, __shfl_down(mn, off));
    mx = fmax(mx, __shfl_down(mx, off));
  }
  __shared__ double part[BLOCK / 64][GM_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[wave][0] = s1; part[wave][1] = s2; part[wave][2] = s3;
    part[wave][3] = s4; part[wave][4] = mn; part[wave][5] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
      s1 += part[w][0]; s2 += part[w][1]; s3 += part[w][2]; s4 += part[w][3];
      mn = fmin(mn, part[w][4]); mx = fmax(mx, part[w][5]);
    }
    if (mn <= mx) {  // the block saw at least one non-NaN row
      glob_slot_agg<HF_AGG_SUM>(&gtab[0], s1);
      glob_slot_agg<HF_AGG_SUM>(&gtab[1], s2);
      glob_slot_agg<HF_AGG_SUM>(&gtab[2], s3);
      glob_slot_agg<HF_AGG_SUM>(&gtab[3], s4);
      glob_slot_agg<HF_AGG_MIN>(&gtab[4], mn);
      glob_slot_agg<HF_AGG_MAX>(&gtab[5], mx);
    }
  }
}

// ---- hash-table groupby accumulate (unbounded key ranges) ----

__device__ __forceinline__ uint64_t hash_mix64(uint64_t x) {
  // splitmix64 finalizer
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

constexpr long long HASH_EMPTY = 0x8000000000000000LL;  // INT64_MIN sentinel

template <int NVALS, bool COUNTS, int AOP>
__global__ void __launch_bounds__(BLOCK) k_gb_hash_accum(
    const int64_t* __restrict__ keys, GbPtrs ptrs, int64_t n, int64_t H,
    long long* __restrict__ tkey, double* __restrict__ sums,
    unsigned long long* __restrict__ rowcnt,
    unsigned long long* __restrict__ counts,
    unsigned long long* __restrict__ err_full) {
  const int64_t stride_len = H + 1;  // +1: the INT64_MIN special slot
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const long long k = keys[i];
    int64_t slot;
    if (k == HASH_EMPTY) {
      slot = H;
    } else {
      uint64_t h = hash_mix64((uint64_t)k) & (uint64_t)(H - 1);
      slot = -1;
      // bounded sweep: a chain this long means the table is effectively
      // full — fail fast so the host can grow and retry
      const int64_t maxprobe = H < 4096 ? H : 4096;
      for (int64_t probes = 0; probes < maxprobe; ++probes) {
        const long long cur = (long long)atomicCAS(
            (unsigned long long*)&tkey[h], (unsigned long long)HASH_EMPTY,
            (unsigned long long)k);
        if (cur == HASH_EMPTY || cur == k) {
          slot = (int64_t)h;
          break;
        }
        h = (h + 1) & (uint64_t)(H - 1);
      }
      if (slot < 0) {
        atomicAdd(err_full, 1ULL);
        continue;
      }
    }
    atomicAdd(&rowcnt[slot], 1ULL);
#pragma unroll
    for (int c = 0; c < NVALS; ++c) {
      const double v = ptrs.vals[c][i];
      if (v == v) {
        glob_slot_agg<AOP>(&sums[(int64_t)c * stride_len + slot], v);
        if (COUNTS) atomicAdd(&counts[(int64_t)c * stride_len + slot], 1ULL);
      }
    }
  }
}

// Deterministic counter-based RNG fills (bench/test data generation on
// device — bench.py's synthetic frames are born in HBM so the bench is GPU
// work, not host numpy; oracle.rand_* mirrors these formulas bit-exactly
// for the verify gate).  splitmix64 finalizer over (seed + index).
__device__ __forceinline__ uint64_t rng_mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ void __launch_bounds__(BLOCK) k_fill_randint(
    int64_t* __restrict__ p, int64_t n, uint64_t seed, int64_t lo,
    uint64_t span) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    p[i] = lo + (int64_t)(rng_mix64(seed + (uint64_t)i) % span);
}

__global__ void __launch_bounds__(BLOCK) k_fill_randf64(
    double* __restrict__ p, int64_t n, uint64_t seed) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    p[i] = (double)(rng_mix64(seed + (uint64_t)i) >> 11) *
           (1.0 / 9007199254740992.0);
}

// inverse-CDF draw (zipf and friends): u uniform in [0,1), output =
// np.searchsorted(cdf, u, side='right') on a sorted f64 cdf column
__global__ void __launch_bounds__(BLOCK) k_fill_randcdf(
    int64_t* __restrict__ p, int64_t n, uint64_t seed,
    const double* __restrict__ cdf, int64_t m) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const double u = (double)(rng_mix64(seed + (uint64_t)i) >> 11) *
                     (1.0 / 9007199254740992.0);
    int64_t a = 0, b = m;          // first idx with cdf[idx] > u
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (cdf[mid] <= u) a = mid + 1; else b = mid;
    }
    p[i] = a;
  }
}

__global__ void __launch_bounds__(BLOCK) k_i64_to_u32(
    const int64_t* __restrict__ in, unsigned* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (unsigned)in[i];
}

__global__ void __launch_bounds__(BLOCK) k_fill_i64(int64_t* __restrict__ p,
                                                    int64_t v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// ---- compaction: present slots (rowcnt>0) -> ascending keys + columns ----
// Fixed tile partitioning so prefix order == slot order.
constexpr int COMPACT_TILE = 4096;  // slots per tile, one 256-thread block/tile

__global__ void __launch_bounds__(BLOCK) k_compact_count(
    const unsigned long long* __restrict__ rowcnt, int64_t n_slots,
    int64_t* __restrict__ tile_counts) {
  const int64_t t0 = (int64_t)blockIdx.x * COMPACT_TILE;
  const int64_t t1 = min(t0 + (int64_t)COMPACT_TILE, n_slots);
  int local = 0;
  for (int64_t s = t0 + threadIdx.x; s < t1; s += blockDim.x)
    local += (rowcnt[s] != 0);
  // block reduce
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
  __shared__ int s_c[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_c[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < BLOCK / 64; ++w) tot += s_c[w];
    tile_counts[blockIdx.x] = tot;
  }
}

// single-workgroup exclusive scan of tile_counts (ntiles <= 1M/4096*32 ~ small)
__global__ void __launch_bounds__(1024) k_compact_scan(
    int64_t* __restrict__ tile_counts, int64_t ntiles, int64_t* __restrict__ total) {
  __shared__ int64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  __shared__ int64_t buf[1024];
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    int64_t v = (i < ntiles) ? tile_counts[i] : 0;
    // Hillis–Steele inclusive scan in LDS
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      int64_t add = (threadIdx.x >= off) ? buf[threadIdx.x - off] : 0;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    const int64_t incl = buf[threadIdx.x];
    if (i < ntiles) tile_counts[i] = carry + incl - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

template <bool COUNTS>
__global__ void __launch_bounds__(BLOCK) k_compact_scatter(
    const double* __restrict__ sums, const unsigned long long* __restrict__ rowcnt,
    const unsigned long long* __restrict__ counts, int nvals,
    int64_t key_min, int64_t n_slots,
    const int64_t* __restrict__ tile_offsets,
    int64_t* __restrict__ out_keys, double* const* __restrict__ out_sums,
    int64_t* const* __restrict__ out_counts) {
  const int64_t t0 = (int64_t)blockIdx.x * COMPACT_TILE;
  const int64_t t1 = min(t0 + (int64_t)COMPACT_TILE, n_slots);
  __shared__ int64_t s_base;
  __shared__ int s_wave_cnt[BLOCK / 64];
  if (threadIdx.x == 0) s_base = tile_offsets[blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t s = chunk + threadIdx.x;
    const bool pred = (s < t1) && (rowcnt[s] != 0);
    const uint64_t ballot = __ballot(pred);
    if (lane == 0) s_wave_cnt[wave] = __popcll(ballot);
    __syncthreads();
    int64_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += s_wave_cnt[w];
    if (pred) {
      const int64_t pos = s_base + wave_base +
          __popcll(ballot & ((lane == 63) ? ~0ULL >> 1 : ((1ULL << lane) - 1)));
      out_keys[pos] = key_min + s;
      for (int c = 0; c < nvals; ++c) {
        out_sums[c][pos] = sums[(int64_t)c * n_slots + s];
        if (COUNTS) out_counts[c][pos] = (int64_t)counts[(int64_t)c * n_slots + s];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += s_wave_cnt[w];
      s_base += tot;
    }
    __syncthreads();
  }
}

// The group map of a compaction (GbKeyCache::d_gidx): slot -> output row with
// the ranking of k_compact_scatter, 0xFFFFFFFF for absent slots.
__global__ void __launch_bounds__(BLOCK) k_gb_gidx(
    const unsigned long long* __restrict__ rowcnt, int64_t n_slots,
    const int64_t* __restrict__ tile_offsets, unsigned* __restrict__ gidx) {
  const int64_t t0 = (int64_t)blockIdx.x * COMPACT_TILE;
  const int64_t t1 = min(t0 + (int64_t)COMPACT_TILE, n_slots);
  __shared__ int64_t s_base;
  __shared__ int s_wave_cnt[BLOCK / 64];
  if (threadIdx.x == 0) s_base = tile_offsets[blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t s = chunk + threadIdx.x;
    const bool pred = (s < t1) && (rowcnt[s] != 0);
    const uint64_t ballot = __ballot(pred);
    if (lane == 0) s_wave_cnt[wave] = __popcll(ballot);
    __syncthreads();
    int64_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += s_wave_cnt[w];
    if (s < t1)
      gidx[s] = pred ? (unsigned)(s_base + wave_base +
                                  __popcll(ballot & ((1ULL << lane) - 1)))
                     : 0xFFFFFFFFu;
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += s_wave_cnt[w];
      s_base += tot;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Join kernels — broadcast-right dense-range CSR inner join
// (device form of MergeImpl.row_axis_merge, merge.py:104-178; see
// include/hipframe.h).  Build: count -> scan -> fill -> order fixup.
// Probe: two passes so the output preserves pandas' match order exactly
// (left row order, right row order within key): pass A stores per-left-row
// (offset, count) and per-tile totals; a scan of tile totals gives exact
// output positions; pass B emits.
// ---------------------------------------------------------------------------

constexpr int JOIN_TILE = 4096;           // left rows per probe tile
constexpr int JOIN_MAX_DUP = 4096;        // right rows per key cap (fixup sort)

__global__ void __launch_bounds__(BLOCK) k_hist_u32(
    const int64_t* __restrict__ keys, int64_t n, int64_t key_min,
    int64_t n_slots, unsigned* __restrict__ cnt,
    unsigned long long* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i] - key_min;
    if ((uint64_t)k < (uint64_t)n_slots)
      atomicAdd(&cnt[k], 1u);
    else
      atomicAdd(err, 1ULL);
  }
}

// tile sums of a u32 array (for the big exclusive scan building the CSR)
__global__ void __launch_bounds__(BLOCK) k_tile_sums_u32(
    const unsigned* __restrict__ v, int64_t n, int64_t* __restrict__ sums) {
  const int64_t t0 = (int64_t)blockIdx.x * JOIN_TILE;
  const int64_t t1 = min(t0 + (int64_t)JOIN_TILE, n);
  long long local = 0;
  for (int64_t s = t0 + threadIdx.x; s < t1; s += blockDim.x) local += v[s];
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
  __shared__ long long sc[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sc[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tot = 0;
    for (int w = 0; w < BLOCK / 64; ++w) tot += sc[w];
    sums[blockIdx.x] = tot;
  }
}

// apply tile bases: csr[s] = tile_base + local exclusive prefix; also writes
// csr[n] = grand total (u64 offsets)
__global__ void __launch_bounds__(BLOCK) k_scan_apply_u32(
    const unsigned* __restrict__ v, int64_t n,
    const int64_t* __restrict__ tile_bases, const int64_t* __restrict__ total,
    unsigned long long* __restrict__ csr) {
  __shared__ unsigned long long s_run;
  const int64_t t0 = (int64_t)blockIdx.x * JOIN_TILE;
  const int64_t t1 = min(t0 + (int64_t)JOIN_TILE, n);
  if (threadIdx.x == 0) s_run = (unsigned long long)tile_bases[blockIdx.x];
  __shared__ int s_wave_sum[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t s = chunk + threadIdx.x;
    const unsigned x = (s < t1) ? v[s] : 0;
    // wave-inclusive scan
    unsigned incl = x;
    for (int d = 1; d < 64; d <<= 1) {
      unsigned up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave_sum[wave] = (int)incl;
    __syncthreads();
    unsigned wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += (unsigned)s_wave_sum[w];
    if (s < t1) csr[s] = s_run + wave_base + incl - x;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += (unsigned)s_wave_sum[w];
      s_run += tot;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) csr[n] = (unsigned long long)*total;
}

struct JoinPtrs {
  double* vals[GB_MAX_VALS];
};
struct JoinConstPtrs {
  const double* vals[GB_MAX_VALS];
};

template <int NR>
__global__ void __launch_bounds__(BLOCK) k_join_fill(
    const int64_t* __restrict__ keys, JoinConstPtrs rv, int64_t n,
    int64_t key_min, int64_t n_slots, const unsigned long long* __restrict__ csr,
    unsigned* __restrict__ cursor, unsigned* __restrict__ jidx, JoinPtrs jv) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i] - key_min;
    if ((uint64_t)k >= (uint64_t)n_slots) continue;  // counted in hist err
    const unsigned r = atomicAdd(&cursor[k], 1u);
    const int64_t pos = (int64_t)csr[k] + r;
    jidx[pos] = (unsigned)i;
#pragma unroll
    for (int c = 0; c < NR; ++c) jv.vals[c][pos] = rv.vals[c][i];
  }
}

// restore right-row order within each key (pandas match order): tiny
// insertion sort per multi-occupancy slot, one thread per slot
template <int NR>
__global__ void __launch_bounds__(BLOCK) k_join_fixup(
    const unsigned long long* __restrict__ csr, int64_t n_slots,
    unsigned* __restrict__ jidx, JoinPtrs jv,
    unsigned long long* __restrict__ err) {
  int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; s < n_slots; s += stride) {
    const int64_t lo = (int64_t)csr[s], hi = (int64_t)csr[s + 1];
    const int64_t cnt = hi - lo;
    if (cnt <= 1) continue;
    if (cnt > JOIN_MAX_DUP) {
      atomicAdd(err, 1ULL);
      continue;
    }
    for (int64_t a = lo + 1; a < hi; ++a) {
      const unsigned ki = jidx[a];
      double kv[NR > 0 ? NR : 1];
#pragma unroll
      for (int c = 0; c < NR; ++c) kv[c] = jv.vals[c][a];
      int64_t b = a - 1;
      while (b >= lo && jidx[b] > ki) {
        jidx[b + 1] = jidx[b];
#pragma unroll
        for (int c = 0; c < NR; ++c) jv.vals[c][b + 1] = jv.vals[c][b];
        --b;
      }
      jidx[b + 1] = ki;
#pragma unroll
      for (int c = 0; c < NR; ++c) jv.vals[c][b + 1] = kv[c];
    }
  }
}

// probe pass A: per-left-row offset+count, per-tile match totals
__global__ void __launch_bounds__(BLOCK) k_probe_count(
    const int64_t* __restrict__ lkeys, int64_t n, int64_t key_min,
    int64_t n_slots, const unsigned long long* __restrict__ csr,
    unsigned long long* __restrict__ offs, unsigned* __restrict__ cnts,
    int64_t* __restrict__ tile_sums) {
  const int64_t t0 = (int64_t)blockIdx.x * JOIN_TILE;
  const int64_t t1 = min(t0 + (int64_t)JOIN_TILE, n);
  long long local = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += blockDim.x) {
    const int64_t k = lkeys[i] - key_min;
    unsigned c = 0;
    unsigned long long o = 0;
    if ((uint64_t)k < (uint64_t)n_slots) {
      o = csr[k];
      c = (unsigned)(csr[k + 1] - o);
    }
    offs[i] = o;
    cnts[i] = c;
    local += c;
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
  __shared__ long long sc[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sc[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tot = 0;
    for (int w = 0; w < BLOCK / 64; ++w) tot += sc[w];
    tile_sums[blockIdx.x] = tot;
  }
}

// probe pass B: emit matches at exact positions
template <int NR>
__global__ void __launch_bounds__(BLOCK) k_probe_emit(
    const int64_t* __restrict__ lkeys, int64_t n, int64_t lbase,
    const unsigned long long* __restrict__ offs,
    const unsigned* __restrict__ cnts, const int64_t* __restrict__ tile_bases,
    const unsigned* __restrict__ jidx_unused, JoinConstPtrs jv,
    int64_t* __restrict__ out_keys, int64_t* __restrict__ out_lidx,
    JoinPtrs out_r) {
  __shared__ unsigned long long s_run;
  __shared__ int s_wave_sum[BLOCK / 64];
  const int64_t t0 = (int64_t)blockIdx.x * JOIN_TILE;
  const int64_t t1 = min(t0 + (int64_t)JOIN_TILE, n);
  if (threadIdx.x == 0) s_run = (unsigned long long)tile_bases[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t i = chunk + threadIdx.x;
    const unsigned c = (i < t1) ? cnts[i] : 0;
    unsigned incl = c;
    for (int d = 1; d < 64; d <<= 1) {
      unsigned up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave_sum[wave] = (int)incl;
    __syncthreads();
    unsigned wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += (unsigned)s_wave_sum[w];
    if (i < t1 && c) {
      int64_t dst = (int64_t)(s_run + wave_base + incl - c);
      const int64_t k = lkeys[i];
      const unsigned long long o = offs[i];
      for (unsigned j = 0; j < c; ++j) {
        out_keys[dst + j] = k;
        out_lidx[dst + j] = lbase + i;
#pragma unroll
        for (int cc = 0; cc < NR; ++cc)
          out_r.vals[cc][dst + j] = jv.vals[cc][o + j];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += (unsigned)s_wave_sum[w];
      s_run += tot;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Sort kernels — stable LSD radix over (u32 key, u32 idx) pairs.
// A "tile" is 64 lanes x SORT_RPT rows owned by ONE wave: lanes are in
// order and the per-step leader loop ranks same-digit lanes by lane id, so
// every pass is stable without cross-wave coordination.
// ---------------------------------------------------------------------------

constexpr int SORT_RPT = 32;                 // rows per lane per tile
constexpr int SORT_TILE = 64 * SORT_RPT;     // 2048 rows per wave-tile
constexpr int SORT_WPB = 4;                  // waves per block

__global__ void __launch_bounds__(BLOCK) k_sort_pack(
    const int64_t* __restrict__ keys, int64_t n, int64_t key_min,
    int64_t key_span, int ascending, unsigned long long* __restrict__ pairs) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const unsigned k = (unsigned)(keys[i] - key_min);
    const unsigned kk = ascending ? k : (unsigned)key_span - k;
    pairs[i] = ((unsigned long long)(unsigned)i << 32) | kk;
  }
}

// per-wave-tile digit histogram -> C[tile][256] (row-major, coalesced)
__global__ void __launch_bounds__(BLOCK) k_sort_count(
    const unsigned long long* __restrict__ pairs, int64_t n, int shift,
    unsigned* __restrict__ C, int64_t ntiles) {
  __shared__ unsigned hist[SORT_WPB][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t wtiles_per_block = SORT_WPB;
  for (int64_t tile = (int64_t)blockIdx.x * wtiles_per_block + wave;
       tile < ntiles; tile += (int64_t)gridDim.x * wtiles_per_block) {
    for (int d = lane; d < 256; d += 64) hist[wave][d] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t t0 = tile * SORT_TILE;
#pragma unroll 4
    for (int j = 0; j < SORT_RPT; ++j) {
      const int64_t row = t0 + (int64_t)j * 64 + lane;
      if (row < n) {
        const unsigned d = ((unsigned)pairs[row] >> shift) & 255u;
        atomicAdd(&hist[wave][d], 1u);  // LDS, same-wave only
      }
    }
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < 256; d += 64) C[tile * 256 + d] = hist[wave][d];
  }
}

// 32x32 tiled transpose: C[ntiles][256] -> CT[256][ntiles]
__global__ void __launch_bounds__(1024) k_transpose256(
    const unsigned* __restrict__ C, unsigned* __restrict__ CT,
    int64_t ntiles) {
  __shared__ unsigned t[32][33];
  const int64_t tx0 = (int64_t)blockIdx.x * 32;       // tile-index block
  const int dy = (int)(blockIdx.y * 32);              // digit block (0..224)
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;  // 32x32 threads
  const int64_t src_row = tx0 + ly;
  if (src_row < ntiles) t[ly][lx] = C[src_row * 256 + dy + lx];
  __syncthreads();
  const int64_t dst_col = tx0 + lx;
  if (dst_col < ntiles) CT[(int64_t)(dy + ly) * ntiles + dst_col] = t[lx][ly];
}

// stable scatter: each wave re-walks its tile in order; same-digit lanes
// are matched with 8 BIT BALLOTS (round 2 — the old per-distinct-digit
// leader loop ran ~50 serial iterations per 64-row step; bit-ballot cut
// one pass 29.4 -> 17.5 ms at 1e9 rows, profiles/r02/sort_ballot.log):
// lanes sharing this lane's digit = AND over digit bits of
// (bit ? ballot : ~ballot); rank = popcount(same & below); the lowest
// member advances the digit base.
__global__ void __launch_bounds__(BLOCK) k_sort_scatter(
    const unsigned long long* __restrict__ pairs, int64_t n, int shift,
    const unsigned long long* __restrict__ offs,   // [256][ntiles] exclusive
    int64_t ntiles, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long base[SORT_WPB][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1ULL;
  for (int64_t tile = (int64_t)blockIdx.x * SORT_WPB + wave; tile < ntiles;
       tile += (int64_t)gridDim.x * SORT_WPB) {
    for (int d = lane; d < 256; d += 64)
      base[wave][d] = offs[(int64_t)d * ntiles + tile];
    __builtin_amdgcn_wave_barrier();
    const int64_t t0 = tile * SORT_TILE;
    for (int j = 0; j < SORT_RPT; ++j) {
      const int64_t row = t0 + (int64_t)j * 64 + lane;
      const bool valid = row < n;
      const unsigned long long p = valid ? pairs[row] : 0;
      const unsigned d = ((unsigned)p >> shift) & 255u;
      unsigned long long same = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        same &= ((d >> b) & 1u) ? m : ~m;
      }
      if (valid) {
        const unsigned rank = (unsigned)__popcll(same & below);
        const unsigned long long pos = base[wave][d] + rank;
        if (lane == __ffsll((long long)same) - 1)
          base[wave][d] += __popcll(same);
        out[pos] = p;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- wide variant: u64 shifted keys + u32 origins as two arrays (for key
// spans beyond 2^27; up to 8 digit passes) ----

__global__ void __launch_bounds__(BLOCK) k_sort_pack_wide(
    const int64_t* __restrict__ keys, int64_t n, int64_t key_min,
    uint64_t key_span, int ascending, unsigned long long* __restrict__ karr,
    unsigned* __restrict__ iarr) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const uint64_t k = (uint64_t)(keys[i] - key_min);
    karr[i] = ascending ? k : key_span - k;
    iarr[i] = (unsigned)i;
  }
}

__global__ void __launch_bounds__(BLOCK) k_sort_count_wide(
    const unsigned long long* __restrict__ karr, int64_t n, int shift,
    unsigned* __restrict__ C, int64_t ntiles) {
  __shared__ unsigned hist[SORT_WPB][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t tile = (int64_t)blockIdx.x * SORT_WPB + wave; tile < ntiles;
       tile += (int64_t)gridDim.x * SORT_WPB) {
    for (int d = lane; d < 256; d += 64) hist[wave][d] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t t0 = tile * SORT_TILE;
#pragma unroll 4
    for (int j = 0; j < SORT_RPT; ++j) {
      const int64_t row = t0 + (int64_t)j * 64 + lane;
      if (row < n) {
        const unsigned d = (unsigned)(karr[row] >> shift) & 255u;
        atomicAdd(&hist[wave][d], 1u);
      }
    }
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < 256; d += 64) C[tile * 256 + d] = hist[wave][d];
  }
}

__global__ void __launch_bounds__(BLOCK) k_sort_scatter_wide(
    const unsigned long long* __restrict__ karr,
    const unsigned* __restrict__ iarr, int64_t n, int shift,
    const unsigned long long* __restrict__ offs, int64_t ntiles,
    unsigned long long* __restrict__ karr_out, unsigned* __restrict__ iarr_out) {
  __shared__ unsigned long long base[SORT_WPB][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t tile = (int64_t)blockIdx.x * SORT_WPB + wave; tile < ntiles;
       tile += (int64_t)gridDim.x * SORT_WPB) {
    for (int d = lane; d < 256; d += 64)
      base[wave][d] = offs[(int64_t)d * ntiles + tile];
    __builtin_amdgcn_wave_barrier();
    const int64_t t0 = tile * SORT_TILE;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    for (int j = 0; j < SORT_RPT; ++j) {
      const int64_t row = t0 + (int64_t)j * 64 + lane;
      const bool valid = row < n;
      const unsigned long long k = valid ? karr[row] : 0;
      const unsigned idx = valid ? iarr[row] : 0;
      const unsigned d = (unsigned)(k >> shift) & 255u;
      // bit-ballot same-digit matching (see k_sort_scatter)
      unsigned long long same = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        same &= ((d >> b) & 1u) ? m : ~m;
      }
      if (valid) {
        const unsigned rank = (unsigned)__popcll(same & below);
        const unsigned long long pos = base[wave][d] + rank;
        if (lane == __ffsll((long long)same) - 1)
          base[wave][d] += __popcll(same);
        karr_out[pos] = k;
        iarr_out[pos] = idx;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_sort_unpack_wide(
    const unsigned* __restrict__ iarr, int64_t n, int64_t* __restrict__ perm) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) perm[i] = (int64_t)iarr[i];
}

__global__ void __launch_bounds__(BLOCK) k_sort_unpack(
    const unsigned long long* __restrict__ pairs, int64_t n,
    int64_t* __restrict__ perm) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) perm[i] = (int64_t)(pairs[i] >> 32);
}

__global__ void __launch_bounds__(BLOCK) k_fill_f64(double* __restrict__ p,
                                                    double v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

__global__ void __launch_bounds__(BLOCK) k_fixup_empty(
    const double* __restrict__ val, const int64_t* __restrict__ cnt,
    double* __restrict__ out, int64_t n) {
  const double nanv = __longlong_as_double(0x7FF8000000000000LL);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = cnt[i] ? val[i] : nanv;
}

// ---- compare + filter kernels ----

// S is the scalar's type: double (an int64 row is promoted to double, as
// pandas does against a float operand) or long long (exact int64 compare)
template <int OP, typename T, typename S>
__device__ __forceinline__ long long cmp1(T x, S s) {
  switch (OP) {
    case HF_CMP_GT: return x > s;
    case HF_CMP_GE: return x >= s;
    case HF_CMP_LT: return x < s;
    case HF_CMP_LE: return x <= s;
    case HF_CMP_EQ: return x == s;
    case HF_CMP_NE: return !(x == s);  // NaN != s -> true (pandas)
    case HF_CMP_NOTNA: return x == x;  // int64: always 1
  }
  return 0;
}

template <int OP, typename T, typename S>
__global__ void __launch_bounds__(BLOCK) k_compare(const T* __restrict__ in,
                                                   long long* __restrict__ out,
                                                   S s, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = cmp1<OP, T, S>(in[i], s);
}

constexpr int FILT_TILE = 4096;

__global__ void __launch_bounds__(BLOCK) k_filter_count(
    const long long* __restrict__ mask, int64_t n, int64_t* __restrict__ sums) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  long long local = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += blockDim.x)
    local += (mask[i] != 0);
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
  __shared__ long long sc[BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sc[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tot = 0;
    for (int w = 0; w < BLOCK / 64; ++w) tot += sc[w];
    sums[blockIdx.x] = tot;
  }
}

// order-preserving compaction: ballot-ranked within tile (the same pattern
// as k_compact_scatter).  IOTA: emit base + row index instead of data.
template <typename T, bool IOTA>
__global__ void __launch_bounds__(BLOCK) k_filter_scatter(
    const long long* __restrict__ mask, const T* __restrict__ in, int64_t n,
    const int64_t* __restrict__ tile_bases, int64_t iota_base,
    T* __restrict__ out) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  __shared__ int64_t s_base;
  __shared__ int s_wave_cnt[BLOCK / 64];
  if (threadIdx.x == 0) s_base = tile_bases[blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t i = chunk + threadIdx.x;
    const bool pred = (i < t1) && (mask[i] != 0);
    const uint64_t ballot = __ballot(pred);
    if (lane == 0) s_wave_cnt[wave] = __popcll(ballot);
    __syncthreads();
    int64_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += s_wave_cnt[w];
    if (pred) {
      const int64_t pos = s_base + wave_base +
          __popcll(ballot & ((lane == 63) ? ~0ULL >> 1 : ((1ULL << lane) - 1)));
      out[pos] = IOTA ? (T)(iota_base + i) : in[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += s_wave_cnt[w];
      s_base += tot;
    }
    __syncthreads();
  }
}

// ---- sort-based groupby kernels ----

__global__ void __launch_bounds__(BLOCK) k_head_flags(
    const int64_t* __restrict__ k, int64_t n, long long* __restrict__ head) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    head[i] = (i == 0) || (k[i] != k[i - 1]);
}

// per-row run id = (heads at positions <= i) - 1, via the filter plan's
// tile bases; one device atomic per row into the per-run aggregate
template <int AOP, bool CNT, bool ROWCNT, bool HAVE_VAL>
__global__ void __launch_bounds__(BLOCK) k_segagg(
    const long long* __restrict__ head, const double* __restrict__ vals,
    int64_t n, const int64_t* __restrict__ tile_bases,
    double* __restrict__ gsums, unsigned long long* __restrict__ growcnt,
    unsigned long long* __restrict__ gcounts) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  __shared__ int64_t s_base;
  __shared__ int s_wave_cnt[BLOCK / 64];
  if (threadIdx.x == 0) s_base = tile_bases[blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t chunk = t0; chunk < t1; chunk += blockDim.x) {
    const int64_t i = chunk + threadIdx.x;
    const bool pred = (i < t1) && (head[i] != 0);
    const uint64_t ballot = __ballot(pred);
    if (lane == 0) s_wave_cnt[wave] = __popcll(ballot);
    __syncthreads();
    int64_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += s_wave_cnt[w];
    if (i < t1) {
      // inclusive count of heads <= i within the tile, minus 1 for run id
      const int64_t run =
          s_base + wave_base +
          __popcll(ballot & ((lane == 63) ? ~0ULL : ((2ULL << lane) - 1))) - 1;
      if (ROWCNT) atomicAdd(&growcnt[run], 1ULL);
      if (HAVE_VAL) {
        const double v = vals[i];
        if (v == v) {
          glob_slot_agg<AOP>(&gsums[run], v);
          if (CNT) atomicAdd(&gcounts[run], 1ULL);
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t tot = 0;
      for (int w = 0; w < BLOCK / 64; ++w) tot += s_wave_cnt[w];
      s_base += tot;
    }
    __syncthreads();
  }
}

template <typename T, int OP>
__device__ __forceinline__ T cs_ident() {
  if (OP == HF_AGG_MIN)
    return (sizeof(T) == 8 && (T)0.5 == 0) ? (T)INT64_MAX
                                           : (T)__builtin_huge_val();
  if (OP == HF_AGG_MAX)
    return (sizeof(T) == 8 && (T)0.5 == 0) ? (T)INT64_MIN
                                           : (T)-__builtin_huge_val();
  if (OP == HF_AGG_PROD) return T(1);
  return T(0);
}
template <typename T, int OP>
__device__ __forceinline__ T cs_comb(T a, T b) {
  if (OP == HF_AGG_MIN) return a < b ? a : b;
  if (OP == HF_AGG_MAX) return a > b ? a : b;
  if (OP == HF_AGG_PROD) return a * b;
  return a + b;
}
template <typename T, int OP>
__device__ __forceinline__ T cs_load(const T* p_, int64_t i) {
  const T v = p_[i];
  return (v != v) ? cs_ident<T, OP>() : v;  // NaN skipped (f64)
}

// Scan STATE.  Every op carries a plain T except the f64 product, which
// carries the running product as an unevaluated sum hi + lo (double-double).
// A rounded product hands the relative errors of both operands on in full,
// so a plain f64 prefix of k factors holds all k-1 roundings of its tree
// (measured 1.9e-11 at 4.2M rows of factors near 1, where every thread run
// restarts at exactly 1 and the roundings do not average out); with the
// error term kept, each combine costs ~u^2 and the output rounds once.
struct cs_dd { double hi, lo; };
template <typename T, int OP> struct cs_state { using type = T; };
template <> struct cs_state<double, HF_AGG_PROD> { using type = cs_dd; };

__device__ __forceinline__ cs_dd cs_dd_mul(cs_dd a, cs_dd b) {
  // no contraction here: fusing p's multiply into `p + lo` below would add
  // the error term e a second time
#pragma clang fp contract(off)
  const double p = a.hi * b.hi;
  // after overflow, at zero and on NaN there is no error term to keep: the
  // state stays the plain product's inf / 0 / NaN
  if (!(fabs(p) < __builtin_huge_val()) || p == 0.0) return cs_dd{p, 0.0};
  const double e = __builtin_fma(a.hi, b.hi, -p);  // exact: a.hi*b.hi - p
  const double lo = e + (a.hi * b.lo + a.lo * b.hi);
  const double hi = p + lo;
  return cs_dd{hi, lo - (hi - p)};
}
template <typename T, int OP, typename S = typename cs_state<T, OP>::type>
__device__ __forceinline__ S cs_lift(T v) {
  if constexpr (std::is_same<S, cs_dd>::value) return cs_dd{v, 0.0};
  else return v;
}
template <typename T, int OP, typename S = typename cs_state<T, OP>::type>
__device__ __forceinline__ S cs_sident() {
  return cs_lift<T, OP>(cs_ident<T, OP>());
}
template <typename T, int OP, typename S = typename cs_state<T, OP>::type>
__device__ __forceinline__ S cs_scomb(S a, S b) {
  if constexpr (std::is_same<S, cs_dd>::value) return cs_dd_mul(a, b);
  else return cs_comb<T, OP>(a, b);
}
template <typename T, int OP, typename S = typename cs_state<T, OP>::type>
__device__ __forceinline__ T cs_value(S s) {
  if constexpr (std::is_same<S, cs_dd>::value) return s.hi + s.lo;
  else return s;
}
template <typename S>
__device__ __forceinline__ S cs_shfl_down(S v, int off) {
  if constexpr (std::is_same<S, cs_dd>::value)
    return cs_dd{__shfl_down(v.hi, off), __shfl_down(v.lo, off)};
  else return (S)__shfl_down(v, off);
}

template <typename T, int OP>
__global__ void __launch_bounds__(BLOCK) k_cumsum_tiles(
    const T* __restrict__ in, int64_t n,
    typename cs_state<T, OP>::type* __restrict__ tile_sums) {
  using S = typename cs_state<T, OP>::type;
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  S local = cs_sident<T, OP>();
  for (int64_t i = t0 + threadIdx.x; i < t1; i += blockDim.x)
    local = cs_scomb<T, OP>(local, cs_lift<T, OP>(cs_load<T, OP>(in, i)));
  __shared__ S sc[BLOCK / 64];
  for (int off = 32; off > 0; off >>= 1)
    local = cs_scomb<T, OP>(local, cs_shfl_down(local, off));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sc[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    S tot = cs_sident<T, OP>();
    for (int w = 0; w < BLOCK / 64; ++w) tot = cs_scomb<T, OP>(tot, sc[w]);
    tile_sums[blockIdx.x] = tot;
  }
}

template <typename T, int OP>
__global__ void __launch_bounds__(1024) k_cumsum_scan_tiles(
    typename cs_state<T, OP>::type* __restrict__ tile_sums, int64_t ntiles) {
  using S = typename cs_state<T, OP>::type;
  // exclusive scan under cs_comb: track each element's PREFIX (exclusive)
  // explicitly since min/max have no inverse
  __shared__ S carry;
  if (threadIdx.x == 0) carry = cs_sident<T, OP>();
  __syncthreads();
  __shared__ S buf[1024];
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    S v = (i < ntiles) ? tile_sums[i] : cs_sident<T, OP>();
    buf[threadIdx.x] = v;
    __syncthreads();
    S excl = cs_sident<T, OP>();
    for (int off = 1; off < 1024; off <<= 1) {
      S add = (threadIdx.x >= off) ? buf[threadIdx.x - off]
                                   : cs_sident<T, OP>();
      __syncthreads();
      buf[threadIdx.x] = cs_scomb<T, OP>(buf[threadIdx.x], add);
      __syncthreads();
    }
    const S incl = buf[threadIdx.x];
    __syncthreads();
    buf[threadIdx.x] = incl;  // reuse buf to read neighbor inclusives
    __syncthreads();
    // exclusive = inclusive of the previous lane (or identity at lane 0)
    excl = (threadIdx.x == 0) ? cs_sident<T, OP>() : buf[threadIdx.x - 1];
    if (i < ntiles) tile_sums[i] = cs_scomb<T, OP>(carry, excl);
    __syncthreads();
    if (threadIdx.x == 1023) carry = cs_scomb<T, OP>(carry, incl);
    __syncthreads();
  }
}

template <typename T, int OP>
__global__ void __launch_bounds__(BLOCK) k_cumsum_apply(
    const T* __restrict__ in, int64_t n,
    const typename cs_state<T, OP>::type* __restrict__ tile_base,
    T* __restrict__ out) {
  using S = typename cs_state<T, OP>::type;
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  constexpr int PER = FILT_TILE / BLOCK;  // elems per thread
  // stage the tile through LDS so HBM access stays COALESCED (striped)
  // while each thread scans PER CONSECUTIVE elements from LDS
  __shared__ T stage[FILT_TILE];
  for (int j = 0; j < PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) stage[(int)(i - t0)] = in[i];
  }
  __syncthreads();
  const int s0 = threadIdx.x * PER;
  const int lim = (int)(t1 - t0);
  S loc[PER];
  S run = cs_sident<T, OP>();
  for (int j = 0; j < PER; ++j) {
    if (s0 + j < lim) {
      const T v = stage[s0 + j];
      run = cs_scomb<T, OP>(
          run, cs_lift<T, OP>((v != v) ? cs_ident<T, OP>() : v));
    }
    loc[j] = run;  // inclusive within the thread's segment
  }
  // exclusive base across threads: scan thread totals, read neighbor
  __shared__ S buf[BLOCK];
  buf[threadIdx.x] = run;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    S add = (threadIdx.x >= off) ? buf[threadIdx.x - off]
                                 : cs_sident<T, OP>();
    __syncthreads();
    buf[threadIdx.x] = cs_scomb<T, OP>(buf[threadIdx.x], add);
    __syncthreads();
  }
  const S incl = buf[threadIdx.x];
  __syncthreads();
  buf[threadIdx.x] = incl;
  __syncthreads();
  const S texcl = (threadIdx.x == 0) ? cs_sident<T, OP>()
                                     : buf[threadIdx.x - 1];
  const S tbase = cs_scomb<T, OP>(tile_base[blockIdx.x], texcl);
  __syncthreads();
  for (int j = 0; j < PER; ++j) {
    if (s0 + j < lim) {
      const T v0 = stage[s0 + j];
      stage[s0 + j] =
          (v0 != v0) ? v0 : cs_value<T, OP>(cs_scomb<T, OP>(tbase, loc[j]));
    }
  }
  __syncthreads();
  for (int j = 0; j < PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) out[i] = stage[(int)(i - t0)];
  }
}

__global__ void __launch_bounds__(BLOCK) k_f64_ordered(
    const double* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    double x = in[i] + 0.0;  // -0.0 -> +0.0 (pandas groups them together)
    // canonicalize NaN (any sign/payload) to one ordered value: pandas
    // treats every NaN as equal — groupby keys, sort ties AND merge keys
    // (pandas matches NaN==NaN in merges)
    long long v = (x != x) ? 0x7FF8000000000000LL
                           : __double_as_longlong(x);
    // signed total order: non-negative floats keep their bits (already
    // increasing as signed i64); negative floats reverse below zero
    out[i] = (v < 0) ? (~v ^ 0x8000000000000000LL) : v;
  }
}

__global__ void __launch_bounds__(BLOCK) k_ordered_f64(
    const int64_t* __restrict__ in, double* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const long long v = in[i];
    out[i] = __longlong_as_double(
        (v < 0) ? ~(v ^ 0x8000000000000000LL) : v);
  }
}

__global__ void __launch_bounds__(BLOCK) k_search_sorted(
    const int64_t* __restrict__ keys, int64_t n,
    const int64_t* __restrict__ sorted, int64_t m,
    int64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i];
    int64_t lo = 0, hi = m;
    while (lo < hi) {  // lower_bound; first levels stay L2-resident
      const int64_t mid = (lo + hi) >> 1;
      if (sorted[mid] < k) lo = mid + 1; else hi = mid;
    }
    out[i] = (lo < m && sorted[lo] == k) ? lo : -1;
  }
}

__global__ void __launch_bounds__(BLOCK) k_shuffle_dest(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ split,
    int nsplit, long long* __restrict__ dest, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t k = keys[i];
    int d = 0;
    for (int j = 0; j < nsplit; ++j) d += (split[j] <= k);
    dest[i] = d;
  }
}

__global__ void __launch_bounds__(BLOCK) k_gather_f64(
    const double* __restrict__ src, const int64_t* __restrict__ idx,
    double* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = src[idx[i]];
}
__global__ void __launch_bounds__(BLOCK) k_gather_i64(
    const int64_t* __restrict__ src, const int64_t* __restrict__ idx,
    int64_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = src[idx[i]];
}

template <typename T>
__global__ void __launch_bounds__(BLOCK) k_gather_fill(
    const T* __restrict__ src, const int64_t* __restrict__ idx, T fill,
    T* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t j = idx[i];
    out[i] = j < 0 ? fill : src[j];
  }
}

// ---------------------------------------------------------------------------
// As-of probe (pandas merge_asof; hf_asof_idx in the header states the row
// contract).  The right side is ascending in the pair order (rby, ron); each
// left row (b, l) runs one bound search in that order and keeps the position
// next to the bound, fenced to its own group and to the tolerance.  Every
// compare is in the column's own type: int64 keys are never promoted, and
// an int64 distance is the unsigned difference of the ordered pair.
// ---------------------------------------------------------------------------
template <typename T> struct AsofDist;
template <> struct AsofDist<int64_t> {
  using type = unsigned long long;
  // hi >= lo
  static __device__ __forceinline__ type of(int64_t hi, int64_t lo) {
    return (type)hi - (type)lo;
  }
};
template <> struct AsofDist<double> {
  using type = double;
  static __device__ __forceinline__ type of(double hi, double lo) {
    return hi - lo;
  }
};

// First p in [lo, hi) whose pair is >= (b, l) (upper = false) or > (b, l)
// (upper = true); hi when there is none.
template <typename T, bool HAS_BY>
__device__ __forceinline__ int64_t asof_bound(
    const int64_t* __restrict__ rby, const T* __restrict__ ron, int64_t lo,
    int64_t hi, int64_t b, T l, bool upper) {
  while (lo < hi) {  // the first levels stay L2-resident
    const int64_t mid = (lo + hi) >> 1;
    const T r = ron[mid];
    bool below = (r < l) | (upper & (r == l));
    if (HAS_BY) {
      const int64_t gb = rby[mid];
      below = (gb < b) | ((gb == b) & below);
    }
    if (below) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename T, bool HAS_BY>
__device__ __forceinline__ bool asof_is_key(
    const int64_t* __restrict__ rby, const T* __restrict__ ron, int64_t p,
    int64_t b, T l) {
  return ron[p] == l && (!HAS_BY || rby[p] == b);
}

// One left row.  `first` is the bound the direction needs (backward: upper
// bound when exact matches count, else lower; forward the other way round).
// The opposite bound, which only nearest needs, differs from it only across
// a run of right rows equal to (b, l), so it costs a second search on exact
// hits alone.
template <typename T, bool HAS_BY, int DIR>
__device__ __forceinline__ int64_t asof_row(
    const int64_t* __restrict__ rby, const T* __restrict__ ron, int64_t m,
    int64_t b, T l, bool allow_exact, bool has_tol,
    typename AsofDist<T>::type tol) {
  using D = AsofDist<T>;
  int64_t ub_or_lb_back, lb_or_ub_fwd;  // backward: bound - 1; forward: bound
  if (DIR == HF_ASOF_BACKWARD) {
    ub_or_lb_back = asof_bound<T, HAS_BY>(rby, ron, 0, m, b, l, allow_exact);
    lb_or_ub_fwd = m;
  } else if (DIR == HF_ASOF_FORWARD) {
    lb_or_ub_fwd = asof_bound<T, HAS_BY>(rby, ron, 0, m, b, l, !allow_exact);
    ub_or_lb_back = 0;
  } else if (allow_exact) {
    // backward wants the upper bound, forward the lower
    const int64_t ub = asof_bound<T, HAS_BY>(rby, ron, 0, m, b, l, true);
    ub_or_lb_back = ub;
    lb_or_ub_fwd = ub;
    if (ub > 0 && asof_is_key<T, HAS_BY>(rby, ron, ub - 1, b, l))
      lb_or_ub_fwd = asof_bound<T, HAS_BY>(rby, ron, 0, ub - 1, b, l, false);
  } else {
    // backward wants the lower bound, forward the upper
    const int64_t lb = asof_bound<T, HAS_BY>(rby, ron, 0, m, b, l, false);
    ub_or_lb_back = lb;
    lb_or_ub_fwd = lb;
    if (lb < m && asof_is_key<T, HAS_BY>(rby, ron, lb, b, l))
      lb_or_ub_fwd = asof_bound<T, HAS_BY>(rby, ron, lb + 1, m, b, l, true);
  }
  int64_t pb = -1, pf = -1;
  typename D::type db = 0, df = 0;
  if (DIR != HF_ASOF_FORWARD) {
    const int64_t p = ub_or_lb_back - 1;
    if (p >= 0 && (!HAS_BY || rby[p] == b)) {
      db = D::of(l, ron[p]);
      if (!has_tol || !(db > tol)) pb = p;
    }
  }
  if (DIR != HF_ASOF_BACKWARD) {
    const int64_t p = lb_or_ub_fwd;
    if (p < m && (!HAS_BY || rby[p] == b)) {
      df = D::of(ron[p], l);
      if (!has_tol || !(df > tol)) pf = p;
    }
  }
  if (DIR == HF_ASOF_BACKWARD) return pb;
  if (DIR == HF_ASOF_FORWARD) return pf;
  if (pb >= 0 && pf >= 0) return db <= df ? pb : pf;  // a tie goes backward
  return pb >= 0 ? pb : pf;
}

template <typename T, bool HAS_BY, int DIR>
__global__ void __launch_bounds__(BLOCK) k_asof_idx(
    const T* __restrict__ lon, const int64_t* __restrict__ lby, int64_t n,
    const T* __restrict__ ron, const int64_t* __restrict__ rby, int64_t m,
    int allow_exact, int has_tol, typename AsofDist<T>::type tol,
    int64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    out[i] = asof_row<T, HAS_BY, DIR>(rby, ron, m, HAS_BY ? lby[i] : 0,
                                      lon[i], allow_exact != 0, has_tol != 0,
                                      tol);
}

// Sorted-left form: no by column and lon ascending, so the ASOF_TILE
// consecutive left rows of a block can only match inside one contiguous right
// window.  Two global searches (the tile's first and last key) bound it, one
// position wider on each side for the backward candidate below the first key
// and the forward candidate above the last.  A window of at most ASOF_WIN
// keys is copied into LDS with coalesced loads and every row searches there;
// a longer one is searched in place, which is still a far shorter range than
// m.  Rows go to lanes strided by BLOCK: a wave's 64 lanes hold 64
// consecutive rows, so the left loads and the result stores coalesce with no
// staging and neighbouring lanes walk nearly the same search path.
// An lon that is not ascending gives wrong positions but no wild read: every
// search stays inside [w_lo, w_hi), itself clamped to [0, m].
constexpr int ASOF_TILE = 2048;
constexpr int ASOF_PER = ASOF_TILE / BLOCK;
constexpr int ASOF_WIN = 2544;  // with s_w just under 20 KiB of LDS, so
                                // 8 workgroups (8 waves/SIMD) fit a CU

template <typename T, int DIR>
__global__ void __launch_bounds__(BLOCK) k_asof_idx_sorted(
    const T* __restrict__ lon, int64_t n, const T* __restrict__ ron,
    int64_t m, int allow_exact, int has_tol, typename AsofDist<T>::type tol,
    int64_t* __restrict__ out) {
  __shared__ T s_win[ASOF_WIN];
  __shared__ int64_t s_w[2];
  const int64_t t0 = (int64_t)blockIdx.x * ASOF_TILE;
  const int64_t t1 = min(t0 + (int64_t)ASOF_TILE, n);
  T lv[ASOF_PER];
#pragma unroll
  for (int j = 0; j < ASOF_PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    lv[j] = i < t1 ? lon[i] : T{};
  }
  // one lane of two different waves each runs one of the bounding searches
  if (threadIdx.x == 0)
    s_w[0] = max(asof_bound<T, false>(nullptr, ron, 0, m, 0, lon[t0], false)
                     - 1, (int64_t)0);
  if (threadIdx.x == 64)
    s_w[1] = min(asof_bound<T, false>(nullptr, ron, 0, m, 0, lon[t1 - 1],
                                      true) + 1, m);
  __syncthreads();
  const int64_t w_lo = s_w[0];
  const int64_t wn = s_w[1] - w_lo;
  const bool in_lds = wn <= ASOF_WIN;  // uniform over the block
  if (in_lds) {
    for (int j = threadIdx.x; j < wn; j += BLOCK) s_win[j] = ron[w_lo + j];
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < ASOF_PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) {
      const int64_t p =
          in_lds ? asof_row<T, false, DIR>(nullptr, s_win, wn, 0, lv[j],
                                           allow_exact != 0, has_tol != 0,
                                           tol)
                 : asof_row<T, false, DIR>(nullptr, ron + w_lo, wn, 0, lv[j],
                                           allow_exact != 0, has_tol != 0,
                                           tol);
      out[i] = p < 0 ? -1 : p + w_lo;
    }
  }
}

// Cross-join row indices: lidx[i] = i / nr, ridx[i] = i % nr — the gather
// indices materializing a cartesian product (pandas merge how='cross').
__global__ void __launch_bounds__(BLOCK) k_cross_idx(
    int64_t n, int64_t nr, int64_t* __restrict__ lidx,
    int64_t* __restrict__ ridx) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    lidx[i] = i / nr;
    ridx[i] = i - (i / nr) * nr;
  }
}

// Inverse of gather: out[idx[i]] = src[i].  idx must be a permutation of
// [0, n) (the caller holds a sort_perm) so writes never collide; reads are
// coalesced and the 8 B scattered writes coalesce in L2 like the radix
// scatter's do.
template <typename T>
__global__ void __launch_bounds__(BLOCK) k_scatter(
    const T* __restrict__ src, const int64_t* __restrict__ idx,
    T* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[idx[i]] = src[i];
}

// ---------------------------------------------------------------------------
// Segmented scan (groupby transforms: cumsum/cummin/cummax WITHIN key runs
// of a key-sorted column — the device form of pandas
// DataFrameGroupBy.cumsum, groupby.py "transform" family).
// State is the pair (f, v) — "range contains a segment head", "aggregate of
// the range's tail segment" — under
//   seg_comb((fa,va), (fb,vb)) = (fa|fb, fb ? vb : cs_comb(va,vb))
// which is associative but NOT commutative: every fold/scan below is an
// ordered left-to-right pass (the plain cumsum kernels' strided folds and
// shfl tree reductions are commutative-only and cannot be reused).
// NaN elements (f64) emit NaN at their position and contribute the identity
// to the running state (pandas cum* skipna); min/max propagate through the
// same cs_* helpers as hf_cumsum.  Three phases like hf_cumsum: per-tile
// summaries, one-block exclusive tile scan, per-element apply.
// ---------------------------------------------------------------------------
template <typename T, int OP>
__global__ void __launch_bounds__(BLOCK) k_seg_tiles(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t n,
    typename cs_state<T, OP>::type* __restrict__ tile_v,
    unsigned* __restrict__ tile_f) {
  using S = typename cs_state<T, OP>::type;
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  constexpr int PER = FILT_TILE / BLOCK;
  __shared__ T sv[FILT_TILE];
  __shared__ unsigned char sf[FILT_TILE];
  for (int j = 0; j < PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) {
      sv[(int)(i - t0)] = in[i];
      sf[(int)(i - t0)] = heads[i] != 0;
    }
  }
  __syncthreads();
  const int s0 = threadIdx.x * PER;
  const int lim = (int)(t1 - t0);
  unsigned char f = 0;
  S v = cs_sident<T, OP>();
  for (int j = 0; j < PER; ++j) {
    if (s0 + j < lim) {
      const T x = sv[s0 + j];
      const S xv = cs_lift<T, OP>((x != x) ? cs_ident<T, OP>() : x);
      if (sf[s0 + j]) { f = 1; v = xv; }
      else v = cs_scomb<T, OP>(v, xv);
    }
  }
  __shared__ S bv[BLOCK];
  __shared__ unsigned char bf[BLOCK];
  bv[threadIdx.x] = v;
  bf[threadIdx.x] = f;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    S pv = cs_sident<T, OP>();
    unsigned char pf = 0;
    if (threadIdx.x >= off) { pv = bv[threadIdx.x - off];
                              pf = bf[threadIdx.x - off]; }
    __syncthreads();
    const unsigned char nf = pf | bf[threadIdx.x];
    const S nv = bf[threadIdx.x] ? bv[threadIdx.x]
                                 : cs_scomb<T, OP>(pv, bv[threadIdx.x]);
    __syncthreads();
    bv[threadIdx.x] = nv;
    bf[threadIdx.x] = nf;
    __syncthreads();
  }
  if (threadIdx.x == BLOCK - 1) {
    tile_v[blockIdx.x] = bv[threadIdx.x];
    tile_f[blockIdx.x] = bf[threadIdx.x];
  }
}

template <typename T, int OP>
__global__ void __launch_bounds__(1024) k_seg_scan_tiles(
    typename cs_state<T, OP>::type* __restrict__ tile_v,
    unsigned* __restrict__ tile_f, int64_t ntiles) {
  using S = typename cs_state<T, OP>::type;
  __shared__ S carry_v;
  __shared__ unsigned carry_f;
  if (threadIdx.x == 0) { carry_v = cs_sident<T, OP>(); carry_f = 0; }
  __shared__ S bv[1024];
  __shared__ unsigned char bf[1024];
  __syncthreads();
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    S v = cs_sident<T, OP>();
    unsigned char f = 0;
    if (i < ntiles) { v = tile_v[i]; f = (unsigned char)tile_f[i]; }
    bv[threadIdx.x] = v;
    bf[threadIdx.x] = f;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      S pv = cs_sident<T, OP>();
      unsigned char pf = 0;
      if (threadIdx.x >= off) { pv = bv[threadIdx.x - off];
                                pf = bf[threadIdx.x - off]; }
      __syncthreads();
      const unsigned char nf = pf | bf[threadIdx.x];
      const S nv = bf[threadIdx.x] ? bv[threadIdx.x]
                                   : cs_scomb<T, OP>(pv, bv[threadIdx.x]);
      __syncthreads();
      bv[threadIdx.x] = nv;
      bf[threadIdx.x] = nf;
      __syncthreads();
    }
    const S incl_v = bv[threadIdx.x];
    const unsigned char incl_f = bf[threadIdx.x];
    // exclusive = carry ⊕ previous lane's inclusive (identity at lane 0)
    const S pv = (threadIdx.x == 0) ? cs_sident<T, OP>()
                                    : bv[threadIdx.x - 1];
    const unsigned char pf = (threadIdx.x == 0) ? 0 : bf[threadIdx.x - 1];
    const unsigned ef = carry_f | pf;
    const S ev = pf ? pv : cs_scomb<T, OP>(carry_v, pv);
    if (i < ntiles) { tile_v[i] = ev; tile_f[i] = ef; }
    __syncthreads();  // all lanes read carry before 1023 advances it
    if (threadIdx.x == 1023) {
      carry_v = incl_f ? incl_v : cs_scomb<T, OP>(carry_v, incl_v);
      carry_f = carry_f | incl_f;
    }
    __syncthreads();
  }
}

template <typename T, int OP>
__global__ void __launch_bounds__(BLOCK) k_seg_apply(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t n,
    const typename cs_state<T, OP>::type* __restrict__ tile_v,
    const unsigned* __restrict__ tile_f, T* __restrict__ out) {
  using S = typename cs_state<T, OP>::type;
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  constexpr int PER = FILT_TILE / BLOCK;
  __shared__ T sv[FILT_TILE];
  __shared__ unsigned char sf[FILT_TILE];
  for (int j = 0; j < PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) {
      sv[(int)(i - t0)] = in[i];
      sf[(int)(i - t0)] = heads[i] != 0;
    }
  }
  __syncthreads();
  const int s0 = threadIdx.x * PER;
  const int lim = (int)(t1 - t0);
  S lv[PER];
  unsigned char lf[PER];
  unsigned char f = 0;
  S v = cs_sident<T, OP>();
  for (int j = 0; j < PER; ++j) {
    if (s0 + j < lim) {
      const T x = sv[s0 + j];
      const S xv = cs_lift<T, OP>((x != x) ? cs_ident<T, OP>() : x);
      if (sf[s0 + j]) { f = 1; v = xv; }
      else v = cs_scomb<T, OP>(v, xv);
    }
    lv[j] = v;  // inclusive pair within the thread's run, per element
    lf[j] = f;
  }
  __shared__ S bv[BLOCK];
  __shared__ unsigned char bf[BLOCK];
  bv[threadIdx.x] = v;
  bf[threadIdx.x] = f;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    S pv = cs_sident<T, OP>();
    unsigned char pf = 0;
    if (threadIdx.x >= off) { pv = bv[threadIdx.x - off];
                              pf = bf[threadIdx.x - off]; }
    __syncthreads();
    const unsigned char nf = pf | bf[threadIdx.x];
    const S nv = bf[threadIdx.x] ? bv[threadIdx.x]
                                 : cs_scomb<T, OP>(pv, bv[threadIdx.x]);
    __syncthreads();
    bv[threadIdx.x] = nv;
    bf[threadIdx.x] = nf;
    __syncthreads();
  }
  // thread base = tile exclusive pair ⊕ preceding threads' inclusive pair
  const S pv = (threadIdx.x == 0) ? cs_sident<T, OP>() : bv[threadIdx.x - 1];
  const unsigned char pf = (threadIdx.x == 0) ? 0 : bf[threadIdx.x - 1];
  const S base_v = pf ? pv : cs_scomb<T, OP>(tile_v[blockIdx.x], pv);
  __syncthreads();
  for (int j = 0; j < PER; ++j) {
    if (s0 + j < lim) {
      const T x = sv[s0 + j];
      const S r = lf[j] ? lv[j] : cs_scomb<T, OP>(base_v, lv[j]);
      sv[s0 + j] = (x != x) ? x : cs_value<T, OP>(r);
    }
  }
  __syncthreads();
  for (int j = 0; j < PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) out[i] = sv[(int)(i - t0)];
  }
}

// ---------------------------------------------------------------------------
// Exponentially weighted mean (pandas ewm(...).mean(); hf_ewm_mean in the
// header states the row-by-row state machine).  Two CHAINED first-order
// linear recurrences, both scanned as affine maps under the one ordered,
// division-free combine
//   (a1,b1) then (a2,b2) = (a2*a1, a2*b1 + b2)
//   weights  W_t = P_t W_{t-1} + Q_t   (plus nobs_t, the segmented count of
//                                       valid rows, in the same state)
//   mean     M_t = A_t M_{t-1} + B_t   with A_t, B_t built per row from
//                                       W_{t-1} and nobs_{t-1}
// A numerator/denominator scan is NOT used: alpha = 1 and any NaN gap long
// enough for d^gap to underflow make it 0/0 where pandas carries the last
// mean forward.  Here the only division is per row by ow + nw >= nw > 0.
// Five launches: weight tile summaries, exclusive tile scan, mean tile
// summaries (each tile rebuilds W/nobs from its entry state), exclusive tile
// scan, apply.  Like the segmented scan the combine is not commutative, so
// every fold is an ordered left-to-right pass: per thread over PER
// consecutive rows, wave-level shfl_up scan, then the wave totals in order.
// ---------------------------------------------------------------------------
struct EwW {  // weight map (p, q) + segmented valid-row count (keep, cnt)
  double p, q;
  long long cnt, keep;
  static __device__ __forceinline__ EwW ident() { return {1.0, 0.0, 0, 1}; }
  static __device__ __forceinline__ EwW then(const EwW& f, const EwW& g) {
    return {g.p * f.p, g.p * f.q + g.q, g.keep ? f.cnt + g.cnt : g.cnt,
            f.keep & g.keep};
  }
  __device__ __forceinline__ EwW shfl_up(int off) const {
    return {__shfl_up(p, off), __shfl_up(q, off), __shfl_up(cnt, off),
            __shfl_up(keep, off)};
  }
};
struct EwM {  // mean map (a, b)
  double a, b;
  static __device__ __forceinline__ EwM ident() { return {1.0, 0.0}; }
  static __device__ __forceinline__ EwM then(const EwM& f, const EwM& g) {
    return {g.a * f.a, g.a * f.b + g.b};
  }
  __device__ __forceinline__ EwM shfl_up(int off) const {
    return {__shfl_up(a, off), __shfl_up(b, off)};
  }
};
struct EwPar {
  double d;       // 1 - alpha
  double nw;      // weight of a new observation: 1 (adjust) or alpha
  double pval;    // P of a valid row: d (adjust) or 0
  double pnan;    // P of a NaN row: d, or 1 under ignore_na
  long long thresh;  // emit when nobs >= thresh = max(min_periods, 1)
};

// Ordered exclusive scan of one S per thread over an NT-thread block; *total
// receives the whole block's fold in every thread.  wtot is NT/64 shared
// slots, free for reuse on return.
template <typename S, int NT>
__device__ __forceinline__ S ew_block_excl(S v, S* wtot, S* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const S prev = v.shfl_up(off);
    if (lane >= off) v = S::then(prev, v);
  }
  if (lane == 63) wtot[wave] = v;
  S ex = v.shfl_up(1);
  if (lane == 0) ex = S::ident();
  __syncthreads();
  S pre = S::ident(), tot = S::ident();
  for (int w = 0; w < NT / 64; ++w) {
    if (w == wave) pre = tot;
    tot = S::then(tot, wtot[w]);
  }
  *total = tot;
  __syncthreads();
  return S::then(pre, ex);
}

constexpr int EW_PER = FILT_TILE / BLOCK;
// LDS slot of tile row i: one pad double per thread run keeps the per-thread
// sequential walks (stride EW_PER doubles between lanes) off the same banks
__device__ __forceinline__ int ew_slot(int i) { return i + i / EW_PER; }
constexpr int EW_STAGE = FILT_TILE + BLOCK;

// coalesced tile load into LDS; int64 values convert here
template <typename T, bool HEADS>
__device__ __forceinline__ void ew_stage(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t t0,
    int64_t t1, double* sv, unsigned char* sf) {
  for (int j = 0; j < EW_PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) {
      sv[ew_slot((int)(i - t0))] = (double)in[i];
      if (HEADS) sf[(int)(i - t0)] = heads[i] != 0;
    }
  }
  __syncthreads();
}

// the weight/count map of one thread's run of rows [s0, s0 + EW_PER)
template <bool HEADS>
__device__ __forceinline__ EwW ew_w_fold(const double* sv,
                                         const unsigned char* sf, int s0,
                                         int lim, const EwPar& k) {
  EwW s = EwW::ident();
#pragma unroll
  for (int j = 0; j < EW_PER; ++j) {
    if (s0 + j < lim) {
      const double x = sv[ew_slot(s0 + j)];
      const bool valid = x == x;
      double p = valid ? k.pval : k.pnan;
      if (HEADS && sf[s0 + j]) { p = 0.0; s.keep = 0; s.cnt = 0; }
      s.p *= p;
      s.q = p * s.q + (valid ? 1.0 : 0.0);
      s.cnt += valid;
    }
  }
  return s;
}

// One row: advance (W, nobs) and return the row's mean map.
__device__ __forceinline__ EwM ew_row(double x, bool head, double& W,
                                      long long& nobs, const EwPar& k) {
  if (head) { W = 0.0; nobs = 0; }
  EwM m;
  if (x == x) {
    const double ow = k.d * W;
    if (nobs == 0) {
      m.a = 0.0;
      m.b = x;
    } else {
      const double s = ow + k.nw;
      m.a = ow / s;
      m.b = k.nw * x / s;
    }
    W = k.pval * W + 1.0;
    nobs += 1;
  } else {
    m.a = head ? 0.0 : 1.0;
    m.b = 0.0;
    W *= k.pnan;
  }
  return m;
}

template <typename T, bool HEADS>
__global__ void __launch_bounds__(BLOCK) k_ewm_w_tiles(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t n,
    EwPar k, EwW* __restrict__ tile_w) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  __shared__ double sv[EW_STAGE];
  __shared__ unsigned char sf[HEADS ? FILT_TILE : 1];
  __shared__ EwW wtot[BLOCK / 64];
  ew_stage<T, HEADS>(in, heads, t0, t1, sv, sf);
  const EwW s = ew_w_fold<HEADS>(sv, sf, threadIdx.x * EW_PER,
                                 (int)(t1 - t0), k);
  EwW tot;
  ew_block_excl<EwW, BLOCK>(s, wtot, &tot);
  if (threadIdx.x == 0) tile_w[blockIdx.x] = tot;
}

// In-place exclusive scan of the tile summaries, 1024 per iteration with the
// running carry held by every thread.  Both recurrences start from the zero
// state, so afterwards tile_w[t].q / .cnt are tile t's entry W / nobs and
// tile_m[t].b its entry mean.
template <typename S>
__global__ void __launch_bounds__(1024) k_ewm_scan_tiles(
    S* __restrict__ tiles, int64_t ntiles) {
  __shared__ S wtot[1024 / 64];
  S carry = S::ident();
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const S v = (i < ntiles) ? tiles[i] : S::ident();
    S tot;
    const S ex = ew_block_excl<S, 1024>(v, wtot, &tot);
    if (i < ntiles) tiles[i] = S::then(carry, ex);
    carry = S::then(carry, tot);
  }
}

template <typename T, bool HEADS>
__global__ void __launch_bounds__(BLOCK) k_ewm_m_tiles(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t n,
    EwPar k, const EwW* __restrict__ tile_w, EwM* __restrict__ tile_m) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  __shared__ double sv[EW_STAGE];
  __shared__ unsigned char sf[HEADS ? FILT_TILE : 1];
  __shared__ EwW wtot[BLOCK / 64];
  __shared__ EwM mtot[BLOCK / 64];
  ew_stage<T, HEADS>(in, heads, t0, t1, sv, sf);
  const int s0 = threadIdx.x * EW_PER;
  const int lim = (int)(t1 - t0);
  EwW wt;
  const EwW we = ew_block_excl<EwW, BLOCK>(
      ew_w_fold<HEADS>(sv, sf, s0, lim, k), wtot, &wt);
  const EwW entry = tile_w[blockIdx.x];
  double W = we.p * entry.q + we.q;
  long long nobs = we.keep ? entry.cnt + we.cnt : we.cnt;
  EwM m = EwM::ident();
#pragma unroll
  for (int j = 0; j < EW_PER; ++j) {
    if (s0 + j < lim)
      m = EwM::then(m, ew_row(sv[ew_slot(s0 + j)], HEADS && sf[s0 + j], W,
                              nobs, k));
  }
  EwM tot;
  ew_block_excl<EwM, BLOCK>(m, mtot, &tot);
  if (threadIdx.x == 0) tile_m[blockIdx.x] = tot;
}

template <typename T, bool HEADS>
__global__ void __launch_bounds__(BLOCK) k_ewm_apply(
    const T* __restrict__ in, const int64_t* __restrict__ heads, int64_t n,
    EwPar k, const EwW* __restrict__ tile_w, const EwM* __restrict__ tile_m,
    double* __restrict__ out) {
  const int64_t t0 = (int64_t)blockIdx.x * FILT_TILE;
  const int64_t t1 = min(t0 + (int64_t)FILT_TILE, n);
  __shared__ double sv[EW_STAGE];
  __shared__ unsigned char sf[HEADS ? FILT_TILE : 1];
  __shared__ EwW wtot[BLOCK / 64];
  __shared__ EwM mtot[BLOCK / 64];
  ew_stage<T, HEADS>(in, heads, t0, t1, sv, sf);
  const int s0 = threadIdx.x * EW_PER;
  const int lim = (int)(t1 - t0);
  EwW wt;
  const EwW we = ew_block_excl<EwW, BLOCK>(
      ew_w_fold<HEADS>(sv, sf, s0, lim, k), wtot, &wt);
  const EwW entry = tile_w[blockIdx.x];
  double W = we.p * entry.q + we.q;
  const long long nobs0 = we.keep ? entry.cnt + we.cnt : we.cnt;
  long long nobs = nobs0;
  // inclusive mean map of the thread's run up to each row, in registers
  double la[EW_PER], lb[EW_PER];
  EwM m = EwM::ident();
#pragma unroll
  for (int j = 0; j < EW_PER; ++j) {
    if (s0 + j < lim)
      m = EwM::then(m, ew_row(sv[ew_slot(s0 + j)], HEADS && sf[s0 + j], W,
                              nobs, k));
    la[j] = m.a;
    lb[j] = m.b;
  }
  EwM mt;
  const EwM me = ew_block_excl<EwM, BLOCK>(m, mtot, &mt);
  const double M0 = me.a * tile_m[blockIdx.x].b + me.b;
  // each thread rewrites only its own run's slots: NaN rows are still
  // readable as NaN until their turn, so nobs is recounted from LDS
  nobs = nobs0;
#pragma unroll
  for (int j = 0; j < EW_PER; ++j) {
    if (s0 + j < lim) {
      const double x = sv[ew_slot(s0 + j)];
      if (HEADS && sf[s0 + j]) nobs = 0;
      nobs += (x == x);
      sv[ew_slot(s0 + j)] = (nobs >= k.thresh) ? la[j] * M0 + lb[j]
                                               : __builtin_nan("");
    }
  }
  __syncthreads();
  for (int j = 0; j < EW_PER; ++j) {
    const int64_t i = t0 + (int64_t)j * BLOCK + threadIdx.x;
    if (i < t1) out[i] = sv[ew_slot((int)(i - t0))];
  }
}

}  // namespace

struct hf_join {
  int64_t key_min, n_slots, n_right;
  int nr;
  unsigned long long* d_csr;   // [n_slots+1]
  unsigned* d_jidx;            // [n_right] right row index, key-grouped
  double* d_jval[GB_MAX_VALS]; // [nr][n_right] right values in CSR order
                               // (opaque 8 B payloads — i64 or f64)
  int dtypes[GB_MAX_VALS];     // per right column
};

namespace {
template <int OP>
int launch_map_f64(const hf_col* in, double s, hf_col* out) {
  const int64_t n = in->len;
  return timed_launch("map_f64", [&] {
    hipLaunchKernelGGL(k_map_f64<OP>, dim3(grid_for((n >> 1) + 1)), dim3(BLOCK), 0,
                       g.stream, (const double*)in->dptr, (double*)out->dptr, s, n);
  });
}
template <int OP>
int launch_map_i64(const hf_col* in, int64_t s, hf_col* out) {
  const int64_t n = in->len;
  return timed_launch("map_i64", [&] {
    hipLaunchKernelGGL(k_map_i64<OP>, dim3(grid_for((n >> 1) + 1)), dim3(BLOCK), 0,
                       g.stream, (const int64_t*)in->dptr, (int64_t*)out->dptr, s, n);
  });
}
}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int hf_init(int gpu) {
  if (g.inited && g.gpu == gpu) return HF_OK;
  if (g.inited) hf_shutdown();
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return set_hip_err("hf_init", e);
  if (gpu < 0 || gpu >= n)
    return set_err(HF_ERR_ARG, "hf_init", "gpu index out of range");
  HF_HIP("hf_init", hipSetDevice(gpu));
  HF_HIP("hf_init", hipStreamCreate(&g.stream));
  HF_HIP("hf_init", hipMalloc(&g.d_scratch, SCRATCH_BYTES));
  HF_HIP("hf_init", hipMemset(g.d_scratch, 0, SCRATCH_BYTES));
  g.gpu = gpu;
  g.inited = true;
  return HF_OK;
}

int hf_shutdown(void) {
  if (!g.inited) return HF_OK;
  hipStreamSynchronize(g.stream);
  g_cache.trim();
  g_dev_live = 0;  // blocks still out are only forgotten from here on
  for (auto& p : g.pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  g.pending.clear();
  g.stats.clear();
  if (g.d_scratch) hipFree(g.d_scratch);
  hipStreamDestroy(g.stream);
  g = State{};
  return HF_OK;
}

int hf_device_count(int* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *out = 0; return set_hip_err("hf_device_count", e); }
  *out = n;
  return HF_OK;
}

const char* hf_last_error(void) { return g_err.c_str(); }

int hf_sync(void) {
  HF_NEED_INIT("hf_sync");
  HF_HIP("hf_sync", hipStreamSynchronize(g.stream));
  return HF_OK;
}

// ---- memory ----

int hf_col_alloc(int64_t len, int dtype, hf_col** out) {
  HF_NEED_INIT("hf_col_alloc");
  if (len < 0 || dtype_size(dtype) == 0 || !out)
    return set_err(HF_ERR_ARG, "hf_col_alloc", "bad len/dtype");
  void* d = nullptr;
  int64_t bytes = len * dtype_size(dtype);
  if (bytes == 0) bytes = 8;  // keep zero-length columns addressable
  HF_HIP("hf_col_alloc", dev_alloc((void**)&d, bytes, g.stream));
  hf_col* c = new hf_col{d, len, dtype, g.gpu};
  *out = c;
  return HF_OK;
}

int hf_put(const void* host, int64_t len, int dtype, hf_col** out) {
  HF_NEED_INIT("hf_put");
  if (!out) return set_err(HF_ERR_ARG, "hf_put", "null");
  ColOut col;
  int rc = col.alloc(len, dtype);
  if (rc != HF_OK) return rc;
  if (len > 0)
    HF_HIP("hf_put", hipMemcpyAsync(col.get()->dptr, host, len * dtype_size(dtype),
                                    hipMemcpyHostToDevice, g.stream));
  col.commit(out);
  return HF_OK;
}

int hf_get(const hf_col* col, void* host) {
  HF_NEED_INIT("hf_get");
  if (!col || !host) return set_err(HF_ERR_ARG, "hf_get", "null");
  if (col->len > 0)
    HF_HIP("hf_get", hipMemcpyAsync(host, col->dptr, col->len * dtype_size(col->dtype),
                                    hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_get", hipStreamSynchronize(g.stream));
  return HF_OK;
}

int hf_col_free(hf_col* col) {
  if (!col) return HF_OK;
  if (g.inited && col->dptr) dev_free(col->dptr, g.stream);
  col->gb.release();
  delete col;
  return HF_OK;
}

int64_t hf_col_len(const hf_col* c) { return c ? c->len : -1; }
int hf_col_dtype(const hf_col* c) { return c ? c->dtype : -1; }
uintptr_t hf_col_dptr(const hf_col* c) { return c ? (uintptr_t)c->dptr : 0; }

int hf_alloc_raw(int64_t bytes, uintptr_t* dptr) {
  HF_NEED_INIT("hf_alloc_raw");
  void* d = nullptr;
  HF_HIP("hf_alloc_raw", dev_alloc((void**)&d, bytes, g.stream));
  *dptr = (uintptr_t)d;
  return HF_OK;
}
int hf_free_raw(uintptr_t dptr) {
  HF_NEED_INIT("hf_free_raw");
  HF_HIP("hf_free_raw", dev_free((void*)dptr, g.stream));
  return HF_OK;
}
int hf_dev_live(int64_t* blocks) {
  if (!blocks) return set_err(HF_ERR_ARG, "hf_dev_live", "null");
  *blocks = g_dev_live;
  return HF_OK;
}
int hf_memset_raw(uintptr_t dptr, int value, int64_t bytes) {
  HF_NEED_INIT("hf_memset_raw");
  HF_HIP("hf_memset_raw", hipMemsetAsync((void*)dptr, value, bytes, g.stream));
  return HF_OK;
}

// ---- map ----

int hf_map_scalar(int op, const hf_col* in, double scalar, hf_col** out) {
  HF_NEED_INIT("hf_map_scalar");
  if (!in || !out) return set_err(HF_ERR_ARG, "hf_map_scalar", "null");
  ColOut o;
  if (op == HF_MAP_CAST_F64) {
    if (in->dtype != HF_INT64)
      return set_err(HF_ERR_ARG, "hf_map_scalar", "cast_f64 needs int64 input");
    int rc = o.alloc(in->len, HF_FLOAT64);
    if (rc != HF_OK) return rc;
    rc = timed_launch("cast_i64_f64", [&] {
      hipLaunchKernelGGL(k_cast_i64_f64, dim3(grid_for(in->len)), dim3(BLOCK), 0,
                         g.stream, (const int64_t*)in->dptr, o.data<double>(),
                         in->len);
    });
    return o.commit_if(rc, out);
  }
  if (op == HF_MAP_CAST_I64) {
    if (in->dtype != HF_FLOAT64)
      return set_err(HF_ERR_ARG, "hf_map_scalar", "cast_i64 needs f64 input");
    int rc = o.alloc(in->len, HF_INT64);
    if (rc != HF_OK) return rc;
    rc = timed_launch("cast_f64_i64", [&] {
      hipLaunchKernelGGL(k_cast_f64_i64, dim3(grid_for(in->len)), dim3(BLOCK), 0,
                         g.stream, (const double*)in->dptr, o.data<int64_t>(),
                         in->len);
    });
    return o.commit_if(rc, out);
  }
  if (in->dtype == HF_INT64) return hf_map_scalar_i64(op, in, (int64_t)scalar, out);
  int rc = o.alloc(in->len, HF_FLOAT64);
  if (rc != HF_OK) return rc;
  switch (op) {
    case HF_MAP_ADD:    rc = launch_map_f64<HF_MAP_ADD>(in, scalar, o.get()); break;
    case HF_MAP_SUB:    rc = launch_map_f64<HF_MAP_SUB>(in, scalar, o.get()); break;
    case HF_MAP_RSUB:   rc = launch_map_f64<HF_MAP_RSUB>(in, scalar, o.get()); break;
    case HF_MAP_MUL:    rc = launch_map_f64<HF_MAP_MUL>(in, scalar, o.get()); break;
    case HF_MAP_DIV:    rc = launch_map_f64<HF_MAP_DIV>(in, scalar, o.get()); break;
    case HF_MAP_RDIV:   rc = launch_map_f64<HF_MAP_RDIV>(in, scalar, o.get()); break;
    case HF_MAP_FILLNA: rc = launch_map_f64<HF_MAP_FILLNA>(in, scalar, o.get()); break;
    case HF_MAP_ABS:    rc = launch_map_f64<HF_MAP_ABS>(in, scalar, o.get()); break;
    case HF_MAP_NEG:    rc = launch_map_f64<HF_MAP_NEG>(in, scalar, o.get()); break;
    case HF_MAP_SQRT:   rc = launch_map_f64<HF_MAP_SQRT>(in, scalar, o.get()); break;
    case HF_MAP_MIN:    rc = launch_map_f64<HF_MAP_MIN>(in, scalar, o.get()); break;
    case HF_MAP_MAX:    rc = launch_map_f64<HF_MAP_MAX>(in, scalar, o.get()); break;
    case HF_MAP_ROUND:  rc = launch_map_f64<HF_MAP_ROUND>(in, scalar, o.get()); break;
    default:
      rc = set_err(HF_ERR_UNSUPPORTED, "hf_map_scalar", "unknown op");
  }
  return o.commit_if(rc, out);
}

int hf_map_scalar_i64(int op, const hf_col* in, int64_t scalar, hf_col** out) {
  HF_NEED_INIT("hf_map_scalar_i64");
  if (!in || !out) return set_err(HF_ERR_ARG, "hf_map_scalar_i64", "null");
  if (in->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_map_scalar_i64", "int64 column required");
  ColOut o;
  int rc = o.alloc(in->len, HF_INT64);
  if (rc != HF_OK) return rc;
  switch (op) {
    case HF_MAP_ADD:  rc = launch_map_i64<HF_MAP_ADD>(in, scalar, o.get()); break;
    case HF_MAP_SUB:  rc = launch_map_i64<HF_MAP_SUB>(in, scalar, o.get()); break;
    case HF_MAP_RSUB: rc = launch_map_i64<HF_MAP_RSUB>(in, scalar, o.get()); break;
    case HF_MAP_MUL:  rc = launch_map_i64<HF_MAP_MUL>(in, scalar, o.get()); break;
    case HF_MAP_ABS:  rc = launch_map_i64<HF_MAP_ABS>(in, scalar, o.get()); break;
    case HF_MAP_NEG:  rc = launch_map_i64<HF_MAP_NEG>(in, scalar, o.get()); break;
    case HF_MAP_MIN:  rc = launch_map_i64<HF_MAP_MIN>(in, scalar, o.get()); break;
    case HF_MAP_MAX:  rc = launch_map_i64<HF_MAP_MAX>(in, scalar, o.get()); break;
    case HF_MAP_IDIV:
      rc = scalar == 0
               ? set_err(HF_ERR_ARG, "hf_map_scalar_i64", "floordiv by zero")
               : launch_map_i64<HF_MAP_IDIV>(in, scalar, o.get());
      break;
    case HF_MAP_IMOD:
      rc = scalar == 0 ? set_err(HF_ERR_ARG, "hf_map_scalar_i64", "mod by zero")
                       : launch_map_i64<HF_MAP_IMOD>(in, scalar, o.get());
      break;
    default:
      rc = set_err(HF_ERR_UNSUPPORTED, "hf_map_scalar_i64",
                   "op not defined for int64 (div promotes via cast_f64)");
  }
  return o.commit_if(rc, out);
}

// ---- binary ----

int hf_binary(int op, const hf_col* a, const hf_col* b, hf_col** out) {
  HF_NEED_INIT("hf_binary");
  if (!a || !b || !out) return set_err(HF_ERR_ARG, "hf_binary", "null");
  if (a->len != b->len)
    return set_err(HF_ERR_ARG, "hf_binary", "length mismatch");
  if (a->dtype != b->dtype)
    return set_err(HF_ERR_ARG, "hf_binary", "dtype mismatch (cast first)");
  const bool f64 = a->dtype == HF_FLOAT64;
  if (!f64 && op == HF_BIN_DIV)
    return set_err(HF_ERR_UNSUPPORTED, "hf_binary", "int64 div promotes via cast_f64");
  ColOut o;
  int rc = o.alloc(a->len, a->dtype);
  if (rc != HF_OK) return rc;
  const int64_t n = a->len;
  // dispatch with typed wrappers
  auto Lf = [&](auto opTag) {
    constexpr int O = decltype(opTag)::value;
    return timed_launch("bin_f64", [&] {
      hipLaunchKernelGGL((k_bin<O, double, double2>), dim3(grid_for((n >> 1) + 1)),
                         dim3(BLOCK), 0, g.stream, (const double*)a->dptr,
                         (const double*)b->dptr, o.data<double>(), n);
    });
  };
  auto Li = [&](auto opTag) {
    constexpr int O = decltype(opTag)::value;
    return timed_launch("bin_i64", [&] {
      hipLaunchKernelGGL((k_bin<O, int64_t, longlong2>), dim3(grid_for((n >> 1) + 1)),
                         dim3(BLOCK), 0, g.stream, (const int64_t*)a->dptr,
                         (const int64_t*)b->dptr, o.data<int64_t>(), n);
    });
  };
  switch (op) {
    case HF_BIN_ADD: rc = f64 ? Lf(int_tag<HF_BIN_ADD>{}) : Li(int_tag<HF_BIN_ADD>{}); break;
    case HF_BIN_SUB: rc = f64 ? Lf(int_tag<HF_BIN_SUB>{}) : Li(int_tag<HF_BIN_SUB>{}); break;
    case HF_BIN_MUL: rc = f64 ? Lf(int_tag<HF_BIN_MUL>{}) : Li(int_tag<HF_BIN_MUL>{}); break;
    case HF_BIN_DIV: rc = Lf(int_tag<HF_BIN_DIV>{}); break;
    case HF_BIN_MIN: rc = f64 ? Lf(int_tag<HF_BIN_MIN>{}) : Li(int_tag<HF_BIN_MIN>{}); break;
    case HF_BIN_MAX: rc = f64 ? Lf(int_tag<HF_BIN_MAX>{}) : Li(int_tag<HF_BIN_MAX>{}); break;
    default:
      rc = set_err(HF_ERR_UNSUPPORTED, "hf_binary", "unknown op");
  }
  return o.commit_if(rc, out);
}

// ---- reduce ----

int hf_reduce(const hf_col* in, hf_reduce_result* out) {
  HF_NEED_INIT("hf_reduce");
  if (!in || !out) return set_err(HF_ERR_ARG, "hf_reduce", "null");
  ReduceAccF64* dF = (ReduceAccF64*)g.d_scratch;
  ReduceAccI64* dI = (ReduceAccI64*)((char*)g.d_scratch + 64);
  hipLaunchKernelGGL(k_reduce_init, dim3(1), dim3(1), 0, g.stream, dF, dI);
  const int64_t n = in->len;
  int rc;
  if (in->dtype == HF_FLOAT64) {
    rc = timed_launch("reduce_f64", [&] {
      hipLaunchKernelGGL(k_reduce_f64, dim3(grid_for((n >> 1) + 1)), dim3(BLOCK), 0,
                         g.stream, (const double*)in->dptr, n, dF);
    });
  } else {
    rc = timed_launch("reduce_i64", [&] {
      hipLaunchKernelGGL(k_reduce_i64, dim3(grid_for((n >> 1) + 1)), dim3(BLOCK), 0,
                         g.stream, (const int64_t*)in->dptr, n, dI);
    });
  }
  if (rc != HF_OK) return rc;
  ReduceAccF64 hF;
  ReduceAccI64 hI;
  HF_HIP("hf_reduce", hipMemcpyAsync(&hF, dF, sizeof(hF), hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_reduce", hipMemcpyAsync(&hI, dI, sizeof(hI), hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_reduce", hipStreamSynchronize(g.stream));
  if (in->dtype == HF_FLOAT64) {
    out->sum = hF.sum;
    out->count = (int64_t)hF.count;
    out->mn = hF.mn;
    out->mx = hF.mx;
    out->isum = (int64_t)hF.sum;
    out->imn = (int64_t)hF.mn;
    out->imx = (int64_t)hF.mx;
  } else {
    out->sum = (double)hI.sum;
    out->count = (int64_t)hI.count;
    out->mn = (double)hI.mn;
    out->mx = (double)hI.mx;
    out->isum = hI.sum;
    out->imn = hI.mn;
    out->imx = hI.mx;
  }
  return HF_OK;
}

// ---- groupby ----

}  // extern "C" (the radix-path helpers below are C++ templates)

namespace {

// Per-bucket histogram of an (immutable) key column, cached host-side on the
// hf_col — repeated groupbys on the same keys skip the P0 pass entirely.
int ensure_host_hist(hf_col* keys, int64_t key_min, int64_t n_slots,
                     int64_t nb, int range_log) {
  // keyed on the exact n_slots, not only the bucket count: rows between two
  // n_slots inside the same last bucket change that bucket's region size
  GbKeyCache& kc = keys->gb;
  if (!kc.hist.empty() && kc.hist_kmin == key_min && kc.hist_nb == nb &&
      kc.hist_nslots == n_slots)
    return HF_OK;
  // the radix layout cache and the scatter plan derive from this histogram:
  // invalidate with it
  kc.drop_derived();
  DevBuf d_h;
  HF_HIP("gb_hist", d_h.alloc(nb * 8));
  HF_HIP("gb_hist", hipMemsetAsync(d_h.as<void>(), 0, nb * 8, g.stream));
  const int64_t n = keys->len;
  int rc = timed_launch("gb_hist", [&] {
    hipLaunchKernelGGL(k_gb_hist, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                       (uint32_t)(nb * 4), g.stream, (const int64_t*)keys->dptr,
                       n, key_min, n_slots, (int)nb, range_log,
                       d_h.as<unsigned long long>());
  });
  if (rc != HF_OK) return rc;
  std::vector<int64_t> h((size_t)nb);
  HF_HIP("gb_hist", hipMemcpyAsync(h.data(), d_h.as<void>(), nb * 8,
                                   hipMemcpyDeviceToHost, g.stream));
  HF_HIP("gb_hist", hipStreamSynchronize(g.stream));
  kc.hist = std::move(h);
  kc.hist_kmin = key_min;
  kc.hist_nb = nb;
  kc.hist_nslots = n_slots;
  return HF_OK;
}

template <int AOP>
int gb_dense_path(const hf_col* keys, const GbPtrs& ptrs, int nvals,
                  int64_t key_min, int64_t n_slots, uintptr_t sums,
                  uintptr_t rowcnt, uintptr_t counts,
                  unsigned long long* d_err) {
  const int64_t n = keys->len;
  const bool cnt = counts != 0;
  int64_t grid = n / 65536 + 1;
  if (grid > 512) grid = 512;
  auto L = [&](auto rTag, auto cTag, auto vTag, const double* v, double* gs,
               unsigned long long* gc) {
    constexpr bool R = decltype(rTag)::value, C = decltype(cTag)::value,
                   V = decltype(vTag)::value;
    const uint32_t lds =
        (uint32_t)(n_slots * ((V ? 8 : 0) + 1 + (C ? 4 : 0)));
    return timed_launch("gb_dense", [&] {
      hipLaunchKernelGGL((k_gb_dense<R, C, V, AOP>), dim3((uint32_t)grid),
                         dim3(512), lds, g.stream, (const int64_t*)keys->dptr,
                         v, n, key_min, n_slots, gs,
                         (unsigned long long*)rowcnt, gc, d_err);
    });
  };
  using T = std::true_type;
  using F = std::false_type;
  if (nvals == 0) return L(T{}, F{}, F{}, nullptr, nullptr, nullptr);
  for (int c = 0; c < nvals; ++c) {
    double* gs = (double*)sums + (int64_t)c * n_slots;
    unsigned long long* gc =
        cnt ? (unsigned long long*)counts + (int64_t)c * n_slots : nullptr;
    int rc = with_bool(c == 0, [&](auto rTag) {
      return with_bool(cnt, [&](auto cTag) {
        return L(rTag, cTag, T{}, ptrs.vals[c], gs, gc);
      });
    });
    if (rc != HF_OK) return rc;
  }
  return HF_OK;
}

int ensure_keys32(hf_col* keys, int64_t key_min) {
  GbKeyCache& kc = keys->gb;
  if (kc.d_k32 && kc.k32_min == key_min) return HF_OK;
  drop_dev(kc.d_k32);
  const int64_t n = keys->len;
  HF_HIP("keys32", dev_alloc(&kc.d_k32, (n > 0 ? n : 1) * 4, g.stream));
  int rc = timed_launch("gb_keys32", [&] {
    hipLaunchKernelGGL(k_conv_keys32, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                       0, g.stream, (const int64_t*)keys->dptr, n, key_min,
                       (unsigned*)kc.d_k32);
  });
  if (rc != HF_OK) return rc;
  kc.k32_min = key_min;
  return HF_OK;
}

// Exact per-bucket regions, 64-row aligned; u32 cursors cap one partition
// at ~4.29e9 rows (shard larger frames).  The cursor-init array and the
// work items derive only from the cached histogram, so they cache on the
// immutable key column too: steady-state groupby calls copy cursors D2D
// and never touch the host (no pageable H2D, no mid-op sync).
// Work-item starts are off + done: off is a multiple of 64 and done a
// multiple of AGG_CHUNK, so every start is even (k_gb_bucket_agg relies on it).
static_assert(AGG_CHUNK % 2 == 0, "k_gb_bucket_agg needs even item starts");

template <int RL>
int ensure_radix_layout(hf_col* keys, int64_t nb) {
  GbKeyCache& kc = keys->gb;
  if (kc.d_curinit && kc.radix_rl == RL) return HF_OK;
  kc.drop_derived();
  std::vector<unsigned> cur_init((size_t)nb);
  std::vector<GbWorkItem> work;
  std::vector<unsigned> item0((size_t)nb + 1);
  int64_t off = 0;
  for (int64_t b = 0; b < nb; ++b) {
    cur_init[b] = (unsigned)off;
    item0[b] = (unsigned)work.size();
    const int64_t rows_b = kc.hist[b];
    int64_t done = 0;
    while (done < rows_b) {
      const int64_t len = std::min(AGG_CHUNK, rows_b - done);
      work.push_back(GbWorkItem{off + done, (int32_t)b, (int32_t)len});
      done += len;
    }
    off += (rows_b + 63) & ~63LL;
  }
  item0[nb] = (unsigned)work.size();
  if (off > 0xFFFFFFF0LL)
    return set_err(HF_ERR_UNSUPPORTED, "hf_groupby_accum",
                   "partition too large for radix scatter (shard it)");
  DevBuf d_curinit, d_work, d_item0;
  HF_HIP("gb_radix", d_curinit.alloc(nb * 4));
  HF_HIP("gb_radix", d_item0.alloc((nb + 1) * 4));
  HF_HIP("gb_radix", hipMemcpyAsync(d_item0.as<void>(), item0.data(),
                                    (nb + 1) * 4, hipMemcpyHostToDevice,
                                    g.stream));
  HF_HIP("gb_radix",
         d_work.alloc(std::max<size_t>(work.size(), 1) * sizeof(GbWorkItem)));
  HF_HIP("gb_radix", hipMemcpyAsync(d_curinit.as<void>(), cur_init.data(),
                                    nb * 4, hipMemcpyHostToDevice, g.stream));
  if (!work.empty())
    HF_HIP("gb_radix", hipMemcpyAsync(d_work.as<void>(), work.data(),
                                      work.size() * sizeof(GbWorkItem),
                                      hipMemcpyHostToDevice, g.stream));
  // host vectors must outlive the async H2D of pageable memory
  HF_HIP("gb_radix", hipStreamSynchronize(g.stream));
  kc.d_curinit = d_curinit.release();
  kc.d_work = d_work.release();
  kc.d_item0 = d_item0.release();
  kc.work_n = (int64_t)work.size();
  kc.radix_rows = off;
  kc.radix_rl = RL;
  return HF_OK;
}

// payload rows one radix call allocates (never a zero-byte block)
int64_t radix_alloc_rows(const GbKeyCache& kc) {
  return std::max<int64_t>(kc.radix_rows, 64);
}
// tiles of a plan (the odd last row is a row of the last tile) and the rows
// of its tile-major payload
int64_t gb_plan_tiles(int64_t n) {
  return (n + GB_PLAN_TILE - 1) / GB_PLAN_TILE;
}
int64_t gb_plan_rows(int64_t n) {
  return std::max<int64_t>(gb_plan_tiles(n), 1) * GB_PLAN_TILE;
}
int64_t gb_item_cut(int64_t n) {
  return std::min(GB_ITEM_CUT_MAX,
                  std::max(GB_ITEM_CUT_MIN, n / GB_ITEMS_MIN));
}
uint32_t gb_tile_grid(int64_t ntiles) {
  return (uint32_t)std::min<int64_t>(std::max<int64_t>(ntiles, 1), 2048);
}

// What P1 does with the scatter plan of the key column (see GbKeyCache).
enum class GbPlan {
  None,    // plan-less: scatter keys + values on every call
  Record,  // plan buffers are allocated; this call scatters and records
  Replay,  // a valid plan exists: permute values only
};

// Valid plan -> Replay, else allocate one -> Record.  HF_GB_PLAN=0 (read
// once) or a failed plan allocation selects the plan-less path; this never
// fails the call.  Every plan buffer is allocated here, the work items at the
// bound the histogram gives (a bucket of r rows is cut into at most
// (r - 1 + ntiles * GB_TILE_COST) / cut + 1 items), so nothing can fail after
// the record.
GbPlan ensure_plan(hf_col* keys, int rl, int64_t key_min, int64_t n_slots,
                   int64_t nb) {
  static const bool plan_env = [] {
    const char* e = getenv("HF_GB_PLAN");
    return !(e && e[0] == '0');
  }();
  if (!plan_env) return GbPlan::None;
  GbKeyCache& kc = keys->gb;
  if (kc.plan_rl == rl && kc.plan_kmin == key_min && kc.plan_nslots == n_slots)
    return GbPlan::Replay;
  kc.drop_plan();
  const int64_t n = keys->len;
  const int64_t cut = gb_item_cut(n);
  int64_t items_max = 1;
  for (int64_t b = 0; b < nb; ++b)
    if (kc.hist[b] > 0)
      items_max +=
          (kc.hist[b] - 1 + gb_plan_tiles(n) * GB_TILE_COST) / cut + 1;
  DevBuf dst, rk, runs, items, item0, order, meta;
  if (dst.alloc((n + 2) * 2) != hipSuccess ||
      rk.alloc(gb_plan_rows(n) * 2) != hipSuccess ||
      runs.alloc(std::max<int64_t>(gb_plan_tiles(n), 1) * nb * 4) !=
          hipSuccess ||
      items.alloc(items_max * sizeof(GbTileItem)) != hipSuccess ||
      order.alloc(items_max * 4) != hipSuccess ||
      // item0[nb + 1], then the per-bucket item counts [nb]
      item0.alloc((2 * nb + 1) * 4) != hipSuccess ||
      meta.alloc(8) != hipSuccess) {
    (void)hipGetLastError();
    return GbPlan::None;
  }
  kc.d_plan_dst = dst.release();
  kc.d_plan_rk = rk.release();
  kc.d_plan_runs = runs.release();
  kc.d_plan_items = items.release();
  kc.d_plan_item0 = item0.release();
  kc.d_plan_order = order.release();
  kc.d_plan_meta = meta.release();
  return GbPlan::Record;
}

// The arguments every P1/P2 launch of one radix call shares.
struct GbRadixCall {
  hf_col* keys;
  int64_t nb, key_min, n_slots;
  unsigned long long* d_err;
  double* r0;          // scattered values (each column in turn on a plan)
  double* r1;          // second column, plan-less path only
  unsigned short* rk;  // scattered low keys (the plan's own on a plan)
  unsigned* d_cur;     // this call's bucket cursors (plan-less path only)
  bool tiled;          // on a plan: tile-major payload, GbTileItem work
};

// P1 scatter (pipelined): 12288-row tiles as 1024x12 for <=1 value column
// — 147 KB LDS, 1 block/CU of 16 waves (round-2 probe: 1024x12 edges out
// 512x24 and both beat the round-1 kernel by ~17%); 6144-row tiles as
// 512x12 for 2 columns.
// REC, the plan record: the same staging on the int64 keys (no u32 copy),
// first value column only, at the plan's 1024x12 geometry, written tile-major;
// then the plan's work items are cut on the device and the host reads their
// count back, once.
template <int RL, bool REC>
int radix_scatter(const GbRadixCall& a, const GbPtrs& ptrs, int nvals) {
  GbKeyCache& kc = a.keys->gb;
  const int64_t n = a.keys->len;
  GbPlanRec rec{};
  if (REC) {
    unsigned long long* meta = (unsigned long long*)kc.d_plan_meta;
    HF_HIP("gb_radix", hipMemsetAsync(meta, 0, 8, g.stream));
    rec = GbPlanRec{(unsigned short*)kc.d_plan_dst, (unsigned*)kc.d_plan_runs,
                    meta};
  }
  int rc = with_nvals<(REC ? 1 : 2)>(
      REC ? std::min(nvals, 1) : nvals, [&](auto nvTag) {
        constexpr int NV = decltype(nvTag)::value;
        constexpr int BLK = NV < 2 ? GB_PLAN_BLK : 512;
        constexpr int64_t TILE = (int64_t)BLK * GB_PLAN_RPT;
        const uint32_t sgrid =
            gb_tile_grid(((REC ? n : n & ~1LL) + TILE - 1) / TILE);
        const uint32_t lds =
            (uint32_t)(TILE * (8 * NV + 4) + a.nb * 12 + 16);
        return timed_launch(REC ? "gb_plan_record" : "gb_scatter", [&] {
          hipLaunchKernelGGL(
              (k_gb_scatter<NV, GB_PLAN_RPT, BLK, RL, REC>), dim3(sgrid),
              dim3(BLK), lds, g.stream, (const int64_t*)a.keys->dptr,
              (const unsigned*)kc.d_k32, ptrs.vals[0], ptrs.vals[1], n,
              a.key_min, a.n_slots, (int)a.nb, a.d_cur, a.r0, a.r1, a.rk,
              a.d_err, rec);
        });
      });
  if (!REC || rc != HF_OK) return rc;
  unsigned* item0 = (unsigned*)kc.d_plan_item0;
  unsigned* nitems = item0 + a.nb + 1;
  const int64_t ntiles = gb_plan_tiles(n);
  GbTileItem* d_items = (GbTileItem*)kc.d_plan_items;
  rc = timed_launch("gb_plan_items", [&] {
    hipLaunchKernelGGL(k_gb_plan_items<false>, dim3((uint32_t)a.nb), dim3(64),
                       0, g.stream, rec.runs, ntiles, (int)a.nb,
                       gb_item_cut(n), nitems, item0, d_items);
  });
  if (rc != HF_OK) return rc;
  rc = timed_launch("gb_plan_items", [&] {
    hipLaunchKernelGGL(k_gb_plan_items<true>, dim3((uint32_t)a.nb), dim3(64),
                       0, g.stream, rec.runs, ntiles, (int)a.nb,
                       gb_item_cut(n), nitems, item0, d_items);
  });
  if (rc != HF_OK) return rc;
  unsigned total = 0;
  HF_HIP("gb_radix", hipMemcpyAsync(&total, item0 + a.nb, 4,
                                    hipMemcpyDeviceToHost, g.stream));
  HF_HIP("gb_radix", hipStreamSynchronize(g.stream));
  // Dispatch order, costliest item first (cost as in the cut: rows +
  // GB_TILE_COST per tile), so that the kernel's tail is made of its cheapest
  // items; a few hundred to a few thousand items to sort.
  if (total > 0) {
    std::vector<GbTileItem> it(total);
    HF_HIP("gb_radix", hipMemcpyAsync(it.data(), d_items,
                                      total * sizeof(GbTileItem),
                                      hipMemcpyDeviceToHost, g.stream));
    HF_HIP("gb_radix", hipStreamSynchronize(g.stream));
    std::vector<int64_t> cost(total);
    for (unsigned i = 0; i < total; ++i) {
      const bool last = i + 1 == total || it[i + 1].bucket != it[i].bucket;
      const int64_t rows =
          (last ? kc.hist[it[i].bucket] : (int64_t)it[i + 1].row0) -
          it[i].row0;
      cost[i] = rows + GB_TILE_COST * (it[i].tile_end - it[i].tile_begin);
    }
    std::vector<unsigned> ord(total);
    for (unsigned i = 0; i < total; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(),
                     [&](unsigned x, unsigned y) { return cost[x] > cost[y]; });
    HF_HIP("gb_radix", hipMemcpyAsync(kc.d_plan_order, ord.data(), total * 4,
                                      hipMemcpyHostToDevice, g.stream));
    HF_HIP("gb_radix", hipStreamSynchronize(g.stream));
  }
  kc.plan_items_n = total;
  kc.plan_kmin = a.key_min;
  kc.plan_nslots = a.n_slots;
  kc.plan_rl = RL;
  return HF_OK;
}

// The replay writeout uses non-temporal stores unless HF_GB_NT_STORE=0 (read
// once; 1 selects them whatever the default), so both flavours can be
// measured in one build.
bool gb_replay_nt() {
  static const bool nt = [] {
    const char* e = getenv("HF_GB_NT_STORE");
    return e ? e[0] == '1' : GB_REPLAY_NT_DEFAULT;
  }();
  return nt;
}

// P1 on a recorded plan: the value permutation of one column into r0.
int radix_replay(const GbRadixCall& a, const double* v, bool add_err) {
  const GbKeyCache& kc = a.keys->gb;
  const int64_t n = a.keys->len;
  const uint32_t lds = (uint32_t)((int64_t)GB_PLAN_TILE * 8);
  return with_bool(gb_replay_nt(), [&](auto ntTag) {
    return timed_launch("gb_scatter", [&] {
      hipLaunchKernelGGL(
          (k_gb_replay<GB_PLAN_RPT, GB_PLAN_BLK, decltype(ntTag)::value>),
          dim3(gb_tile_grid(gb_plan_tiles(n))), dim3(GB_PLAN_BLK), lds,
          g.stream, (const unsigned short*)kc.d_plan_dst, v, n,
          (const unsigned long long*)kc.d_plan_meta, a.r0, a.d_err,
          add_err ? 1 : 0);
    });
  });
}

// A replayed call that permutes nothing (no value column, or no in-range row
// at all) still has to carry the recorded out-of-range count to the error
// word.
int radix_plan_err(const GbRadixCall& a) {
  return timed_launch("gb_plan_err", [&] {
    hipLaunchKernelGGL(k_gb_plan_err, dim3(1), dim3(64), 0, g.stream,
                       (const unsigned long long*)a.keys->gb.d_plan_meta,
                       a.d_err);
  });
}

// P2 aggregate of one scattered column (or of the keys alone).
template <int RL, int AOP, bool R, bool C, bool V>
int radix_agg(const GbRadixCall& a, const double* v, double* gs,
              unsigned long long* growcnt, unsigned long long* gc) {
  const GbKeyCache& kc = a.keys->gb;
  return with_bool(a.tiled, [&](auto tTag) {
    constexpr bool T = decltype(tTag)::value;
    return timed_launch("gb_bucket_agg", [&] {
      hipLaunchKernelGGL(
          (k_gb_bucket_agg<R, C, V, RL, AOP, false, T>),
          dim3((uint32_t)(T ? kc.plan_items_n : kc.work_n)),
          dim3(gb_p2_block(RL)), 0, g.stream, v, a.rk,
          T ? (const void*)kc.d_plan_items : (const void*)kc.d_work,
          a.n_slots, gs, growcnt, gc, nullptr, nullptr,
          (const unsigned*)kc.d_plan_runs, gb_plan_tiles(a.keys->len),
          (const unsigned*)kc.d_plan_order);
    });
  });
}

// Bucket width (log2) of the radix path for a key range, 0 = range too wide.
// Sum-only uses 8192-key buckets (bigger scatter chunks; the u8-touch agg
// table still fits 2 blocks/CU); count/mean use 4096 (3 blocks/CU with the
// counts table).
// Sum-only calls on more than GB_RL14_ABOVE slots use 16384-key buckets:
// half as many buckets make the write runs of a replay tile twice as long
// (profiles/r09).  Up to that bound 8192-key buckets number at most 32, so a
// 12288-row tile already writes runs of 384 rows and more, where the measured
// run-length curve is flat (3.62 ms at 396 rows, 3.65 at 792).  HF_GB_RL=13
// (read once) keeps 8192-key buckets, for A/B runs inside one build.
constexpr int64_t GB_RL14_ABOVE = 1 << 18;
int gb_radix_rl(int64_t n_slots, bool want_cnt) {
  static const bool rl14_env = [] {
    const char* e = getenv("HF_GB_RL");
    return !(e && strcmp(e, "13") == 0);
  }();
  const int64_t nb13 = (n_slots + (1 << 13) - 1) >> 13;
  const int64_t nb12 = (n_slots + (1 << 12) - 1) >> 12;
  if (!want_cnt && nb13 <= GB_MAX_BUCKETS)
    return (rl14_env && n_slots > GB_RL14_ABOVE) ? 14 : 13;
  return (want_cnt && nb12 <= GB_MAX_BUCKETS) ? 12
         : (nb13 <= GB_MAX_BUCKETS) ? 13 : 0;
}

// with_bool on want-counts.  RL = 14 has no counts instantiation (its LDS
// would not fit) and gb_radix_rl never selects it with counts.
template <int RL, typename F>
int with_cnt(bool cnt, F&& f) {
  if constexpr (RL >= 14) {
    if (cnt)
      return set_err(HF_ERR_UNSUPPORTED, "gb_radix",
                     "16384-slot buckets carry no counts");
    return f(std::false_type{});
  } else {
    return with_bool(cnt, std::forward<F>(f));
  }
}

// The steady state of hf_groupby_reduce on a column whose plan is recorded
// and whose group map is armed: per value column replay -> P2 with the
// partial-table flush -> combine straight into the output column.  No dense
// tables, no memsets, no compaction count/scan, no D2H copy, no sync.  The
// caller has checked that the plan matches (RL, key_min, n_slots); an armed
// map implies a zero recorded out-of-range count, so the error word is not
// touched.
template <int RL, int AOP>
int gb_radix_mapped(hf_col* keys, const GbPtrs& ptrs, int nvals,
                    int64_t key_min, int64_t n_slots, bool want_counts,
                    GroupOut& o) {
  const GbKeyCache& kc = keys->gb;
  const int64_t ng = kc.n_groups;
  int rc = o.keys.alloc(ng, HF_INT64);
  if (rc != HF_OK) return rc;
  if (ng > 0)
    HF_HIP("hf_groupby_reduce",
           hipMemcpyAsync(o.keys.data<void>(), kc.d_gkeys, ng * 8,
                          hipMemcpyDeviceToDevice, g.stream));
  if (nvals == 0) return HF_OK;
  constexpr int64_t RANGE = 1 << RL;
  const int64_t nb = (n_slots + RANGE - 1) >> RL;
  // one partial buffer serves every value column in turn, like r0
  DevBuf r0, part_sums, part_cnt;
  HF_HIP("hf_groupby_reduce", r0.alloc(gb_plan_rows(keys->len) * 8));
  HF_HIP("hf_groupby_reduce", part_sums.alloc(kc.plan_items_n * RANGE * 8));
  if (want_counts)
    HF_HIP("hf_groupby_reduce", part_cnt.alloc(kc.plan_items_n * RANGE * 4));
  const GbRadixCall a{keys, nb, key_min, n_slots, nullptr, r0.as<double>(),
                      nullptr, (unsigned short*)kc.d_plan_rk, nullptr, true};
  for (int c = 0; c < nvals; ++c) {
    rc = o.sums[c].alloc(ng, HF_FLOAT64);
    if (rc == HF_OK && want_counts) rc = o.cnts[c].alloc(ng, HF_INT64);
    if (rc == HF_OK) rc = radix_replay(a, ptrs.vals[c], false);
    if (rc != HF_OK) return rc;
    rc = with_cnt<RL>(want_counts, [&](auto cTag) {
      constexpr bool C = decltype(cTag)::value;
      int r = timed_launch("gb_bucket_agg", [&] {
        hipLaunchKernelGGL(
            (k_gb_bucket_agg<false, C, true, RL, AOP, true, true>),
            dim3((uint32_t)kc.plan_items_n), dim3(gb_p2_block(RL)), 0,
            g.stream, a.r0, a.rk, (const void*)kc.d_plan_items, n_slots,
            nullptr, nullptr, nullptr, part_sums.as<double>(),
            part_cnt.as<unsigned>(), (const unsigned*)kc.d_plan_runs,
            gb_plan_tiles(keys->len), (const unsigned*)kc.d_plan_order);
      });
      if (r != HF_OK) return r;
      // the compaction of this path, so it keeps that stat name
      return timed_launch("gb_compact_scatter", [&] {
        hipLaunchKernelGGL(
            (k_gb_combine<RL, AOP, C>),
            dim3((uint32_t)((n_slots + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
            g.stream, (const unsigned*)kc.d_gidx,
            (const unsigned*)kc.d_plan_item0,
            part_sums.as<double>(), part_cnt.as<unsigned>(), n_slots,
            o.sums[c].data<double>(),
            C ? o.cnts[c].data<int64_t>() : nullptr);
      });
    });
    if (rc != HF_OK) return rc;
  }
  return HF_OK;
}

// The radix groupby driver: plan mode -> (layout) -> P1 -> per column
// (replay?) -> P2.  The region layout is built only for the plan-less path.
// Every temporary is scoped, so any early return gives its blocks back to the
// allocator.
template <int RL, int AOP>
int gb_radix_path(hf_col* keys, const GbPtrs& ptrs, int nvals, int64_t key_min,
                  int64_t n_slots, uintptr_t sums, uintptr_t rowcnt,
                  uintptr_t counts, unsigned long long* d_err,
                  bool with_rowcnt = true) {
  GbKeyCache& kc = keys->gb;
  const int64_t nb = (n_slots + (1 << RL) - 1) >> RL;
  int rc = ensure_host_hist(keys, key_min, n_slots, nb, RL);
  if (rc != HF_OK) return rc;
  const GbPlan mode = ensure_plan(keys, RL, key_min, n_slots, nb);
  if (mode == GbPlan::None) {
    rc = ensure_radix_layout<RL>(keys, nb);
    if (rc != HF_OK) return rc;
    rc = ensure_keys32(keys, key_min);
    if (rc != HF_OK) return rc;
  }
  const int64_t rows = mode == GbPlan::None ? radix_alloc_rows(kc)
                                            : gb_plan_rows(keys->len);
  DevBuf r0, r1, rk, d_cur;
  if (nvals > 0) HF_HIP("gb_radix", r0.alloc(rows * 8));
  if (mode == GbPlan::None) {
    if (nvals > 1) HF_HIP("gb_radix", r1.alloc(rows * 8));
    HF_HIP("gb_radix", rk.alloc(rows * 2));
    HF_HIP("gb_radix", d_cur.alloc(nb * 4));
    HF_HIP("gb_radix", hipMemcpyAsync(d_cur.as<void>(), kc.d_curinit, nb * 4,
                                      hipMemcpyDeviceToDevice, g.stream));
  }
  const GbRadixCall a{keys, nb, key_min, n_slots, d_err, r0.as<double>(),
                      r1.as<double>(),
                      mode == GbPlan::None ? rk.as<unsigned short>()
                                           : (unsigned short*)kc.d_plan_rk,
                      d_cur.as<unsigned>(), mode != GbPlan::None};
  // P1 (a replayed plan permutes per column, in the P2 loop below)
  if (mode == GbPlan::None)
    rc = radix_scatter<RL, false>(a, ptrs, nvals);
  else if (mode == GbPlan::Record)
    rc = radix_scatter<RL, true>(a, ptrs, nvals);
  const int64_t work_n = a.tiled ? kc.plan_items_n : kc.work_n;
  if (rc == HF_OK && mode == GbPlan::Replay && (nvals == 0 || work_n == 0))
    rc = radix_plan_err(a);
  if (rc != HF_OK || work_n == 0) return rc;
  // P2 aggregate, one column per launch
  unsigned long long* growcnt = (unsigned long long*)rowcnt;
  if (nvals == 0)
    return radix_agg<RL, AOP, true, false, false>(a, nullptr, nullptr, growcnt,
                                                  nullptr);
  const bool cnt = counts != 0;
  for (int c = 0; c < nvals; ++c) {
    // plan path: replay(column) -> agg(column) through the one r0; the
    // record pass has already scattered column 0
    if (mode == GbPlan::Replay || (mode == GbPlan::Record && c > 0)) {
      rc = radix_replay(a, ptrs.vals[c], mode == GbPlan::Replay && c == 0);
      if (rc != HF_OK) return rc;
    }
    const double* v = (c == 0 || mode != GbPlan::None) ? a.r0 : a.r1;
    double* gs = (double*)sums + (int64_t)c * n_slots;
    unsigned long long* gc =
        cnt ? (unsigned long long*)counts + (int64_t)c * n_slots : nullptr;
    rc = with_bool(c == 0 && with_rowcnt, [&](auto rTag) {
      return with_cnt<RL>(cnt, [&](auto cTag) {
        return radix_agg<RL, AOP, decltype(rTag)::value,
                         decltype(cTag)::value, true>(a, v, gs, growcnt, gc);
      });
    });
    if (rc != HF_OK) return rc;
  }
  return HF_OK;
}

}  // namespace

extern "C" {

int hf_groupby_accum(const hf_col* keys, const hf_col* const* vals, int nvals,
                     int agg_op, int64_t key_min, int64_t n_slots,
                     uintptr_t sums, uintptr_t rowcnt, uintptr_t counts) {
  HF_NEED_INIT("hf_groupby_accum");
  if (!keys || !vals || nvals < 0 || nvals > GB_MAX_VALS)
    return set_err(HF_ERR_ARG, "hf_groupby_accum", "bad args (nvals<=8)");
  if (agg_op < HF_AGG_SUM || agg_op > HF_AGG_MAX)
    return set_err(HF_ERR_ARG, "hf_groupby_accum", "bad agg_op");
  if (keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_groupby_accum", "keys must be int64");
  if (n_slots <= 0) return set_err(HF_ERR_ARG, "hf_groupby_accum", "n_slots<=0");
  GbPtrs ptrs{};
  for (int c = 0; c < nvals; ++c) {
    if (!vals[c] || vals[c]->dtype != HF_FLOAT64 || vals[c]->len != keys->len)
      return set_err(HF_ERR_ARG, "hf_groupby_accum",
                     "vals must be float64 columns of keys' length");
    ptrs.vals[c] = (const double*)vals[c]->dptr;
  }
  const int64_t n = keys->len;
  unsigned long long* d_err = scratch_at(SCRATCH_GB_ERR);
  // path selection (DESIGN.md §GroupBy kernels): LDS-dense for small ranges,
  // radix partition for the north-star range, global atomics as the wide
  // fallback (slow but correct for any range below the slot cap)
  auto route = [&](auto aopTag) -> int {
    constexpr int AOP = decltype(aopTag)::value;
    if (n > 0 && n_slots <= GB_DENSE_MAX)
      return gb_dense_path<AOP>(keys, ptrs, nvals, key_min, n_slots, sums,
                                rowcnt, counts, d_err);
    const int rl_ok = gb_radix_rl(n_slots, counts != 0);
    if (n > 0 && rl_ok) {
      // wide frames run the radix path in chunks of 2 value columns
      // (re-reading keys per chunk still beats the atomic fallback ~5x)
      int rc2 = HF_OK;
      for (int c0 = 0; c0 < (nvals ? nvals : 1) && rc2 == HF_OK; c0 += 2) {
        GbPtrs sub{};
        const int nv = nvals == 0 ? 0 : std::min(2, nvals - c0);
        for (int c = 0; c < nv; ++c) sub.vals[c] = ptrs.vals[c0 + c];
        const uintptr_t ssub = sums + (uintptr_t)c0 * n_slots * 8;
        const uintptr_t csub =
            counts ? counts + (uintptr_t)c0 * n_slots * 8 : 0;
        auto radix = [&](auto rlTag) {
          return gb_radix_path<decltype(rlTag)::value, AOP>(
              const_cast<hf_col*>(keys), sub, nv, key_min, n_slots, ssub,
              rowcnt, csub, d_err, c0 == 0);
        };
        rc2 = with_rl(rl_ok, radix);
        if (nvals == 0) break;
      }
      return rc2;
    }
    return -1;  // fall through to the atomic path
  };
  int routed = with_aop(agg_op, route);
  if (routed != -1) return routed;
  return with_nvals<GB_MAX_VALS>(nvals, [&](auto nvTag) {
    return with_bool(counts != 0, [&](auto cntTag) {
      return with_aop(agg_op, [&](auto aopTag) {
        return timed_launch("gb_accum", [&] {
          hipLaunchKernelGGL((k_gb_accum<decltype(nvTag)::value,
                                         decltype(cntTag)::value,
                                         decltype(aopTag)::value>),
                             dim3(grid_for((n >> 1) + 1)), dim3(BLOCK), 0,
                             g.stream, (const int64_t*)keys->dptr, ptrs, n,
                             key_min, n_slots, (double*)sums,
                             (unsigned long long*)rowcnt,
                             (unsigned long long*)counts, d_err);
        });
      });
    });
  });
}

int hf_group_moments(const hf_col* gid, const hf_col* val, uintptr_t centre,
                     int64_t n_groups, uintptr_t table) {
  HF_NEED_INIT("hf_group_moments");
  if (!val || val->dtype != HF_FLOAT64 || !centre || !table)
    return set_err(HF_ERR_ARG, "hf_group_moments",
                   "val must be float64; centre/table must be non-null");
  if (n_groups <= 0)
    return set_err(HF_ERR_ARG, "hf_group_moments", "n_groups<=0");
  if (gid && (gid->dtype != HF_INT64 || gid->len != val->len))
    return set_err(HF_ERR_ARG, "hf_group_moments",
                   "gid must be an int64 column of val's length");
  if (!gid && n_groups != 1)
    return set_err(HF_ERR_ARG, "hf_group_moments",
                   "a null gid means one group (n_groups must be 1)");
  const int64_t n = val->len;
  if (n == 0) return HF_OK;
  const double* d_val = (const double*)val->dptr;
  const double* d_c = (const double*)centre;
  double* d_tab = (double*)table;
  if (!gid) {
    int64_t grid = grid_for((n >> 1) + 1);
    if (grid > 1024) grid = 1024;  // six same-address atomics per block
    return timed_launch("gm_one", [&] {
      hipLaunchKernelGGL(k_gm_one, dim3((uint32_t)grid), dim3(BLOCK), 0,
                         g.stream, d_val, n, d_c, d_tab);
    });
  }
  unsigned long long* d_err = scratch_at(SCRATCH_GM_ERR);
  HF_HIP("hf_group_moments", hipMemsetAsync(d_err, 0, 8, g.stream));
  const int64_t* d_gid = (const int64_t*)gid->dptr;
  int rc;
  if (n_groups <= GM_LDS_MAX) {
    int64_t grid = n / 65536 + 1;
    if (grid > 512) grid = 512;
    const uint32_t lds = (uint32_t)(n_groups * ((GM_ROWS + 1) * 8 + 1));
    rc = timed_launch("gm_lds", [&] {
      hipLaunchKernelGGL(k_gm_lds, dim3((uint32_t)grid), dim3(512), lds,
                         g.stream, d_gid, d_val, n, d_c, n_groups, d_tab,
                         d_err);
    });
  } else {
    rc = timed_launch("gm_global", [&] {
      hipLaunchKernelGGL(k_gm_global, dim3((uint32_t)grid_for((n >> 1) + 1)),
                         dim3(BLOCK), 0, g.stream, d_gid, d_val, n, d_c,
                         n_groups, d_tab, d_err);
    });
  }
  if (rc != HF_OK) return rc;
  unsigned long long h_err = 0;
  HF_HIP("hf_group_moments",
         hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_group_moments", hipStreamSynchronize(g.stream));
  if (h_err)
    return set_err(HF_ERR_ARG, "hf_group_moments",
                   "gid >= n_groups (rows were not accumulated)");
  return HF_OK;
}

// The body of hf_groupby_compact.  gidx (u32[n_slots], may be null) also
// receives the group map of this compaction: slot -> output row, from the
// rowcnt table and tile offsets at hand.
static int gb_compact(uintptr_t sums, uintptr_t rowcnt, uintptr_t counts,
                      int nvals, int64_t key_min, int64_t n_slots,
                      hf_col** out_keys, hf_col** out_sums,
                      hf_col** out_counts, int64_t* n_groups, unsigned* gidx) {
  HF_NEED_INIT("hf_groupby_compact");
  if (!rowcnt || nvals < 0 || nvals > GB_MAX_VALS || !out_keys || !n_groups)
    return set_err(HF_ERR_ARG, "hf_groupby_compact", "bad args");
  const int64_t ntiles = (n_slots + COMPACT_TILE - 1) / COMPACT_TILE;
  // check the accumulate-phase error word
  unsigned long long h_err = 0;
  unsigned long long* d_err = scratch_at(SCRATCH_GB_ERR);
  HF_HIP("hf_groupby_compact",
         hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost, g.stream));
  // tile counts
  DevBuf tiles_buf;
  HF_HIP("hf_groupby_compact", tiles_buf.alloc((ntiles + 1) * 8));
  int64_t* d_tiles = tiles_buf.as<int64_t>();
  int64_t* d_total = scratch_at<int64_t>(SCRATCH_NGROUPS);
  int rc = timed_launch("gb_compact_count", [&] {
    hipLaunchKernelGGL(k_compact_count, dim3((uint32_t)ntiles), dim3(BLOCK), 0,
                       g.stream, (const unsigned long long*)rowcnt, n_slots, d_tiles);
  });
  if (rc != HF_OK) return rc;
  rc = timed_launch("gb_compact_scan", [&] {
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, g.stream, d_tiles,
                       ntiles, d_total);
  });
  if (rc != HF_OK) return rc;
  int64_t total = 0;
  HF_HIP("hf_groupby_compact",
         hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_groupby_compact", hipStreamSynchronize(g.stream));
  if (h_err != 0) {
    char buf[128];
    snprintf(buf, sizeof buf,
             "%llu keys fell outside [key_min, key_min+n_slots) during accumulate",
             h_err);
    hipMemsetAsync(d_err, 0, 8, g.stream);
    return set_err(HF_ERR_ARG, "hf_groupby_compact", buf);
  }
  // allocate outputs
  const bool want_counts = counts && out_counts;
  GroupOut o(nvals, want_counts);
  rc = o.keys.alloc(total, HF_INT64);
  if (rc != HF_OK) return rc;
  std::vector<double*> h_sum_ptrs(nvals ? nvals : 1);
  std::vector<int64_t*> h_cnt_ptrs(nvals ? nvals : 1);
  for (int c = 0; c < nvals; ++c) {
    rc = o.sums[c].alloc(total, HF_FLOAT64);
    if (rc != HF_OK) return rc;
    h_sum_ptrs[c] = o.sums[c].data<double>();
    if (want_counts) {
      rc = o.cnts[c].alloc(total, HF_INT64);
      if (rc != HF_OK) return rc;
      h_cnt_ptrs[c] = o.cnts[c].data<int64_t>();
    }
  }
  // ship the per-column output pointer arrays to the device
  DevBuf sum_ptrs_buf, cnt_ptrs_buf;
  HF_HIP("hf_groupby_compact",
         sum_ptrs_buf.alloc(sizeof(double*) * (nvals ? nvals : 1)));
  HF_HIP("hf_groupby_compact",
         cnt_ptrs_buf.alloc(sizeof(int64_t*) * (nvals ? nvals : 1)));
  double** d_sum_ptrs = sum_ptrs_buf.as<double*>();
  int64_t** d_cnt_ptrs = cnt_ptrs_buf.as<int64_t*>();
  HF_HIP("hf_groupby_compact",
         hipMemcpyAsync(d_sum_ptrs, h_sum_ptrs.data(), sizeof(double*) * nvals,
                        hipMemcpyHostToDevice, g.stream));
  if (want_counts)
    HF_HIP("hf_groupby_compact",
           hipMemcpyAsync(d_cnt_ptrs, h_cnt_ptrs.data(), sizeof(int64_t*) * nvals,
                          hipMemcpyHostToDevice, g.stream));
  rc = with_bool(want_counts, [&](auto cTag) {
    return timed_launch("gb_compact_scatter", [&] {
      hipLaunchKernelGGL(k_compact_scatter<decltype(cTag)::value>,
                         dim3((uint32_t)ntiles), dim3(BLOCK), 0, g.stream,
                         (const double*)sums, (const unsigned long long*)rowcnt,
                         (const unsigned long long*)counts, nvals, key_min,
                         n_slots, d_tiles, o.keys.data<int64_t>(), d_sum_ptrs,
                         d_cnt_ptrs);
    });
  });
  if (rc != HF_OK) return rc;
  if (gidx) {
    rc = timed_launch("gb_gidx", [&] {
      hipLaunchKernelGGL(k_gb_gidx, dim3((uint32_t)ntiles), dim3(BLOCK), 0,
                         g.stream, (const unsigned long long*)rowcnt, n_slots,
                         d_tiles, gidx);
    });
    if (rc != HF_OK) return rc;
  }
  o.commit(out_keys, out_sums, out_counts);
  *n_groups = total;
  return HF_OK;
}

int hf_groupby_compact(uintptr_t sums, uintptr_t rowcnt, uintptr_t counts,
                       int nvals, int64_t key_min, int64_t n_slots,
                       hf_col** out_keys, hf_col** out_sums, hf_col** out_counts,
                       int64_t* n_groups) {
  return gb_compact(sums, rowcnt, counts, nvals, key_min, n_slots, out_keys,
                    out_sums, out_counts, n_groups, nullptr);
}

int hf_groupby_radix_rl(int64_t n_slots, int want_counts) {
  return n_slots > 0 ? gb_radix_rl(n_slots, want_counts != 0) : 0;
}

int hf_groupby_reduce(const hf_col* keys, const hf_col* const* vals, int nvals,
                      int agg_op, int want_counts, int64_t key_min,
                      int64_t n_slots, hf_col** out_keys, hf_col** out_sums,
                      hf_col** out_counts, int64_t* n_groups) {
  HF_NEED_INIT("hf_groupby_reduce");
  if (!keys || !vals || nvals < 0 || nvals > GB_MAX_VALS || !out_keys ||
      !n_groups || (nvals > 0 && !out_sums) || (want_counts && !out_counts))
    return set_err(HF_ERR_ARG, "hf_groupby_reduce", "bad args (nvals<=8)");
  if (agg_op < HF_AGG_SUM || agg_op > HF_AGG_MAX)
    return set_err(HF_ERR_ARG, "hf_groupby_reduce", "bad agg_op");
  if (keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_groupby_reduce", "keys must be int64");
  if (n_slots <= 0)
    return set_err(HF_ERR_ARG, "hf_groupby_reduce", "n_slots<=0");
  GbPtrs ptrs{};
  for (int c = 0; c < nvals; ++c) {
    if (!vals[c] || vals[c]->dtype != HF_FLOAT64 || vals[c]->len != keys->len)
      return set_err(HF_ERR_ARG, "hf_groupby_reduce",
                     "vals must be float64 columns of keys' length");
    ptrs.vals[c] = (const double*)vals[c]->dptr;
  }
  hf_col* kcol = const_cast<hf_col*>(keys);
  GbKeyCache& kc = kcol->gb;
  const bool cnt = want_counts != 0;
  // the route hf_groupby_accum takes for this call, and the plan it would find
  const int rl = (keys->len > 0 && n_slots > GB_DENSE_MAX)
                     ? gb_radix_rl(n_slots, cnt) : 0;
  const bool plan_ok = rl != 0 && kc.plan_rl == rl &&
                       kc.plan_kmin == key_min && kc.plan_nslots == n_slots;
  if (plan_ok && kc.d_gidx) {
    GroupOut o(nvals, cnt);
    const int rc = with_aop(agg_op, [&](auto aopTag) {
      return with_rl(rl, [&](auto rlTag) {
        return gb_radix_mapped<decltype(rlTag)::value,
                               decltype(aopTag)::value>(
            kcol, ptrs, nvals, key_min, n_slots, cnt, o);
      });
    });
    if (rc != HF_OK) return rc;
    o.commit(out_keys, out_sums, out_counts);
    *n_groups = kc.n_groups;
    return HF_OK;
  }
  // every other case: dense tables of this call's own, then the two-call path
  const int64_t tab = (int64_t)(nvals ? nvals : 1) * n_slots;
  DevBuf sums, rowcnt, counts, gidx;
  HF_HIP("hf_groupby_reduce", sums.alloc(tab * 8));
  HF_HIP("hf_groupby_reduce", rowcnt.alloc(n_slots * 8));
  if (cnt) HF_HIP("hf_groupby_reduce", counts.alloc(tab * 8));
  int rc = HF_OK;
  if (agg_op == HF_AGG_SUM)
    HF_HIP("hf_groupby_reduce",
           hipMemsetAsync(sums.as<void>(), 0, tab * 8, g.stream));
  else
    rc = hf_fill_f64((uintptr_t)sums.as<void>(),
                     agg_op == HF_AGG_MIN ? INFINITY : -INFINITY, tab);
  if (rc != HF_OK) return rc;
  HF_HIP("hf_groupby_reduce",
         hipMemsetAsync(rowcnt.as<void>(), 0, n_slots * 8, g.stream));
  if (cnt)
    HF_HIP("hf_groupby_reduce",
           hipMemsetAsync(counts.as<void>(), 0, tab * 8, g.stream));
  rc = hf_groupby_accum(keys, vals, nvals, agg_op, key_min, n_slots,
                        (uintptr_t)sums.as<void>(),
                        (uintptr_t)rowcnt.as<void>(),
                        (uintptr_t)counts.as<void>());
  if (rc != HF_OK) return rc;
  // arm the group map when this call ran on a valid recorded plan; a failed
  // map allocation only leaves the column on this path
  const bool arm = rl != 0 && kc.plan_rl == rl && kc.plan_kmin == key_min &&
                   kc.plan_nslots == n_slots && kc.plan_items_n > 0 && !kc.d_gidx;
  if (arm && gidx.alloc(n_slots * 4) != hipSuccess) (void)hipGetLastError();
  hf_col* okeys = nullptr;
  rc = gb_compact((uintptr_t)sums.as<void>(), (uintptr_t)rowcnt.as<void>(),
                  (uintptr_t)counts.as<void>(), nvals, key_min, n_slots,
                  &okeys, out_sums, out_counts, n_groups, gidx.as<unsigned>());
  if (rc != HF_OK) return rc;  // a nonzero error word lands here: never armed
  *out_keys = okeys;
  if (gidx.as<void>() && *n_groups > 0) {
    DevBuf gkeys;
    if (gkeys.alloc(*n_groups * 8) != hipSuccess) {
      (void)hipGetLastError();
    } else if (hipMemcpyAsync(gkeys.as<void>(), okeys->dptr, *n_groups * 8,
                              hipMemcpyDeviceToDevice, g.stream) ==
               hipSuccess) {
      kc.d_gidx = gidx.release();
      kc.d_gkeys = gkeys.release();
      kc.n_groups = *n_groups;
    }
  }
  return HF_OK;
}

int hf_col_concat(const hf_col* const* cols, int ncols, hf_col** out) {
  HF_NEED_INIT("hf_col_concat");
  if (!cols || ncols <= 0 || !out)
    return set_err(HF_ERR_ARG, "hf_col_concat", "bad args");
  const int dt = cols[0]->dtype;
  int64_t total = 0;
  for (int i = 0; i < ncols; ++i) {
    if (!cols[i] || cols[i]->dtype != dt)
      return set_err(HF_ERR_ARG, "hf_col_concat", "dtype mismatch");
    total += cols[i]->len;
  }
  ColOut o;
  int rc = o.alloc(total, dt);
  if (rc != HF_OK) return rc;
  char* dst = o.data<char>();
  const int64_t esz = dtype_size(dt);
  for (int i = 0; i < ncols; ++i) {
    const int64_t bytes = cols[i]->len * esz;
    if (bytes > 0)
      HF_HIP("hf_col_concat",
             hipMemcpyAsync(dst, cols[i]->dptr, bytes,
                            hipMemcpyDeviceToDevice, g.stream));
    dst += bytes;
  }
  o.commit(out);
  return HF_OK;
}

int hf_fill_i64(uintptr_t dptr, int64_t value, int64_t n) {
  HF_NEED_INIT("hf_fill_i64");
  if (n <= 0) return HF_OK;
  return timed_launch("fill_i64", [&] {
    hipLaunchKernelGGL(k_fill_i64, dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0,
                       g.stream, (int64_t*)dptr, value, n);
  });
}

int hf_fill_randint(hf_col* col, uint64_t seed, int64_t lo, int64_t hi) {
  HF_NEED_INIT("hf_fill_randint");
  if (!col || col->dtype != HF_INT64 || hi <= lo)
    return set_err(HF_ERR_ARG, "hf_fill_randint", "int64 col, hi > lo");
  if (col->len == 0) return HF_OK;
  return timed_launch("fill_randint", [&] {
    hipLaunchKernelGGL(k_fill_randint, dim3((uint32_t)grid_for(col->len)),
                       dim3(BLOCK), 0, g.stream, (int64_t*)col->dptr,
                       col->len, seed, lo, (uint64_t)(hi - lo));
  });
}

int hf_fill_randf64(hf_col* col, uint64_t seed) {
  HF_NEED_INIT("hf_fill_randf64");
  if (!col || col->dtype != HF_FLOAT64)
    return set_err(HF_ERR_ARG, "hf_fill_randf64", "float64 col");
  if (col->len == 0) return HF_OK;
  return timed_launch("fill_randf64", [&] {
    hipLaunchKernelGGL(k_fill_randf64, dim3((uint32_t)grid_for(col->len)),
                       dim3(BLOCK), 0, g.stream, (double*)col->dptr,
                       col->len, seed);
  });
}

int hf_fill_randcdf(hf_col* col, uint64_t seed, const hf_col* cdf) {
  HF_NEED_INIT("hf_fill_randcdf");
  if (!col || col->dtype != HF_INT64 || !cdf || cdf->dtype != HF_FLOAT64 ||
      cdf->len <= 0)
    return set_err(HF_ERR_ARG, "hf_fill_randcdf",
                   "int64 col, non-empty float64 cdf");
  if (col->len == 0) return HF_OK;
  return timed_launch("fill_randcdf", [&] {
    hipLaunchKernelGGL(k_fill_randcdf, dim3((uint32_t)grid_for(col->len)),
                       dim3(BLOCK), 0, g.stream, (int64_t*)col->dptr,
                       col->len, seed, (const double*)cdf->dptr, cdf->len);
  });
}

int hf_groupby_hash_accum(const hf_col* keys, const hf_col* const* vals,
                          int nvals, int agg_op, int64_t H,
                          uintptr_t tkey, uintptr_t sums, uintptr_t rowcnt,
                          uintptr_t counts) {
  HF_NEED_INIT("hf_groupby_hash_accum");
  if (!keys || nvals < 0 || nvals > GB_MAX_VALS || H < 2 || (H & (H - 1)))
    return set_err(HF_ERR_ARG, "hf_groupby_hash_accum",
                   "bad args (H power of 2, nvals<=8)");
  if (keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_groupby_hash_accum", "keys must be int64");
  GbPtrs ptrs{};
  for (int c = 0; c < nvals; ++c) {
    if (!vals[c] || vals[c]->dtype != HF_FLOAT64 || vals[c]->len != keys->len)
      return set_err(HF_ERR_ARG, "hf_groupby_hash_accum",
                     "vals must be float64 columns of keys' length");
    ptrs.vals[c] = (const double*)vals[c]->dptr;
  }
  const int64_t n = keys->len;
  if (n == 0) return HF_OK;
  unsigned long long* d_full = scratch_at(SCRATCH_HASH_FULL);
  return with_nvals<GB_MAX_VALS>(nvals, [&](auto nvTag) {
    return with_bool(counts != 0, [&](auto cTag) {
      return with_aop(agg_op, [&](auto aTag) {
        return timed_launch("gb_hash_accum", [&] {
          hipLaunchKernelGGL((k_gb_hash_accum<decltype(nvTag)::value,
                                              decltype(cTag)::value,
                                              decltype(aTag)::value>),
                             dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0,
                             g.stream, (const int64_t*)keys->dptr, ptrs, n, H,
                             (long long*)tkey, (double*)sums,
                             (unsigned long long*)rowcnt,
                             (unsigned long long*)counts, d_full);
        });
      });
    });
  });
}

int hf_groupby_hash_compact(uintptr_t tkey, uintptr_t sums, uintptr_t rowcnt,
                            uintptr_t counts, int nvals, int64_t H,
                            hf_col** out_keys, hf_col** out_sums,
                            hf_col** out_counts, int64_t* n_groups) {
  HF_NEED_INIT("hf_groupby_hash_compact");
  if (!tkey || !rowcnt || nvals < 0 || nvals > GB_MAX_VALS || !out_keys ||
      !n_groups)
    return set_err(HF_ERR_ARG, "hf_groupby_hash_compact", "bad args");
  // surface "table full" from the accumulate phase
  unsigned long long h_full = 0;
  unsigned long long* d_full = scratch_at(SCRATCH_HASH_FULL);
  HF_HIP("hf_groupby_hash_compact",
         hipMemcpyAsync(&h_full, d_full, 8, hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_groupby_hash_compact", hipStreamSynchronize(g.stream));
  if (h_full) {
    hipMemsetAsync(d_full, 0, 8, g.stream);
    return set_err(HF_ERR_UNSUPPORTED, "hf_groupby_hash_compact",
                   "hash table full — retry with a larger H");
  }
  const int64_t L = H + 1;
  const int gpu = g.gpu;
  // filter present slots (rowcnt doubles as the nonzero mask)
  hf_col mask_view{(void*)rowcnt, L, HF_INT64, gpu};
  const bool want_counts = counts && out_counts;
  ColOut ckeys;
  std::vector<ColOut> csums(nvals), ccnts(counts ? nvals : 0);
  int64_t kept = 0;
  {
    hf_filterplan* plan = nullptr;
    int rc = hf_filter_plan(&mask_view, &plan, &kept);
    if (rc != HF_OK) return rc;
    const PlanOwner plan_owner(plan, hf_filter_plan_free);
    hf_col tkey_view{(void*)tkey, L, HF_INT64, gpu};
    rc = hf_filter_apply(plan, &tkey_view, ckeys.slot());
    for (int c = 0; c < nvals && rc == HF_OK; ++c) {
      hf_col sv{(char*)sums + (int64_t)c * L * 8, L, HF_FLOAT64, gpu};
      rc = hf_filter_apply(plan, &sv, csums[c].slot());
      if (rc == HF_OK && counts) {
        hf_col cv{(char*)counts + (int64_t)c * L * 8, L, HF_INT64, gpu};
        rc = hf_filter_apply(plan, &cv, ccnts[c].slot());
      }
    }
    if (rc != HF_OK) return rc;
  }
  // sort surviving keys (wide radix handles any int64 range) and gather
  ColOut perm;
  GroupOut o(nvals, want_counts);
  int rc = hf_sort_perm(ckeys.get(), 1, perm.slot());
  if (rc == HF_OK) rc = hf_gather(ckeys.get(), perm.get(), o.keys.slot());
  for (int c = 0; c < nvals && rc == HF_OK; ++c) {
    rc = hf_gather(csums[c].get(), perm.get(), o.sums[c].slot());
    if (rc == HF_OK && want_counts)
      rc = hf_gather(ccnts[c].get(), perm.get(), o.cnts[c].slot());
  }
  if (rc != HF_OK) return rc;
  o.commit(out_keys, out_sums, out_counts);
  *n_groups = kept;
  return HF_OK;
}

static const int64_t* plan_tiles(const hf_filterplan* p);

int hf_cumsum(const hf_col* col, int agg_op, hf_col** out) {
  HF_NEED_INIT("hf_cumsum");
  if (!col || !out) return set_err(HF_ERR_ARG, "hf_cumsum", "null");
  if (agg_op != HF_AGG_SUM && agg_op != HF_AGG_MIN &&
      agg_op != HF_AGG_MAX && agg_op != HF_AGG_PROD)
    return set_err(HF_ERR_ARG, "hf_cumsum", "bad agg_op");
  const int64_t n = col->len;
  ColOut o;
  int rc = o.alloc(n, col->dtype);
  if (rc != HF_OK) return rc;
  if (n == 0) { o.commit(out); return HF_OK; }
  const int64_t ntiles = (n + FILT_TILE - 1) / FILT_TILE;
  DevBuf ts;  // per-tile scan state; 16 B holds the f64 product's pair
  HF_HIP("hf_cumsum", ts.alloc(ntiles * sizeof(cs_dd)));
  rc = with_scan_op(agg_op, [&](auto opTag) {
    return with_dtype(col->dtype, [&](auto tTag) -> int {
      using T = decltype(tTag);
      constexpr int OP = decltype(opTag)::value;
      using S = typename cs_state<T, OP>::type;
      int r2 = timed_launch("cumsum_tiles", [&] {
        hipLaunchKernelGGL((k_cumsum_tiles<T, OP>), dim3((uint32_t)ntiles),
                           dim3(BLOCK), 0, g.stream, (const T*)col->dptr, n,
                           ts.as<S>());
      });
      if (r2 != HF_OK) return r2;
      r2 = timed_launch("cumsum_scan", [&] {
        hipLaunchKernelGGL((k_cumsum_scan_tiles<T, OP>), dim3(1), dim3(1024),
                           0, g.stream, ts.as<S>(), ntiles);
      });
      if (r2 != HF_OK) return r2;
      return timed_launch("cumsum_apply", [&] {
        hipLaunchKernelGGL((k_cumsum_apply<T, OP>), dim3((uint32_t)ntiles),
                           dim3(BLOCK), 0, g.stream, (const T*)col->dptr, n,
                           (const S*)ts.as<S>(), o.data<T>());
      });
    });
  });
  return o.commit_if(rc, out);
}

int hf_seg_cumsum(const hf_col* col, const hf_col* heads, int agg_op,
                  hf_col** out) {
  HF_NEED_INIT("hf_seg_cumsum");
  if (!col || !heads || !out)
    return set_err(HF_ERR_ARG, "hf_seg_cumsum", "null");
  if (heads->dtype != HF_INT64 || heads->len != col->len)
    return set_err(HF_ERR_ARG, "hf_seg_cumsum",
                   "heads must be an int64 0/1 column of the same length");
  if (agg_op != HF_AGG_SUM && agg_op != HF_AGG_MIN &&
      agg_op != HF_AGG_MAX && agg_op != HF_AGG_PROD)
    return set_err(HF_ERR_ARG, "hf_seg_cumsum", "bad agg_op");
  const int64_t n = col->len;
  ColOut o;
  int rc = o.alloc(n, col->dtype);
  if (rc != HF_OK) return rc;
  if (n == 0) { o.commit(out); return HF_OK; }
  const int64_t ntiles = (n + FILT_TILE - 1) / FILT_TILE;
  DevBuf tv, tf;
  HF_HIP("hf_seg_cumsum", tv.alloc(ntiles * sizeof(cs_dd)));
  HF_HIP("hf_seg_cumsum", tf.alloc(ntiles * 4));
  rc = with_scan_op(agg_op, [&](auto opTag) {
    return with_dtype(col->dtype, [&](auto tTag) -> int {
      using T = decltype(tTag);
      constexpr int OP = decltype(opTag)::value;
      using S = typename cs_state<T, OP>::type;
      int r2 = timed_launch("seg_tiles", [&] {
        hipLaunchKernelGGL((k_seg_tiles<T, OP>), dim3((uint32_t)ntiles),
                           dim3(BLOCK), 0, g.stream, (const T*)col->dptr,
                           (const int64_t*)heads->dptr, n, tv.as<S>(),
                           tf.as<unsigned>());
      });
      if (r2 != HF_OK) return r2;
      r2 = timed_launch("seg_scan", [&] {
        hipLaunchKernelGGL((k_seg_scan_tiles<T, OP>), dim3(1), dim3(1024),
                           0, g.stream, tv.as<S>(), tf.as<unsigned>(), ntiles);
      });
      if (r2 != HF_OK) return r2;
      return timed_launch("seg_apply", [&] {
        hipLaunchKernelGGL((k_seg_apply<T, OP>), dim3((uint32_t)ntiles),
                           dim3(BLOCK), 0, g.stream, (const T*)col->dptr,
                           (const int64_t*)heads->dptr, n,
                           (const S*)tv.as<S>(),
                           (const unsigned*)tf.as<unsigned>(), o.data<T>());
      });
    });
  });
  return o.commit_if(rc, out);
}

int hf_ewm_mean(const hf_col* col, const hf_col* heads, double alpha,
                int adjust, int ignore_na, int64_t min_periods,
                hf_col** out) {
  HF_NEED_INIT("hf_ewm_mean");
  if (!col || !out) return set_err(HF_ERR_ARG, "hf_ewm_mean", "null");
  if (!(alpha > 0.0 && alpha <= 1.0))
    return set_err(HF_ERR_ARG, "hf_ewm_mean", "alpha must be in (0, 1]");
  if (min_periods < 0)
    return set_err(HF_ERR_ARG, "hf_ewm_mean", "min_periods must be >= 0");
  if (col->dtype != HF_FLOAT64 && col->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_ewm_mean", "col must be f64 or i64");
  if (heads && (heads->dtype != HF_INT64 || heads->len != col->len))
    return set_err(HF_ERR_ARG, "hf_ewm_mean",
                   "heads must be an int64 0/1 column of the same length");
  const int64_t n = col->len;
  ColOut o;
  int rc = o.alloc(n, HF_FLOAT64);
  if (rc != HF_OK) return rc;
  if (n == 0) { o.commit(out); return HF_OK; }
  const int64_t ntiles = (n + FILT_TILE - 1) / FILT_TILE;
  EwPar k;
  k.d = 1.0 - alpha;
  k.nw = adjust ? 1.0 : alpha;
  k.pval = adjust ? k.d : 0.0;
  k.pnan = ignore_na ? 1.0 : k.d;
  k.thresh = min_periods > 1 ? min_periods : 1;
  DevBuf tw, tm;
  HF_HIP("hf_ewm_mean", tw.alloc(ntiles * (int64_t)sizeof(EwW)));
  HF_HIP("hf_ewm_mean", tm.alloc(ntiles * (int64_t)sizeof(EwM)));
  EwW* d_tw = tw.as<EwW>();
  EwM* d_tm = tm.as<EwM>();
  rc = with_bool(heads != nullptr, [&](auto hTag) {
    return with_dtype(col->dtype, [&](auto tTag) -> int {
      using T = decltype(tTag);
      constexpr bool H = decltype(hTag)::value;
      const T* in = (const T*)col->dptr;
      const int64_t* hd = H ? (const int64_t*)heads->dptr : nullptr;
      const dim3 grid((uint32_t)ntiles);
      int r2 = timed_launch("ewm_w_tiles", [&] {
        hipLaunchKernelGGL((k_ewm_w_tiles<T, H>), grid, dim3(BLOCK), 0,
                           g.stream, in, hd, n, k, d_tw);
      });
      if (r2 != HF_OK) return r2;
      r2 = timed_launch("ewm_w_scan", [&] {
        hipLaunchKernelGGL((k_ewm_scan_tiles<EwW>), dim3(1), dim3(1024), 0,
                           g.stream, d_tw, ntiles);
      });
      if (r2 != HF_OK) return r2;
      r2 = timed_launch("ewm_m_tiles", [&] {
        hipLaunchKernelGGL((k_ewm_m_tiles<T, H>), grid, dim3(BLOCK), 0,
                           g.stream, in, hd, n, k, (const EwW*)d_tw, d_tm);
      });
      if (r2 != HF_OK) return r2;
      r2 = timed_launch("ewm_m_scan", [&] {
        hipLaunchKernelGGL((k_ewm_scan_tiles<EwM>), dim3(1), dim3(1024), 0,
                           g.stream, d_tm, ntiles);
      });
      if (r2 != HF_OK) return r2;
      return timed_launch("ewm_apply", [&] {
        hipLaunchKernelGGL((k_ewm_apply<T, H>), grid, dim3(BLOCK), 0,
                           g.stream, in, hd, n, k, (const EwW*)d_tw,
                           (const EwM*)d_tm, o.data<double>());
      });
    });
  });
  return o.commit_if(rc, out);
}

int hf_cross_idx(int64_t nl, int64_t nr, hf_col** lidx, hf_col** ridx) {
  HF_NEED_INIT("hf_cross_idx");
  if (!lidx || !ridx || nl < 0 || nr <= 0)
    return set_err(HF_ERR_ARG, "hf_cross_idx", "bad args");
  const int64_t n = nl * nr;
  ColOut o[2];
  for (ColOut& c : o) {
    const int rc = c.alloc(n, HF_INT64);
    if (rc != HF_OK) return rc;
  }
  if (n > 0) {
    const int rc = timed_launch("cross_idx", [&] {
      hipLaunchKernelGGL(k_cross_idx, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                         0, g.stream, n, nr, o[0].data<int64_t>(),
                         o[1].data<int64_t>());
    });
    if (rc != HF_OK) {
      *lidx = *ridx = nullptr;
      return rc;
    }
  }
  o[0].commit(lidx);
  o[1].commit(ridx);
  return HF_OK;
}

int hf_scatter(const hf_col* col, const hf_col* idx, hf_col** out) {
  HF_NEED_INIT("hf_scatter");
  if (!col || !idx || !out) return set_err(HF_ERR_ARG, "hf_scatter", "null");
  if (idx->dtype != HF_INT64 || idx->len != col->len)
    return set_err(HF_ERR_ARG, "hf_scatter",
                   "index must be an int64 permutation of the column");
  ColOut o;
  int rc = o.alloc(col->len, col->dtype);
  if (rc != HF_OK) return rc;
  const int64_t n = col->len;
  if (n == 0) { o.commit(out); return HF_OK; }
  rc = with_dtype(col->dtype, [&](auto tTag) {
    using T = decltype(tTag);
    return timed_launch("scatter", [&] {
      hipLaunchKernelGGL((k_scatter<T>), dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream, (const T*)col->dptr,
                         (const int64_t*)idx->dptr, o.data<T>(), n);
    });
  });
  return o.commit_if(rc, out);
}

int hf_ordered_i64(const hf_col* col, int direction, hf_col** out) {
  HF_NEED_INIT("hf_ordered_i64");
  if (!col || !out) return set_err(HF_ERR_ARG, "hf_ordered_i64", "null");
  const int want = direction ? HF_INT64 : HF_FLOAT64;
  if (col->dtype != want)
    return set_err(HF_ERR_ARG, "hf_ordered_i64",
                   direction ? "inverse needs an int64 column"
                             : "forward needs a float64 column");
  const int64_t n = col->len;
  ColOut o;
  int rc = o.alloc(n, direction ? HF_FLOAT64 : HF_INT64);
  if (rc != HF_OK) return rc;
  if (n > 0)
    rc = timed_launch("f64_ordered", [&] {
      if (direction)
        hipLaunchKernelGGL(k_ordered_f64, dim3((uint32_t)grid_for(n)),
                           dim3(BLOCK), 0, g.stream,
                           (const int64_t*)col->dptr, o.data<double>(), n);
      else
        hipLaunchKernelGGL(k_f64_ordered, dim3((uint32_t)grid_for(n)),
                           dim3(BLOCK), 0, g.stream,
                           (const double*)col->dptr, o.data<int64_t>(), n);
    });
  return o.commit_if(rc, out);
}

int hf_search_sorted(const hf_col* keys, const hf_col* sorted_uniq,
                     hf_col** out) {
  HF_NEED_INIT("hf_search_sorted");
  if (!keys || !sorted_uniq || !out)
    return set_err(HF_ERR_ARG, "hf_search_sorted", "null");
  if (keys->dtype != HF_INT64 || sorted_uniq->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_search_sorted", "int64 columns required");
  const int64_t n = keys->len;
  ColOut o;
  int rc = o.alloc(n, HF_INT64);
  if (rc != HF_OK) return rc;
  if (n > 0)
    rc = timed_launch("search_sorted", [&] {
      hipLaunchKernelGGL(k_search_sorted, dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream,
                         (const int64_t*)keys->dptr, n,
                         (const int64_t*)sorted_uniq->dptr,
                         sorted_uniq->len, o.data<int64_t>());
    });
  return o.commit_if(rc, out);
}

int hf_shuffle_dest(const hf_col* keys, const int64_t* splitters, int nsplit,
                    hf_col** dest) {
  HF_NEED_INIT("hf_shuffle_dest");
  if (!keys || !dest || nsplit < 0 || nsplit > 63 ||
      (nsplit && !splitters))
    return set_err(HF_ERR_ARG, "hf_shuffle_dest", "bad args");
  if (keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_shuffle_dest", "keys must be int64");
  const int64_t n = keys->len;
  ColOut o;
  int rc = o.alloc(n, HF_INT64);
  if (rc != HF_OK) return rc;
  DevBuf split;
  if (nsplit) {
    HF_HIP("hf_shuffle_dest", split.alloc(nsplit * 8));
    HF_HIP("hf_shuffle_dest",
           hipMemcpyAsync(split.as<void>(), splitters, nsplit * 8,
                          hipMemcpyHostToDevice, g.stream));
  }
  if (n > 0) {
    rc = timed_launch("shuffle_dest", [&] {
      hipLaunchKernelGGL(k_shuffle_dest, dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream,
                         (const int64_t*)keys->dptr, split.as<int64_t>(),
                         nsplit, o.data<long long>(), n);
    });
  }
  // splitters are host memory borrowed only until the H2D lands
  if (nsplit) hipStreamSynchronize(g.stream);
  return o.commit_if(rc, dest);
}

int hf_memcpy_dd(uintptr_t dst, uintptr_t src, int64_t bytes) {
  HF_NEED_INIT("hf_memcpy_dd");
  if (bytes < 0 || (bytes && (!dst || !src)))
    return set_err(HF_ERR_ARG, "hf_memcpy_dd", "bad args");
  if (bytes)
    HF_HIP("hf_memcpy_dd",
           hipMemcpyAsync((void*)dst, (void*)src, (size_t)bytes,
                          hipMemcpyDeviceToDevice, g.stream));
  return HF_OK;
}

int hf_groupby_sorted(const hf_col* sorted_keys, const hf_col* const* vals,
                      int nvals, int agg_op, int want_counts,
                      hf_col** out_keys, hf_col** out_sums,
                      hf_col** out_counts, int64_t* n_groups) {
  HF_NEED_INIT("hf_groupby_sorted");
  if (!sorted_keys || nvals < 0 || nvals > GB_MAX_VALS || !out_keys ||
      !n_groups)
    return set_err(HF_ERR_ARG, "hf_groupby_sorted", "bad args");
  if (sorted_keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_groupby_sorted", "keys must be int64");
  for (int c = 0; c < nvals; ++c)
    if (!vals[c] || vals[c]->dtype != HF_FLOAT64 ||
        vals[c]->len != sorted_keys->len)
      return set_err(HF_ERR_ARG, "hf_groupby_sorted",
                     "vals must be float64 columns of keys' length");
  const int64_t n = sorted_keys->len;
  // head flags -> filter plan (run count + tile bases)
  ColOut head;
  int rc = head.alloc(n, HF_INT64);
  if (rc != HF_OK) return rc;
  if (n > 0) {
    rc = timed_launch("gb_sorted_heads", [&] {
      hipLaunchKernelGGL(k_head_flags, dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream,
                         (const int64_t*)sorted_keys->dptr, n,
                         head.data<long long>());
    });
    if (rc != HF_OK) return rc;
  }
  hf_filterplan* plan = nullptr;
  int64_t C = 0;
  rc = hf_filter_plan(head.get(), &plan, &C);
  if (rc != HF_OK) return rc;
  const PlanOwner plan_owner(plan, hf_filter_plan_free);
  // outputs: unique keys (filter of sorted keys) + per-run aggregates
  const bool cnt = want_counts != 0;
  GroupOut o(nvals, cnt && out_counts);
  rc = hf_filter_apply(plan, sorted_keys, o.keys.slot());
  if (rc != HF_OK) return rc;
  // per-run aggregate buffers
  const int64_t Ca = C > 0 ? C : 1;
  DevBuf gsums_buf, growcnt_buf, gcounts_buf;
  HF_HIP("hf_groupby_sorted", gsums_buf.alloc(Ca * 8 * (nvals ? nvals : 1)));
  HF_HIP("hf_groupby_sorted", growcnt_buf.alloc(Ca * 8));
  if (cnt)
    HF_HIP("hf_groupby_sorted",
           gcounts_buf.alloc(Ca * 8 * (nvals ? nvals : 1)));
  double* gsums = gsums_buf.as<double>();
  unsigned long long* growcnt = growcnt_buf.as<unsigned long long>();
  unsigned long long* gcounts = gcounts_buf.as<unsigned long long>();
  if (nvals) {
    const double init =
        agg_op == HF_AGG_SUM ? 0.0
        : agg_op == HF_AGG_MIN ? __builtin_huge_val() : -__builtin_huge_val();
    rc = timed_launch("fill_f64", [&] {
      hipLaunchKernelGGL(k_fill_f64, dim3((uint32_t)grid_for(Ca * nvals)),
                         dim3(BLOCK), 0, g.stream, gsums, init, Ca * nvals);
    });
    if (rc != HF_OK) return rc;
  }
  HF_HIP("hf_groupby_sorted", hipMemsetAsync(growcnt, 0, Ca * 8, g.stream));
  if (cnt && nvals)
    HF_HIP("hf_groupby_sorted",
           hipMemsetAsync(gcounts, 0, Ca * 8 * nvals, g.stream));
  // aggregate per column (ROWCNT on the first launch only)
  const int64_t ntiles = n > 0 ? (n + FILT_TILE - 1) / FILT_TILE : 1;
  if (n > 0) {
    rc = with_aop(agg_op, [&](auto aTag) {
      auto seg = [&](auto cTag, auto rTag, auto vTag, const double* v,
                     double* gs, unsigned long long* gc) {
        return timed_launch("gb_segagg", [&] {
          hipLaunchKernelGGL(
              (k_segagg<decltype(aTag)::value, decltype(cTag)::value,
                        decltype(rTag)::value, decltype(vTag)::value>),
              dim3((uint32_t)ntiles), dim3(BLOCK), 0, g.stream,
              head.data<const long long>(), v, n, plan_tiles(plan), gs,
              growcnt, gc);
        });
      };
      using T = std::true_type;
      using F = std::false_type;
      if (nvals == 0) return seg(F{}, T{}, F{}, nullptr, nullptr, nullptr);
      for (int c = 0; c < nvals; ++c) {
        double* gs = gsums + (int64_t)c * Ca;
        unsigned long long* gc = cnt ? gcounts + (int64_t)c * Ca : nullptr;
        const double* v = (const double*)vals[c]->dptr;
        const int r = with_bool(cnt, [&](auto cTag) {
          return with_bool(c == 0, [&](auto rTag) {
            return seg(cTag, rTag, T{}, v, gs, gc);
          });
        });
        if (r != HF_OK) return r;
      }
      return (int)HF_OK;
    });
    if (rc != HF_OK) return rc;
  }
  // copy the aggregates out as columns
  for (int c = 0; c < nvals; ++c) {
    rc = o.sums[c].alloc(C, HF_FLOAT64);
    if (rc != HF_OK) return rc;
    HF_HIP("hf_groupby_sorted",
           hipMemcpyAsync(o.sums[c].get()->dptr, gsums + (int64_t)c * Ca,
                          Ca * 8, hipMemcpyDeviceToDevice, g.stream));
    if (cnt && out_counts) {
      rc = o.cnts[c].alloc(C, HF_INT64);
      if (rc != HF_OK) return rc;
      HF_HIP("hf_groupby_sorted",
             hipMemcpyAsync(o.cnts[c].get()->dptr, gcounts + (int64_t)c * Ca,
                            Ca * 8, hipMemcpyDeviceToDevice, g.stream));
    }
  }
  o.commit(out_keys, out_sums, out_counts);
  *n_groups = C;
  return HF_OK;
}

int hf_col_slice(const hf_col* col, int64_t start, int64_t len, hf_col** out) {
  HF_NEED_INIT("hf_col_slice");
  if (!col || !out || start < 0 || len < 0 || start + len > col->len)
    return set_err(HF_ERR_ARG, "hf_col_slice", "bad range");
  ColOut o;
  int rc = o.alloc(len, col->dtype);
  if (rc != HF_OK) return rc;
  const int64_t esz = dtype_size(col->dtype);
  if (len > 0)
    HF_HIP("hf_col_slice",
           hipMemcpyAsync(o.get()->dptr, (const char*)col->dptr + start * esz,
                          len * esz, hipMemcpyDeviceToDevice, g.stream));
  o.commit(out);
  return HF_OK;
}

// ---- join ----

// HF_JOIN_DEBUG: host-side CSR verification (monotone, steps match the
// histogram, total == rows), reported on stderr
static void join_debug_check(const unsigned* d_cnt,
                             const unsigned long long* d_csr, int64_t n_slots,
                             int64_t n) {
  std::vector<unsigned> h_cnt((size_t)n_slots);
  std::vector<unsigned long long> h_csr((size_t)n_slots + 1);
  hipMemcpyAsync(h_cnt.data(), d_cnt, n_slots * 4, hipMemcpyDeviceToHost,
                 g.stream);
  hipMemcpyAsync(h_csr.data(), d_csr, (n_slots + 1) * 8,
                 hipMemcpyDeviceToHost, g.stream);
  hipStreamSynchronize(g.stream);
  unsigned long long run = 0;
  int bad = 0;
  for (int64_t s = 0; s < n_slots && bad < 5; ++s) {
    if (h_csr[s] != run) {
      fprintf(stderr,
              "[join_debug] csr[%lld]=%llu expect %llu (cnt[s]=%u, "
              "tile=%lld)\n",
              (long long)s, h_csr[s], run, h_cnt[s], (long long)(s / 4096));
      ++bad;
    }
    run += h_cnt[s];
  }
  if (h_csr[n_slots] != run)
    fprintf(stderr, "[join_debug] csr[n]=%llu expect %llu\n", h_csr[n_slots],
            run);
  unsigned long long mx = 0;
  for (int64_t s = 0; s < n_slots; ++s)
    if (h_cnt[s] > mx) mx = h_cnt[s];
  fprintf(stderr, "[join_debug] hist total=%llu rows=%lld max_mult=%llu "
          "bad=%d\n", run, (long long)n, mx, bad);
}

// Per-slot histogram of the right keys (left in d_cnt) -> j->d_csr, the
// exclusive offsets of each key's run.
static int join_csr(const hf_col* rkeys, hf_join* j, unsigned* d_cnt,
                    int64_t* d_tiles, int64_t ntiles) {
  const int64_t n = j->n_right, n_slots = j->n_slots;
  unsigned long long* d_hist_err = scratch_at(SCRATCH_JOIN_HIST_ERR);
  int64_t* d_total = scratch_at<int64_t>(SCRATCH_NGROUPS);
  HF_HIP("hf_join_build", DevBuf::alloc_into(j->d_csr, (n_slots + 1) * 8));
  unsigned long long* d_csr = j->d_csr;
  int rc = timed_launch("join_hist", [&] {
    hipLaunchKernelGGL(k_hist_u32, dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0,
                       g.stream, (const int64_t*)rkeys->dptr, n, j->key_min,
                       n_slots, d_cnt, d_hist_err);
  });
  if (rc != HF_OK) return rc;
  rc = timed_launch("join_scan", [&] {
    hipLaunchKernelGGL(k_tile_sums_u32, dim3((uint32_t)ntiles), dim3(BLOCK), 0,
                       g.stream, d_cnt, n_slots, d_tiles);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, g.stream,
                       d_tiles, ntiles, d_total);
    hipLaunchKernelGGL(k_scan_apply_u32, dim3((uint32_t)ntiles), dim3(BLOCK),
                       0, g.stream, d_cnt, n_slots, d_tiles, d_total, d_csr);
  });
  if (rc != HF_OK) return rc;
  if (getenv("HF_JOIN_DEBUG")) join_debug_check(d_cnt, d_csr, n_slots, n);
  return HF_OK;
}

// Allocate j's row-index and payload arrays and fill them in CSR order;
// d_cnt is reused as the per-slot fill cursor.
static int join_fill(const hf_col* rkeys, const JoinConstPtrs& rv, hf_join* j,
                     unsigned* d_cnt) {
  const int64_t n = j->n_right, n_slots = j->n_slots;
  unsigned long long* d_fix_err = scratch_at(SCRATCH_JOIN_FIXUP_ERR);
  HF_HIP("hf_join_build", hipMemsetAsync(d_cnt, 0, n_slots * 4, g.stream));
  const int64_t alloc_n = n > 0 ? n : 1;
  HF_HIP("hf_join_build", DevBuf::alloc_into(j->d_jidx, alloc_n * 4));
  JoinPtrs jv{};
  for (int c = 0; c < j->nr; ++c) {
    HF_HIP("hf_join_build", DevBuf::alloc_into(j->d_jval[c], alloc_n * 8));
    jv.vals[c] = j->d_jval[c];
  }
  return with_nvals<GB_MAX_VALS>(j->nr, [&](auto nrTag) {
    constexpr int NR = decltype(nrTag)::value;
    int r2 = timed_launch("join_fill", [&] {
      hipLaunchKernelGGL((k_join_fill<NR>), dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream, (const int64_t*)rkeys->dptr,
                         rv, n, j->key_min, n_slots, j->d_csr, d_cnt,
                         j->d_jidx, jv);
    });
    if (r2 != HF_OK) return r2;
    return timed_launch("join_fixup", [&] {
      hipLaunchKernelGGL((k_join_fixup<NR>), dim3(2048), dim3(BLOCK), 0,
                         g.stream, j->d_csr, n_slots, j->d_jidx, jv, d_fix_err);
    });
  });
}

// Surface the hist/fixup error words; a key beyond the in-thread fixup's
// duplicate cap refills j from a stable sort.
static int join_check(const hf_col* rkeys, const hf_col* const* rvals,
                      hf_join* j) {
  const int64_t n = j->n_right;
  unsigned long long* d_hist_err = scratch_at(SCRATCH_JOIN_HIST_ERR);
  unsigned long long* d_fix_err = scratch_at(SCRATCH_JOIN_FIXUP_ERR);
  unsigned long long h_err[2] = {0, 0};
  HF_HIP("hf_join_build",
         hipMemcpyAsync(&h_err[0], d_hist_err, 8, hipMemcpyDeviceToHost,
                        g.stream));
  HF_HIP("hf_join_build",
         hipMemcpyAsync(&h_err[1], d_fix_err, 8, hipMemcpyDeviceToHost,
                        g.stream));
  HF_HIP("hf_join_build", hipStreamSynchronize(g.stream));
  if (h_err[0]) {
    hipMemsetAsync(d_hist_err, 0, 8, g.stream);
    hipMemsetAsync(d_fix_err, 0, 8, g.stream);
    char buf[160];
    snprintf(buf, sizeof buf,
             "%llu right keys outside [key_min, key_min+n_slots)",
             h_err[0]);
    return set_err(HF_ERR_ARG, "hf_join_build", buf);
  }
  if (!h_err[1]) return HF_OK;
  // keys beyond the 4096-duplicate in-thread fixup (round 2): rebuild
  // ORDER-CORRECT from a stable ascending key sort — within equal keys
  // the stable sort preserves original right order, which is exactly
  // the CSR layout (the offsets are fill-independent and already
  // computed).  Removes the per-key multiplicity cap entirely.
  hipMemsetAsync(d_fix_err, 0, 8, g.stream);
  ColOut perm;
  int rc = hf_sort_perm(rkeys, 1, perm.slot());
  if (rc != HF_OK) return rc;
  rc = timed_launch("join_sortfill", [&] {
    hipLaunchKernelGGL(k_i64_to_u32, dim3((uint32_t)grid_for(n)),
                       dim3(BLOCK), 0, g.stream, perm.data<const int64_t>(),
                       j->d_jidx, n);
  });
  for (int c = 0; c < j->nr && rc == HF_OK; ++c) {
    ColOut sv;
    rc = hf_gather(rvals[c], perm.get(), sv.slot());
    if (rc != HF_OK) break;
    if (hipMemcpyAsync(j->d_jval[c], sv.get()->dptr, n * 8,
                       hipMemcpyDeviceToDevice, g.stream) != hipSuccess)
      rc = set_err(HF_ERR_HIP, "hf_join_build", "sortfill copy");
  }
  return rc;
}

int hf_join_build(const hf_col* rkeys, const hf_col* const* rvals, int nr,
                  int64_t key_min, int64_t n_slots, hf_join** out) {
  HF_NEED_INIT("hf_join_build");
  if (!rkeys || nr < 0 || nr > GB_MAX_VALS || !out || n_slots <= 0)
    return set_err(HF_ERR_ARG, "hf_join_build", "bad args (nr<=8)");
  if (rkeys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_join_build", "right keys must be int64");
  if (n_slots > (1LL << 27))
    return set_err(HF_ERR_UNSUPPORTED, "hf_join_build",
                   "right key range too large for the dense-range CSR "
                   "(hash build is a later round)");
  JoinConstPtrs rv{};
  for (int c = 0; c < nr; ++c) {
    // the join only MOVES right payloads (8 B opaque), so both dtypes pass
    if (!rvals[c] || dtype_size(rvals[c]->dtype) != 8 ||
        rvals[c]->len != rkeys->len)
      return set_err(HF_ERR_ARG, "hf_join_build",
                     "right vals must be 8-byte columns of keys' length");
    rv.vals[c] = (const double*)rvals[c]->dptr;
  }
  JoinOwner j(new hf_join{}, hf_join_free);
  j->key_min = key_min;
  j->n_slots = n_slots;
  j->n_right = rkeys->len;
  j->nr = nr;
  for (int c = 0; c < nr; ++c) j->dtypes[c] = rvals[c]->dtype;
  int rc;
  {
    // histogram / fill cursor and scan tiles: back to the allocator before
    // the error-word readback and a possible sorted refill
    const int64_t ntiles = (n_slots + JOIN_TILE - 1) / JOIN_TILE;
    DevBuf cnt, tiles;
    HF_HIP("hf_join_build", cnt.alloc(n_slots * 4));
    HF_HIP("hf_join_build",
           hipMemsetAsync(cnt.as<void>(), 0, n_slots * 4, g.stream));
    HF_HIP("hf_join_build", tiles.alloc(ntiles * 8));
    rc = join_csr(rkeys, j.get(), cnt.as<unsigned>(), tiles.as<int64_t>(),
                  ntiles);
    if (rc == HF_OK) rc = join_fill(rkeys, rv, j.get(), cnt.as<unsigned>());
  }
  if (rc == HF_OK) rc = join_check(rkeys, rvals, j.get());
  if (rc != HF_OK) return rc;
  *out = j.release();
  return HF_OK;
}

int hf_join_free(hf_join* j) {
  if (!j) return HF_OK;
  if (g.inited) {
    if (j->d_csr) dev_free(j->d_csr, g.stream);
    if (j->d_jidx) dev_free(j->d_jidx, g.stream);
    for (int c = 0; c < j->nr; ++c)
      if (j->d_jval[c]) dev_free(j->d_jval[c], g.stream);
  }
  delete j;
  return HF_OK;
}

int hf_join_probe(const hf_join* j, const hf_col* lkeys, hf_col** out_keys,
                  hf_col** out_lidx, hf_col** out_rcols, int64_t* n_out) {
  HF_NEED_INIT("hf_join_probe");
  if (!j || !lkeys || !out_keys || !out_lidx || !n_out)
    return set_err(HF_ERR_ARG, "hf_join_probe", "null");
  if (lkeys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_join_probe", "left keys must be int64");
  const int64_t n = lkeys->len;
  const int64_t ntiles = n > 0 ? (n + JOIN_TILE - 1) / JOIN_TILE : 1;
  int64_t* d_total = scratch_at<int64_t>(SCRATCH_NGROUPS);
  const int64_t alloc_n = n > 0 ? n : 1;
  DevBuf offs, cnts, tiles;
  HF_HIP("hf_join_probe", offs.alloc(alloc_n * 8));
  HF_HIP("hf_join_probe", cnts.alloc(alloc_n * 4));
  HF_HIP("hf_join_probe", tiles.alloc(ntiles * 8));
  unsigned long long* d_offs = offs.as<unsigned long long>();
  unsigned* d_cnts = cnts.as<unsigned>();
  int64_t* d_tiles = tiles.as<int64_t>();
  HF_HIP("hf_join_probe", hipMemsetAsync(d_tiles, 0, ntiles * 8, g.stream));
  int rc = HF_OK;
  if (n > 0) {
    rc = timed_launch("join_probe_count", [&] {
      hipLaunchKernelGGL(k_probe_count, dim3((uint32_t)ntiles), dim3(BLOCK), 0,
                         g.stream, (const int64_t*)lkeys->dptr, n, j->key_min,
                         j->n_slots, j->d_csr, d_offs, d_cnts, d_tiles);
    });
    if (rc != HF_OK) return rc;
  }
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, g.stream, d_tiles,
                     ntiles, d_total);
  int64_t total = 0;
  HF_HIP("hf_join_probe",
         hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_join_probe", hipStreamSynchronize(g.stream));
  ColOut keys, lidx;
  std::vector<ColOut> rcols(j->nr);
  rc = keys.alloc(total, HF_INT64);
  if (rc != HF_OK) return rc;
  rc = lidx.alloc(total, HF_INT64);
  if (rc != HF_OK) return rc;
  JoinPtrs outr{};
  JoinConstPtrs jvc{};
  for (int c = 0; c < j->nr; ++c) {
    rc = rcols[c].alloc(total, j->dtypes[c]);
    if (rc != HF_OK) return rc;
    outr.vals[c] = rcols[c].data<double>();
    jvc.vals[c] = j->d_jval[c];
  }
  if (n > 0 && total > 0) {
    rc = with_nvals<GB_MAX_VALS>(j->nr, [&](auto nrTag) {
      constexpr int NR = decltype(nrTag)::value;
      return timed_launch("join_probe_emit", [&] {
        hipLaunchKernelGGL((k_probe_emit<NR>), dim3((uint32_t)ntiles),
                           dim3(BLOCK), 0, g.stream,
                           (const int64_t*)lkeys->dptr, n, (int64_t)0, d_offs,
                           d_cnts, d_tiles, j->d_jidx, jvc,
                           keys.data<int64_t>(), lidx.data<int64_t>(), outr);
      });
    });
    if (rc != HF_OK) return rc;
  }
  keys.commit(out_keys);
  lidx.commit(out_lidx);
  for (int c = 0; c < j->nr; ++c) rcols[c].commit(&out_rcols[c]);
  *n_out = total;
  return HF_OK;
}

int hf_gather(const hf_col* col, const hf_col* idx, hf_col** out) {
  HF_NEED_INIT("hf_gather");
  if (!col || !idx || !out) return set_err(HF_ERR_ARG, "hf_gather", "null");
  if (idx->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_gather", "index must be int64");
  ColOut o;
  int rc = o.alloc(idx->len, col->dtype);
  if (rc != HF_OK) return rc;
  const int64_t n = idx->len;
  if (n == 0) { o.commit(out); return HF_OK; }
  rc = timed_launch("gather", [&] {
    if (col->dtype == HF_FLOAT64)
      hipLaunchKernelGGL(k_gather_f64, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                         0, g.stream, (const double*)col->dptr,
                         (const int64_t*)idx->dptr, o.data<double>(), n);
    else
      hipLaunchKernelGGL(k_gather_i64, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                         0, g.stream, (const int64_t*)col->dptr,
                         (const int64_t*)idx->dptr, o.data<int64_t>(), n);
  });
  return o.commit_if(rc, out);
}

int hf_gather_fill(const hf_col* col, const hf_col* idx, double fill_f64,
                   int64_t fill_i64, hf_col** out) {
  HF_NEED_INIT("hf_gather_fill");
  if (!col || !idx || !out)
    return set_err(HF_ERR_ARG, "hf_gather_fill", "null");
  if (idx->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_gather_fill", "index must be int64");
  if (col->dtype != HF_FLOAT64 && col->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_gather_fill", "col must be f64 or i64");
  const int64_t n = idx->len;
  ColOut o;
  int rc = o.alloc(n, col->dtype);
  if (rc != HF_OK) return rc;
  if (n == 0) { o.commit(out); return HF_OK; }
  rc = with_dtype(col->dtype, [&](auto tTag) {
    using T = decltype(tTag);
    const T fill = std::is_same<T, double>::value ? (T)fill_f64 : (T)fill_i64;
    return timed_launch("gather_fill", [&] {
      hipLaunchKernelGGL((k_gather_fill<T>), dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream, (const T*)col->dptr,
                         (const int64_t*)idx->dptr, fill, o.data<T>(), n);
    });
  });
  return o.commit_if(rc, out);
}

int hf_asof_idx(const hf_col* lon, const hf_col* lby, const hf_col* ron,
                const hf_col* rby, int direction, int allow_exact,
                int has_tol, int64_t tol_i64, double tol_f64,
                hf_col** out_idx) {
  HF_NEED_INIT("hf_asof_idx");
  if (!lon || !ron || !out_idx)
    return set_err(HF_ERR_ARG, "hf_asof_idx", "null");
  if (lon->dtype != ron->dtype ||
      (lon->dtype != HF_INT64 && lon->dtype != HF_FLOAT64))
    return set_err(HF_ERR_ARG, "hf_asof_idx",
                   "on columns must both be int64 or both float64");
  if ((lby == nullptr) != (rby == nullptr))
    return set_err(HF_ERR_ARG, "hf_asof_idx", "by column on one side only");
  if (lby && (lby->dtype != HF_INT64 || rby->dtype != HF_INT64 ||
              lby->len != lon->len || rby->len != ron->len))
    return set_err(HF_ERR_ARG, "hf_asof_idx",
                   "by columns must be int64 of their on column's length");
  if (direction < HF_ASOF_BACKWARD || direction > HF_ASOF_NEAREST)
    return set_err(HF_ERR_ARG, "hf_asof_idx", "direction must be 0, 1 or 2");
  if (has_tol && (lon->dtype == HF_INT64 ? tol_i64 < 0 : !(tol_f64 >= 0.0)))
    return set_err(HF_ERR_ARG, "hf_asof_idx", "tolerance must be >= 0");
  const int64_t n = lon->len, m = ron->len;
  ColOut o;
  int rc = o.alloc(n, HF_INT64);
  if (rc != HF_OK) return rc;
  if (n == 0) { o.commit(out_idx); return HF_OK; }
  // Without a by column lon is ascending (the contract), which is what the
  // sorted-left form needs.  HF_ASOF_FORM=1 keeps such calls on the general
  // form (measurements, and the tests that compare the two).
  const char* form = getenv("HF_ASOF_FORM");
  const bool sorted_form = !lby && !(form && form[0] == '1');
  auto with_dir = [&](auto&& f) {
    return direction == HF_ASOF_BACKWARD  ? f(int_tag<HF_ASOF_BACKWARD>{})
           : direction == HF_ASOF_FORWARD ? f(int_tag<HF_ASOF_FORWARD>{})
                                          : f(int_tag<HF_ASOF_NEAREST>{});
  };
  rc = with_dtype(lon->dtype, [&](auto tTag) {
    using T = decltype(tTag);
    using D = typename AsofDist<T>::type;
    const D tol = std::is_same<T, double>::value ? (D)tol_f64 : (D)tol_i64;
    return with_bool(lby != nullptr, [&](auto bTag) {
      constexpr bool B = decltype(bTag)::value;
      const int64_t* lb = B ? (const int64_t*)lby->dptr : nullptr;
      const int64_t* rb = B ? (const int64_t*)rby->dptr : nullptr;
      return with_dir([&](auto dTag) {
        constexpr int DIR = decltype(dTag)::value;
        if constexpr (!B) {
          if (sorted_form)
            return timed_launch("asof_idx", [&] {
              hipLaunchKernelGGL(
                  (k_asof_idx_sorted<T, DIR>),
                  dim3((uint32_t)((n + ASOF_TILE - 1) / ASOF_TILE)),
                  dim3(BLOCK), 0, g.stream, (const T*)lon->dptr, n,
                  (const T*)ron->dptr, m, allow_exact, has_tol, tol,
                  o.data<int64_t>());
            });
        }
        return timed_launch("asof_idx", [&] {
          hipLaunchKernelGGL((k_asof_idx<T, B, DIR>),
                             dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0,
                             g.stream, (const T*)lon->dptr, lb, n,
                             (const T*)ron->dptr, rb, m, allow_exact, has_tol,
                             tol, o.data<int64_t>());
        });
      });
    });
  });
  return o.commit_if(rc, out_idx);
}

// The digit-offset part of one radix pass, shared by the narrow and the wide
// sort: per-tile digit counts C[tile][digit] -> exclusive scatter offsets
// offs[digit][tile].  Called inside the pass's timed_launch.
static void sort_digit_offsets(const unsigned* C, unsigned* CT,
                               int64_t* scan_tiles, unsigned long long* offs,
                               int64_t ntiles) {
  const int64_t L = ntiles * 256;
  const int64_t scan_tiles_n = (L + JOIN_TILE - 1) / JOIN_TILE;
  int64_t* d_total = scratch_at<int64_t>(SCRATCH_NGROUPS);
  hipLaunchKernelGGL(k_transpose256, dim3((uint32_t)((ntiles + 31) / 32), 8),
                     dim3(1024), 0, g.stream, C, CT, ntiles);
  hipLaunchKernelGGL(k_tile_sums_u32, dim3((uint32_t)scan_tiles_n),
                     dim3(BLOCK), 0, g.stream, CT, L, scan_tiles);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, g.stream,
                     scan_tiles, scan_tiles_n, d_total);
  hipLaunchKernelGGL(k_scan_apply_u32, dim3((uint32_t)scan_tiles_n),
                     dim3(BLOCK), 0, g.stream, CT, L, scan_tiles, d_total,
                     offs);
}

int hf_sort_perm(const hf_col* keys, int ascending, hf_col** out_perm) {
  HF_NEED_INIT("hf_sort_perm");
  if (!keys || !out_perm) return set_err(HF_ERR_ARG, "hf_sort_perm", "null");
  if (keys->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_sort_perm", "sort key must be int64");
  const int64_t n = keys->len;
  if (n >= (1LL << 31))
    return set_err(HF_ERR_UNSUPPORTED, "hf_sort_perm",
                   "partition too large (u32 origin indices)");
  hf_reduce_result r{};
  int rc = n > 0 ? hf_reduce(keys, &r) : HF_OK;
  if (rc != HF_OK) return rc;
  ColOut perm;
  rc = perm.alloc(n, HF_INT64);
  if (rc != HF_OK) return rc;
  if (n == 0) { perm.commit(out_perm); return HF_OK; }
  const int64_t key_min = r.imn;
  const uint64_t span = (uint64_t)r.imx - (uint64_t)r.imn;  // mod-2^64 safe
  // narrow: origin index packed under the shifted key in one u64;
  // wide: u64 shifted keys + u32 origins, up to 8 digit passes
  const bool wide = span >= (1ULL << 27);
  int bits = 0;
  while (bits < 64 && (span >> bits) != 0) ++bits;
  const int passes = (bits + 7) / 8;
  const int64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  const int64_t L = ntiles * 256;
  const int64_t scan_tiles_n = (L + JOIN_TILE - 1) / JOIN_TILE;
  DevBuf kA_buf, kB_buf, iA_buf, iB_buf, C_buf, CT_buf, offs_buf, scan_buf;
  HF_HIP("hf_sort_perm", kA_buf.alloc(n * 8));
  HF_HIP("hf_sort_perm", kB_buf.alloc(n * 8));
  if (wide) {
    HF_HIP("hf_sort_perm", iA_buf.alloc(n * 4));
    HF_HIP("hf_sort_perm", iB_buf.alloc(n * 4));
  }
  HF_HIP("hf_sort_perm", C_buf.alloc(L * 4));
  HF_HIP("hf_sort_perm", CT_buf.alloc(L * 4));
  HF_HIP("hf_sort_perm", offs_buf.alloc((L + 1) * 8));
  HF_HIP("hf_sort_perm", scan_buf.alloc(scan_tiles_n * 8));
  using u64 = unsigned long long;
  u64 *kcur = kA_buf.as<u64>(), *kalt = kB_buf.as<u64>();
  unsigned *icur = iA_buf.as<unsigned>(), *ialt = iB_buf.as<unsigned>();
  unsigned *C = C_buf.as<unsigned>(), *CT = CT_buf.as<unsigned>();
  u64* offs = offs_buf.as<u64>();
  int64_t* scan_tiles = scan_buf.as<int64_t>();
  const uint32_t wgrid =
      (uint32_t)std::min<int64_t>((ntiles + SORT_WPB - 1) / SORT_WPB, 2048);
  if (wide) {
    rc = timed_launch("sort_pack", [&] {
      hipLaunchKernelGGL(k_sort_pack_wide, dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream, (const int64_t*)keys->dptr,
                         n, key_min, span, ascending, kcur, icur);
    });
    for (int p = 0; p < passes && rc == HF_OK; ++p) {
      const int shift = 8 * p;
      rc = timed_launch("sort_pass", [&] {
        hipLaunchKernelGGL(k_sort_count_wide, dim3(wgrid), dim3(BLOCK), 0,
                           g.stream, kcur, n, shift, C, ntiles);
        sort_digit_offsets(C, CT, scan_tiles, offs, ntiles);
        hipLaunchKernelGGL(k_sort_scatter_wide, dim3(wgrid), dim3(BLOCK), 0,
                           g.stream, kcur, icur, n, shift, offs, ntiles, kalt,
                           ialt);
      });
      std::swap(kcur, kalt);
      std::swap(icur, ialt);
    }
    if (rc == HF_OK)
      rc = timed_launch("sort_unpack", [&] {
        hipLaunchKernelGGL(k_sort_unpack_wide, dim3((uint32_t)grid_for(n)),
                           dim3(BLOCK), 0, g.stream, icur, n,
                           perm.data<int64_t>());
      });
  } else {
    rc = timed_launch("sort_pack", [&] {
      hipLaunchKernelGGL(k_sort_pack, dim3((uint32_t)grid_for(n)), dim3(BLOCK),
                         0, g.stream, (const int64_t*)keys->dptr, n, key_min,
                         span, ascending, kcur);
    });
    for (int p = 0; p < passes && rc == HF_OK; ++p) {
      const int shift = 8 * p;
      rc = timed_launch("sort_pass", [&] {
        hipLaunchKernelGGL(k_sort_count, dim3(wgrid), dim3(BLOCK), 0, g.stream,
                           kcur, n, shift, C, ntiles);
        sort_digit_offsets(C, CT, scan_tiles, offs, ntiles);
        hipLaunchKernelGGL(k_sort_scatter, dim3(wgrid), dim3(BLOCK), 0,
                           g.stream, kcur, n, shift, offs, ntiles, kalt);
      });
      std::swap(kcur, kalt);
    }
    if (rc == HF_OK)
      rc = timed_launch("sort_unpack", [&] {
        hipLaunchKernelGGL(k_sort_unpack, dim3((uint32_t)grid_for(n)),
                           dim3(BLOCK), 0, g.stream, kcur, n,
                           perm.data<int64_t>());
      });
  }
  return perm.commit_if(rc, out_perm);
}

int hf_fill_f64(uintptr_t dptr, double value, int64_t n) {
  HF_NEED_INIT("hf_fill_f64");
  if (n <= 0) return HF_OK;
  return timed_launch("fill_f64", [&] {
    hipLaunchKernelGGL(k_fill_f64, dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0,
                       g.stream, (double*)dptr, value, n);
  });
}

int hf_fixup_empty(const hf_col* val, const hf_col* cnt, hf_col** out) {
  HF_NEED_INIT("hf_fixup_empty");
  if (!val || !cnt || !out || val->len != cnt->len ||
      val->dtype != HF_FLOAT64 || cnt->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_fixup_empty", "bad args");
  ColOut o;
  int rc = o.alloc(val->len, HF_FLOAT64);
  if (rc != HF_OK) return rc;
  if (val->len == 0) { o.commit(out); return HF_OK; }
  rc = timed_launch("fixup_empty", [&] {
    hipLaunchKernelGGL(k_fixup_empty, dim3((uint32_t)grid_for(val->len)),
                       dim3(BLOCK), 0, g.stream, (const double*)val->dptr,
                       (const int64_t*)cnt->dptr, o.data<double>(),
                       val->len);
  });
  return o.commit_if(rc, out);
}

// ---- compare + filter ----

struct hf_filterplan {
  const long long* mask;   // borrowed: caller keeps the mask column alive
  int64_t n, total, ntiles;
  int64_t* d_tiles;        // exclusive per-tile kept offsets
};

static const int64_t* plan_tiles(const hf_filterplan* p) { return p->d_tiles; }

int hf_compare_scalar(int op, const hf_col* col, double scalar, hf_col** out) {
  HF_NEED_INIT("hf_compare_scalar");
  if (!col || !out) return set_err(HF_ERR_ARG, "hf_compare_scalar", "null");
  if (op < HF_CMP_GT || op > HF_CMP_NOTNA)
    return set_err(HF_ERR_ARG, "hf_compare_scalar", "unknown op");
  ColOut o;
  int rc = o.alloc(col->len, HF_INT64);
  if (rc != HF_OK) return rc;
  const int64_t n = col->len;
  auto L = [&](auto opTag, auto tTag) {
    constexpr int O = decltype(opTag)::value;
    using T = typename decltype(tTag)::type;
    return timed_launch("compare", [&] {
      hipLaunchKernelGGL((k_compare<O, T, double>), dim3((uint32_t)grid_for(n)),
                         dim3(BLOCK), 0, g.stream, (const T*)col->dptr,
                         o.data<long long>(), scalar, n);
    });
  };
  struct F64 { using type = double; };
  struct I64 { using type = long long; };
  const bool f = col->dtype == HF_FLOAT64;
  switch (op) {
#define HF_CMP_CASE(O) \
  case O: rc = f ? L(int_tag<O>{}, F64{}) : L(int_tag<O>{}, I64{}); break;
    HF_CMP_CASE(HF_CMP_GT) HF_CMP_CASE(HF_CMP_GE) HF_CMP_CASE(HF_CMP_LT)
    HF_CMP_CASE(HF_CMP_LE) HF_CMP_CASE(HF_CMP_EQ) HF_CMP_CASE(HF_CMP_NE)
    HF_CMP_CASE(HF_CMP_NOTNA)
#undef HF_CMP_CASE
  }
  return o.commit_if(rc, out);
}

int hf_compare_scalar_i64(int op, const hf_col* col, int64_t scalar,
                          hf_col** out) {
  HF_NEED_INIT("hf_compare_scalar_i64");
  if (!col || !out) return set_err(HF_ERR_ARG, "hf_compare_scalar_i64", "null");
  if (op < HF_CMP_GT || op > HF_CMP_NOTNA)
    return set_err(HF_ERR_ARG, "hf_compare_scalar_i64", "unknown op");
  if (col->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_compare_scalar_i64", "int64 column required");
  ColOut o;
  int rc = o.alloc(col->len, HF_INT64);
  if (rc != HF_OK) return rc;
  const int64_t n = col->len;
  const long long s = (long long)scalar;
  auto L = [&](auto opTag) {
    constexpr int O = decltype(opTag)::value;
    return timed_launch("compare", [&] {
      hipLaunchKernelGGL((k_compare<O, long long, long long>),
                         dim3((uint32_t)grid_for(n)), dim3(BLOCK), 0, g.stream,
                         (const long long*)col->dptr, o.data<long long>(), s, n);
    });
  };
  switch (op) {
#define HF_CMP_CASE(O) \
  case O: rc = L(int_tag<O>{}); break;
    HF_CMP_CASE(HF_CMP_GT) HF_CMP_CASE(HF_CMP_GE) HF_CMP_CASE(HF_CMP_LT)
    HF_CMP_CASE(HF_CMP_LE) HF_CMP_CASE(HF_CMP_EQ) HF_CMP_CASE(HF_CMP_NE)
    HF_CMP_CASE(HF_CMP_NOTNA)
#undef HF_CMP_CASE
  }
  return o.commit_if(rc, out);
}

int hf_filter_plan(const hf_col* mask, hf_filterplan** out, int64_t* n_kept) {
  HF_NEED_INIT("hf_filter_plan");
  if (!mask || !out || !n_kept)
    return set_err(HF_ERR_ARG, "hf_filter_plan", "null");
  if (mask->dtype != HF_INT64)
    return set_err(HF_ERR_ARG, "hf_filter_plan", "mask must be int64 0/1");
  const int64_t n = mask->len;
  const int64_t ntiles = n > 0 ? (n + FILT_TILE - 1) / FILT_TILE : 1;
  PlanOwner p(new hf_filterplan{}, hf_filter_plan_free);
  p->mask = (const long long*)mask->dptr;
  p->n = n;
  p->ntiles = ntiles;
  HF_HIP("hf_filter_plan", DevBuf::alloc_into(p->d_tiles, ntiles * 8));
  HF_HIP("hf_filter_plan", hipMemsetAsync(p->d_tiles, 0, ntiles * 8, g.stream));
  int64_t* d_total = scratch_at<int64_t>(SCRATCH_NGROUPS);
  int rc = HF_OK;
  if (n > 0) {
    rc = timed_launch("filter_count", [&] {
      hipLaunchKernelGGL(k_filter_count, dim3((uint32_t)ntiles), dim3(BLOCK), 0,
                         g.stream, p->mask, n, p->d_tiles);
    });
    if (rc != HF_OK) return rc;
  }
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, g.stream,
                     p->d_tiles, ntiles, d_total);
  HF_HIP("hf_filter_plan",
         hipMemcpyAsync(&p->total, d_total, 8, hipMemcpyDeviceToHost, g.stream));
  HF_HIP("hf_filter_plan", hipStreamSynchronize(g.stream));
  *n_kept = p->total;
  *out = p.release();
  return HF_OK;
}

int hf_filter_plan_free(hf_filterplan* p) {
  if (!p) return HF_OK;
  if (g.inited && p->d_tiles) dev_free(p->d_tiles, g.stream);
  delete p;
  return HF_OK;
}

int hf_filter_apply(const hf_filterplan* p, const hf_col* col, hf_col** out) {
  HF_NEED_INIT("hf_filter_apply");
  if (!p || !col || !out) return set_err(HF_ERR_ARG, "hf_filter_apply", "null");
  if (col->len != p->n)
    return set_err(HF_ERR_ARG, "hf_filter_apply", "length mismatch");
  ColOut o;
  int rc = o.alloc(p->total, col->dtype);
  if (rc != HF_OK) return rc;
  if (p->n == 0 || p->total == 0) { o.commit(out); return HF_OK; }
  rc = timed_launch("filter_scatter", [&] {
    if (col->dtype == HF_FLOAT64)
      hipLaunchKernelGGL((k_filter_scatter<double, false>),
                         dim3((uint32_t)p->ntiles), dim3(BLOCK), 0, g.stream,
                         p->mask, (const double*)col->dptr, p->n, p->d_tiles,
                         (int64_t)0, o.data<double>());
    else
      hipLaunchKernelGGL((k_filter_scatter<long long, false>),
                         dim3((uint32_t)p->ntiles), dim3(BLOCK), 0, g.stream,
                         p->mask, (const long long*)col->dptr, p->n, p->d_tiles,
                         (int64_t)0, o.data<long long>());
  });
  return o.commit_if(rc, out);
}

int hf_filter_iota(const hf_filterplan* p, int64_t base, hf_col** out) {
  HF_NEED_INIT("hf_filter_iota");
  if (!p || !out) return set_err(HF_ERR_ARG, "hf_filter_iota", "null");
  ColOut o;
  int rc = o.alloc(p->total, HF_INT64);
  if (rc != HF_OK) return rc;
  if (p->n == 0 || p->total == 0) { o.commit(out); return HF_OK; }
  rc = timed_launch("filter_iota", [&] {
    hipLaunchKernelGGL((k_filter_scatter<long long, true>),
                       dim3((uint32_t)p->ntiles), dim3(BLOCK), 0, g.stream,
                       p->mask, (const long long*)nullptr, p->n, p->d_tiles,
                       base, o.data<long long>());
  });
  return o.commit_if(rc, out);
}

// ---- profiling ----

int hf_profiling(int enable) {
  HF_NEED_INIT("hf_profiling");
  g.profiling = enable != 0;
  return HF_OK;
}

int hf_kernel_stats(const char* name, int64_t* launches, double* total_ms) {
  HF_NEED_INIT("hf_kernel_stats");
  int rc = resolve_stats("hf_kernel_stats");
  if (rc != HF_OK) return rc;
  auto it = g.stats.find(name);
  if (it == g.stats.end()) {
    *launches = 0;
    *total_ms = 0.0;
    return HF_OK;
  }
  *launches = it->second.first;
  *total_ms = it->second.second;
  return HF_OK;
}

int hf_kernel_stats_reset(void) {
  HF_NEED_INIT("hf_kernel_stats_reset");
  int rc = resolve_stats("hf_kernel_stats_reset");
  if (rc != HF_OK) return rc;
  g.stats.clear();
  return HF_OK;
}

}  // extern "C"
