// rmi_lookup.hip -- the device index: batched lookup, bounded search and the acceptance check of a trained two-layer RMI
// (include/rmi_hip.h, "querying a trained RMI on the device").
//
// lookup is the emitted C++ `lookup(key, &err)` (codegen.rs:621-717, rmi_amd/codegen.py) evaluated per query with the same
// IEEE operations: the root function (std::fma, exp1 / phi of stdlib.rs), modelIndex -- FCLAMP(fpred, L - 1.0) for roots with
// a bounds check, the raw prediction for cubic / radix / radix tables / bradix --, the leaf's std::fma, *err = row[ppl] and
// FCLAMP(fpred, n - 1.0).  Built with -ffp-contract=off like the training kernels, so no other operation fuses.
//
// search: the lower bound of the query among the resident keys.  The window of candidate positions [guess - err, guess + err]
// (clamped to [0, n]) is widened by one key on either side, so that one bisection of keys[lo, hi) also tells whether the lower
// bound lies inside the window: a result at lo (keys[a - 1] >= q) means it is further left, a result at hi (keys[b] < q) further
// right.  Then a galloping search outward from that edge (steps 1, 2, 4, ...) and a bisection of the bracket it finds.  Every
// bisection stops at 128 / sizeof(K) keys -- one 128-byte line of the key array, 16 u64 / f64 keys or 32 u32 keys -- and reads
// them with one batch of independent loads (one memory round trip) and counts.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rmi_device.hip.h"
#include "rmi_lookup_launch.h"

namespace rmi {

// root functions as the emitted C++ has them
enum : int { LR_LINEAR = 0,      // linear / linear_spline / robust_linear: fma(beta, x, alpha), FCLAMP
             LR_CUBIC = 1,       // cubic: (uint64_t) fpred, no bounds check
             LR_LOGLINEAR = 2,   // exp1(fma(beta, x, alpha)), FCLAMP
             LR_NORMAL = 3,      // phi((x - mean) / stdev) * scale, FCLAMP
             LR_RADIX = 4,       // (x << prefix) >> (64 - bits), no bounds check
             LR_TABLE = 5,       // table[((x << prefix) >> prefix) >> shift], no bounds check
             LR_BRADIX_HIGH = 6, // balanced_radix.rs:132-141
             LR_BRADIX_LOW = 7,  // balanced_radix.rs:143-152
             LR_COUNT = 8 };

enum : int { LM_LOOKUP = 0, LM_SEARCH = 1, LM_SEARCH_COOP = 2 };
constexpr int COOP_G = 8;                // lanes per query of the cooperative search

struct LookupArgs {
  RootP r;                               // p0..p3, prefix, bits (radix tables: the shift), L, table; cap = bradix clamp
  const unsigned char* rows;             // L rows of (params..., err), PPL * 8 + 8 bytes each
  int has_err;
  const void* keys;                      // resident keys (search)
  uint64_t n;                            // num_rows of the model = resident key count
  double nm1;                            // n - 1.0, the bound of the final FCLAMP
  const void* q;
  uint64_t nq;
  unsigned long long* guess;             // lookup: guess (required) and err (may be null)
  unsigned long long* err;
  unsigned long long* pos;               // search: lower bounds (may be null)
  unsigned long long* cnt;               // [0] fallbacks, [1] root_oob
};

// Rust / C++ `x as u64` for a non-negative x below 2^64 is truncation; sat_f64_to_u64 also maps NaN and negatives to 0.
// FCLAMP(inp, bound) of the emitted code: inp < 0 -> 0, inp > bound -> bound, else (size_t)inp (NaN: 0 here, UB there)
__device__ __forceinline__ uint64_t fclamp(double inp, double bound) {
  if (inp < 0.0) return 0ull;
  return inp > bound ? (uint64_t)bound : sat_f64_to_u64(inp);
}

// modelIndex of the emitted lookup; `oob` where the emitted code has no defined result (raw prediction outside [0, L), NaN)
template <int LR, typename K>
__device__ __forceinline__ uint64_t model_index(const RootP& r, K k, bool& oob) {
  const uint64_t L = r.L;
  if constexpr (LR <= LR_NORMAL) {
    constexpr int RK = LR == LR_CUBIC ? K_CUBIC : LR == LR_LOGLINEAR ? K_LOGLINEAR : LR == LR_NORMAL ? K_NORMAL : K_LINEAR;
    const double f = root_eval_f<RK>(r, KeyTraits<K>::as_float(k));
    if constexpr (LR == LR_CUBIC) {
      // (uint64_t) fpred: defined for -1 < fpred < 2^64; an index from L on reads past the leaf array
      oob = !(f > -1.0 && f < (double)L);
      if (oob) return f >= (double)L ? L - 1 : 0ull;
      return sat_f64_to_u64(f);
    } else {
      oob = (f != f);
      return fclamp(f, (double)L - 1.0);
    }
  } else {
    uint64_t ip;
    if constexpr (LR == LR_TABLE) {
      ip = (uint64_t)r.table[radix_table_slot(r, KeyTraits<K>::as_uint(k))];
    } else {
      ip = root_predict<K_RADIX>(r, k);
      if constexpr (LR == LR_BRADIX_HIGH) ip = ip > r.cap ? r.cap : ip;
      if constexpr (LR == LR_BRADIX_LOW) ip = ip < r.cap ? 0ull : ip - r.cap;
    }
    oob = ip >= L;
    return oob ? L - 1 : ip;
  }
}

// The line of keys: lower bound in [base, base + len), len <= 128 / sizeof(K), from one batch of loads at immediate offsets of
// one address (the batch is moved left where it would run past the last key; key sets shorter than a line: loads clamped)
template <typename K>
__device__ __forceinline__ uint64_t line_count(const K* __restrict__ keys, uint64_t n, uint64_t base, uint64_t len, K q) {
  constexpr uint64_t LN = 128 / sizeof(K);
  K v[LN];
  uint64_t s;
  if (n >= LN) {
    s = base + LN <= n ? base : n - LN;
    const K* __restrict__ p = keys + s;
#pragma unroll
    for (uint64_t j = 0; j < LN; j++) v[j] = p[j];
  } else {
    s = 0;
#pragma unroll
    for (uint64_t j = 0; j < LN; j++) v[j] = keys[j < n ? j : n - 1];
  }
  uint64_t c = 0;
#pragma unroll
  for (uint64_t j = 0; j < LN; j++) c += (s + j >= base && s + j < base + len && v[j] < q) ? 1u : 0u;
  return base + c;
}

// lower bound of q in keys[base, base + len) (keys[base - 1] < q <= keys[base + len] assumed): a result in [base, base + len]
template <typename K>
__device__ __forceinline__ uint64_t lb_lane(const K* __restrict__ keys, uint64_t n, uint64_t base, uint64_t len, K q) {
  constexpr uint64_t LN = 128 / sizeof(K);
  while (len > LN) {
    const uint64_t half = len >> 1;
    const bool lt = keys[base + half] < q;
    base = lt ? base + half + 1 : base;
    len = lt ? len - half - 1 : half;
  }
  return line_count(keys, n, base, len, q);
}

// the same with the COOP_G lanes of a group (j = lane in the group): eight probes, one at the end of each eighth of the
// range, a round; the last line read by the group together, 128 / sizeof(K) / COOP_G keys a lane.  Group-uniform control flow.
template <typename K>
__device__ __forceinline__ uint64_t lb_coop(const K* __restrict__ keys, uint64_t n, uint64_t base, uint64_t len, K q, int j) {
  constexpr uint64_t LN = 128 / sizeof(K);
  const int gsh = (int)(threadIdx.x & 63u) & ~(COOP_G - 1);
  while (len > LN) {
    const uint64_t w = (len + COOP_G - 1) / COOP_G;
    const uint64_t idx = base + (uint64_t)(j + 1) * w - 1;
    const bool valid = idx < base + len;
    const bool lt = valid && keys[valid ? idx : base] < q;
    const unsigned int c = __popcll((__ballot(lt) >> gsh) & ((1ull << COOP_G) - 1));
    const uint64_t nb = base + (uint64_t)c * w;
    const uint64_t rest = base + len - nb;
    len = rest < w - 1 ? rest : w - 1;
    base = nb;
  }
  constexpr uint64_t PER = LN / COOP_G;
  const uint64_t s0 = n >= LN ? (base + LN <= n ? base : n - LN) : 0ull;
  const uint64_t s = s0 + (uint64_t)j * PER;
  uint64_t c = 0;
#pragma unroll
  for (uint64_t t = 0; t < PER; t++) {
    const uint64_t i = s + t;
    const K v = keys[i < n ? i : n - 1];
    c += (i >= base && i < base + len && v < q) ? 1u : 0u;
  }
#pragma unroll
  for (int m = COOP_G / 2; m >= 1; m >>= 1) c += (uint64_t)__shfl_xor((unsigned int)c, m, 64);
  return base + c;
}

template <bool COOP, typename K>
__device__ __forceinline__ uint64_t lb(const K* __restrict__ keys, uint64_t n, uint64_t base, uint64_t len, K q, int j) {
  if constexpr (COOP) return lb_coop(keys, n, base, len, q, j);
  else return lb_lane(keys, n, base, len, q);
}

// lower bound of q given the guess g (< n) and the error e; *outside: it lies outside [g - e, g + e].  One call site of the
// bisection (a loop of at most two trips: the window, then the bracket the gallop found), so that its line of keys is
// compiled once.
template <bool COOP, typename K>
__device__ __forceinline__ uint64_t window_search(const K* __restrict__ keys, uint64_t n, uint64_t g, uint64_t e, K q, int j,
                                                  bool& outside) {
  const uint64_t a = g > e ? g - e : 0ull;
  const uint64_t b = e >= n - g ? n : g + e;
  const uint64_t lo = a > 0 ? a - 1 : 0ull, hi = b < n ? b + 1 : n;
  uint64_t base = lo, len = hi - lo, p;
  outside = false;
  for (bool first = true;; first = false) {
    p = lb<COOP>(keys, n, base, len, q, j);
    if (!first) break;
    const bool left = a > 0 && p == lo;        // keys[a - 1] >= q
    const bool right = b < n && p == hi;       // keys[b] < q
    if (!left && !right) break;
    outside = true;
    uint64_t l, h, step = 1;
    if (left) {
      // keys[h] >= q; gallop towards 0 until a key < q
      h = lo; l = 0;
      while (h > 0) {
        const uint64_t pr = h > step ? h - step : 0ull;
        if (keys[pr] < q) { l = pr + 1; break; }
        h = pr; step <<= 1;
      }
    } else {
      // keys[l - 1] < q; gallop towards n until a key >= q
      l = hi; h = n;
      while (l < n) {
        const uint64_t pr = n - l > step ? l - 1 + step : n - 1;
        if (!(keys[pr] < q)) { h = pr; break; }
        l = pr + 1; step <<= 1;
      }
    }
    base = l; len = h - l;
  }
  return p;
}

template <int LR, int PPL, typename K, int MODE>
__global__ __launch_bounds__(256) void k_rmi_lookup(LookupArgs a) {
  constexpr bool COOP = MODE == LM_SEARCH_COOP;
  constexpr int G = COOP ? COOP_G : 1;
  const K* __restrict__ qs = (const K*)a.q;
  const K* __restrict__ keys = (const K*)a.keys;
  const int j = COOP ? (int)(threadIdx.x & (G - 1)) : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x / G;
  unsigned long long fb = 0, oob_n = 0;
  for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G; i < a.nq; i += stride) {
    const K q = qs[i];
    bool oob;
    const uint64_t mi = model_index<LR>(a.r, q, oob);
    const double* row = (const double*)(a.rows + mi * (uint64_t)(PPL * 8 + 8));
    const double x = KeyTraits<K>::as_float(q);
    double fpred;
    if constexpr (PPL == 4) fpred = __builtin_fma(__builtin_fma(__builtin_fma(row[0], x, row[1]), x, row[2]), x, row[3]);
    else fpred = __builtin_fma(row[1], x, row[0]);
    const uint64_t g = fclamp(fpred, a.nm1);
    const uint64_t e = a.has_err ? ((const unsigned long long*)row)[PPL] : 0ull;
    if (j == 0) oob_n += oob ? 1u : 0u;
    if constexpr (MODE == LM_LOOKUP) {
      a.guess[i] = g;
      if (a.err != nullptr && a.has_err) a.err[i] = e;
    } else {
      bool outside;
      const uint64_t p = window_search<COOP>(keys, a.n, g, e, q, j, outside);
      if (j == 0) {
        fb += outside ? 1u : 0u;
        if (a.pos != nullptr) a.pos[i] = p;
      }
    }
  }
  // one vector atomic per wave for each counter
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    fb += __shfl_xor(fb, m, 64);
    oob_n += __shfl_xor(oob_n, m, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (fb) atomicAdd(&a.cnt[0], fb);
    if (oob_n) atomicAdd(&a.cnt[1], oob_n);
  }
}

template <int LR, int PPL, typename K>
static void launch_t(int mode, unsigned int grid, const LookupArgs& a, hipStream_t s) {
  if (mode == LM_LOOKUP) hipLaunchKernelGGL((k_rmi_lookup<LR, PPL, K, LM_LOOKUP>), dim3(grid), dim3(256), 0, s, a);
  else if (mode == LM_SEARCH) hipLaunchKernelGGL((k_rmi_lookup<LR, PPL, K, LM_SEARCH>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_rmi_lookup<LR, PPL, K, LM_SEARCH_COOP>), dim3(grid), dim3(256), 0, s, a);
}

template <int LR, typename K>
static void launch_ppl(int ppl, int mode, unsigned int grid, const LookupArgs& a, hipStream_t s) {
  if (ppl == 4) launch_t<LR, 4, K>(mode, grid, a, s); else launch_t<LR, 2, K>(mode, grid, a, s);
}

template <typename K>
static void launch_root(int lr, int ppl, int mode, unsigned int grid, const LookupArgs& a, hipStream_t s) {
  switch (lr) {
    case LR_LINEAR: launch_ppl<LR_LINEAR, K>(ppl, mode, grid, a, s); break;
    case LR_CUBIC: launch_ppl<LR_CUBIC, K>(ppl, mode, grid, a, s); break;
    case LR_LOGLINEAR: launch_ppl<LR_LOGLINEAR, K>(ppl, mode, grid, a, s); break;
    case LR_NORMAL: launch_ppl<LR_NORMAL, K>(ppl, mode, grid, a, s); break;
    case LR_RADIX: launch_ppl<LR_RADIX, K>(ppl, mode, grid, a, s); break;
    case LR_TABLE: launch_ppl<LR_TABLE, K>(ppl, mode, grid, a, s); break;
    case LR_BRADIX_HIGH: launch_ppl<LR_BRADIX_HIGH, K>(ppl, mode, grid, a, s); break;
    default: launch_ppl<LR_BRADIX_LOW, K>(ppl, mode, grid, a, s); break;
  }
}

}  // namespace rmi

using namespace rmi;

struct rmi_hip_index {
  rmi_hip_ctx* ctx = nullptr;
  int device = 0;
  int dtype = RMI_KEY_U64;
  int lr = LR_LINEAR;
  int ppl = 2;
  int has_err = 1;
  int variant = 0;
  uint64_t L = 0, n = 0;
  RootP rp = {};
  unsigned char* d_rows = nullptr;
  uint32_t* d_table = nullptr;
  unsigned long long* d_cnt = nullptr;   // [fallbacks, root_oob]
  unsigned long long* h_cnt = nullptr;   // pinned
  hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace rmi {
void index_release(rmi_hip_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->d_rows) (void)hipFree(ix->d_rows);
  if (ix->d_table) (void)hipFree(ix->d_table);
  if (ix->d_cnt) (void)hipFree(ix->d_cnt);
  if (ix->h_cnt) (void)hipHostFree(ix->h_cnt);
  for (auto& e : ix->ev) if (e) (void)hipEventDestroy(e);
  delete ix;
}
}  // namespace rmi

static int ix_fail(rmi_hip_ctx* c, hipError_t e, const char* what) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s failed: %s (rmi_lookup.hip)", what, hipGetErrorString(e));
  ctx_set_error(c, buf);
  return RMI_ERR_HIP;
}
#define IXCHK(c, call) do { hipError_t _e = (call); if (_e != hipSuccess) return ix_fail(c, _e, #call); } while (0)

static int table_bits_of(int kind) {
  switch (kind) {
    case RMI_MODEL_RADIX8: return 8;
    case RMI_MODEL_RADIX18: return 18;
    case RMI_MODEL_RADIX22: return 22;
    case RMI_MODEL_RADIX26: return 26;
    case RMI_MODEL_RADIX28: return 28;
    default: return -1;
  }
}

// root parameters -> (root function, RootP); RMI_ERR_* for a root the index does not take
static int root_setup(const rmi_hip_model_params* root, uint64_t L, int& lr, RootP& rp) {
  rp = RootP{};
  rp.p0 = root->p[0]; rp.p1 = root->p[1]; rp.p2 = root->p[2]; rp.p3 = root->p[3];
  rp.prefix = (uint32_t)root->ip[0]; rp.bits = (uint32_t)root->ip[1];
  rp.L = L; rp.cap = L - 1; rp.oob_cap = L - 1;
  switch (root->kind) {
    case RMI_MODEL_LINEAR: case RMI_MODEL_LINEAR_SPLINE: case RMI_MODEL_ROBUST_LINEAR: lr = LR_LINEAR; break;
    case RMI_MODEL_CUBIC: lr = LR_CUBIC; break;
    case RMI_MODEL_LOGLINEAR: lr = LR_LOGLINEAR; break;
    case RMI_MODEL_NORMAL: lr = LR_NORMAL; break;
    case RMI_MODEL_RADIX: lr = LR_RADIX; break;
    case RMI_MODEL_BRADIX: lr = root->ip[3] ? LR_BRADIX_HIGH : LR_BRADIX_LOW; rp.cap = root->ip[2]; break;
    case RMI_MODEL_LOGNORMAL: case RMI_MODEL_HISTOGRAM: return RMI_ERR_UNSUPPORTED_MODEL;
    default:
      if (table_bits_of(root->kind) < 0) return RMI_ERR_UNKNOWN_MODEL;
      lr = LR_TABLE;
      if (root->ip[1] != (uint64_t)table_bits_of(root->kind)) return RMI_ERR_BAD_ARG;
      rp.bits = (root->ip[0] + root->ip[1] > 64) ? 0u : (uint32_t)(64 - (root->ip[0] + root->ip[1]));   // radix.rs:140-153
  }
  return RMI_OK;
}

static int index_alloc(rmi_hip_ctx* c, const CtxLookupView& v, rmi_hip_index* ix, uint64_t row_bytes, uint64_t table_entries) {
  ix->ctx = c;
  ix->device = v.device;
  IXCHK(c, hipSetDevice(v.device));
  IXCHK(c, hipMalloc((void**)&ix->d_rows, ix->L * row_bytes));
  if (table_entries) IXCHK(c, hipMalloc((void**)&ix->d_table, table_entries * 4));
  IXCHK(c, hipMalloc((void**)&ix->d_cnt, 4 * sizeof(unsigned long long)));
  IXCHK(c, hipHostMalloc((void**)&ix->h_cnt, 4 * sizeof(unsigned long long), 0));
  for (auto& e : ix->ev) IXCHK(c, hipEventCreate(&e));
  ix->rp.table = ix->d_table;
  return RMI_OK;
}

static int finish_create(rmi_hip_ctx* c, rmi_hip_index* ix, int rc, rmi_hip_index** out) {
  if (rc) { index_release(ix); return rc; }
  ctx_register_index(c, ix, true);
  *out = ix;
  return RMI_OK;
}

static bool key_dtype_ok(int dtype) { return dtype == RMI_KEY_U64 || dtype == RMI_KEY_U32 || dtype == RMI_KEY_F64; }

extern "C" {

int rmi_hip_index_from_result(rmi_hip_ctx* c, const rmi_hip_model_params* root, uint64_t generation, rmi_hip_index** out) {
  if (!c || !root || !out) return RMI_ERR_BAD_ARG;
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  if (v.last_L == 0 || generation != v.generation || !v.rows) {
    ctx_set_error(c, "rmi_hip_index_from_result: the arrays of that training are gone (trained again since, or a shard)");
    return RMI_ERR_BAD_ARG;
  }
  rmi_hip_index* ix = new (std::nothrow) rmi_hip_index();
  if (!ix) return RMI_ERR_HIP;
  ix->L = v.last_L; ix->n = v.n; ix->dtype = v.dtype; ix->ppl = v.last_ppl; ix->has_err = 1;
  int rc = root_setup(root, ix->L, ix->lr, ix->rp);
  if (rc) { delete ix; return rc; }
  uint64_t tab = 0;
  if (ix->lr == LR_TABLE) {
    tab = 1ull << root->ip[1];
    if (!v.table || v.table_entries != tab) { delete ix; return RMI_ERR_BAD_ARG; }
  }
  const uint64_t row_bytes = (uint64_t)ix->ppl * 8 + 8;
  rc = index_alloc(c, v, ix, row_bytes, tab);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(ix->d_rows, v.rows, ix->L * row_bytes, hipMemcpyDeviceToDevice, v.stream);
    if (e == hipSuccess && tab) e = hipMemcpyAsync(ix->d_table, v.table, tab * 4, hipMemcpyDeviceToDevice, v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
    if (e != hipSuccess) rc = ix_fail(c, e, "copy of the rows");
  }
  return finish_create(c, ix, rc, out);
}

int rmi_hip_index_from_arrays(rmi_hip_ctx* c, const rmi_hip_model_params* root, int leaf_kind, uint64_t num_leaves,
                              uint64_t num_rows, int dtype, const double* params, const uint64_t* errors,
                              const uint32_t* root_table, uint64_t table_entries, rmi_hip_index** out) {
  if (!c || !root || !out || !params || num_leaves == 0 || num_leaves > (1ull << 32) || num_rows == 0 || !key_dtype_ok(dtype))
    return RMI_ERR_BAD_ARG;
  int ppl;
  switch (leaf_kind) {
    case RMI_MODEL_LINEAR: case RMI_MODEL_LINEAR_SPLINE: case RMI_MODEL_ROBUST_LINEAR: ppl = 2; break;
    case RMI_MODEL_CUBIC: ppl = 4; break;
    case RMI_MODEL_LOGNORMAL: case RMI_MODEL_HISTOGRAM: case RMI_MODEL_LOGLINEAR: case RMI_MODEL_NORMAL: return RMI_ERR_UNSUPPORTED_MODEL;
    default: return leaf_kind >= 0 && leaf_kind <= RMI_MODEL_HISTOGRAM ? RMI_ERR_RESTRICTION : RMI_ERR_UNKNOWN_MODEL;
  }
  rmi_hip_index* ix = new (std::nothrow) rmi_hip_index();
  if (!ix) return RMI_ERR_HIP;
  ix->L = num_leaves; ix->n = num_rows; ix->dtype = dtype; ix->ppl = ppl; ix->has_err = errors != nullptr;
  int rc = root_setup(root, ix->L, ix->lr, ix->rp);
  if (rc) { delete ix; return rc; }
  uint64_t tab = 0;
  if (ix->lr == LR_TABLE) {
    tab = 1ull << root->ip[1];
    if (!root_table || table_entries != tab) { delete ix; return RMI_ERR_BAD_ARG; }
  }
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  const uint64_t row_bytes = (uint64_t)ppl * 8 + 8;
  std::vector<uint64_t> rows(num_leaves * (ppl + 1));
  for (uint64_t i = 0; i < num_leaves; i++) {
    std::memcpy(&rows[i * (ppl + 1)], params + i * ppl, (size_t)ppl * 8);
    rows[i * (ppl + 1) + ppl] = errors ? errors[i] : 0ull;
  }
  rc = index_alloc(c, v, ix, row_bytes, tab);
  if (!rc) {
    hipError_t e = hipMemcpy(ix->d_rows, rows.data(), num_leaves * row_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && tab) e = hipMemcpy(ix->d_table, root_table, tab * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = ix_fail(c, e, "upload of the rows");
  }
  return finish_create(c, ix, rc, out);
}

int rmi_hip_index_set_variant(rmi_hip_index* ix, int variant) {
  if (!ix || variant < 0 || variant > 1) return RMI_ERR_BAD_ARG;
  ix->variant = variant;
  return RMI_OK;
}

void rmi_hip_index_destroy(rmi_hip_index* ix) {
  if (!ix) return;
  if (ix->ctx) ctx_register_index(ix->ctx, ix, false);
  index_release(ix);
}

}  // extern "C"

static int run(rmi_hip_ctx* c, const rmi_hip_index* ix, int mode, const void* q, uint64_t nq, unsigned long long* guess,
               unsigned long long* err, unsigned long long* pos, rmi_hip_search_stats* st) {
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  if (st) *st = rmi_hip_search_stats{nq, 0, 0, 0};
  if (nq == 0) return RMI_OK;
  IXCHK(c, hipSetDevice(ix->device));
  LookupArgs a;
  a.r = ix->rp; a.rows = ix->d_rows; a.has_err = ix->has_err;
  a.keys = v.keys; a.n = ix->n; a.nm1 = (double)ix->n - 1.0;
  a.q = q; a.nq = nq; a.guess = guess; a.err = err; a.pos = pos; a.cnt = ix->d_cnt;
  const uint64_t G = mode == LM_SEARCH_COOP ? COOP_G : 1;
  const uint64_t want = (nq * G + 255) / 256;
  const uint64_t cap = (uint64_t)(v.n_cu > 0 ? v.n_cu : 256) * 8;       // 8 blocks of 4 waves per CU, striding over the queries
  const unsigned int grid = (unsigned int)(want < cap ? want : cap);
  IXCHK(c, hipMemsetAsync(ix->d_cnt, 0, 2 * sizeof(unsigned long long), v.stream));
  if (st) IXCHK(c, hipEventRecord(ix->ev[0], v.stream));
  switch (ix->dtype) {
    case RMI_KEY_U64: launch_root<uint64_t>(ix->lr, ix->ppl, mode, grid, a, v.stream); break;
    case RMI_KEY_U32: launch_root<uint32_t>(ix->lr, ix->ppl, mode, grid, a, v.stream); break;
    default: launch_root<double>(ix->lr, ix->ppl, mode, grid, a, v.stream); break;
  }
  IXCHK(c, hipGetLastError());
  if (!st) return RMI_OK;
  IXCHK(c, hipEventRecord(ix->ev[1], v.stream));
  IXCHK(c, hipMemcpyAsync(ix->h_cnt, ix->d_cnt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
  IXCHK(c, hipStreamSynchronize(v.stream));
  float ms = 0.f;
  IXCHK(c, hipEventElapsedTime(&ms, ix->ev[0], ix->ev[1]));
  st->fallbacks = mode == LM_LOOKUP ? 0 : ix->h_cnt[0];
  st->root_oob = ix->h_cnt[1];
  st->device_ns = (uint64_t)((double)ms * 1e6);
  return RMI_OK;
}

extern "C" {

int rmi_hip_index_lookup(rmi_hip_ctx* c, const rmi_hip_index* ix, const void* d_queries, uint64_t nq, int dtype,
                         uint64_t* d_guess, uint64_t* d_err, rmi_hip_search_stats* st) {
  if (!c || !ix || dtype != ix->dtype || (nq && (!d_queries || !d_guess))) return RMI_ERR_BAD_ARG;
  return run(c, ix, LM_LOOKUP, d_queries, nq, (unsigned long long*)d_guess, (unsigned long long*)d_err, nullptr, st);
}

int rmi_hip_index_search(rmi_hip_ctx* c, const rmi_hip_index* ix, const void* d_queries, uint64_t nq, int dtype,
                         uint64_t* d_pos, rmi_hip_search_stats* st) {
  if (!c || !ix || dtype != ix->dtype || (nq && !d_queries)) return RMI_ERR_BAD_ARG;
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  if (!v.keys || v.n == 0) return RMI_ERR_NO_KEYS;
  if (v.n != ix->n || v.dtype != ix->dtype) {
    ctx_set_error(c, "rmi_hip_index_search: the resident keys are not the index's (key count or dtype)");
    return RMI_ERR_BAD_ARG;
  }
  return run(c, ix, ix->variant ? LM_SEARCH_COOP : LM_SEARCH, d_queries, nq, nullptr, nullptr, (unsigned long long*)d_pos, st);
}

int rmi_hip_index_verify(rmi_hip_ctx* c, const rmi_hip_index* ix, uint64_t* checked, uint64_t* outside) {
  if (!c || !ix || !checked || !outside) return RMI_ERR_BAD_ARG;
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  rmi_hip_search_stats st;
  const int rc = rmi_hip_index_search(c, ix, v.keys, v.n, v.dtype, nullptr, &st);
  if (rc) return rc;
  *checked = st.queries;
  *outside = st.fallbacks;
  return RMI_OK;
}

int rmi_hip_device_alloc(rmi_hip_ctx* c, uint64_t bytes, void** d_out) {
  if (!c || !d_out) return RMI_ERR_BAD_ARG;
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  IXCHK(c, hipSetDevice(v.device));
  IXCHK(c, hipMalloc(d_out, bytes ? bytes : 8));
  return RMI_OK;
}

int rmi_hip_device_free(rmi_hip_ctx* c, void* d_ptr) {
  if (!c) return RMI_ERR_BAD_ARG;
  if (d_ptr) IXCHK(c, hipFree(d_ptr));
  return RMI_OK;
}

int rmi_hip_copy(rmi_hip_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c || (bytes && (!dst || !src))) return RMI_ERR_BAD_ARG;
  if (!bytes) return RMI_OK;
  CtxLookupView v;
  ctx_lookup_view(c, &v);
  IXCHK(c, hipSetDevice(v.device));
  IXCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, v.stream));
  IXCHK(c, hipStreamSynchronize(v.stream));
  return RMI_OK;
}

}  // extern "C"
