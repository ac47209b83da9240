// rmi_route.h -- which kernels a training runs: the route planner.  Plain host C++17 (no HIP): rmi_hip.hip plans every
// training with plan_route and launches the route it returns; tests/route_check.cpp prints routes on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <functional>

#include "../../include/rmi_hip.h"

namespace rmi_route {

// the kernels of pipelines 3-5 (and the one-pass kernel) index keys with 32 bits
constexpr uint64_t IDX32_LIMIT = (1ull << 32) - (1ull << 16);
constexpr uint64_t SIGMA_MIN_LEAF = 32;   // average keys per leaf below which the one-pass modes take the exact kernels
constexpr uint64_t SCAN_SKEW_LISTED = 512;   // tiles the short form of k_spline_scan left: above, the key set counts as skewed

// The environment's settings, read once per context (rmi_hip_create).
struct Knobs {
  int pipeline = 3;                   // RMI_HIP_PIPELINE: 2 = the streaming passes of round 2 (cubic / robust leaves take them anyway), 3 = all
  bool lanes_search = true;           // RMI_HIP_LANES_SEARCH=0: leaf boundaries by the bucketing scan even where the root allows the search
  bool opt_tail = true;               // RMI_HIP_OPT_TAIL=0: the list kernels in-stream (else behind the synchronisation, if a leaf was listed)
  uint64_t host_min = 262144;         // RMI_HIP_HOST_MIN: listed leaves of more points go to host cores (a wave: 7 ms for 262 144, a core: 1); 0: never
  bool host_min_set = false;          // ... given: the threshold alone decides (else only where the AVERAGE leaf is far below it)
  bool regs = true;                   // RMI_HIP_REGS=0: k_leaf_lanes for everything (pipeline 3)
  bool regs_forced = false;           // RMI_HIP_REGS=1: k_leaf_regs wherever it applies, whatever the number of groups
  int regs_u32 = 2;                   // RMI_HIP_REGS_U32, 4-byte keys: 2 = k_leaf_regs at two waves per SIMD, 1 = at one, 0 = k_leaf_lanes
  unsigned int regs_grid = 0;         // RMI_HIP_REGS_GRID: persistent waves of k_leaf_regs (0: 4 per CU, 8 for the two-wave variant)
  unsigned int regs_max_avg = 208;    // RMI_HIP_REGS_MAX_AVG: average keys per leaf above which most groups would not fit the stash (k_leaf_regs<K, LONG>)
  unsigned int regs_long_max_avg = 640;   // RMI_HIP_REGS_LONG_MAX_AVG: ... up to which k_leaf_regs<K, LONG> takes them; above: k_leaf_lanes
  bool regs_backoff = true;           // RMI_HIP_REGS_BACKOFF=0: k_leaf_regs also for key sets on which it listed most groups last time
  bool cubic_margin = true;           // RMI_HIP_CUBIC_MARGIN=0: cubic roots always with the per-key verification (k_leaf_lanes, pipeline 3)
  double cubic_margin_scale = 1.0;    // RMI_HIP_CUBIC_MARGIN_SCALE (testing): widens the margin (1e13: every leaf is verified key by key)
  bool lean = true;                   // RMI_HIP_LEAN=0: k_spline_scan writes all five arrays (else the rows and the bucket table only)
  unsigned int scan_waves = 0;        // RMI_HIP_SCAN_WAVES: persistent waves per scan kernel at most (0: as many as the device holds)
  uint64_t fit_threads = 131072;      // RMI_HIP_FIT_THREADS: lanes of pass A, pipeline 2 (256 CUs x 8 waves x 64)
  int fit_min_chunk = 64;             // RMI_HIP_FIT_MIN_CHUNK: its smallest chunk
  unsigned int long_min = 4096;       // RMI_HIP_LONG_MIN (>= 64): leaves with more points go to the long-leaf kernels
};

inline Knobs read_knobs() {
  Knobs k;
  auto env = [](const char* name) -> const char* { const char* v = std::getenv(name); return v && *v ? v : nullptr; };
  if (const char* v = env("RMI_HIP_PIPELINE")) k.pipeline = std::atoi(v) >= 3 ? 3 : 2;
  if (const char* v = env("RMI_HIP_LANES_SEARCH")) k.lanes_search = std::atoi(v) != 0;
  if (const char* v = env("RMI_HIP_OPT_TAIL")) k.opt_tail = std::atoi(v) != 0;
  if (const char* v = env("RMI_HIP_HOST_MIN")) { k.host_min = std::strtoull(v, nullptr, 10); k.host_min_set = true; }
  if (const char* v = env("RMI_HIP_REGS")) { k.regs = std::atoi(v) != 0; k.regs_forced = k.regs; }
  if (const char* v = env("RMI_HIP_REGS_U32")) k.regs_u32 = std::atoi(v);
  if (const char* v = env("RMI_HIP_REGS_GRID")) k.regs_grid = (unsigned int)std::atoi(v);
  if (const char* v = env("RMI_HIP_REGS_MAX_AVG")) k.regs_max_avg = (unsigned int)std::atoi(v);
  if (const char* v = env("RMI_HIP_REGS_LONG_MAX_AVG")) k.regs_long_max_avg = (unsigned int)std::atoi(v);
  if (const char* v = env("RMI_HIP_REGS_BACKOFF")) k.regs_backoff = std::atoi(v) != 0;
  if (const char* v = env("RMI_HIP_CUBIC_MARGIN")) k.cubic_margin = std::atoi(v) != 0;
  if (const char* v = env("RMI_HIP_CUBIC_MARGIN_SCALE")) k.cubic_margin_scale = std::atof(v);
  if (const char* v = env("RMI_HIP_LEAN")) k.lean = std::atoi(v) != 0;
  if (const char* v = env("RMI_HIP_SCAN_WAVES")) k.scan_waves = (unsigned int)std::atoi(v);
  if (const char* v = env("RMI_HIP_FIT_THREADS")) k.fit_threads = std::strtoull(v, nullptr, 10);
  if (const char* v = env("RMI_HIP_FIT_MIN_CHUNK")) k.fit_min_chunk = std::atoi(v);
  if (const char* v = env("RMI_HIP_LONG_MIN")) { const long l = std::atol(v); if (l >= 64) k.long_min = (unsigned int)l; }
  return k;
}

// What the route of a training depends on.
struct RouteIn {
  int root_kind = RMI_MODEL_LINEAR, leaf_kind = RMI_MODEL_LINEAR, key_type = RMI_KEY_U64;   // RMI_MODEL_*, RMI_KEY_*
  uint64_t n = 0, n_it = 0, L_own = 0;   // keys of the whole key set (of a shard: the global count), keys and leaves of this launch
  // the root: monotone by arithmetic?
  bool slope_ok = false;              // linear root: slope >= 0, both coefficients finite
  bool cubic_finite = false;          // cubic root: every coefficient finite
  std::function<bool()> common_prefix;     // radix root: every key shares its top `prefix` bits (reads the first and last key)
  std::function<bool()> cubic_increasing;  // cubic root: increasing over the keys' range as an exact polynomial (the same two keys)
  int fit_mode = 0;                   // rmi_hip_set_fit_mode
  bool stream_mode = false, defer_sync = false;   // a chunk of a streamed training; the caller synchronises and finishes (rmi_hip_train_sharded)
  bool rows_ext = false;              // the rows go to a caller's buffer (rmi_hip_set_rows_output)
  int peer_fuse_n = 0, n_cu = 256;    // direct exchange: peers whose tables the leaf kernels store rows to; compute units
  // what RouteMemory remembers of this key set and leaf count: the one-pass kernel listed most leaves, k_leaf_regs most groups; the tiles
  // k_spline_scan's short form left (~0u: not known), hundreds of them (the long-leaf instance)
  bool sigma_hinted = false, regs_off = false, scan_skew = false;
  unsigned int scan_hint = ~0u;
};

// The decision.
struct Route {
  int pipeline = 2;                   // what rmi_hip_last_pipeline reports: 2 (streaming passes), 3 (k_leaf_lanes), 4 (k_leaf_regs), 5 (k_spline_scan)
  bool sigma = false;                 // the one-pass kernel k_sigma2 (fit modes 1 / 2; reported as pipeline 2)
  // leaf boundaries
  bool search = false;                // k_leaf_samples + k_leaf_search (else, pipelines 3 / 4: the bucketing scan + fill)
  bool init_folded = false;           // no k_init: k_leaf_samples carries it
  // pipelines 3-5
  bool fused = false;                 // the error pass fused behind the fit (else k_err_range + k_finalize)
  bool optimistic = false;            // k_lane_reduce publishes the result early; the list kernels behind the synchronisation
  bool listed_late = false;           // pipeline 4: the groups k_leaf_regs listed run behind the synchronisation too
  bool peers = false;                 // the leaf kernels store the rows to the peers' tables
  bool giants = false, giants_early = false;   // giant leaves go to host cores; their list out in front of k_list (fitted beside it)
  int regs = -1;                      // pipeline 4: the k_leaf_regs variant (0, 1 = LONG, 2 = 4-byte keys at two waves per SIMD)
  unsigned int regs_grid = 0;         // ... and its persistent waves
  bool verify = false;                // cubic root: k_leaf_lanes<.., K_CUBIC> verifies every key's target
  bool cubic_margin = false;          // cubic root, pipeline 4: k_regs_finalize<K, K_CUBIC> checks every leaf's margin instead
  // pipeline 5 (k_spline_scan): the root is monotone by arithmetic (the short form of a tile); rows and bucket table only (k_lean_arrays
  // derives the rest when asked); waves for the general form's tiles, the long-leaf instance (RouteMemory)
  bool scan_mono = false, lean = false, long_leaves = false;
  unsigned int listed_hint = ~0u;
  bool lanes() const { return pipeline >= 3; }
  bool init_arrays() const { return pipeline != 5 && !init_folded; }   // k_init prepares leaf_start / maxerr / run
};

inline Route plan_route(const Knobs& k, const RouteIn& in) {
  Route r;
  const bool idx32 = in.n < IDX32_LIMIT, u32 = in.key_type == RMI_KEY_U32;
  const bool linear_leaf = in.leaf_kind == RMI_MODEL_LINEAR;        // (robust_linear leaves: their own fit, pipeline 2)
  const bool linear_root = in.root_kind == RMI_MODEL_LINEAR || in.root_kind == RMI_MODEL_ROBUST_LINEAR || in.root_kind == RMI_MODEL_LINEAR_SPLINE;
  const bool radix_root = in.root_kind == RMI_MODEL_RADIX || in.root_kind == RMI_MODEL_BRADIX, cubic_root = in.root_kind == RMI_MODEL_CUBIC;
  const uint64_t L = in.L_own;
  // pipeline 5: linear_spline leaves in one key-parallel pass -- every root, every key type, any number of keys (an empty shard as well)
  const bool scan = k.pipeline >= 3 && in.leaf_kind == RMI_MODEL_LINEAR_SPLINE && idx32;
  // one pass from sufficient statistics: leaves of a few dozen keys on average, not a key set on which it listed most leaves
  r.sigma = linear_leaf && in.fit_mode != 0 && !in.sigma_hinted && idx32 && in.n_it >= SIGMA_MIN_LEAF * L && in.n_it >= 4096;
  // the leaf-lane kernels (tiny key sets: the streaming passes)
  const bool lanes = (k.pipeline >= 3 && linear_leaf && !r.sigma && in.n_it >= 1024) || scan;
  r.fused = lanes && idx32;
  if (linear_root) { r.search = lanes && k.lanes_search && in.slope_ok; r.scan_mono = scan && in.slope_ok; }
  // cubic roots are not monotone by arithmetic: the search may assume it when the fused error pass verifies every key's target
  if (cubic_root) r.search = lanes && k.lanes_search && r.fused && linear_leaf && in.cubic_finite;
  if (radix_root && ((lanes && k.lanes_search) || scan)) {
    // (key << prefix) >> (64 - bits) is monotone in the key exactly when no key loses a distinguishing bit to the shift
    r.search = in.common_prefix();
    r.scan_mono = scan && r.search;
  }
  if (scan) r.search = false;                                       // (the scan finds the leaf starts itself)
  r.init_folded = !scan && r.fused && r.search;
  r.optimistic = r.fused && k.opt_tail && !in.stream_mode;
  r.peers = r.fused && in.peer_fuse_n > 0 && r.optimistic;
  r.listed_late = r.optimistic && !in.defer_sync && !r.peers;
  // giant leaves go to the host where this call ends with its own synchronisation, and are the OUTLIERS of a skewed key set: where the
  // average leaf is within a factor of four of the threshold nearly every leaf would go (400 M u32 keys in 1 024 leaves: 680 ms on the
  // host against 14 ms on the device)
  const bool giants_pay = k.host_min > 0 && (k.host_min_set || in.n_it / (L ? L : 1) <= k.host_min / 4);
  r.giants = linear_leaf && (r.sigma || r.fused) && giants_pay && !in.stream_mode && !in.defer_sync;
  r.giants_early = r.giants && (r.sigma || r.optimistic);
  if (r.sigma || !lanes) return r;                                  // (pipeline 2)
  if (scan) {
    // (a streamed / sharded training fills the arrays shard by shard, rows in a caller's buffer may be gone when the arrays are asked for;
    //  the general form's kernel gets twice as many waves as tiles the last training of this key set and leaf count left to it, and 64 more)
    r.pipeline = 5; r.lean = k.lean && !in.stream_mode && !in.defer_sync && !in.rows_ext; r.listed_hint = in.scan_hint; r.long_leaves = in.scan_skew;
    return r;
  }
  r.pipeline = 3;
  // pipeline 4: linear leaves short enough on average that most groups of 64 fit k_leaf_regs, not a key set on which it listed most groups
  // last time
  const uint64_t wb = (L + 63) / 64, resident = 4ull * (uint64_t)in.n_cu;   // groups of 64 leaves; resident waves of k_leaf_regs
  const bool regs_long = in.n_it > (uint64_t)k.regs_max_avg * L;   // long leaves on average: the LONG variant
  const unsigned int cap = k.regs_long_max_avg > k.regs_max_avg ? k.regs_long_max_avg : k.regs_max_avg;
  bool regs = r.fused && k.regs && !in.regs_off && in.n_it <= (uint64_t)cap * L && (!u32 || k.regs_u32);
  // Between one and two and a half groups per resident wave (M's shard at 8 GPUs: 2 048 groups on 1 024 waves) k_leaf_regs runs two rounds
  // of a group each behind its 20 us of start-up, k_leaf_lanes ONE round on twice the waves: 0.110 against 0.120 ms at 2 048 groups, equal
  // at 1 024, 0.186 against 0.177 at 4 096
  if (!regs_long && !k.regs_forced && k.regs_grid == 0 && wb > resident && 2 * wb <= 5 * resident) regs = false;
  // a cubic root on pipeline 4: increasing over the keys' range, every leaf's end keys clear their leaf's interval by the rounding bound
  // (k_regs_finalize<K, K_CUBIC>) -- else the per-key verification of k_leaf_lanes
  if (cubic_root && linear_leaf && r.search && regs && k.cubic_margin) r.cubic_margin = in.cubic_increasing();
  r.verify = cubic_root && linear_leaf && r.search && !r.cubic_margin;
  if (regs && !r.verify) {
    r.pipeline = 4;
    const bool w2 = u32 && k.regs_u32 >= 2;                           // two waves per SIMD
    r.regs = w2 ? 2 : regs_long ? 1 : 0;
    const uint64_t grid = k.regs_grid ? k.regs_grid : (w2 ? 8ull : 4ull) * (uint64_t)in.n_cu;
    r.regs_grid = (unsigned int)(grid > wb ? wb : grid);
  }
  return r;
}

// What the last trainings taught about a key set (`epoch`: the context's key-set counter), per leaf count.
struct RouteKey { uint64_t epoch; uint64_t L_own; int fit_mode; };
struct TrainCounts { uint64_t scan_listed, flag_count, merged_count; unsigned int regs_listed; };
struct RouteMemory {
  // A key set on which the one-pass kernel hands most leaves to the exact list kernels (duplicate-heavy keys; keys whose f64 images collapse,
  // guarded mode) is served faster by the exact path: 1.1 against 13.8 ms on 200 M duplicate-heavy keys.  Per (key set, leaf count, mode).
  uint64_t hint_epoch = 0, hint_L[8] = {};
  int hint_n = 0, hint_mode = -1;
  // ... likewise k_leaf_regs listing most groups (duplicate-heavy keys): the next trainings go to k_leaf_lanes, 0.80 against 2.25 ms
  uint64_t regs_off_epoch = 0, regs_off_L[8] = {};
  int regs_off_n = 0;
  // k_spline_scan: how many tiles the short form left the last time, and (key set, leaves) whose short form listed hundreds of tiles:
  // a skewed key set -- its next trainings take the long-leaf instance
  uint64_t scan_hint_epoch = 0, scan_hint_L = 0; unsigned int scan_hint_n = ~0u;
  uint64_t scan_skew_epoch = ~0ull, scan_skew_L = 0;

  void lookup(const RouteKey& key, RouteIn* in) const {
    in->sigma_hinted = hint_epoch == key.epoch && hint_mode == key.fit_mode && std::count(hint_L, hint_L + std::min(hint_n, 8), key.L_own) > 0;
    in->regs_off = regs_off_epoch == key.epoch && std::count(regs_off_L, regs_off_L + std::min(regs_off_n, 8), key.L_own) > 0;
    in->scan_hint = (scan_hint_epoch == key.epoch && scan_hint_L == key.L_own) ? scan_hint_n : ~0u;
    in->scan_skew = scan_skew_epoch == key.epoch && scan_skew_L == key.L_own;
  }

  void learn(const RouteKey& key, const Route& r, const Knobs& k, bool stream_mode, const TrainCounts& t) {
    if (r.pipeline == 5 && !stream_mode) {
      scan_hint_epoch = key.epoch; scan_hint_L = key.L_own; scan_hint_n = (unsigned int)(t.scan_listed < 0xFFFFFFFFull ? t.scan_listed : 0xFFFFFFFFull);
      if (t.scan_listed > SCAN_SKEW_LISTED) { scan_skew_epoch = key.epoch; scan_skew_L = key.L_own; }
    }
    if (r.sigma && (t.flag_count - t.merged_count) * 4 > key.L_own) {   // most leaves went through the list kernels
      if (hint_epoch != key.epoch || hint_mode != key.fit_mode) { hint_epoch = key.epoch; hint_mode = key.fit_mode; hint_n = 0; }
      hint_L[hint_n % 8] = key.L_own; hint_n++;
    }
    if (k.regs_backoff && k.regs && (uint64_t)t.regs_listed * 4 > (key.L_own + 63) / 64) {   // most groups went on the list
      if (regs_off_epoch != key.epoch) { regs_off_epoch = key.epoch; regs_off_n = 0; }
      regs_off_L[regs_off_n % 8] = key.L_own; regs_off_n++;
    }
  }
};

}  // namespace rmi_route
