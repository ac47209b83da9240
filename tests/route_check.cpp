// route_check.cpp -- prints the route planner's decisions (rmi_amd/csrc/rmi_route.h) on the CPU, for tests/test_route_cpu.py.
// The knobs come from the environment (read_knobs).  Every line of standard input is one training on one RouteMemory:
//   root=<model> leaf=<model> key=u64|u32|f64 n=<keys> [n_it=<keys of the launch; default n>] L=<leaves>
//   [slope_ok=1 cubic_finite=1 prefix=1 increasing=1 fit_mode=0 stream=0 defer=0 rows_ext=0 peers=0 n_cu=256 epoch=1]
//   [learn=1 scan_listed=0 flag_count=0 merged_count=0 regs_listed=0]   (after planning: RouteMemory::learn with these counts)
// and prints the route as key=value pairs, with how often the two edge-key facts were asked for.  The line `knobs` prints the knobs.
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../rmi_amd/csrc/rmi_route.h"

using namespace rmi_route;

static int model(const std::string& s) {
  static const std::map<std::string, int> m = {
      {"linear", RMI_MODEL_LINEAR}, {"linear_spline", RMI_MODEL_LINEAR_SPLINE}, {"cubic", RMI_MODEL_CUBIC}, {"radix", RMI_MODEL_RADIX},
      {"robust_linear", RMI_MODEL_ROBUST_LINEAR}, {"loglinear", RMI_MODEL_LOGLINEAR}, {"normal", RMI_MODEL_NORMAL},
      {"radix8", RMI_MODEL_RADIX8}, {"radix18", RMI_MODEL_RADIX18}, {"radix22", RMI_MODEL_RADIX22}, {"radix26", RMI_MODEL_RADIX26},
      {"radix28", RMI_MODEL_RADIX28}, {"bradix", RMI_MODEL_BRADIX}};
  return m.at(s);
}

int main() {
  const Knobs k = read_knobs();
  RouteMemory mem;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "knobs") {
      std::printf("pipeline=%d lanes_search=%d opt_tail=%d host_min=%llu host_min_set=%d regs=%d regs_forced=%d regs_u32=%d regs_grid=%u "
                  "regs_max_avg=%u regs_long_max_avg=%u regs_backoff=%d cubic_margin=%d cubic_margin_scale=%g lean=%d scan_waves=%u "
                  "fit_threads=%llu fit_min_chunk=%d long_min=%u\n",
                  k.pipeline, k.lanes_search, k.opt_tail, (unsigned long long)k.host_min, k.host_min_set, k.regs, k.regs_forced, k.regs_u32,
                  k.regs_grid, k.regs_max_avg, k.regs_long_max_avg, k.regs_backoff, k.cubic_margin, k.cubic_margin_scale, k.lean, k.scan_waves,
                  (unsigned long long)k.fit_threads, k.fit_min_chunk, k.long_min);
      continue;
    }
    std::map<std::string, std::string> a = {{"root", "linear"}, {"leaf", "linear"}, {"key", "u64"}, {"slope_ok", "1"}, {"cubic_finite", "1"},
                                            {"prefix", "1"}, {"increasing", "1"}, {"n_cu", "256"}, {"epoch", "1"}};
    std::istringstream ws(line);
    for (std::string w; ws >> w;) {
      const size_t eq = w.find('=');
      a[w.substr(0, eq)] = w.substr(eq + 1);
    }
    auto num = [&](const char* key) -> unsigned long long { return a.count(key) ? std::stoull(a[key]) : 0ull; };
    RouteIn in;
    in.root_kind = model(a["root"]); in.leaf_kind = model(a["leaf"]);
    in.key_type = a["key"] == "u32" ? RMI_KEY_U32 : a["key"] == "f64" ? RMI_KEY_F64 : RMI_KEY_U64;
    in.n = num("n"); in.n_it = a.count("n_it") ? num("n_it") : in.n; in.L_own = num("L");
    in.slope_ok = num("slope_ok"); in.cubic_finite = num("cubic_finite");
    int asked_prefix = 0, asked_increasing = 0;
    const bool prefix = num("prefix"), increasing = num("increasing");
    in.common_prefix = [&]() { asked_prefix++; return prefix; };
    in.cubic_increasing = [&]() { asked_increasing++; return increasing; };
    in.fit_mode = (int)num("fit_mode"); in.stream_mode = num("stream"); in.defer_sync = num("defer"); in.rows_ext = num("rows_ext");
    in.peer_fuse_n = (int)num("peers"); in.n_cu = (int)num("n_cu");
    const RouteKey key = {num("epoch"), in.L_own, in.fit_mode};
    mem.lookup(key, &in);
    const Route r = plan_route(k, in);
    if (num("learn"))
      mem.learn(key, r, k, in.stream_mode, {num("scan_listed"), num("flag_count"), num("merged_count"), (unsigned int)num("regs_listed")});
    std::printf("pipeline=%d sigma=%d search=%d init_arrays=%d init_folded=%d fused=%d optimistic=%d listed_late=%d peers=%d giants=%d "
                "giants_early=%d regs=%d regs_grid=%u verify=%d cubic_margin=%d scan_mono=%d lean=%d listed_hint=%u long_leaves=%d "
                "asked_prefix=%d asked_increasing=%d\n",
                r.pipeline, r.sigma, r.search, r.init_arrays(), r.init_folded, r.fused, r.optimistic, r.listed_late, r.peers, r.giants,
                r.giants_early, r.regs, r.regs_grid, r.verify, r.cubic_margin, r.scan_mono, r.lean, r.listed_hint, r.long_leaves,
                asked_prefix, asked_increasing);
  }
  return 0;
}
