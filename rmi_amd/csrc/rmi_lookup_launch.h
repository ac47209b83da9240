// rmi_lookup_launch.h -- what the device index (rmi_lookup.hip) needs from a context of rmi_hip.hip: the two translation units
// share no types but these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rmi_hip.h"

namespace rmi {

// A context as the index sees it: its device, stream, resident keys and the last training's rows.
struct CtxLookupView {
  int device;
  hipStream_t stream;
  const void* keys;
  uint64_t n;
  int dtype;
  int n_cu;
  uint64_t generation;            // rmi_hip_result.generation of the last training (0: none)
  uint64_t last_L;                // its leaves (0: the arrays are gone, or a shard / streamed training owns them)
  int last_ppl;
  const void* rows;               // its packed rows (L * (ppl * 8 + 8) bytes, device)
  const uint32_t* table;          // the context's radix-table hint table (device), if any
  uint64_t table_entries;
};
void ctx_lookup_view(const rmi_hip_ctx* c, CtxLookupView* v);
void ctx_set_error(rmi_hip_ctx* c, const char* msg);
// the context frees the indexes still registered with it in rmi_hip_destroy (index_release)
void ctx_register_index(rmi_hip_ctx* c, rmi_hip_index* ix, bool add);
void index_release(rmi_hip_index* ix);

}  // namespace rmi
