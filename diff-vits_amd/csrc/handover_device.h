// The one bounded wait and the one report of the in-launch hand-overs (HandoverParams / HandoverStatus, dv_common.h).
// Every wait inside a launch of the default schedule is a handover_wait: gnx_finish_table (gnx_device.h: the GroupNorm
// exchange of k_gemm, k_conv3*, k_chain_ff, k_chain_xa_ff and k_ff_split), the all-gather of h and of the attention output
// in k_qkv_split, and the partial sums of k_ff_split.  (persist.hip, off by default, has a barrier of its own.)
//   when it gives up:      at the first unsatisfied poll after more than spin_max polls - or, looked at every 64th poll, as soon
//                          as ANY launch has reported: that run is lost already and will be repeated, waiting on costs ~0.4 s
//                          per launch for nothing;
//   what it leaves behind: a wave that ran out of polls writes the HandoverStatus record (a wave that leaves because the run is
//                          lost writes nothing) and the caller goes on with whatever words it has - the results of the run
//                          are invalid from here on, nothing hangs;
//   who reads it:          dv_unet_health (engine.hip) before every later call on the handle, dv_unet_handover_status for
//                          engine.py, which re-plans without hand-overs and repeats the run.
#pragma once
#include "dv_common.h"

// One lane calls it.  `id`: the launch's HandoverParams::words.  Payload first, then the word the host and the other waits look at.
__device__ __forceinline__ void handover_report(unsigned* status, const void* id, unsigned code, unsigned detail) {
  HandoverStatus* const r = reinterpret_cast<HandoverStatus*>(status);
  r->id = (unsigned)(size_t)id; r->wg = blockIdx.x; r->code = code; r->detail = detail;
  __hip_atomic_store(&r->timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Called by a whole wave.  `poll()` reads what the lane still misses and returns whether the lane has everything (it keeps its own
// state: the words it has seen, the last flag value).  True: every lane was satisfied.  False: gave up (see above) - `code` says
// which wait, the detail word is the number of lanes still missing something.  A plain function template: a capturing
// always_inline lambda around an epilogue step has cost k_gemm's 128 x 128 tile 40 registers before (gnx_block_stats).
template <typename Poll>
__device__ __forceinline__ bool handover_wait(Poll poll, unsigned* status, const int spin_max, const void* id, const unsigned code) {
  for (int spins = 0;; ++spins) {
    const bool ok = poll();
    if (__all(ok)) return true;
    const bool lost = (spins & 63) == 63 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
    if (lost) return false;
    if (spins > spin_max) {
      const unsigned missing = (unsigned)__builtin_popcountll(__ballot(!ok));
      if (__lane_id() == 0) handover_report(status, id, code, missing);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
