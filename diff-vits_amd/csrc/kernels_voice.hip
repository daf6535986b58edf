// Enrolled voices (engine.hip: dv_voice_capture / dv_unet_bind_voices): a voice record is a snapshot of one batch row of
// every persistent buffer the conditioning schedule (dv_unet_set_cond) writes and the step schedule reads - the K / V^T
// fragments of the transformer blocks, the key-bias rows, the pooled-text row, ... - laid end to end in 16-byte chunks.
//
//   k_voice_gather    buffers' row r  -> record       (after a dv_unet_set_cond: snapshot)
//   k_voice_scatter   record          -> buffers' row r  (bind: the bytes set_cond would have written there)
//
// Grid = (16-byte chunks of one record / VOICE_THREADS, rows of this call).  The conditioning segment table (VoiceSeg[],
// device memory, sorted by first chunk) says which buffer a chunk belongs to (one search per workgroup); the (row, record) pairs of the call travel in
// the kernel's argument block, which the device reads like any other memory (blockIdx.y is uniform: scalar loads): no
// upload, no allocation, no wait - the launch can be captured into a graph, and a replay reads the pairs the capture saw.
// A segment whose bytes per utterance are a multiple of 16 moves as uint4 (every base is 256-byte aligned, so a row's
// slice is 16-byte aligned too); any other segment - the [B, L] mask bias at an L that is no multiple of 4 - has unaligned
// slices and moves float by float: the RECORD is padded to whole chunks (zeros), never the buffer.  Every byte is
// written by exactly one thread; plain vector loads and stores.
#include "dv_common.h"

namespace {

constexpr int VOICE_THREADS = 256;

struct VoicePair { char* rec; int32_t row; int32_t pad_; };
struct VoiceArgs {
  const VoiceSeg* segs;
  int32_t nseg;
  uint32_t chunks;                       // 16-byte chunks of one record
  VoicePair pairs[DV_VOICE_MAX_ROWS];
};
static_assert(sizeof(VoiceArgs) <= 4096, "the argument block of a launch holds 4 KiB");

template <bool SCATTER>
__device__ __forceinline__ void voice_move(const VoiceArgs& a) {
  const uint32_t c = blockIdx.x * VOICE_THREADS + threadIdx.x;
  if (c >= a.chunks) return;
  // the last segment that starts at or before chunk c: searched once per workgroup for its first chunk (uniform: scalar loads),
  // then each thread steps over the few segment starts inside the workgroup's 4 KiB of the record
  const uint32_t c_wg = blockIdx.x * VOICE_THREADS;
  int lo = 0, hi = a.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.segs[mid].chunk0 <= c_wg) lo = mid; else hi = mid - 1;
  }
  while (lo + 1 < a.nseg && a.segs[lo + 1].chunk0 <= c) ++lo;
  const VoiceSeg s = a.segs[lo];
  const VoicePair p = a.pairs[blockIdx.y];
  const uint32_t off = (c - s.chunk0) * 16u;             // < s.bytes: the table gives a segment ceil(bytes / 16) chunks
  char* buf = s.base + (size_t)p.row * s.bytes + off;
  char* rec = p.rec + (size_t)c * 16u;
  if ((s.bytes & 15u) == 0) {
    if (SCATTER) *reinterpret_cast<uint4*>(buf) = *reinterpret_cast<const uint4*>(rec);
    else *reinterpret_cast<uint4*>(rec) = *reinterpret_cast<const uint4*>(buf);
    return;
  }
  const uint32_t left = s.bytes - off, nw = (left < 16u ? left : 16u) / 4u;   // floats of this chunk that exist in the buffer
  uint32_t* b32 = reinterpret_cast<uint32_t*>(buf);
  uint32_t* r32 = reinterpret_cast<uint32_t*>(rec);
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    if (SCATTER) { if (i < nw) b32[i] = r32[i]; }
    else r32[i] = i < nw ? b32[i] : 0u;
  }
}

__global__ __launch_bounds__(VOICE_THREADS) void k_voice_gather(const VoiceArgs a) { voice_move<false>(a); }
__global__ __launch_bounds__(VOICE_THREADS) void k_voice_scatter(const VoiceArgs a) { voice_move<true>(a); }

hipError_t voice_launch(bool scatter, const VoiceSeg* segs_dev, int nseg, uint32_t chunks, const int32_t* rows, void* const* recs,
                        int n, hipStream_t st) {
  if (!segs_dev || nseg < 1 || chunks < 1 || !rows || !recs || n < 1) return hipErrorInvalidValue;
  // (one launch per call up to DV_VOICE_MAX_ROWS rows - what an argument block holds; a larger batch takes one more per
  // DV_VOICE_MAX_ROWS rows)
  for (int r0 = 0; r0 < n; r0 += DV_VOICE_MAX_ROWS) {
    const int m = n - r0 < DV_VOICE_MAX_ROWS ? n - r0 : DV_VOICE_MAX_ROWS;
    VoiceArgs a{};
    a.segs = segs_dev; a.nseg = nseg; a.chunks = chunks;
    for (int i = 0; i < m; ++i) { a.pairs[i].rec = static_cast<char*>(recs[r0 + i]); a.pairs[i].row = rows[r0 + i]; }
    const dim3 grid((chunks + VOICE_THREADS - 1) / VOICE_THREADS, m);
    if (scatter) hipLaunchKernelGGL(k_voice_scatter, grid, dim3(VOICE_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_voice_gather, grid, dim3(VOICE_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_voice_gather(const VoiceSeg* segs_dev, int nseg, uint32_t chunks, const int32_t* rows, void* const* recs, int n,
                               hipStream_t st) {
  return voice_launch(false, segs_dev, nseg, chunks, rows, recs, n, st);
}

hipError_t launch_voice_scatter(const VoiceSeg* segs_dev, int nseg, uint32_t chunks, const int32_t* rows, void* const* recs, int n,
                                hipStream_t st) {
  return voice_launch(true, segs_dev, nseg, chunks, rows, recs, n, st);
}
