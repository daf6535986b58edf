// Forced alignment of a recording against its phonemes: the score tensor and the monotonic alignment search of the reference's
// training forward (model3.py:767-794; monotonic_align/core.py), as two kernels that never leave the device.
//
//   k_mas_scores   neg_cent[b, y, x] = log N(z[b, :, y]; m_p[b, :, x], exp(logs_p[b, :, x])) summed over the C channels, in plain
//                  fp32 on the vector ALU.  One workgroup of 256 threads per 64 frames x 64 tokens, 4 x 4 cells per thread, the
//                  channel axis staged through LDS in chunks of 16.  ORDER OF THE ROUNDINGS (the test's bound is derived from it;
//                  every product, sum and fused multiply-add below is ONE float32 rounding, nothing is contracted or reassociated):
//                      s    = expf(-2 * logs_p)            (-2 * logs_p is exact; expf: at most 1 ulp, counted as 2 roundings)
//                      ms   = m_p * s                      (1)          per (token, channel), while the chunk is staged
//                      mm   = -0.5 * (m_p * m_p)           (1; the factor is exact)
//                      zz   = -0.5 * (z * z)               (1)          per (frame, channel)
//                      a_x  = a_x + (K - logs_p)           K = float32(-0.5 log 2 pi) (1), the difference (1), then one rounding
//                      d_x  = fma(mm, s, d_x)              per channel, channels in ascending order; a_x and d_x are the two
//                                                          per-token sums: ONE thread per token of the tile accumulates them
//                                                          (once per token and tile, 1/64 of the cell work, never once per cell)
//                      p_yx = fma(zz, s, p_yx)             one rounding per channel, ascending
//                      r_yx = fma(z, ms, r_yx)             one rounding per channel, ascending
//                      out  = ((a_x + p_yx) + r_yx) + d_x  (3)
//                  A summand therefore passes through at most 2 (s) + 1 (ms / mm / zz, or K and the difference: 2 without s) + C (its
//                  running sum) + 3 (the final additions) = C + 6 roundings, each at most 2^-24 relative to a partial sum that the
//                  sum of the summands' magnitudes bounds.  The test allows (C + 6) * 2^-23 * that sum: twice the first-order
//                  figure, which covers the second-order terms.  Cells outside an utterance's t_y x t_x are written as zeros
//                  (lengths clamped to 0 .. Ty / 0 .. Tx).  No MFMA: the tensor is under 1 GFLOP at the product's sizes.
//   k_mas_path     the search.  One wave per utterance; lane l owns columns [8 l, 8 l + 8) (Tx <= 512: the text encoder's own limit).
//                  Forward, rows y = 0 .. t_y - 1:  Q[y][x] = V[y][x] + max(P, C) with C = Q[y-1][x] (-1e9 where x == y) and
//                  P = Q[y-1][x-1] (x == 0: 0 in row 0, -1e9 below) - ONE fp32 addition per cell, which is bit for bit the reference's
//                  add-in-double-store-float32 (the double rounding of a sum of two floats is innocuous; -1e9 is exact in float32).
//                  The previous row lives in 8 registers per lane, the neighbour Q[y-1][8 l - 1] arrives by one cross-lane move
//                  (DPP wave shift) per row, there is no barrier in the row loop, and the rows of V are requested MAS_PF rows ahead
//                  into a register ring (addresses clamped into the utterance, never predicated).  Every column is computed in
//                  every row: a cell outside the band max(0, t_x + y - t_y) <= x <= min(t_x - 1, y) holds an arbitrary finite number
//                  that no in-band cell and no decision ever reads (an in-band cell's two predecessors are in the band of row y - 1).
//                  Q is not kept.  What is kept is the DECISION BIT of each cell, the backward condition evaluated while row y - 1 is
//                  in registers:  bit[y][x] = x != 0 and (x == y or Q[y-1][x] < Q[y-1][x-1])  (strict: a tie stays on the token) -
//                  one byte per lane and row.  The bytes live in LDS, ceil(Tx / 8) per row, while Ty * ceil(Tx / 8) <= 65536 (always
//                  when Ty <= 1024 - Ty * 64 bytes fit - and e.g. Ty <= 3449 at Tx = 150); beyond that they go to the caller's
//                  scratch (64 bytes per row) and come back to LDS 1024 rows at a time for the walk.  Ty <= 16384 (three minutes of
//                  frames), more is refused.  Backward: lane 0 walks down from (t_y - 1, t_x - 1) reading one bit per row and writes
//                  frame_token; durations[x] = lower_bound(frame_token, x + 1) - lower_bound(frame_token, x), one binary search pair
//                  per lane and column - no atomics, ordinary vector stores only.
//                  An utterance with t_x < 1, t_y < 1, t_x > t_y (the reference's loop is empty or its path garbage there) or a length
//                  beyond the padded dimensions is never searched: its durations AND frame_token rows are all -1, the other utterances
//                  are unaffected, nothing outside the buffers is touched - a value the caller checks, like y_len = -1 of the
//                  regulator.  Scores that are not finite give an unspecified (in-range) path.
//   k_mas_path<.., true> is the same kernel with two clock stamps (tools/align_bench.py: which part of a wave's time is the row
//                  loop); the product's instantiation executes no stamp.
// Ordering is by kernel boundary alone; nothing allocates or waits.
#include "../../include/dvits_hip.h"
#include "dv_common.h"

#include <cmath>

int dv_fail(int code, const char* fmt, ...);

namespace {

constexpr int MAS_TILE = 64;              // frames and tokens per score tile
constexpr int MAS_KC = 16;                // channels per LDS stage
constexpr int MAS_THREADS = 256;
constexpr int MAS_MAX_TX = 512;
constexpr int MAS_MAX_TY = 16384;
constexpr int MAS_LDS_BYTES = 65536;      // decision bits held in LDS
constexpr int MAS_WALK_ROWS = MAS_LDS_BYTES / 64;   // rows of scratch bits staged per walk chunk
constexpr int MAS_PF = 4;                 // rows of V in flight
constexpr float MAS_NEG = -1e9f;

__device__ __forceinline__ int mas_clamp_len(int64_t l, int T) { return l < 0 ? 0 : (l > T ? T : (int)l); }

__global__ __launch_bounds__(MAS_THREADS) void k_mas_scores(const float* __restrict__ z, const float* __restrict__ m_p,
                                                            const float* __restrict__ logs_p, const int64_t* __restrict__ y_lengths,
                                                            const int64_t* __restrict__ x_lengths, int C, int Ty, int Tx,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_z[MAS_KC][MAS_TILE], s_zz[MAS_KC][MAS_TILE];      // frames
  __shared__ __attribute__((aligned(16))) float s_s[MAS_KC][MAS_TILE], s_ms[MAS_KC][MAS_TILE];      // tokens
  __shared__ float s_mm[MAS_KC][MAS_TILE], s_kl[MAS_KC][MAS_TILE];
  __shared__ __attribute__((aligned(16))) float s_a[MAS_TILE], s_d[MAS_TILE];
  const int b = blockIdx.z, y0 = blockIdx.y * MAS_TILE, x0 = blockIdx.x * MAS_TILE, tid = threadIdx.x;
  const int ty = mas_clamp_len(y_lengths[b], Ty), tx = mas_clamp_len(x_lengths[b], Tx);
  const int cx = (tid & 15) * 4, cy = (tid >> 4) * 4;          // this thread's 4 tokens / 4 frames inside the tile
  if (y0 >= ty || x0 >= tx) {                                  // a tile of padding only (uniform over the workgroup)
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        if (y0 + cy + i < Ty && x0 + cx + j < Tx) out[((int64_t)b * Ty + y0 + cy + i) * Tx + x0 + cx + j] = 0.0f;
    return;
  }
  const float K = -0.91893853320467274178f;                    // -0.5 log(2 pi), rounded to float32 by the compiler
  const int col = tid & 63, k4 = tid >> 6;                     // staging: column of the tile, channel k4 + 4 i of the chunk
  const float* zb = z + (int64_t)b * C * Ty;
  const float* mb = m_p + (int64_t)b * C * Tx;
  const float* lb = logs_p + (int64_t)b * C * Tx;
  float p[4][4], r[4][4], a = 0.0f, d = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) p[i][j] = r[i][j] = 0.0f;
  for (int c0 = 0; c0 < C; c0 += MAS_KC) {
    const int kc = C - c0 < MAS_KC ? C - c0 : MAS_KC;
#pragma unroll
    for (int i = 0; i < MAS_KC / 4; ++i) {
      const int k = k4 + 4 * i, c = c0 + k;
      float zv = 0.0f, mv = 0.0f, lv = 0.0f;
      if (c < C) {
        if (y0 + col < Ty) zv = zb[(int64_t)c * Ty + y0 + col];
        if (x0 + col < Tx) { mv = mb[(int64_t)c * Tx + x0 + col]; lv = lb[(int64_t)c * Tx + x0 + col]; }
      }
      const float sv = expf(__fmul_rn(-2.0f, lv));
      s_z[k][col] = zv;
      s_zz[k][col] = __fmul_rn(-0.5f, __fmul_rn(zv, zv));
      s_s[k][col] = sv;
      s_ms[k][col] = __fmul_rn(mv, sv);
      s_mm[k][col] = __fmul_rn(-0.5f, __fmul_rn(mv, mv));
      s_kl[k][col] = __fsub_rn(K, lv);
    }
    __syncthreads();
    if (tid < MAS_TILE) {                                      // the two per-token sums: one thread per token, channels ascending
      for (int k = 0; k < kc; ++k) {
        a = __fadd_rn(a, s_kl[k][tid]);
        d = __fmaf_rn(s_mm[k][tid], s_s[k][tid], d);
      }
    }
    for (int k = 0; k < kc; ++k) {
      const float4 zv = *reinterpret_cast<const float4*>(&s_z[k][cy]), zz = *reinterpret_cast<const float4*>(&s_zz[k][cy]);
      const float4 sv = *reinterpret_cast<const float4*>(&s_s[k][cx]), ms = *reinterpret_cast<const float4*>(&s_ms[k][cx]);
      const float zr[4] = {zv.x, zv.y, zv.z, zv.w}, zzr[4] = {zz.x, zz.y, zz.z, zz.w};
      const float sr[4] = {sv.x, sv.y, sv.z, sv.w}, msr[4] = {ms.x, ms.y, ms.z, ms.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[i][j] = __fmaf_rn(zzr[i], sr[j], p[i][j]);
          r[i][j] = __fmaf_rn(zr[i], msr[j], r[i][j]);
        }
    }
    __syncthreads();                                           // the stage is rewritten by the next chunk
  }
  if (tid < MAS_TILE) { s_a[tid] = a; s_d[tid] = d; }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + cy + i;
    if (y >= Ty) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + cx + j;
      if (x >= Tx) continue;
      const float v = __fadd_rn(__fadd_rn(__fadd_rn(s_a[cx + j], p[i][j]), r[i][j]), s_d[cx + j]);
      out[((int64_t)b * Ty + y) * Tx + x] = (y < ty && x < tx) ? v : 0.0f;
    }
  }
}

// lane l <- lane l - 1 over the whole wave (lane 0 keeps its own value: it is never used there)
__device__ __forceinline__ float mas_from_left(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// LDS_BITS: the decision bytes stay in LDS (stride = ceil(Tx / 8) bytes per row); otherwise they go to `scratch`, 64 bytes per row.
template <bool LDS_BITS, bool STAMP>
__global__ __launch_bounds__(64) void k_mas_path(const float* __restrict__ V, const int64_t* __restrict__ y_lengths,
                                                 const int64_t* __restrict__ x_lengths, int Ty, int Tx, int32_t* durations,
                                                 int32_t* frame_token, uint8_t* scratch, int64_t* ticks) {
  __shared__ __attribute__((aligned(16))) uint8_t s_bits[MAS_LDS_BYTES];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t ly = y_lengths[b], lx = x_lengths[b];
  int32_t* dur = durations + (int64_t)b * Tx;
  int32_t* ft = frame_token + (int64_t)b * Ty;
  if (lx < 1 || ly < 1 || lx > ly || lx > Tx || ly > Ty) {     // never searched: a value for the caller (uniform over the wave)
    for (int x = lane; x < Tx; x += 64) dur[x] = -1;
    for (int y = lane; y < Ty; y += 64) ft[y] = -1;
    if (STAMP && lane == 0) ticks[2 * b] = ticks[2 * b + 1] = 0;
    return;
  }
  const int ty = (int)ly, tx = (int)lx;
  const int stride = LDS_BITS ? (Tx + 7) >> 3 : 64;            // bytes of decision bits per row
  uint8_t* gbits = LDS_BITS ? nullptr : scratch + (int64_t)b * Ty * 64;
  const float* v = V + (int64_t)b * Ty * Tx;
  const int x0 = lane * 8;
  int xc[8];                                                   // this lane's columns, clamped into the utterance
#pragma unroll
  for (int j = 0; j < 8; ++j) xc[j] = x0 + j < tx ? x0 + j : tx - 1;
  long long t0 = 0, t1 = 0;
  if (STAMP) t0 = wall_clock64();

  float q[8], vb[MAS_PF][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] = 0.0f;
#pragma unroll
  for (int k = 0; k < MAS_PF; ++k) {
    const float* row = v + (int64_t)(k < ty ? k : ty - 1) * Tx;
#pragma unroll
    for (int j = 0; j < 8; ++j) vb[k][j] = row[xc[j]];
  }
  for (int yb = 0; yb < ty; yb += MAS_PF) {
#pragma unroll
    for (int k = 0; k < MAS_PF; ++k) {
      const int y = yb + k;
      if (y < ty) {                                            // uniform over the wave
        const float left = mas_from_left(q[7]);
        const float first = y == 0 ? 0.0f : MAS_NEG;
        float qn[8];
        unsigned bits = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int x = x0 + j;
          const float prev = j == 0 ? left : q[j - 1];
          const float P = x == 0 ? first : prev;
          const float Cq = x == y ? MAS_NEG : q[j];
          bits |= (unsigned)(x != 0 && (x == y || q[j] < prev)) << j;
          qn[j] = __fadd_rn(vb[k][j], fmaxf(P, Cq));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = qn[j];
        if (LDS_BITS) {
          if (lane < stride) s_bits[y * stride + lane] = (uint8_t)bits;
        } else {
          gbits[(int64_t)y * 64 + lane] = (uint8_t)bits;
        }
        const int yn = y + MAS_PF;                             // the ring slot is free: request the row MAS_PF below
        const float* row = v + (int64_t)(yn < ty ? yn : ty - 1) * Tx;
#pragma unroll
        for (int j = 0; j < 8; ++j) vb[k][j] = row[xc[j]];
      }
    }
  }
  if (STAMP) t1 = wall_clock64();
  __syncthreads();                                             // one wave: orders the bit stores before the walk's loads

  int idx = tx - 1;
  const int chunk = LDS_BITS ? ty : MAS_WALK_ROWS;
  for (int hi = ty; hi > 0; hi -= chunk) {
    const int lo = hi - chunk > 0 ? hi - chunk : 0;
    if (!LDS_BITS) {                                           // rows [lo, hi) of the scratch bits -> LDS, 16 bytes per lane and step
      const uint4* src = reinterpret_cast<const uint4*>(gbits + (int64_t)lo * 64);
      uint4* dst = reinterpret_cast<uint4*>(s_bits);
      for (int i = lane; i < (hi - lo) * 4; i += 64) dst[i] = src[i];
      __syncthreads();
    }
    if (lane == 0) {
      for (int y = hi - 1; y >= lo; --y) {
        ft[y] = idx;
        const unsigned byte = s_bits[(y - lo) * stride + (idx >> 3)];
        idx -= (int)((byte >> (idx & 7)) & 1u);
      }
    }
    __syncthreads();                                           // the stage is rewritten by the next chunk; ft is read below
  }
  for (int y = ty + lane; y < Ty; y += 64) ft[y] = -1;
  // durations: frame_token is non-decreasing over [0, t_y) and holds every token of 0 .. t_x - 1
  for (int x = lane; x < Tx; x += 64) {
    int n = 0;
    if (x < tx) {
      int bound[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {                            // first y in [0, t_y) with frame_token[y] >= x + e, or t_y
        int lo = 0, hi = ty;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (ft[mid] >= x + e) hi = mid; else lo = mid + 1;
        }
        bound[e] = lo;
      }
      n = bound[1] - bound[0];
    }
    dur[x] = n;
  }
  if (STAMP && lane == 0) {
    ticks[2 * b] = t1 - t0;
    ticks[2 * b + 1] = wall_clock64() - t0;
  }
}

bool mas_bits_in_lds(int Ty, int Tx) { return (int64_t)Ty * ((Tx + 7) >> 3) <= MAS_LDS_BYTES; }

int mas_path(const char* who, const float* neg_cent, const int64_t* y_lengths, const int64_t* x_lengths, int32_t B, int32_t Ty,
             int32_t Tx, int32_t* durations, int32_t* frame_token, void* scratch, int64_t scratch_bytes, int64_t* ticks, bool stamp,
             void* stream) {
  if (!neg_cent || !y_lengths || !x_lengths || !durations || !frame_token || (stamp && !ticks))
    return dv_fail(DV_ERR_INVALID, "%s: null argument", who);
  if (B < 1 || Ty < 1 || Tx < 1) return dv_fail(DV_ERR_INVALID, "%s: B = %d, Ty = %d, Tx = %d must be >= 1", who, B, Ty, Tx);
  if (Tx > MAS_MAX_TX || Ty > MAS_MAX_TY)
    return dv_fail(DV_ERR_INVALID, "%s: Tx = %d exceeds %d or Ty = %d exceeds %d", who, Tx, MAS_MAX_TX, Ty, MAS_MAX_TY);
  const int64_t need = dv_op_mas_scratch_bytes(B, Ty, Tx);
  if (need > 0 && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 15)))
    return dv_fail(DV_ERR_INVALID, "%s: Ty = %d, Tx = %d needs %lld bytes of 16-byte aligned scratch (dv_op_mas_scratch_bytes), got %lld",
                   who, Ty, Tx, (long long)need, (long long)(scratch ? scratch_bytes : 0));
  hipStream_t st = (hipStream_t)stream;
  uint8_t* sc = (uint8_t*)scratch;
  const bool lds = need == 0;
  if (lds && !stamp)
    hipLaunchKernelGGL((k_mas_path<true, false>), dim3(B), dim3(64), 0, st, neg_cent, y_lengths, x_lengths, Ty, Tx, durations, frame_token, sc, ticks);
  else if (lds)
    hipLaunchKernelGGL((k_mas_path<true, true>), dim3(B), dim3(64), 0, st, neg_cent, y_lengths, x_lengths, Ty, Tx, durations, frame_token, sc, ticks);
  else if (!stamp)
    hipLaunchKernelGGL((k_mas_path<false, false>), dim3(B), dim3(64), 0, st, neg_cent, y_lengths, x_lengths, Ty, Tx, durations, frame_token, sc, ticks);
  else
    hipLaunchKernelGGL((k_mas_path<false, true>), dim3(B), dim3(64), 0, st, neg_cent, y_lengths, x_lengths, Ty, Tx, durations, frame_token, sc, ticks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return DV_OK;
}

}  // namespace

extern "C" int64_t dv_op_mas_scratch_bytes(int32_t B, int32_t Ty, int32_t Tx) {
  if (B < 1 || Ty < 1 || Tx < 1 || Tx > MAS_MAX_TX || Ty > MAS_MAX_TY) return -1;
  return mas_bits_in_lds(Ty, Tx) ? 0 : (int64_t)B * Ty * 64;
}

extern "C" int dv_op_mas_scores(const float* z, const float* m_p, const float* logs_p, const int64_t* y_lengths,
                                const int64_t* x_lengths, int32_t B, int32_t C, int32_t Ty, int32_t Tx, float* neg_cent, void* stream) {
  if (!z || !m_p || !logs_p || !y_lengths || !x_lengths || !neg_cent) return dv_fail(DV_ERR_INVALID, "dv_op_mas_scores: null argument");
  if (B < 1 || C < 1 || Ty < 1 || Tx < 1)
    return dv_fail(DV_ERR_INVALID, "dv_op_mas_scores: B = %d, C = %d, Ty = %d, Tx = %d must be >= 1", B, C, Ty, Tx);
  if (B > 65535 || Ty > 65535 * MAS_TILE) return dv_fail(DV_ERR_INVALID, "dv_op_mas_scores: B = %d exceeds 65535 or Ty = %d exceeds %d", B, Ty, 65535 * MAS_TILE);
  const dim3 grid((Tx + MAS_TILE - 1) / MAS_TILE, (Ty + MAS_TILE - 1) / MAS_TILE, B);
  hipLaunchKernelGGL(k_mas_scores, grid, dim3(MAS_THREADS), 0, (hipStream_t)stream, z, m_p, logs_p, y_lengths, x_lengths, C, Ty, Tx, neg_cent);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_mas_scores: launch failed: %s", hipGetErrorString(e));
  return DV_OK;
}

extern "C" int dv_op_mas_path(const float* neg_cent, const int64_t* y_lengths, const int64_t* x_lengths, int32_t B, int32_t Ty, int32_t Tx,
                              int32_t* durations, int32_t* frame_token, void* scratch, int64_t scratch_bytes, void* stream) {
  return mas_path("dv_op_mas_path", neg_cent, y_lengths, x_lengths, B, Ty, Tx, durations, frame_token, scratch, scratch_bytes, nullptr,
                  false, stream);
}

extern "C" int dv_op_mas_path_timed(const float* neg_cent, const int64_t* y_lengths, const int64_t* x_lengths, int32_t B, int32_t Ty,
                                    int32_t Tx, int32_t* durations, int32_t* frame_token, void* scratch, int64_t scratch_bytes,
                                    int64_t* ticks, void* stream) {
  return mas_path("dv_op_mas_path_timed", neg_cent, y_lengths, x_lengths, B, Ty, Tx, durations, frame_token, scratch, scratch_bytes, ticks,
                  true, stream);
}
