// Relative-position self-attention of the text encoder (reference attentions.py:142-300, MultiHeadAttention with
// window_size relative key / value embeddings shared by the heads; restated in oracle/text_enc_ref.py rel_attention).
//
// One wave per (utterance, head, 32-query block); a streaming (online-softmax) loop over 32-key tiles of the utterance's VALID
// keys only: the reference's masked_fill(-1e4) gives a padded key exactly zero weight in fp32 for a valid query, so leaving
// the padded keys out is the same result.  Query rows [length, T) are written as zeros (no valid row ever reads them).
//
// Products: S^T = K Q^T and O^T += V^T P^T on the MFMA fragments of attn_tile.h - lane = query, registers = keys / channels;
// Q and K as split bf16 (hi*hi + lo*hi + hi*lo), P and V as the other attention kernels carry them (DV_ATTN_PF16: P one
// fp16 plane, V split fp16).  At this size (T <= a few hundred tokens, 2 heads) the operands are read straight from global
// memory in fragment order - a K fragment is 8 consecutive floats of one key row, a V^T fragment 8 keys of one channel
// (32 lanes = 32 consecutive channels: whole 128-byte lines) - so the kernel has no LDS staging, no DMA and no barrier
// that orders waves: every load is an ordinary compiler-tracked load bounded by the utterance's token count.
//
// The two band terms are <= 2w + 1 dot products of length d per query, in fp32 on the vector ALU:
//   keys:   rel[i][r] = scale q_i . E_k[r] is computed once per query before the loop (LDS, 32 x (2w + 1) floats) and added to
//           the scores of the key tiles that overlap [i - w, i + w];
//   values: the band's FINAL probabilities are needed.  The <= 2w + 1 band scores of a query are carried through the loop
//           (written to LDS when their tile passes; each (query, offset) is met exactly once) and normalised after it with the
//           final running maximum and sum: p = exp2(s - m) / l.  The alternative - recomputing the band's q . k after the loop -
//           repeats 2w + 1 length-d dot products per query in another precision than the scores that entered the softmax; the
//           carried scores ARE those scores, and cost one LDS word each.
#include "attn_tile.h"

namespace {

constexpr int RA_RP = 2 * DV_RELATTN_MAX_WINDOW + 1;   // LDS row pitch (floats) of the per-query band tables: odd, conflict-free

__device__ __forceinline__ void ra_split8(const float4 a, const float4 c2, bf16x8& hi, bf16x8& lo) {
  u32x4 hw, lw;
  hw.x = apk(a.x, a.y); hw.y = apk(a.z, a.w); hw.z = apk(c2.x, c2.y); hw.w = apk(c2.z, c2.w);
  lw.x = apk(a.x - bf_lo(hw.x), a.y - bf_hi(hw.x)); lw.y = apk(a.z - bf_lo(hw.y), a.w - bf_hi(hw.y));
  lw.z = apk(c2.x - bf_lo(hw.z), c2.y - bf_hi(hw.z)); lw.w = apk(c2.z - bf_lo(hw.w), c2.w - bf_hi(hw.w));
  hi = __builtin_bit_cast(bf16x8, hw);
  lo = __builtin_bit_cast(bf16x8, lw);
}

// 16 values of one query row in the transposed-accumulator layout (v[4g + e] = column 8g + 4lh + e of a 32-column fragment)
// -> fp32 and / or split planes; `o` = element offset of the fragment's first column.  Both lanes of a pair are active.
__device__ __forceinline__ void ra_store_frag(const RelAttnParams& p, size_t o, int lh, const float* v) {
  if (p.o) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(p.o + o + 8 * g + 4 * lh) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
  }
  if (p.o_hi) store_planes16(p.o_hi, p.o_lo, o, lh, v, 3);
}

template <int D>
__global__ __launch_bounds__(64) void k_rel_attention(const RelAttnParams p) {
  constexpr int KS = D / 16, NB = D / 32;
  constexpr float LOG2E = 1.44269504088896340736f;
  __shared__ float s_rel[32 * RA_RP];    // scale * log2 e * q_i . E_k[r]
  __shared__ float s_band[32 * RA_RP];   // the band's scores (log2 domain), then its probabilities
  const int lane = threadIdx.x, l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 32;
  const int T = p.T, w = p.window, nrel = 2 * w + 1;
  const long long len64 = p.lengths[b];
  const int len = len64 < 0 ? 0 : (len64 > (long long)T ? T : (int)len64);
  const int qi = q0 + l31;
  const bool q_in = qi < T, q_ok = qi < len;
  const size_t row0 = (size_t)b * T;
  const size_t obase = (row0 + (q_in ? qi : 0)) * p.ldo + (size_t)h * D;

  if (q0 >= len) {                        // a block of padded queries (wave-uniform): zeros
    if (q_in) {
      float z[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) ra_store_frag(p, obase + nb * 32, lh, z);
    }
    return;
  }
  // (len >= 1 from here on; a padded query of a partly valid block computes on q = 0 and is stored as zeros)
  const float qscale = p.scale * LOG2E;
  const float* const qp = p.q + (row0 + (q_ok ? qi : 0)) * p.ldq + (size_t)h * D;

  // ---- Q fragments (B operand of K Q^T): lane (query, lh) holds channels ks*16 + lh*8 .. +8 ----
  bf16x8 qh[KS], ql[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = ks * 16 + lh * 8;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c2 = a;
    if (q_ok) { a = *reinterpret_cast<const float4*>(qp + c); c2 = *reinterpret_cast<const float4*>(qp + c + 4); }
    a.x *= qscale; a.y *= qscale; a.z *= qscale; a.w *= qscale;
    c2.x *= qscale; c2.y *= qscale; c2.z *= qscale; c2.w *= qscale;
    ra_split8(a, c2, qh[ks], ql[ks]);
  }
  // ---- relative key logits of this block's queries, fp32: lane (query, lh) takes offsets lh, lh + 2, ... ----
  for (int r = lh; r < nrel; r += 2) {
    float acc = 0.f;
    if (q_ok) {
      const float* ek = p.emb_k + (size_t)r * D;
#pragma unroll 4
      for (int c = 0; c < D; c += 4) {
        const float4 a = *reinterpret_cast<const float4*>(qp + c);
        const float4 e = *reinterpret_cast<const float4*>(ek + c);
        acc = fmaf(a.x, e.x, acc); acc = fmaf(a.y, e.y, acc); acc = fmaf(a.z, e.z, acc); acc = fmaf(a.w, e.w, acc);
      }
    }
    s_rel[l31 * RA_RP + r] = acc * qscale;
    s_band[l31 * RA_RP + r] = -1e30f;     // offsets whose key does not exist keep this: probability 0
  }
  __syncthreads();

  f32x16 o[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nb][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  const int nt = (len + 31) / 32;
  for (int kt = 0; kt < nt; ++kt) {
    const int k0 = kt * 32;
    // ---- S^T = K Q^T: lane (key l31, lh) reads channels ks*16 + lh*8 .. +8 of its key row (clamped: masked below) ----
    const float* const kp = p.k + (row0 + (size_t)min(k0 + l31, len - 1)) * p.ldk + (size_t)h * D + lh * 8;
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4 a = *reinterpret_cast<const float4*>(kp + ks * 16);
      const float4 c2 = *reinterpret_cast<const float4*>(kp + ks * 16 + 4);
      bf16x8 kh, kl;
      ra_split8(a, c2, kh, kl);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qh[ks], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, ql[ks], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qh[ks], s, 0, 0, 0);
    }
    // ---- key band: only the tiles that overlap [q0 - w, q0 + 31 + w] (wave-uniform); register r = key 8(r>>2) + 4lh + (r&3) ----
    if (k0 <= q0 + 31 + w && k0 + 31 >= q0 - w) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + 8 * (r >> 2) + 4 * lh + (r & 3);
        const int rel = key - qi + w;
        if (rel >= 0 && rel < nrel && key < len) {
          const float v = s[r] + s_rel[l31 * RA_RP + rel];
          s[r] = v;
          s_band[l31 * RA_RP + rel] = v;
        }
      }
    }
    if (k0 + 32 > len) {                  // the utterance's last tile: keys past its length do not exist
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (k0 + 8 * (r >> 2) + 4 * lh + (r & 3) >= len) s[r] = -1e30f;
    }
    // ---- online softmax (lane = query; registers = keys; the two lanes of a pair hold the two halves of a row) ----
    float tmax = m_run;
#pragma unroll
    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
    const float m_new = pair_max32(tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(s[r] - m_new);
      psum += e;
      s[r] = e;
    }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[nb][r] *= alpha;
    // ---- O^T += V^T P^T: element j of lane half lh in k-block kb is key 16kb + 8(j>>2) + 4lh + (j&3) (the order of the
    // score registers 8kb .. 8kb+7); lane l31 of fragment nb is channel nb*32 + l31 ----
    const float* const vp = p.v + row0 * p.ldv + (size_t)h * D + l31;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      size_t voff[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) voff[j] = (size_t)min(k0 + 16 * kb + 8 * (j >> 2) + 4 * lh + (j & 3), len - 1) * p.ldv;
      u32x4 hw;
#if DV_ATTN_PF16
      hw.x = dv_cvt_pk_f16(s[kb * 8 + 0], s[kb * 8 + 1]); hw.y = dv_cvt_pk_f16(s[kb * 8 + 2], s[kb * 8 + 3]);
      hw.z = dv_cvt_pk_f16(s[kb * 8 + 4], s[kb * 8 + 5]); hw.w = dv_cvt_pk_f16(s[kb * 8 + 6], s[kb * 8 + 7]);
      const dv_f16x8 ph = __builtin_bit_cast(dv_f16x8, hw);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = vp[voff[j] + nb * 32];
        unsigned h4[4], l4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dv_split_pk_f16(x[2 * j], x[2 * j + 1], h4[j], l4[j]);
        const u32x4 vh = {h4[0], h4[1], h4[2], h4[3]}, vl = {l4[0], l4[1], l4[2], l4[3]};
        o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(dv_f16x8, vl), ph, o[nb], 0, 0, 0);
        o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(dv_f16x8, vh), ph, o[nb], 0, 0, 0);
      }
#else
      u32x4 lw;
      hw.x = apk(s[kb * 8 + 0], s[kb * 8 + 1]); hw.y = apk(s[kb * 8 + 2], s[kb * 8 + 3]);
      hw.z = apk(s[kb * 8 + 4], s[kb * 8 + 5]); hw.w = apk(s[kb * 8 + 6], s[kb * 8 + 7]);
      lw.x = apk(s[kb * 8 + 0] - bf_lo(hw.x), s[kb * 8 + 1] - bf_hi(hw.x)); lw.y = apk(s[kb * 8 + 2] - bf_lo(hw.y), s[kb * 8 + 3] - bf_hi(hw.y));
      lw.z = apk(s[kb * 8 + 4] - bf_lo(hw.z), s[kb * 8 + 5] - bf_hi(hw.z)); lw.w = apk(s[kb * 8 + 6] - bf_lo(hw.w), s[kb * 8 + 7] - bf_hi(hw.w));
      const bf16x8 ph = __builtin_bit_cast(bf16x8, hw), pl = __builtin_bit_cast(bf16x8, lw);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = vp[voff[j] + nb * 32];
        bf16x8 vh, vl;
        ra_split8(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]), vh, vl);
        o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, ph, o[nb], 0, 0, 0);
        o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, pl, o[nb], 0, 0, 0);
        o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, ph, o[nb], 0, 0, 0);
      }
#endif
    }
  }

  // ---- normalise; the band's final probabilities; the relative value term in fp32 ----
  const float inv = 1.0f / pair_sum32(l_run);
  __syncthreads();                       // the band scores were written by the lanes that held their keys
  for (int r = lh; r < nrel; r += 2) {
    const float sb = s_band[l31 * RA_RP + r];
    s_band[l31 * RA_RP + r] = __builtin_amdgcn_exp2f(sb - m_run) * inv;
  }
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nb][r] = q_ok ? o[nb][r] * inv : 0.f;
  if (q_ok) {
    for (int r = 0; r < nrel; ++r) {
      const float pr = s_band[l31 * RA_RP + r];
      const float* ev = p.emb_v + (size_t)r * D + 4 * lh;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 e = *reinterpret_cast<const float4*>(ev + nb * 32 + 8 * g);
          o[nb][4 * g] = fmaf(pr, e.x, o[nb][4 * g]); o[nb][4 * g + 1] = fmaf(pr, e.y, o[nb][4 * g + 1]);
          o[nb][4 * g + 2] = fmaf(pr, e.z, o[nb][4 * g + 2]); o[nb][4 * g + 3] = fmaf(pr, e.w, o[nb][4 * g + 3]);
        }
    }
  }
  if (q_in) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float v16[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v16[r] = o[nb][r];
      ra_store_frag(p, obase + nb * 32, lh, v16);
    }
  }
}

}  // namespace

hipError_t launch_rel_attention(const RelAttnParams& p, hipStream_t st) {
  if (!p.q || !p.k || !p.v || !p.emb_k || !p.emb_v || !p.lengths || (!p.o && !p.o_hi)) return hipErrorInvalidValue;
  if (p.B < 1 || p.B > 65535 || p.H < 1 || p.H > 65535 || p.T < 1 || p.T > DV_RELATTN_MAX_T) return hipErrorInvalidValue;
  if (p.window < 0 || p.window > DV_RELATTN_MAX_WINDOW) return hipErrorInvalidValue;
  // 16-byte loads of q / k / E rows and 16-byte stores of o: row strides in whole float4s (planes: whole 16-byte groups)
  if (p.ldq % 4 != 0 || p.ldk % 4 != 0 || p.ldo % 8 != 0 || p.ldq < p.H * p.d || p.ldk < p.H * p.d || p.ldv < p.H * p.d || p.ldo < p.H * p.d)
    return hipErrorInvalidValue;
  auto al16 = [](const void* x) { return (reinterpret_cast<size_t>(x) & 15) == 0; };
  if (!al16(p.q) || !al16(p.k) || !al16(p.emb_k) || !al16(p.emb_v) || (p.o && !al16(p.o)) || (p.o_hi && !al16(p.o_hi)) || (p.o_lo && !al16(p.o_lo)))
    return hipErrorInvalidValue;
  const dim3 grid((p.T + 31) / 32, p.H, p.B), block(64);
  switch (p.d) {
    case 32: hipLaunchKernelGGL(k_rel_attention<32>, grid, block, 0, st, p); break;
    case 64: hipLaunchKernelGGL(k_rel_attention<64>, grid, block, 0, st, p); break;
    case 128: hipLaunchKernelGGL(k_rel_attention<128>, grid, block, 0, st, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
