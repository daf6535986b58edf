// Vocoder behind the C ABI (dv_voc_*, include/dvits_hip.h): the Vocos ConvNeXt-1D backbone and its ISTFT head
// (charactr/vocos-mel-24khz; restated in fp64 in tests/vocoder_cases.py), the stage behind the sampler's mel.
//
// An engine beside the encoders': dv_voc_prepare() turns (config, state dict, B, T) into a static list of launches over
// channels-last rows m = b * T + t.  Every dependency is a kernel boundary.  Per forward, 4 n_layers + 6 launches:
//   k_voc_pack    mel [B, n_mels, T] -> split planes [B T, Kp], keep mask
//   k_gemm        embed as a seven-tap implicit GEMM (taps outside [0, T) read the zero page, taps at t >= L_b the packed zeros)
//   k_ln_affine   norm (eps 1e-6, row mask)
//   per layer:    k_dw7_ln (dwconv + norm -> planes) -> k_gemm pwconv1 (row mask) -> k_voc_gelu (-> planes) ->
//                 k_gemm pwconv2 with gamma folded into weight and bias, + residual, row mask
//   k_ln_affine   final_layer_norm -> planes
//   k_gemm        head.out (N = n_fft + 2, row mask)
//   k_istft_head  magnitude / phase -> inverse FFT -> window -> overlap-add -> envelope -> wave, samples
// The GELU of pwconv1 is a small kernel of the vocoder's own, not a new k_gemm epilogue: the set of k_gemm instantiations, which
// the existing tests enumerate, stays what it was.  Padding rows hold exact zeros after every step.
// DVITS_KEEP_INTERMEDIATES=1: every layer writes buffers of its own so that the probes stay valid.
#include "engine_core.h"

struct dv_voc : RowEngine {
  dv_voc_cfg cfg{};
  std::vector<void*> temp_w;                 // gamma-folded fp32 weights: freed once the prepare that made them has drained
  struct { const float* mel = nullptr; const int64_t* lengths = nullptr; float* wave = nullptr; int64_t* samples = nullptr; } io;
};

namespace {

enum { VOC_MAX_T = 1 << 20 };

void voc_release_prepared(dv_voc* v, bool keep_packed) {
  v->release_prepared();
  if (!keep_packed) { free_owned(v->temp_w); v->release_packed(); }
}

struct VPlan : RowPlan {
  dv_voc* v;
  int C, I, L, Cin, Kin, NH;

  // src fp32 [N, Cw, taps] -> split planes [rup(N, 128)][Kp] (K order: tap, channel padded to c_pad)
  const PackedW3* pack(const std::string& key, const float* src, const float* bias, int N, int Cw, int taps, int c_pad) {
    auto it = v->packed.find(key);
    if (it != v->packed.end()) return &it->second;
    if (!src || !bias) return nullptr;
    PackedW3 pw;
    pw.N = N; pw.Kp = taps * c_pad; pw.N_pad = rup(N, 128);
    const size_t elems = (size_t)pw.N_pad * pw.Kp;
    pw.hi = dmalloc<bf16_t>(elems, v->owned_w, true);
    pw.lo = dmalloc<bf16_t>(elems, v->owned_w, true);
    pw.bias = dmalloc<float>((size_t)pw.N_pad, v->owned_w, true);
    if (!pw.hi || !pw.lo || !pw.bias) return nullptr;
    PackSpec s{};
    s.src = src; s.N = N; s.kind = taps > 1 ? 1 : 0; s.C = Cw; s.taps = taps; s.c_pad = c_pad; s.k_off = 0; s.n_off = 0;
    s.kscale = nullptr; s.geglu = 0;
    if (launch_pack_weight(s, pw.hi, pw.lo, pw.Kp, st) != hipSuccess) { err.set(DV_ERR_HIP, "pack_weight launch failed"); return nullptr; }
    if (hipMemcpyAsync(pw.bias, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { err.set(DV_ERR_HIP, "bias copy failed"); return nullptr; }
    v->packed[key] = pw;
    return &v->packed[key];
  }
  int fail() const { return err.fail(); }

  int build() {
    dv_voc* vv = v;
    const int Bn = B, Tn = T, Cn = C, Cinn = Cin, Kinn = Kin, NHn = NH;
    const size_t MC = (size_t)M * C, MI = (size_t)M * I;
    if (!zero_page()) return fail();

    // ---- weights (once per weight set) ----
    const std::string bb = "backbone.";
    const PackedW3* w_embed = pack("embed", W(bb + "embed.weight", (size_t)C * Cin * 7), W(bb + "embed.bias", (size_t)C), C, Cin, 7, Kin);
    const PackedW3* w_head = pack("head", W("head.out.weight", (size_t)NH * C), W("head.out.bias", (size_t)NH), NH, C, 1, C);
    const float* n_g = W(bb + "norm.weight", (size_t)C); const float* n_b = W(bb + "norm.bias", (size_t)C);
    const float* f_g = W(bb + "final_layer_norm.weight", (size_t)C); const float* f_b = W(bb + "final_layer_norm.bias", (size_t)C);
    const float* window = W("head.istft.window", (size_t)v->cfg.n_fft);
    if (!w_embed || !w_head || !n_g || !n_b || !f_g || !f_b || !window) return fail();
    struct LayerW { const float* dw; const float* db; const float* g; const float* b; const PackedW3* p1; const PackedW3* p2; };
    std::vector<LayerW> lw(L);
    for (int i = 0; i < L; ++i) {
      const std::string p = bb + "convnext." + std::to_string(i) + ".";
      LayerW& l = lw[i];
      l.dw = W(p + "dwconv.weight", (size_t)C * 7); l.db = W(p + "dwconv.bias", (size_t)C);
      l.g = W(p + "norm.weight", (size_t)C); l.b = W(p + "norm.bias", (size_t)C);
      l.p1 = pack(p + "pw1", W(p + "pwconv1.weight", (size_t)I * C), W(p + "pwconv1.bias", (size_t)I), I, C, 1, C);
      if (v->packed.count(p + "pw2")) {
        l.p2 = &v->packed[p + "pw2"];
      } else {
        // layer scale folded: W'[n, :] = gamma[n] W[n, :], b' = gamma b
        const float* w2 = W(p + "pwconv2.weight", (size_t)C * I); const float* b2 = W(p + "pwconv2.bias", (size_t)C);
        const float* gam = W(p + "gamma", (size_t)C);
        float* wf = dmalloc<float>((size_t)C * I, v->temp_w, false);
        float* bf = dmalloc<float>((size_t)C, v->temp_w, false);
        if (!w2 || !b2 || !gam || !wf || !bf) return fail();
        if (launch_voc_fold_gamma(w2, b2, gam, wf, bf, C, I, st) != hipSuccess) { err.set(DV_ERR_HIP, "gamma fold launch failed"); return fail(); }
        l.p2 = pack(p + "pw2", wf, bf, C, I, 1, I);
      }
      if (!l.dw || !l.db || !l.g || !l.b || !l.p1 || !l.p2) return fail();
    }

    // ---- buffers ----
    auto f32 = [&](size_t n) { return dmalloc<float>(n, v->owned, false); };
    auto b16 = [&](size_t n) { return dmalloc<bf16_t>(n, v->owned, false); };
    bf16_t* in_hi = b16((size_t)M * Kin); bf16_t* in_lo = b16((size_t)M * Kin);
    float* keep = f32((size_t)M);
    float* e0 = f32(MC);
    float* x = f32(MC);
    float* logits = f32((size_t)M * NH);
    bf16_t* f_hi = b16(MC); bf16_t* f_lo = b16(MC);
    float* fin = v->keep ? f32(MC) : nullptr;
    if (!in_hi || !in_lo || !keep || !e0 || !x || !logits || !f_hi || !f_lo || (v->keep && !fin)) return fail();
    struct LayerB { float* y; bf16_t* y_hi; bf16_t* y_lo; float* h; bf16_t* a_hi; bf16_t* a_lo; float* out; };
    // production: one set, the block output ping-pongs between two buffers; kept intermediates: one set per layer
    std::vector<LayerB> lb(v->keep ? L : 1);
    for (auto& s : lb) {
      s = LayerB{v->keep ? f32(MC) : nullptr, b16(MC), b16(MC), f32(MI), b16(MI), b16(MI), v->keep ? f32(MC) : nullptr};
      if (!s.y_hi || !s.y_lo || !s.h || !s.a_hi || !s.a_lo || (v->keep && (!s.y || !s.out))) return fail();
    }
    float* pong = v->keep ? nullptr : e0;          // (e0 is free once `norm` has read it)

    // ---- launches ----
    v->ops.push_back([=](hipStream_t s) { return launch_voc_pack(vv->io.mel, vv->io.lengths, in_hi, in_lo, keep, Bn, Cinn, Tn, Kinn, s); });
    {
      GemmParams g = gp(C);
      g.seg[0] = seg1(in_hi, in_lo, Kin, 7, 3);
      g.out = e0; g.rowmask = keep;
      gemm(g, w_embed, 7 * Cin);
    }
    probe("embed", e0, C);
    v->ops.push_back([=](hipStream_t s) { return launch_ln_affine(e0, n_g, n_b, keep, x, nullptr, nullptr, Bn * Tn, Cn, 1e-6f, s); });
    probe("norm", x, C);
    float* cur = x;
    for (int i = 0; i < L; ++i) {
      const LayerW l = lw[i];
      const LayerB s = lb[v->keep ? i : 0];
      float* nxt = v->keep ? s.out : (cur == x ? pong : x);
      const std::string li = "l" + std::to_string(i);
      {
        const float* xin = cur;
        v->ops.push_back([=](hipStream_t q) {
          return launch_dw7_ln(xin, l.dw, l.db, l.g, l.b, vv->io.lengths, Bn, Tn, Cn, 1e-6f, s.y, s.y_hi, s.y_lo, q);
        });
        v->flops += 2.0 * 7 * (double)M * C;
      }
      if (v->keep) probe(li + ".dwln", s.y, C);
      { GemmParams g = gp(I); g.seg[0] = seg1(s.y_hi, s.y_lo, C, 1, 0); g.out = s.h; g.rowmask = keep; gemm(g, l.p1, C); }
      {
        const int64_t n = (int64_t)M * I;
        v->ops.push_back([=](hipStream_t q) { return launch_voc_gelu(s.h, s.a_hi, s.a_lo, n, q); });
      }
      if (v->keep) v->probes.push_back(RowProbe{li + ".act", nullptr, s.a_hi, s.a_lo, I});
      { GemmParams g = gp(C); g.seg[0] = seg1(s.a_hi, s.a_lo, I, 1, 0); g.epi = EPI_RESIDUAL; g.res = cur; g.out = nxt; g.rowmask = keep; gemm(g, l.p2, I); }
      probe(li + ".out", nxt, C);
      cur = nxt;
    }
    {
      const float* xin = cur;
      v->ops.push_back([=](hipStream_t s) { return launch_ln_affine(xin, f_g, f_b, keep, fin, f_hi, f_lo, Bn * Tn, Cn, 1e-6f, s); });
    }
    if (v->keep) probe("final", fin, C);
    { GemmParams g = gp(NH); g.seg[0] = seg1(f_hi, f_lo, C, 1, 0); g.out = logits; g.rowmask = keep; gemm(g, w_head, C); }
    probe("head", logits, NH);
    v->ops.push_back([=](hipStream_t s) {
      return launch_istft_head(logits, NHn, window, vv->io.lengths, Bn, Tn, vv->io.wave, vv->io.samples, s);
    });
    if (err) return fail();
    return DV_OK;
  }
};

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int dv_voc_create(const dv_voc_cfg* cfg, dv_voc** out) {
  if (!cfg || !out) return dv_fail(DV_ERR_INVALID, "dv_voc_create: null argument");
  *out = nullptr;
  if (cfg->n_fft != 1024 || cfg->hop != 256)
    return dv_fail(DV_ERR_INVALID, "dv_voc_create: n_fft = %d, hop = %d: only 1024 / 256 are built", cfg->n_fft, cfg->hop);
  if (cfg->n_mels < 1 || cfg->n_mels > 4096) return dv_fail(DV_ERR_INVALID, "dv_voc_create: n_mels out of range");
  if (!dw7_ln_supported(cfg->dim)) return dv_fail(DV_ERR_INVALID, "dv_voc_create: dim = %d: k_dw7_ln is built for multiples of 64 up to 512", cfg->dim);
  if (cfg->intermediate < 32 || cfg->intermediate % 32 != 0 || cfg->intermediate > 8192)
    return dv_fail(DV_ERR_INVALID, "dv_voc_create: intermediate = %d must be a multiple of 32, <= 8192", cfg->intermediate);
  if (cfg->n_layers < 1 || cfg->n_layers > 64) return dv_fail(DV_ERR_INVALID, "dv_voc_create: n_layers out of range");
  dv_voc* v = new dv_voc();
  v->cfg = *cfg;
  *out = v;
  return DV_OK;
}

extern "C" void dv_voc_destroy(dv_voc* v) {
  if (!v) return;
  (void)hipDeviceSynchronize();
  voc_release_prepared(v, false);
  v->w.free_all();
  delete v;
}

extern "C" int dv_voc_set_weight(dv_voc* v, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim) {
  return row_set_weight(v, name, dev_ptr, shape, ndim, "dv_voc_set_weight");
}

extern "C" int dv_voc_prepare(dv_voc* v, int32_t B, int32_t T, int32_t precision) {
  if (!v) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: null handle");
  if (B <= 0 || T <= 0) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: B, T must be positive");
  if (precision != DV_PREC_BF16X3 && precision != DV_PREC_BF16) return dv_fail(DV_ERR_INVALID, "unknown precision %d", precision);
  if (T > VOC_MAX_T) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: T = %d exceeds %d frames", T, (int)VOC_MAX_T);
  if (B > 65535) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: B = %d exceeds 65535", B);
  if ((long long)B * T > (1LL << 20)) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: B x T = %lld rows exceed 2^20", (long long)B * T);
  if ((long long)B * T * T >= (1LL << 32)) return dv_fail(DV_ERR_INVALID, "dv_voc_prepare: B x T x T = %lld exceeds k_gemm's 2^32 row arithmetic", (long long)B * T * T);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(gemm_init());
  HIPCHK(voc_init());
  gemm_env_refresh();
  voc_release_prepared(v, !v->weights_dirty);
  v->B = B; v->T = T; v->precision = precision;
  const char* keep = getenv("DVITS_KEEP_INTERMEDIATES");
  v->keep = keep && keep[0] == '1';
  const dv_voc_cfg& c = v->cfg;
  VPlan pl{};
  pl.v = v; pl.e = v; pl.B = B; pl.T = T; pl.M = B * T;
  pl.C = c.dim; pl.I = c.intermediate; pl.L = c.n_layers; pl.Cin = c.n_mels; pl.Kin = rup(c.n_mels, 64); pl.NH = c.n_fft + 2;
  int rc = pl.build();
  if (rc != DV_OK) { voc_release_prepared(v, false); v->weights_dirty = true; return rc; }
  HIPCHK(hipDeviceSynchronize());
  free_owned(v->temp_w);
  v->prepared = true;
  v->weights_dirty = false;
  return DV_OK;
}

extern "C" int dv_voc_forward(dv_voc* v, const float* mel, const int64_t* lengths, float* wave, int64_t* samples, void* stream) {
  if (!v || !mel || !wave || !samples) return dv_fail(DV_ERR_INVALID, "dv_voc_forward: null argument");
  if (!v->prepared) return dv_fail(DV_ERR_STATE, "dv_voc_forward before dv_voc_prepare");
  v->io.mel = mel; v->io.lengths = lengths; v->io.wave = wave; v->io.samples = samples;
  return run_ops(v->ops, (hipStream_t)stream, "vocoder");
}

extern "C" int dv_voc_stats(dv_voc* v, int64_t* n_launch, double* flops) { return row_stats(v, n_launch, flops, "dv_voc"); }

extern "C" int dv_voc_probe(dv_voc* v, const char* name, float* host_out, int64_t capacity, int64_t* dims) {
  return row_probe(v, name, host_out, capacity, dims, "dv_voc");
}

extern "C" int dv_op_dwconv_ln(const float* x, const float* w, const float* b, const float* gamma, const float* beta, const int64_t* lengths,
                               int32_t B, int32_t T, int32_t C, float eps, float* y, uint16_t* y_hi, uint16_t* y_lo, void* stream) {
  if (!x || !w || !b || !gamma || !beta || (!y && !y_hi)) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: null argument");
  if (y_lo && !y_hi) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: y_lo without y_hi");
  if (B < 1 || B > 65535 || T < 1 || (long long)B * T > (1LL << 22)) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: B = %d, T = %d out of range", B, T);
  if (!dw7_ln_supported(C)) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: C = %d must be a multiple of 64 up to 512", C);
  if (!(eps > 0.f)) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: eps must be > 0");
  if (!al16(x) || !al16(y) || !al16(y_hi) || !al16(y_lo)) return dv_fail(DV_ERR_INVALID, "dv_op_dwconv_ln: x and the outputs must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_dw7_ln(x, w, b, gamma, beta, lengths, B, T, C, eps, y, y_hi, y_lo, st);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_dwconv_ln: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

extern "C" int dv_op_istft_head(const float* logits, const float* window, const int64_t* lengths, int32_t B, int32_t T, float* wave,
                                int64_t* samples, void* stream) {
  if (!logits || !window || !wave || !samples) return dv_fail(DV_ERR_INVALID, "dv_op_istft_head: null argument");
  if (B < 1 || B > 65535 || T < 1 || (long long)B * T > (1LL << 22)) return dv_fail(DV_ERR_INVALID, "dv_op_istft_head: B = %d, T = %d out of range", B, T);
  if ((reinterpret_cast<uintptr_t>(window) | reinterpret_cast<uintptr_t>(samples)) & 7) return dv_fail(DV_ERR_INVALID, "dv_op_istft_head: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(voc_init());
  hipError_t e = launch_istft_head(logits, 1026, window, lengths, B, T, wave, samples, st);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_istft_head: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}
