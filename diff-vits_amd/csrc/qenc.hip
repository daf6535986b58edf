// Posterior encoder `enc_q` behind the C ABI (dv_qenc_*, include/dvits_hip.h): PosteriorEncoder over WN (reference
// model3.py:526-572, modules.py:133-210), the stage in front of the forced aligner's scores.
//
// An engine beside the text encoder's: dv_qenc_prepare() turns (config, state dict, B, T) into a static list of launches over
// channels-last rows m = b * T + t.  Every dependency is a kernel boundary.  Per forward, n_layers + 4 launches:
//   k_wn_pack   mel [B, Cin, T] -> split planes [B T, Kp], keep mask; with g its tail blocks are cond_layer: g -> [B, 2H L]
//   k_gemm      pre (Cin -> H, row mask) -> fp32 + planes
//   k_wn_layer  x n_layers (kernels_wn.hip): x ping-pongs between two buffers, the skip sum is accumulated in place
//   k_gemm      proj (H -> 2C, row mask)
//   k_wn_store  z = (m + noise * expf(logs)) * keep, m, logs channels-first
// Weight norm is folded when the weights are packed (k_wn_fold).  Padding rows hold exact zeros after every step.
// DVITS_KEEP_INTERMEDIATES=1: every layer writes buffers of its own (and its gated activations) so that the probes stay valid;
// the launch count is the same.
#include "engine_core.h"

enum { QENC_MAX_T = 16384 };                     // the aligner's own limit on frames (dv_op_mas_path)

struct dv_qenc : RowEngine {
  dv_qenc_cfg cfg{};
  std::vector<void*> temp_w;                 // packing intermediates (folded fp32 weights, planes before the fragment relayout): freed
                                             // once the prepare that made them has drained
  const float* cond_w = nullptr;             // cond_layer with its weight norm folded [2H L, gin] (in `owned_w`)
  struct { const float* y = nullptr; const int64_t* lengths = nullptr; const float* g = nullptr; const float* noise = nullptr;
           float* z = nullptr; float* m = nullptr; float* logs = nullptr; } io;
};

namespace {

void qenc_release_prepared(dv_qenc* q, bool keep_packed) {
  q->release_prepared();
  if (!keep_packed) { free_owned(q->temp_w); q->release_packed(); q->cond_w = nullptr; }
}

struct QPlan : RowPlan {
  dv_qenc* q;
  int H, C, Cin, Kp, L, gin;

  // weight_g * weight_v / ||weight_v|| of a weight-normed convolution `name` with N output channels of per_row weights each
  const float* folded(const std::string& name, int N, int per_row, std::vector<void*>& owner) {
    const float* v = W(name + ".weight_v", (size_t)N * per_row);
    const float* g = W(name + ".weight_g", (size_t)N);
    float* w = dmalloc<float>((size_t)N * per_row, owner, false);
    if (!v || !g || !w) return nullptr;
    if (launch_wn_fold(v, g, w, N, per_row, st) != hipSuccess) { err.set(DV_ERR_HIP, "weight norm launch failed"); return nullptr; }
    return w;
  }
  // src fp32 [N, Cw, taps] -> split planes [rup(N, 128)][Kp] (K order: tap, channel), optionally in GEGLU row order and fragment-major
  const PackedW3* pack(const std::string& key, const float* src, const float* bias, int N, int Cw, int taps, int Kp_, bool gate, bool frag) {
    auto it = q->packed.find(key);
    if (it != q->packed.end()) return &it->second;
    if (!src || !bias) return nullptr;
    PackedW3 pw;
    pw.N = N; pw.Kp = Kp_; pw.N_pad = rup(N, 128);
    const size_t elems = (size_t)pw.N_pad * Kp_;
    pw.hi = dmalloc<bf16_t>(elems, frag ? q->temp_w : q->owned_w, true);
    pw.lo = dmalloc<bf16_t>(elems, frag ? q->temp_w : q->owned_w, true);
    pw.bias = dmalloc<float>((size_t)pw.N_pad, q->owned_w, true);
    if (!pw.hi || !pw.lo || !pw.bias) return nullptr;
    PackSpec s{};
    s.src = src; s.N = N; s.kind = taps > 1 ? 1 : 0; s.C = Cw; s.taps = taps; s.c_pad = taps > 1 ? Cw : Kp_; s.k_off = 0; s.n_off = 0;
    s.kscale = nullptr; s.geglu = gate ? 1 : 0;
    if (launch_pack_weight(s, pw.hi, pw.lo, Kp_, st) != hipSuccess) { err.set(DV_ERR_HIP, "pack_weight launch failed"); return nullptr; }
    if (hipMemcpyAsync(pw.bias, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { err.set(DV_ERR_HIP, "bias copy failed"); return nullptr; }
    if (frag) {
      bf16_t* fh = dmalloc<bf16_t>(elems, q->owned_w, false);
      bf16_t* fl = dmalloc<bf16_t>(elems, q->owned_w, false);
      if (!fh || !fl) return nullptr;
      if (launch_relayout_frag(pw.hi, fh, pw.N_pad, Kp_, st) != hipSuccess || launch_relayout_frag(pw.lo, fl, pw.N_pad, Kp_, st) != hipSuccess) {
        err.set(DV_ERR_HIP, "relayout launch failed"); return nullptr;
      }
      pw.hi = fh; pw.lo = fl;
    }
    q->packed[key] = pw;
    return &q->packed[key];
  }
  int fail() const { return err.fail(); }

  int build() {
    dv_qenc* qq = q;
    const int Bn = B, Tn = T, Hn = H, Cn = C, Cinn = Cin, Kpn = Kp, ginn = gin, Nc = 2 * H * L;
    const size_t MH = (size_t)M * H;
    if (!zero_page()) return fail();

    // ---- weights (once per weight set) ----
    const PackedW3* w_pre = pack("pre", W("pre.weight", (size_t)H * Cin), W("pre.bias", (size_t)H), H, Cin, 1, Kp, false, false);
    const PackedW3* w_proj = pack("proj", W("proj.weight", (size_t)2 * C * H), W("proj.bias", (size_t)2 * C), 2 * C, H, 1, H, false, false);
    if (!w_pre || !w_proj) return fail();
    const float* cond_b = nullptr;
    if (gin > 0) {
      if (!q->cond_w) q->cond_w = folded("enc.cond_layer", Nc, gin, q->owned_w);   // (read by every forward)
      cond_b = W("enc.cond_layer.bias", (size_t)Nc);
      if (!q->cond_w || !cond_b) return fail();
    }
    std::vector<const PackedW3*> w_in(L), w_rs(L);
    for (int i = 0; i < L; ++i) {
      const std::string pi = "enc.in_layers." + std::to_string(i), pr = "enc.res_skip_layers." + std::to_string(i);
      const int N2 = i < L - 1 ? 2 * H : H;
      const bool have = q->packed.count(pi) && q->packed.count(pr);
      w_in[i] = pack(pi, have ? nullptr : folded(pi, 2 * H, H * 5, q->temp_w), have ? nullptr : W(pi + ".bias", (size_t)2 * H), 2 * H, H, 5, 5 * H, true, true);
      w_rs[i] = pack(pr, have ? nullptr : folded(pr, N2, H, q->temp_w), have ? nullptr : W(pr + ".bias", (size_t)N2), N2, H, 1, H, false, true);
      if (!w_in[i] || !w_rs[i]) return fail();
    }

    // ---- buffers ----
    bf16_t* in_hi = dmalloc<bf16_t>((size_t)M * Kp, q->owned, false);
    bf16_t* in_lo = dmalloc<bf16_t>((size_t)M * Kp, q->owned, false);
    float* keep = dmalloc<float>((size_t)M, q->owned, false);
    float* cond = gin > 0 ? dmalloc<float>((size_t)B * Nc, q->owned, false) : nullptr;
    float* z = dmalloc<float>((size_t)M * 2 * C, q->owned, false);
    bf16_t* s_hi = dmalloc<bf16_t>(MH, q->owned, false);
    bf16_t* s_lo = dmalloc<bf16_t>(MH, q->owned, false);
    if (!in_hi || !in_lo || !keep || (gin > 0 && !cond) || !z || !s_hi || !s_lo) return fail();
    struct XSet { float* x; bf16_t* hi; bf16_t* lo; };
    auto xset = [&]() { XSet s{dmalloc<float>(MH, q->owned, false), dmalloc<bf16_t>(MH, q->owned, false), dmalloc<bf16_t>(MH, q->owned, false)}; return s; };
    // production: two x sets (ping-pong) and one skip sum; kept intermediates: one of each per layer
    std::vector<XSet> xs(q->keep ? L : 2);
    for (auto& s : xs) { s = xset(); if (!s.x || !s.hi || !s.lo) return fail(); }
    std::vector<float*> skips(q->keep ? L : 1), acts(q->keep ? L : 0);
    for (auto& s : skips) { s = dmalloc<float>(MH, q->owned, false); if (!s) return fail(); }
    for (auto& a : acts) { a = dmalloc<float>(MH, q->owned, false); if (!a) return fail(); }

    // ---- launches ----
    {
      const float* cw = q->cond_w;
      q->ops.push_back([=](hipStream_t s) {
        return launch_wn_pack(qq->io.y, qq->io.lengths, in_hi, in_lo, keep, Bn, Cinn, Tn, Kpn, ginn > 0 ? qq->io.g : nullptr, cw, cond_b, cond,
                              ginn, Nc, s);
      });
      if (gin > 0) q->flops += 2.0 * B * (double)gin * Nc;
    }
    {
      GemmParams g = gp(H);
      g.seg[0] = seg1(in_hi, in_lo, Kp, 1, 0);
      g.out = xs[0].x; g.out_hi = xs[0].hi; g.out_lo = xs[0].lo; g.rowmask = keep;
      gemm(g, w_pre, Cin);
    }
    probe("pre", xs[0].x, H);
    int cur = 0;
    for (int i = 0; i < L; ++i) {
      const bool last = i == L - 1;
      const int nxt = q->keep ? (last ? cur : i + 1) : cur ^ 1;
      WnLayerParams p{};
      p.x_in = xs[cur].x; p.xh_in = xs[cur].hi; p.xl_in = xs[cur].lo;
      if (!last) { p.x_out = xs[nxt].x; p.xh_out = xs[nxt].hi; p.xl_out = xs[nxt].lo; }
      p.skip_in = q->keep ? (i ? skips[i - 1] : nullptr) : skips[0];
      p.skip_out = q->keep ? skips[i] : skips[0];
      p.sh_out = s_hi; p.sl_out = s_lo;
      p.w1_hi = w_in[i]->hi; p.w1_lo = w_in[i]->lo; p.b1 = w_in[i]->bias;
      p.cond = cond; p.ld_cond = Nc; p.cond_off = 2 * H * i;
      p.w2_hi = w_rs[i]->hi; p.w2_lo = w_rs[i]->lo; p.b2 = w_rs[i]->bias;
      p.acts_out = q->keep ? acts[i] : nullptr;
      p.B = B; p.T = T; p.tiles_per_utt = (T + 63) / 64;
      p.first = i == 0; p.last = last;
      q->ops.push_back([p, qq, Hn, ginn](hipStream_t s) {
        WnLayerParams r = p;
        r.lengths = qq->io.lengths;
        if (!(ginn > 0 && qq->io.g)) r.cond = nullptr;     // (no speaker vector in this call)
        return launch_wn_layer(r, Hn, s);
      });
      q->flops += 2.0 * (double)M * ((double)5 * H * 2 * H + (double)H * (last ? H : 2 * H));
      const std::string li = "layer" + std::to_string(i);
      if (q->keep) probe(li + ".acts", acts[i], H);
      if (!last) probe(li + ".x", xs[nxt].x, H);
      probe(li + ".skip", p.skip_out, H);
      cur = nxt;
    }
    {
      GemmParams g = gp(2 * C);
      g.seg[0] = seg1(s_hi, s_lo, H, 1, 0);
      g.out = z; g.rowmask = keep;
      gemm(g, w_proj, H);
    }
    probe("proj", z, 2 * C);
    q->ops.push_back([=](hipStream_t s) { return launch_wn_store(z, qq->io.noise, qq->io.lengths, qq->io.z, qq->io.m, qq->io.logs, Bn, Tn, Cn, s); });
    if (err) return fail();
    return DV_OK;
  }
};

}  // namespace

extern "C" int dv_qenc_create(const dv_qenc_cfg* cfg, dv_qenc** out) {
  if (!cfg || !out) return dv_fail(DV_ERR_INVALID, "dv_qenc_create: null argument");
  if (cfg->in_channels <= 0 || cfg->in_channels > 4096) return dv_fail(DV_ERR_INVALID, "in_channels out of range");
  if (cfg->out_channels <= 0 || cfg->out_channels > 4096) return dv_fail(DV_ERR_INVALID, "out_channels out of range");
  if (cfg->hidden_channels <= 0 || cfg->hidden_channels > 4096) return dv_fail(DV_ERR_INVALID, "hidden_channels out of range");
  if (cfg->kernel_size < 1 || cfg->kernel_size % 2 != 1) return dv_fail(DV_ERR_INVALID, "kernel_size must be odd");
  if (cfg->dilation_rate < 1) return dv_fail(DV_ERR_INVALID, "dilation_rate must be >= 1");
  if (cfg->n_layers < 1 || cfg->n_layers > 64) return dv_fail(DV_ERR_INVALID, "n_layers out of range");
  if (cfg->gin_channels < 0 || cfg->gin_channels > 4096) return dv_fail(DV_ERR_INVALID, "gin_channels out of range");
  dv_qenc* q = new dv_qenc();
  q->cfg = *cfg;
  *out = q;
  return DV_OK;
}

extern "C" void dv_qenc_destroy(dv_qenc* q) {
  if (!q) return;
  (void)hipDeviceSynchronize();
  qenc_release_prepared(q, false);
  q->w.free_all();
  delete q;
}

extern "C" int dv_qenc_set_weight(dv_qenc* q, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim) {
  return row_set_weight(q, name, dev_ptr, shape, ndim, "dv_qenc_set_weight");
}

extern "C" int dv_qenc_prepare(dv_qenc* q, int32_t B, int32_t T, int32_t precision) {
  if (!q) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: null handle");
  if (B <= 0 || T <= 0) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: B, T must be positive");
  if (precision == DV_PREC_BF16)
    return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: DV_PREC_BF16 is unsupported by the posterior encoder (split-bf16 DV_PREC_BF16X3 only)");
  if (precision != DV_PREC_BF16X3) return dv_fail(DV_ERR_INVALID, "unknown precision %d", precision);
  const dv_qenc_cfg& c = q->cfg;
  if (c.kernel_size != 5) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: kernel_size = %d: k_wn_layer is built for 5 taps", c.kernel_size);
  if (c.dilation_rate != 1) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: dilation_rate = %d: k_wn_layer is built for dilation 1", c.dilation_rate);
  if (!wn_layer_supported(c.hidden_channels))
    return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: hidden_channels = %d: k_wn_layer is instantiated for 256", c.hidden_channels);
  if (c.out_channels % 16 != 0) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: out_channels = %d must be a multiple of 16", c.out_channels);
  if (T > QENC_MAX_T) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: T = %d exceeds the aligner's %d frames", T, (int)QENC_MAX_T);
  if (B > 65535) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: B = %d exceeds 65535", B);
  if ((long long)B * T > (1LL << 22)) return dv_fail(DV_ERR_INVALID, "dv_qenc_prepare: B x T = %lld rows exceed 2^22", (long long)B * T);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(gemm_init());
  HIPCHK(wn_init());
  gemm_env_refresh();
  qenc_release_prepared(q, !q->weights_dirty);
  q->B = B; q->T = T; q->precision = precision;
  const char* keep = getenv("DVITS_KEEP_INTERMEDIATES");
  q->keep = keep && keep[0] == '1';
  QPlan pl{};
  pl.q = q; pl.e = q; pl.B = B; pl.T = T; pl.M = B * T;
  pl.H = c.hidden_channels; pl.C = c.out_channels; pl.Cin = c.in_channels; pl.Kp = rup(c.in_channels, 64); pl.L = c.n_layers; pl.gin = c.gin_channels;
  int rc = pl.build();
  if (rc != DV_OK) { qenc_release_prepared(q, false); q->weights_dirty = true; return rc; }
  HIPCHK(hipDeviceSynchronize());
  free_owned(q->temp_w);
  q->prepared = true;
  q->weights_dirty = false;
  return DV_OK;
}

extern "C" int dv_qenc_forward(dv_qenc* q, const float* y, const int64_t* lengths, const float* g, const float* noise, float* z, float* m,
                               float* logs, void* stream) {
  if (!q || !y || !lengths || !noise || !z || !m || !logs) return dv_fail(DV_ERR_INVALID, "dv_qenc_forward: null argument");
  if (!q->prepared) return dv_fail(DV_ERR_STATE, "dv_qenc_forward before dv_qenc_prepare");
  if (g && q->cfg.gin_channels == 0) return dv_fail(DV_ERR_INVALID, "dv_qenc_forward: g given, but the encoder has no cond_layer (gin_channels = 0)");
  q->io.y = y; q->io.lengths = lengths; q->io.g = g; q->io.noise = noise; q->io.z = z; q->io.m = m; q->io.logs = logs;
  return run_ops(q->ops, (hipStream_t)stream, "posterior encoder");
}

extern "C" int dv_qenc_stats(dv_qenc* q, int64_t* n_launch, double* flops) { return row_stats(q, n_launch, flops, "dv_qenc"); }

extern "C" int dv_qenc_time_layers(dv_qenc* q, int32_t reps, void* stream, float* us_per_pass) {
  if (!q || !us_per_pass || reps < 1) return dv_fail(DV_ERR_INVALID, "dv_qenc_time_layers: bad argument");
  if (!q->prepared || !q->io.lengths) return dv_fail(DV_ERR_STATE, "dv_qenc_time_layers needs a dv_qenc_forward on this schedule first");
  const int L = q->cfg.n_layers;                     // ops: pack, pre, L layers, proj, store
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, st));
  for (int r = 0; r < reps; ++r) {
    int rc = run_ops(q->ops.data() + 2, (size_t)L, st, "posterior encoder layers");
    if (rc != DV_OK) return rc;
  }
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *us_per_pass = ms * 1000.0f / (float)reps;
  return DV_OK;
}

extern "C" int dv_qenc_probe(dv_qenc* q, const char* name, float* host_out, int64_t capacity, int64_t* dims) {
  return row_probe(q, name, host_out, capacity, dims, "dv_qenc");
}
