// Host-side core shared by the engines behind the C ABI (engine.hip, tenc.hip, qenc.hip, voc.hip) and the single-operator entry
// points (ops.hip): error plumbing, the raw-weight store, the plan-time allocator, the launch list and the pieces every planner
// over channels-last rows m = b * T + t needs.
// Host code only: no kernel lives here.
#pragma once
#include "../../include/dvits_hip.h"
#include "dv_common.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

int dv_fail(int code, const char* fmt, ...);   // engine.hip: records the message for dv_last_error(), returns `code`

#define HIPCHK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return dv_fail(DV_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// ----------------------------------------------------------------------------- plan errors
// The first error of a plan wins.  A missing weight or a shape mismatch is DV_ERR_MISSING_WEIGHT; a failed allocation, launch
// or copy is DV_ERR_HIP.
struct PlanError {
  int code = DV_OK;
  std::string msg;
  void set(int c, const std::string& m) { if (code == DV_OK) { code = c; msg = m; } }
  explicit operator bool() const { return code != DV_OK; }
  int fail() const { return code != DV_OK ? dv_fail(code, "%s", msg.c_str()) : dv_fail(DV_ERR_HIP, "the planner gave up without naming a cause"); }
};

// ----------------------------------------------------------------------------- raw weights
struct RawW { float* p = nullptr; std::vector<int64_t> shape; size_t numel = 0; };

// name -> fp32 device copy of a state-dict entry.  What a new weight does to a handle's prepared state is the handle's policy.
struct WeightStore {
  enum : size_t { ANY_NUMEL = ~(size_t)0 };
  std::map<std::string, RawW> recs;

  // the body of every dv_*_set_weight (`what` names the entry point in the messages)
  int set(const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim, const char* what) {
    if (!name || !dev_ptr || !shape || ndim < 1 || ndim > 4) return dv_fail(DV_ERR_INVALID, "%s: bad argument", what);
    size_t n = 1;
    std::vector<int64_t> sh(shape, shape + ndim);
    for (auto s : sh) {
      if (s <= 0) return dv_fail(DV_ERR_INVALID, "%s(%s): non-positive dimension", what, name);
      n *= (size_t)s;
    }
    RawW& r = recs[name];
    if (r.numel != n) {
      if (r.p) (void)hipFree(r.p);
      r.p = nullptr; r.numel = 0;
      HIPCHK(hipMalloc((void**)&r.p, n * sizeof(float)));
    }
    r.shape = sh; r.numel = n;
    HIPCHK(hipMemcpy(r.p, dev_ptr, n * sizeof(float), hipMemcpyDeviceToDevice));
    return DV_OK;
  }
  const RawW* find(const std::string& name, size_t numel, PlanError& err) const {
    auto it = recs.find(name);
    if (it == recs.end()) { err.set(DV_ERR_MISSING_WEIGHT, "missing weight: " + name); return nullptr; }
    if (numel != ANY_NUMEL && it->second.numel != numel) { err.set(DV_ERR_MISSING_WEIGHT, "weight shape mismatch: " + name); return nullptr; }
    return &it->second;
  }
  void free_all() {
    for (auto& kv : recs)
      if (kv.second.p) (void)hipFree(kv.second.p);
    recs.clear();
  }
};

// ----------------------------------------------------------------------------- plan-time device memory
// DVITS_POISON (development; read at every fill, so at every prepare: tests flip it inside one process): memory that a plan
// allocates WITHOUT defining its contents - the denoiser's and the prompt encoder's slab, every dmalloc(zero = false), every
// OpScratch::get(UNWRITTEN) of ops.hip - is filled once, on the plan's stream, before the first operation that could write it:
//   nan   byte 0xFF: every fp32 word and every bf16 half is a NaN
//   big   byte 0x4B: ~1.3e7 as fp32 and as bf16 - finite, so a multiply by a zero mask hides it where it would expose a NaN
// Unset, "0" or anything else: no fill, nothing counted.  Only floating-point payload lives in such memory (indices, counts,
// flags, tickets and the zero page are allocated zeroed: profiles/poison_audit.txt).  dv_poisoned_bytes() is the running total.
inline std::atomic<int64_t>& poisoned_total() { static std::atomic<int64_t> n{0}; return n; }
// ... and dv_unwritten_bytes() the running total of what was REQUESTED that way, counted whether the knob is set or not: the figure a
// test holds the fill against (a plan's own unzeroed bytes = the growth over its prepare)
inline std::atomic<int64_t>& unwritten_total() { static std::atomic<int64_t> n{0}; return n; }
inline int poison_byte() {
  const char* e = getenv("DVITS_POISON");
  if (!e) return -1;
  return strcmp(e, "nan") == 0 ? 0xFF : (strcmp(e, "big") == 0 ? 0x4B : -1);
}
inline hipError_t poison_fill(void* p, size_t bytes, hipStream_t st) {
  if (!p || !bytes) return hipSuccess;
  unwritten_total() += (int64_t)bytes;
  const int b = poison_byte();
  if (b < 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(p, b, bytes, st);
  if (e == hipSuccess) poisoned_total() += (int64_t)bytes;
  return e;
}

// `elems` elements of X (never fewer than 16 bytes), owned by `owner`, optionally zeroed on `st`
template <typename X> X* dmalloc(size_t elems, std::vector<void*>& owner, bool zero, hipStream_t st, PlanError& err) {
  void* p = nullptr;
  const size_t bytes = elems ? elems * sizeof(X) : 16;
  if (hipMalloc(&p, bytes) != hipSuccess) { err.set(DV_ERR_HIP, "hipMalloc failed"); return nullptr; }
  owner.push_back(p);
  if (zero) (void)hipMemsetAsync(p, 0, bytes, st);
  else if (poison_fill(p, bytes, st) != hipSuccess) { err.set(DV_ERR_HIP, "DVITS_POISON fill failed"); return nullptr; }
  return reinterpret_cast<X*>(p);
}
inline void free_owned(std::vector<void*>& owner) {
  for (void* p : owner) (void)hipFree(p);
  owner.clear();
}

// ----------------------------------------------------------------------------- launch lists
typedef std::function<hipError_t(hipStream_t)> OpFn;

// Enqueues `ops` in order.  DVITS_SYNC_OPS=1 (development; latched at the first call): every operation is announced on stderr
// - with `label(i)`, where the caller has one - and waited for, so that a device fault names its launch.
inline int run_ops(const OpFn* ops, size_t n, hipStream_t st, const char* what, const std::function<std::string(int)>& label = nullptr) {
  static const bool sync_ops = [] { const char* e = getenv("DVITS_SYNC_OPS"); return e && e[0] == '1'; }();
  for (size_t k = 0; k < n; ++k) {
    const int i = (int)k;
    if (sync_ops) fprintf(stderr, "[dvits] %s op %d %s\n", what, i, label ? label(i).c_str() : "");
    hipError_t e = ops[k](st);
    if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "%s: op %d failed to launch: %s", what, i, hipGetErrorString(e));
    if (sync_ops && (e = hipStreamSynchronize(st)) != hipSuccess) return dv_fail(DV_ERR_HIP, "%s: op %d failed: %s", what, i, hipGetErrorString(e));
  }
  return DV_OK;
}
inline int run_ops(const std::vector<OpFn>& ops, hipStream_t st, const char* what, const std::function<std::string(int)>& label = nullptr) {
  return run_ops(ops.data(), ops.size(), st, what, label);
}

// ----------------------------------------------------------------------------- GEMMs over rows
struct PackedW3 { bf16_t* hi = nullptr; bf16_t* lo = nullptr; float* bias = nullptr; int Kp = 0, N = 0, N_pad = 0; };

// k_gemm over the unpadded row space [B * T, N]: one operand segment, plain store
inline GemmParams row_gemm_params(int B, int T, int N, const bf16_t* zero_page) {
  GemmParams g{};
  g.nseg = 1; g.B = B; g.T_out = g.T_in = g.Tv_out = g.Tv_in = g.T_virt = T; g.stride = 1; g.up_mode = UP_NONE;
  g.M = B * T; g.N = N; g.epi = EPI_STORE; g.ldo = N; g.ldres = N; g.zero_page = zero_page;
  return g;
}
inline GemmSeg seg1(const bf16_t* hi, const bf16_t* lo, int c, int taps, int pad) {
  GemmSeg s{};
  s.a0_hi = hi; s.a0_lo = lo; s.c0 = c; s.taps = taps; s.pad = pad;
  return s;
}
// `g` against the packed weight `pw` becomes the next launch (its parameters live in `store`: stable addresses)
inline void push_gemm(std::vector<std::unique_ptr<GemmParams>>& store, std::vector<OpFn>& ops, double& flops, GemmParams g, const PackedW3* pw,
                      int k_real, int prec) {
  g.w_hi = pw->hi; g.w_lo = pw->lo; g.Kp = pw->Kp; g.N_pad = pw->N_pad; g.bias = pw->bias;
  store.emplace_back(new GemmParams(g));
  const GemmParams* p = store.back().get();
  ops.push_back([p, prec](hipStream_t s) { return launch_gemm(*p, prec, s); });
  flops += 2.0 * (double)g.M * (double)g.N * (double)k_real;
}

// ----------------------------------------------------------------------------- probes
// Host copy of a kept intermediate [B, T, C]: fp32 rows `p`, or (p null) split planes joined on the host, value = scale * (hi + lo)
// (bf16 bits are the upper half of an fp32; lo may be null).  Utterances lie Tp frames apart (rows of a padded row space are
// skipped).  `dims`, if given, receives [B, T, C]; a null `host_out` asks for the dims alone.
inline int probe_rows(const float* p, const bf16_t* hi, const bf16_t* lo, float scale, int B, int T, int C, int Tp, float* host_out,
                      int64_t capacity, int64_t* dims) {
  const int64_t n = (int64_t)B * T * C;
  if (dims) { dims[0] = B; dims[1] = T; dims[2] = C; }
  if (!host_out) return DV_OK;
  if (capacity < n) return dv_fail(DV_ERR_INVALID, "probe buffer too small");
  HIPCHK(hipDeviceSynchronize());
  const size_t row = (size_t)T * C, pitch = (size_t)Tp * C;
  if (p) {
    HIPCHK(hipMemcpy2D(host_out, row * sizeof(float), p, pitch * sizeof(float), row * sizeof(float), (size_t)B, hipMemcpyDeviceToHost));
    return DV_OK;
  }
  std::vector<bf16_t> h((size_t)n), l;
  HIPCHK(hipMemcpy2D(h.data(), row * sizeof(bf16_t), hi, pitch * sizeof(bf16_t), row * sizeof(bf16_t), (size_t)B, hipMemcpyDeviceToHost));
  if (lo) {
    l.resize((size_t)n);
    HIPCHK(hipMemcpy2D(l.data(), row * sizeof(bf16_t), lo, pitch * sizeof(bf16_t), row * sizeof(bf16_t), (size_t)B, hipMemcpyDeviceToHost));
  }
  auto f32 = [](bf16_t b) { const uint32_t w = (uint32_t)b << 16; float f; memcpy(&f, &w, 4); return f; };
  for (int64_t i = 0; i < n; ++i) host_out[i] = scale * (f32(h[(size_t)i]) + (lo ? f32(l[(size_t)i]) : 0.f));
  return DV_OK;
}

// ----------------------------------------------------------------------------- row-space encoder handles (tenc.hip, qenc.hip)
struct RowProbe { std::string name; const float* p; const bf16_t* hi; const bf16_t* lo; int C; };

// What a handle of an encoder over rows m = b * T + t keeps: the state dict, the packed weights (kept across prepares while
// the weights stay the same) and one prepared (B, T) schedule.
struct RowEngine {
  WeightStore w;
  bool weights_dirty = true;
  bool prepared = false, keep = false;       // keep: DVITS_KEEP_INTERMEDIATES=1 at prepare time
  int B = 0, T = 0, precision = 0;
  std::vector<void*> owned, owned_w;         // per prepared shape / packed weights
  std::map<std::string, PackedW3> packed;
  std::vector<std::unique_ptr<GemmParams>> gemm_store;
  std::vector<OpFn> ops;
  std::vector<RowProbe> probes;
  bf16_t* zero_page = nullptr;
  double flops = 0;

  void release_packed() { free_owned(owned_w); packed.clear(); }
  void release_prepared() {
    free_owned(owned);
    gemm_store.clear(); ops.clear(); probes.clear();
    zero_page = nullptr; prepared = false; flops = 0;
  }
};

// dv_*_set_weight / dv_*_stats / dv_*_probe of such a handle (`what`: the ABI prefix; `e` null: a null handle).  A new weight
// drops the prepared schedule.
inline int row_set_weight(RowEngine* e, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim, const char* what) {
  if (!e) return dv_fail(DV_ERR_INVALID, "%s: bad argument", what);
  int rc = e->w.set(name, dev_ptr, shape, ndim, what);
  if (rc == DV_OK) { e->weights_dirty = true; e->prepared = false; }
  return rc;
}
inline int row_stats(const RowEngine* e, int64_t* n_launch, double* flops, const char* what) {
  if (!e || !e->prepared) return dv_fail(DV_ERR_STATE, "%s_stats before prepare", what);
  if (n_launch) *n_launch = (int64_t)e->ops.size();
  if (flops) *flops = e->flops;
  return DV_OK;
}
inline int row_probe(const RowEngine* e, const char* name, float* host_out, int64_t capacity, int64_t* dims, const char* what) {
  if (!e || !name) return dv_fail(DV_ERR_INVALID, "%s_probe: null argument", what);
  if (!e->prepared) return dv_fail(DV_ERR_STATE, "%s_probe before %s_prepare", what, what);
  for (const RowProbe& p : e->probes)
    if (p.name == name) return probe_rows(p.p, p.hi, p.lo, 1.f, e->B, e->T, p.C, e->T, host_out, capacity, dims);
  return dv_fail(DV_ERR_INVALID, "no probe named %s (prepare with DVITS_KEEP_INTERMEDIATES=1)", name);
}

// The planner of one prepare of such a handle: what TPlan (tenc.hip) and QPlan (qenc.hip) share.
struct RowPlan {
  RowEngine* e = nullptr;
  int B = 0, T = 0, M = 0;
  PlanError err;
  hipStream_t st = nullptr;

  const RawW* raw(const std::string& name, size_t numel) { return e->w.find(name, numel, err); }
  const float* W(const std::string& name, size_t numel) { const RawW* r = raw(name, numel); return r ? r->p : nullptr; }
  template <typename X> X* dmalloc(size_t elems, std::vector<void*>& owner, bool zero) { return ::dmalloc<X>(elems, owner, zero, st, err); }
  bool zero_page() { return (e->zero_page = dmalloc<bf16_t>(DV_ZERO_PAGE_BYTES / sizeof(bf16_t), e->owned, true)) != nullptr; }
  GemmParams gp(int N) const { return row_gemm_params(B, T, N, e->zero_page); }
  void gemm(const GemmParams& g, const PackedW3* pw, int k_real) { push_gemm(e->gemm_store, e->ops, e->flops, g, pw, k_real, e->precision); }
  void probe(const std::string& name, const float* p, int C) { if (e->keep) e->probes.push_back(RowProbe{name, p, nullptr, nullptr, C}); }
};
