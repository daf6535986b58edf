// Host check of the plan side of classifier-free guidance (diff-vits_amd/csrc/sampler.hip: dv_sampler_plan_method,
// dv_plan_set_guidance, the argument validation of dv_sampler_run_custom* / dv_op_cfg_combine, dv_plan_destroy) under
// AddressSanitizer / UBSan: a stand-alone program, sampler.hip compiled with the sanitizers on the host side, every engine
// and kernel entry point it links against stubbed here.  Nothing in it launches on a GPU (every call below is refused, or
// answered, before the first launch).
//
//   mkdir -p build && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all diff-vits_amd/csrc/sampler.hip tools/guidance_plan_check.cc \
//       -o build/guidance_plan_check && build/guidance_plan_check
// prints one line per group of checks and exits non-zero if any failed.
#include "../include/dvits_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <vector>

// ---- what sampler.hip links against (engine.hip, the kernel files): never reached by the calls below
static char g_err[512];
int dv_fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
struct dv_unet;
static int g_stub_calls = 0;
int dv_unet_enqueue(dv_unet*, const float*, int, const float*, const float*, float*, hipStream_t, int) { ++g_stub_calls; return -1; }
int dv_unet_temb_all(dv_unet*, const float*, int, hipStream_t) { ++g_stub_calls; return -1; }
int dv_unet_dims(const dv_unet*, int*, int*, int*, int*, int64_t*) { ++g_stub_calls; return 0; }
int dv_unet_health(const dv_unet*) { ++g_stub_calls; return 0; }
hipError_t launch_lincomb(float*, const float*, const float*, const float*, const float*, const float*, const float*, int64_t, hipStream_t) { ++g_stub_calls; return hipErrorUnknown; }
size_t dyn_thresh_ws_bytes(int) { ++g_stub_calls; return 0; }
hipError_t launch_dyn_thresh(float*, int, int64_t, float, float, uint32_t*, float*, hipStream_t) { ++g_stub_calls; return hipErrorUnknown; }
hipError_t launch_cfg_pair_in(const float*, float*, int64_t, hipStream_t) { ++g_stub_calls; return hipErrorUnknown; }
hipError_t launch_cfg_combine(const float*, float*, int64_t, float, hipStream_t) { ++g_stub_calls; return hipErrorUnknown; }

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_err); ++g_failed; } } while (0)

static int model_cb(void*, const float*, double, float*, void*) { ++g_stub_calls; return 1; }

int main() {
  std::vector<float> betas(1000);
  for (int i = 0; i < 1000; ++i) betas[i] = (float)(1e-4 + (2e-2 - 1e-4) * i / 999.0);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int solvers[] = {DV_SOLVER_DPMPP, DV_SOLVER_UNIPC_BH2, DV_SOLVER_DPM, DV_SOLVER_UNIPC_VARY_NOISE};
  for (int solver : solvers) {
    const bool dpm = solver == DV_SOLVER_DPMPP || solver == DV_SOLVER_DPM;
    for (int method = DV_METHOD_MULTISTEP; method <= (dpm ? DV_METHOD_SINGLESTEP_FIXED : DV_METHOD_MULTISTEP); ++method) {
      dv_plan* p = nullptr;
      CHECK(dv_sampler_plan_method(solver, DV_SCHEDULE_DISCRETE, betas.data(), 1000, 0.0, 0.0, method, 9, 3, DV_SKIP_TIME_UNIFORM, 1,
                                   -1.0, 0.05, 1, &p) == DV_OK && p);
      if (!p) continue;
      int32_t nfe = 0;
      CHECK(dv_plan_info(p, &nfe, nullptr, nullptr) == DV_OK && nfe >= 9);
      // guidance: on, changed, off, on again - and every refusal
      CHECK(dv_plan_set_guidance(p, nan, 1) == DV_ERR_INVALID);
      CHECK(dv_plan_set_guidance(p, inf, 1) == DV_ERR_INVALID);
      CHECK(dv_plan_set_guidance(p, -inf, 1) == DV_ERR_INVALID);
      CHECK(dv_plan_set_guidance(nullptr, 2.0, 1) == DV_ERR_INVALID);
      CHECK(dv_plan_set_guidance(p, 2.0, 1) == DV_OK);
      CHECK(dv_plan_set_guidance(p, 2.0, 1) == DV_OK);
      CHECK(dv_plan_set_guidance(p, -1.0, 1) == DV_OK);
      CHECK(dv_plan_set_guidance(p, nan, 0) == DV_OK);
      CHECK(dv_plan_set_guidance(p, 7.5, 1) == DV_OK);
      // with thresholding beside it
      std::vector<uint8_t> mask((size_t)nfe, 0);
      mask.back() = 1;
      CHECK(dv_plan_set_thresholding(p, 0.9, 0.6, mask.data()) == DV_OK);
      // a guided plan is refused by the callback forms before anything runs (x is host memory: nothing may touch it)
      alignas(16) float x[64] = {0};
      CHECK(dv_sampler_run_custom(p, model_cb, nullptr, x, 64, nullptr) == DV_ERR_INVALID);
      CHECK(dv_sampler_run_custom_rows(p, model_cb, nullptr, x, 2, 64, nullptr) == DV_ERR_INVALID);
      CHECK(dv_sampler_run(p, nullptr, x, nullptr, nullptr) == DV_ERR_INVALID);
      CHECK(dv_plan_set_thresholding(p, -1.0, 1.0, nullptr) == DV_OK);
      CHECK(dv_plan_set_guidance(p, 1.0, 0) == DV_OK);
      dv_plan_destroy(p);
    }
  }
  printf("plans: guidance set / changed / cleared on %d solver and method combinations\n", 8);
  {
    float pair[32] = {0}, out[16] = {0};
    CHECK(dv_op_cfg_combine(nullptr, out, 2, 8, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, nullptr, 2, 8, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 0, 8, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 2049, 8, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 2, 0, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 2, (int64_t)1 << 31, 1.0, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 2, 8, nan, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine(pair, out, 2, 8, inf, nullptr) == DV_ERR_INVALID);
    CHECK(dv_op_cfg_combine((const float*)((const char*)pair + 2), out, 2, 8, 1.0, nullptr) == DV_ERR_INVALID);
    printf("dv_op_cfg_combine: 9 bad argument sets refused\n");
  }
  CHECK(g_stub_calls == 0);
  printf(g_failed ? "%d checks FAILED\n" : "all checks passed, no engine or kernel entry point was reached\n", g_failed);
  return g_failed ? 1 : 0;
}
