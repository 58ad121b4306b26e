// artn_host.h -- host plumbing shared by every translation unit of libartn_hip.so: error reporting, the dynamic-LDS
// opt-in, environment switches, and the launchers that live in objects of their own (units/*.hip) and are called from the
// dispatch in artn_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdlib.h>
#include <string>

#include "artn.h"

struct ArtnPlan; // artn_plan.h

// ----------------------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------------------
struct ArtnHostState {
  std::string err;  // artn_last_error()
  std::string note; // artn_last_plan_note(): why the last planned step fell back to the strided kernel
};
ArtnHostState &artn_host_state(); // the calling thread's; defined once, in artn_api.hip
static int fail(int code, const std::string &msg) {
  artn_host_state().err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(ARTN_E_LAUNCH, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

static bool env_flag(const char *name) {
  const char *v = getenv(name);
  return v && v[0] && v[0] != '0';
}

// Kernels that need more than 64 KiB of dynamic LDS must say so once per device; repeating
// the call per launch is needless host work and is not welcome during stream capture.
template <auto Kern>
static hipError_t ensure_lds(size_t lds) {
  static std::atomic<int> have[16];
  if (lds <= 64 * 1024) return hipSuccess;
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  std::atomic<int> &h = have[dev & 15];
  if ((int)lds <= h.load(std::memory_order_relaxed)) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) h.store((int)lds, std::memory_order_relaxed);
  return e;
}

// ----------------------------------------------------------------------------------------
// launchers with an object of their own (the ~100 artn_k_bits instantiations dominate the build: `make -j` compiles the
// families side by side).  units/<name>.hip defines artn_launch_<name>() and so emits that family's kernels.
// ----------------------------------------------------------------------------------------
#define ARTN_BITS_ARGS const ArtnPlan &p, const float2 *A, const float2 *B1, const float2 *B2, float2 *C, hipStream_t st
#define ARTN_BITS3_ARGS const ArtnPlan &p, const float2 *A, const float2 *B1, const float2 *B2, const float2 *B3, float2 *C, hipStream_t st
#define ARTN_VOID_ARGS const ArtnPlan &p, const void *A, const void *B1, const void *B2, void *C, hipStream_t st
// artn_k_bits<K, *> / artn_k_alt<K, *>, K first-stage contracted bits; K = 5 and 6 in two halves: second-stage counts 0..3 / 4..6
hipError_t artn_launch_bits_k1(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k2(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k3(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k4(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k5h0(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k5h1(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k6h0(ARTN_BITS_ARGS);
hipError_t artn_launch_bits_k6h1(ARTN_BITS_ARGS);
hipError_t artn_launch_bits128(ARTN_VOID_ARGS);     // artn_k_bits128<*, *, false>
hipError_t artn_launch_bits128_acc(ARTN_VOID_ARGS); // artn_k_bits128<*, *, true> (ArtnBitsPlan::accumulate)
hipError_t artn_launch_wide(ARTN_VOID_ARGS);        // artn_k_wide<*, *>
// artn_k_bits3<K, *, *>: development builds only (make dev: -DARTN_DEV_BITS3)
hipError_t artn_launch_bits3_k3(ARTN_BITS3_ARGS);
hipError_t artn_launch_bits3_k4(ARTN_BITS3_ARGS);
hipError_t artn_launch_bits3_k5(ARTN_BITS3_ARGS);
