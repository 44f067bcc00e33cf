// Host-side helpers shared by the four translation units: the error text of the C ABI (no exceptions across the boundary),
// the environment knobs, and the one checked launch path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

// the thread's error text, read back through rv_last_error() (the buffer lives in gemm.hip)
void rv_set_error(const char* msg);
void rv_set_errorf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define RV_CHECK_LAUNCH()                                   \
  do {                                                      \
    hipError_t e__ = hipGetLastError();                     \
    if (e__ != hipSuccess) {                                \
      rv_set_error(hipGetErrorString(e__));                 \
      return 2;                                             \
    }                                                       \
  } while (0)
#define RV_REQUIRE(cond, msg)                               \
  do {                                                      \
    if (!(cond)) {                                          \
      rv_set_error(msg);                                    \
      return 1;                                             \
    }                                                       \
  } while (0)
// RV_REQUIRE inside a check that several entry points share: the message starts with `who`, the entry point that was called
#define RV_REQUIRE_AS(who, cond, what)                      \
  do {                                                      \
    if (!(cond)) {                                          \
      rv_set_errorf("%s: %s", who, what);                   \
      return 1;                                             \
    }                                                       \
  } while (0)

// An A/B knob of the environment.  Every knob has one accessor that keeps the value in a function-local static, so it is read
// once per process, on the first call that needs it.
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// The one launch path.  `lds` = dynamic LDS in bytes: the first launch of THIS instantiation that asks for some raises the
// kernel's limit to it (once per process for the kernels with a fixed size; again only when a later launch asks for more),
// and a limit that cannot be raised is rc 2, not a launch.  Then the launch, whose failure is rc 2 as well.  `stream` is the
// void* of the C ABI.
template <auto Kernel, class... Args>
int launch(int lds, dim3 grid, dim3 block, void* stream, const Args&... args) {
  static int lds_limit = 0;
  if (lds > lds_limit) {
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();                  // or the next launch's RV_CHECK_LAUNCH would report this one
      rv_set_errorf("raising a kernel's dynamic-LDS limit to %d bytes: %s", lds, hipGetErrorString(e));
      return 2;
    }
    lds_limit = lds;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, (hipStream_t)stream, args...);
  RV_CHECK_LAUNCH();
  return 0;
}
