// Force-included in front of the K5 / K8 sources by tools/micro/dispatch_record.hip: launches and HIP queries are recorded, not made.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace evc {
struct GemvRowsLaunch;
struct GemvColsLaunch;
struct ColProblem;
}
extern int g_shim_cus;
void shim_begin(const char *k, dim3 g, dim3 b, size_t lds);
void shim_end();
void shim_arg(int v);
void shim_arg(const evc::GemvRowsLaunch &L);
void shim_arg(const evc::GemvColsLaunch &L);
void shim_arg(const evc::ColProblem &P);
template <class T>
void shim_arg(const T &) {}
template <class... A>
void shim_launch(const char *k, dim3 g, dim3 b, size_t lds, hipStream_t, const A &...a) {
    shim_begin(k, g, b, lds);
    (shim_arg(a), ...);
    shim_end();
}
inline hipError_t shim_hipGetDevice(int *d) { *d = 0; return hipSuccess; }
inline hipError_t shim_hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = g_shim_cus; return hipSuccess; }
inline hipError_t shim_hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
inline hipError_t shim_hipGetLastError() { return hipSuccess; }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, lds, st, ...) shim_launch(#k, g, b, (size_t)(lds), st, __VA_ARGS__)
#define hipGetDevice shim_hipGetDevice
#define hipDeviceGetAttribute shim_hipDeviceGetAttribute
#define hipFuncSetAttribute shim_hipFuncSetAttribute
#define hipGetLastError shim_hipGetLastError
