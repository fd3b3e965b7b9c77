// Force-included in front of every csrc source by tools/micro/launch_record.hip: kernel launches, copies, memsets, event and
// stream calls are recorded, not made; the HIP queries the launchers make are answered from constants.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern int g_shim_cus;
void shim_record_launch(const char *pretty, const void *stub, dim3 g, dim3 b, size_t lds, hipStream_t st, uint64_t arg_hash);
void shim_record_call(const char *what, hipStream_t st, const char *fmt, ...);

// the kernel as the compiler names it (the instantiation: from the symbol of its host stub, shim_record_launch)
template <auto K>
const char *shim_kname() {
    return __PRETTY_FUNCTION__;
}
// FNV-1a over the bytes of every by-value kernel argument, in order
template <class T>
inline void shim_hash(uint64_t &h, const T &v) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&v);
    for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
}
template <class... A>
void shim_launch(const char *pretty, const void *stub, dim3 g, dim3 b, size_t lds, hipStream_t st, const A &...a) {
    uint64_t h = 14695981039346656037ull;
    (shim_hash(h, a), ...);
    shim_record_launch(pretty, stub, g, b, lds, st, h);
}
inline hipError_t shim_hipGetDevice(int *d) { *d = 0; return hipSuccess; }
inline hipError_t shim_hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = g_shim_cus; return hipSuccess; }
inline hipError_t shim_hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
inline hipError_t shim_hipGetLastError() { return hipSuccess; }
hipError_t shim_hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
hipError_t shim_hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                                 hipMemcpyKind kind, hipStream_t st);
hipError_t shim_hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t st);
hipError_t shim_hipEventRecord(hipEvent_t e, hipStream_t st);
hipError_t shim_hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned flags);
hipError_t shim_hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t shim_hipEventSynchronize(hipEvent_t e);
hipError_t shim_hipEventDestroy(hipEvent_t e);
hipError_t shim_hipStreamCreateWithFlags(hipStream_t *s, unsigned flags);
hipError_t shim_hipStreamDestroy(hipStream_t s);
inline hipError_t shim_hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *cs) {
    *cs = hipStreamCaptureStatusNone;
    return hipSuccess;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, lds, st, ...) shim_launch(shim_kname<k>(), reinterpret_cast<const void *>(k), g, b, (size_t)(lds), st, __VA_ARGS__)
#define hipGetDevice shim_hipGetDevice
#define hipDeviceGetAttribute shim_hipDeviceGetAttribute
#define hipFuncSetAttribute shim_hipFuncSetAttribute
#define hipGetLastError shim_hipGetLastError
#define hipMemcpyAsync shim_hipMemcpyAsync
#define hipMemcpy2DAsync shim_hipMemcpy2DAsync
#define hipMemsetAsync shim_hipMemsetAsync
#define hipEventRecord shim_hipEventRecord
#define hipStreamWaitEvent shim_hipStreamWaitEvent
#define hipEventCreateWithFlags shim_hipEventCreateWithFlags
#define hipEventSynchronize shim_hipEventSynchronize
#define hipEventDestroy shim_hipEventDestroy
#define hipStreamCreateWithFlags shim_hipStreamCreateWithFlags
#define hipStreamDestroy shim_hipStreamDestroy
#define hipStreamIsCapturing shim_hipStreamIsCapturing
