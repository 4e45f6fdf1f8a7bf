// common.h - shared host/device helpers for libfadernets_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/fadernets.h"

// Launch errors surface as positive hipError_t through the C ABI (never exceptions).
#define FN_CHECK_LAUNCH()                        \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

const char* fn_comm_strerror(int code);      // comm.hip: text of FN_COMM_ERROR_BASE + ncclResult_t

// ---- per-device caches of the launchers (a process may drive several GPUs): write-once facts in zero-initialised atomics ----
constexpr int FN_MAX_DEVICES = 32;

// the current device, or -1 when it cannot be asked or lies beyond the caches
inline int fn_device() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < FN_MAX_DEVICES ? dev : -1;
}

// compute units of the current device; 0 when it cannot be asked
inline int fn_cu_count() {
    static std::atomic<int> n[FN_MAX_DEVICES];
    const int dev = fn_device();
    if (dev < 0) return 0;
    int c = n[dev].load(std::memory_order_acquire);
    if (c == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        c = prop.multiProcessorCount;
        n[dev].store(c, std::memory_order_release);
    }
    return c;
}

// Lets kernel K use up to `bytes` of dynamic LDS, once per device (setting the attribute twice is harmless, so racing threads may both set it).
// FN_OK, the hipError_t of the attribute call, or no_device (the caller's own code) when the current device cannot be asked.
template <auto K>
int fn_set_max_lds(int bytes, int no_device) {
    static std::atomic<bool> done[FN_MAX_DEVICES];
    const int dev = fn_device();
    if (dev < 0) return no_device;
    if (!done[dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
        done[dev].store(true, std::memory_order_release);
    }
    return FN_OK;
}

__device__ __forceinline__ float fn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float fn_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double fn_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
