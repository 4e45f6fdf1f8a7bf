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
__device__ __forceinline__ int fn_wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t fn_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long fn_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ov = __shfl_xor(v, o, 64);
        v = ov > v ? ov : v;
    }
    return v;
}

// inclusive scan over the 64 lanes: the sum of x over the lanes up to and including `lane` (the caller's own lane index)
template <class T>
__device__ __forceinline__ T fn_wave_scan_add(T x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}
// carry-forward scan: the last non-zero v at or before the lane, 0 where there is none
__device__ __forceinline__ uint32_t fn_wave_scan_last(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(v, o, 64);
        if (lane >= o && v == 0u) v = y;
    }
    return v;
}

// (max, first index holding it) of the lanes' (mx, am) pairs, the same in every lane: torch.max semantics.  Not fn_wave_max: that one is fmaxf, which
// skips a NaN where `>` keeps what it has.  The butterfly runs on copies: with the caller's variables in the loop the compiler allocates registers
// and places waits differently from the kernels that had this loop inline (measured on vocab_sample_kernel: 101 -> 111 us per launch).
__device__ __forceinline__ void fn_wave_argmax(float& mx_io, int& am_io) {
    float mx = mx_io;
    int am = am_io;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (ov > mx || (ov == mx && oa < am)) { mx = ov; am = oa; }
    }
    mx_io = mx, am_io = am;
}

// The head of one row of E logits read lane-strided by one wavefront (lane l: e = l, l + 64, ...): max, first-index argmax (0x7fffffff for a row
// without a value above -inf) and log-sum-exp, the same in every lane.  The heads that promise bit-equal log-probs (fn_vocab_argmax, fn_vocab_sample,
// fn_beam_step) all take them from here: x[e] - lse.
struct FnRowHead {
    float mx, lse;
    int am;
};
__device__ __forceinline__ FnRowHead fn_row_head(const float* __restrict__ x, int E, int lane) {
    FnRowHead h;
    h.mx = -INFINITY, h.am = 0x7fffffff;
    for (int e = lane; e < E; e += 64) {
        const float v = x[e];
        if (v > h.mx) { h.mx = v; h.am = e; }
    }
    fn_wave_argmax(h.mx, h.am);
    float s = 0.f;
    for (int e = lane; e < E; e += 64) s += expf(x[e] - h.mx);
    s = fn_wave_sum(s);
    h.lse = h.mx + logf(s);
    return h;
}

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four words.  The draws of fn_vocab_sample and fn_latent_draw both come from here;
// host/sample_host.h has the same rounds in plain C++.
__device__ __forceinline__ void fn_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Box-Muller on the four words of a quad (fn_latent_draw, step 2): w -> four normals.  fn_latent_draw and fn_posterior_draw both take them from here,
// which is what makes a posterior sample bit-equal to the prior draw's eps at the same counter.
__device__ __forceinline__ void fn_quad_normals(const uint32_t w[4], float n[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float ua = (float)((w[2 * h] >> 8) + 1u) * 0x1p-24f, ub = (float)(w[2 * h + 1] >> 8) * 0x1p-24f;
        const float r = sqrtf(-2.0f * logf(ua));
        float s, c;
        sincospif(2.0f * ub, &s, &c);
        n[2 * h] = r * c;
        n[2 * h + 1] = r * s;
    }
}

// pack(x, v) over V columns: order-preserving key of x in the high half, V - 1 - v in the low half, so the 64-bit maximum is the largest x and, among
// equals, the lowest column (fn_out_argmax_f32, fn_beam_step)
__device__ __forceinline__ unsigned long long fn_pack_best(float x, int v, int V) {
    const uint32_t b = __float_as_uint(x);
    const uint32_t key = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    return ((unsigned long long)key << 32) | (uint32_t)(V - 1 - v);
}
