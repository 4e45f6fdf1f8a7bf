// disentangle.hip - the device side of the latent disentanglement report (disentangle.py): column ranges, the uint8 bin image, the joint histograms of
// every (code column, factor) pair, mid-ranks by counting, centred fp64 sums for Pearson / Spearman, and the mutual-information scores from the
// histograms.  OURS - the reference's run_through_gmm copies every batch to the host and stops there; include/fadernets.h has the definitions and the
// stated order of every fp64 sum.  The argument checks are host/disentangle_host.h's, shared with the host twins.  Built with -ffp-contract=off (the
// Makefile): the bin arithmetic and every term of the centred sums are single IEEE operations, which is what makes the device, the twin and numpy
// agree bit for bit.
#include <cfloat>

#include "common.h"
#include "host/disentangle_host.h"

namespace {

constexpr int CELLS = fn_dis_host::CELLS;

struct CardArgs {
    int32_t card[FN_DIS_MAX_A];
};

// ---- fn_column_range ----
__global__ void range_init_kernel(float* __restrict__ lo, float* __restrict__ hi, int32_t* __restrict__ status, int P) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < P) lo[c] = INFINITY, hi[c] = -INFINITY, status[c] = 0;
}

// min / max of floats through integer atomics on the bit patterns: a value >= 0 orders as a signed int, a negative one in reverse as an unsigned.
// v is never -0.0 (the caller adds 0.0f) and never a NaN.
__device__ __forceinline__ void atomic_min_f32(float* p, float v) {
    if (v >= 0.0f) atomicMin((int*)p, __float_as_int(v));
    else atomicMax((unsigned int*)p, __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* p, float v) {
    if (v >= 0.0f) atomicMax((int*)p, __float_as_int(v));
    else atomicMin((unsigned int*)p, __float_as_uint(v));
}

// 4 x 64 threads: threadIdx.x is the column within the group of 64 (consecutive lanes read consecutive floats), threadIdx.y the row phase;
// blockIdx.y the chunk of FN_DIS_RANGE_CHUNK rows
__global__ __launch_bounds__(256) void range_kernel(const float* __restrict__ x, long ld, int N, int P, float* lo, float* hi, int32_t* status) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= P) return;
    const int r0 = blockIdx.y * FN_DIS_RANGE_CHUNK, r1 = min(N, r0 + FN_DIS_RANGE_CHUNK);
    float a = INFINITY, b = -INFINITY;
    bool bad = false;
    for (int i = r0 + (int)threadIdx.y; i < r1; i += 4) {
        const float v = x[(long)i * ld + c] + 0.0f;
        if (fabsf(v) <= FLT_MAX) a = fminf(a, v), b = fmaxf(b, v);
        else bad = true;
    }
    if (a <= FLT_MAX) atomic_min_f32(lo + c, a), atomic_max_f32(hi + c, b);
    if (bad) atomicOr(status + c, FN_DIS_NONFINITE);
}

// ---- fn_bin_columns ----
// one thread per (row, column): blockIdx.y is the column, consecutive threads write consecutive bytes of its image
__global__ __launch_bounds__(256) void bin_kernel(const float* __restrict__ x, long ld, int N, const float* __restrict__ lo, const float* __restrict__ hi,
                                                  CardArgs ca, int use_card, int bins, uint8_t* __restrict__ img, long n_pad, int32_t* status) {
    const int c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int C = use_card ? ca.card[c] : 0;
    const float v = x[(long)i * ld + c];
    int b;
    if (C == 0) {
        b = fn_dis_host::bin_of(v, lo[c], hi[c], bins);
    } else if (!fn_dis_host::level_of(v, C, &b)) {
        atomicOr(status + c, FN_DIS_BAD_LEVEL);
    }
    img[(long)c * n_pad + i] = (uint8_t)b;
}

// ---- fn_joint_hist ----
// one workgroup per (chunk of FN_DIS_HIST_CHUNK rows, factor a, code column d): a 16 KB LDS table, integer atomics into it, then the non-zero cells
// go to global memory with integer atomics
__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* __restrict__ bz, long ldz, const uint8_t* __restrict__ bf, long ldf, int A, int N,
                                                   int32_t* counts) {
    __shared__ int tab[CELLS];
    const int a = blockIdx.y, d = blockIdx.z;
    for (int k = threadIdx.x; k < CELLS; k += 256) tab[k] = 0;
    __syncthreads();
    const int r0 = blockIdx.x * FN_DIS_HIST_CHUNK, r1 = min(N, r0 + FN_DIS_HIST_CHUNK);
    const uint8_t *pz = bz + (long)d * ldz, *pf = bf + (long)a * ldf;
    for (int i = r0 + (int)threadIdx.x; i < r1; i += 256) atomicAdd(&tab[(pz[i] & 63) * 64 + (pf[i] & 63)], 1);
    __syncthreads();
    int32_t* out = counts + ((long)d * A + a) * CELLS;
    for (int k = threadIdx.x; k < CELLS; k += 256) {
        const int n = tab[k];
        if (n) atomicAdd(out + k, n);
    }
}

// ---- fn_column_ranks ----
// 256 threads own FN_DIS_RANK_ROWS = 4 x 256 rows of column blockIdx.y in registers and walk the whole column in LDS tiles; a tile's tail is NaN
__global__ __launch_bounds__(256) void ranks_kernel(const float* __restrict__ x, long ld, int N, float* __restrict__ ranks, long n_pad) {
    __shared__ float4 tile[FN_DIS_RANK_TILE / 4];
    float* tf = reinterpret_cast<float*>(tile);
    const int c = blockIdx.y, tid = threadIdx.x;
    const float* col = x + c;
    const int i0 = blockIdx.x * FN_DIS_RANK_ROWS + tid;
    float xi[4];
    int less[4], equal[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + r * 256;
        xi[r] = i < N ? col[(long)i * ld] : NAN;
        less[r] = equal[r] = 0;
    }
    for (int j0 = 0; j0 < N; j0 += FN_DIS_RANK_TILE) {
        __syncthreads();          // the previous tile has been read
#pragma unroll
        for (int r = 0; r < FN_DIS_RANK_TILE / 256; ++r) {
            const int j = j0 + r * 256 + tid;
            tf[r * 256 + tid] = j < N ? col[(long)j * ld] : NAN;
        }
        __syncthreads();
        const int n4 = (min(N - j0, FN_DIS_RANK_TILE) + 3) / 4;
        for (int k = 0; k < n4; ++k) {
            const float4 w = tile[k];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                less[r] += (w.x < xi[r]) + (w.y < xi[r]) + (w.z < xi[r]) + (w.w < xi[r]);
                equal[r] += (w.x == xi[r]) + (w.y == xi[r]) + (w.z == xi[r]) + (w.w == xi[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + r * 256;
        if (i < N) ranks[(long)c * n_pad + i] = (float)(2 * less[r] + equal[r] + 1) * 0.5f;
    }
}

// ---- fn_column_corr ----
// one wavefront per X column, 4 per workgroup.  Lane l owns the rows l, l + 64, ...; every wavefront forms the Y sums too (in the same order, so all
// hold the same bits) and the one of column 0 stores them.
__global__ __launch_bounds__(256) void corr_kernel(const float* __restrict__ X, long x_rs, long x_cs, int P, const float* __restrict__ Y, long y_rs,
                                                   long y_cs, int Q, int N, double* __restrict__ mean_x, double* __restrict__ ss_x,
                                                   double* __restrict__ mean_y, double* __restrict__ ss_y, double* __restrict__ cross) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const float* x = X + (long)p * x_cs;
    double sx = 0.0, sy[FN_DIS_MAX_A];
#pragma unroll
    for (int q = 0; q < FN_DIS_MAX_A; ++q) sy[q] = 0.0;
    for (int i = lane; i < N; i += 64) {
        sx += (double)x[(long)i * x_rs];
#pragma unroll
        for (int q = 0; q < FN_DIS_MAX_A; ++q)
            if (q < Q) sy[q] += (double)Y[(long)i * y_rs + (long)q * y_cs];
    }
    const double mx = fn_wave_sum_f64(sx) / (double)N;
    double my[FN_DIS_MAX_A];
#pragma unroll
    for (int q = 0; q < FN_DIS_MAX_A; ++q) my[q] = q < Q ? fn_wave_sum_f64(sy[q]) / (double)N : 0.0;
    double sxx = 0.0, syy[FN_DIS_MAX_A], sxy[FN_DIS_MAX_A];
#pragma unroll
    for (int q = 0; q < FN_DIS_MAX_A; ++q) syy[q] = sxy[q] = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double dx = (double)x[(long)i * x_rs] - mx;
        const double txx = dx * dx;
        sxx += txx;
#pragma unroll
        for (int q = 0; q < FN_DIS_MAX_A; ++q) {
            if (q < Q) {
                const double dy = (double)Y[(long)i * y_rs + (long)q * y_cs] - my[q];
                const double tyy = dy * dy, txy = dx * dy;
                syy[q] += tyy, sxy[q] += txy;
            }
        }
    }
    sxx = fn_wave_sum_f64(sxx);
    if (lane == 0) mean_x[p] = mx, ss_x[p] = sxx;
#pragma unroll
    for (int q = 0; q < FN_DIS_MAX_A; ++q) {
        if (q < Q) {
            const double vyy = fn_wave_sum_f64(syy[q]), vxy = fn_wave_sum_f64(sxy[q]);
            if (lane == 0) {
                cross[(long)p * Q + q] = vxy;
                if (p == 0) mean_y[q] = my[q], ss_y[q] = vyy;
            }
        }
    }
}

// ---- fn_mi_scores ----
// one wavefront per pair, 4 per workgroup.  Lane l owns column bf = l of the 64 x 64 table (consecutive lanes read consecutive counts) and row bz = l
// for the row sums.
__global__ __launch_bounds__(256) void mi_kernel(const int32_t* __restrict__ counts, int pairs, double* __restrict__ out, int32_t* __restrict__ hits) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= pairs) return;
    const int32_t* t = counts + (long)e * CELLS;
    int col = 0, row = 0, h = 0;
    for (int bz = 0; bz < 64; ++bz) {
        const int n = t[bz * 64 + lane];
        col += n;
        const int rs = fn_wave_sum_i32(n);
        if (lane == bz) row = rs;
        h += (int)fn_wave_max_u32((uint32_t)max(n, 0));
    }
    const long T = fn_wave_sum_i32(col);
    double* o = out + (long)e * FN_DIS_MI_COLS;
    if (lane == 0) hits[e] = h;
    if (T == 0) {          // the same in every lane
        if (lane == 0) o[0] = o[1] = o[2] = 0.0;
        return;
    }
    const double dT = (double)T;
    double acc = 0.0;
    for (int bz = 0; bz < 64; ++bz) {
        const long n = t[bz * 64 + lane];
        const long r = __shfl(row, bz, 64);
        if (n > 0) {
            const double term = ((double)n / dT) * log((double)(n * T) / (double)(r * (long)col));
            acc += term;
        }
    }
    double hz = 0.0, hf = 0.0;
    if (row > 0) {
        const double pr = (double)row / dT, term = pr * log(pr);
        hz += term;
    }
    if (col > 0) {
        const double pc = (double)col / dT, term = pc * log(pc);
        hf += term;
    }
    acc = fn_wave_sum_f64(acc), hz = fn_wave_sum_f64(hz), hf = fn_wave_sum_f64(hf);
    if (lane == 0) o[0] = acc, o[1] = -hz, o[2] = -hf;
}

}  // namespace

extern "C" {

int fn_column_range(const float* x, int64_t ld, int N, int P, float* lo, float* hi, int32_t* status, void* stream) {
    const int rc = fn_dis_host::range_check(x, ld, N, P, lo, hi, status);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(range_init_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lo, hi, status, P);
    FN_CHECK_LAUNCH();
    const unsigned chunks = (unsigned)((N + FN_DIS_RANGE_CHUNK - 1) / FN_DIS_RANGE_CHUNK);
    hipLaunchKernelGGL(range_kernel, dim3((unsigned)((P + 63) / 64), chunks), dim3(64, 4), 0, (hipStream_t)stream, x, (long)ld, N, P, lo, hi, status);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_bin_columns(const float* x, int64_t ld, int N, int P, const float* lo, const float* hi, const int32_t* card_host, int bins, uint8_t* img,
                   int64_t n_pad, int32_t* status, void* stream) {
    const int rc = fn_dis_host::bin_check(x, ld, N, P, lo, hi, card_host, bins, img, n_pad, status);
    if (rc != FN_OK) return rc;
    CardArgs ca = {};
    if (card_host)
        for (int c = 0; c < P; ++c) ca.card[c] = card_host[c];
    hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)P), dim3(256), 0, (hipStream_t)stream, x, (long)ld, N, lo, hi, ca,
                       card_host ? 1 : 0, bins, img, (long)n_pad, status);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_joint_hist(const uint8_t* bz_img, int64_t ldz, int D, const uint8_t* bf_img, int64_t ldf, int A, int N, int32_t* counts, void* stream) {
    const int rc = fn_dis_host::hist_check(bz_img, ldz, D, bf_img, ldf, A, N, counts);
    if (rc != FN_OK) return rc;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)D * A * CELLS, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const unsigned chunks = (unsigned)((N + FN_DIS_HIST_CHUNK - 1) / FN_DIS_HIST_CHUNK);
    hipLaunchKernelGGL(hist_kernel, dim3(chunks, (unsigned)A, (unsigned)D), dim3(256), 0, (hipStream_t)stream, bz_img, (long)ldz, bf_img, (long)ldf, A, N,
                       counts);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_column_ranks(const float* x, int64_t ld, int N, int P, float* ranks, int64_t n_pad, void* stream) {
    const int rc = fn_dis_host::ranks_check(x, ld, N, P, ranks, n_pad);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(ranks_kernel, dim3((unsigned)((N + FN_DIS_RANK_ROWS - 1) / FN_DIS_RANK_ROWS), (unsigned)P), dim3(256), 0, (hipStream_t)stream, x,
                       (long)ld, N, ranks, (long)n_pad);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_column_corr(const float* X, int64_t x_rs, int64_t x_cs, int P, const float* Y, int64_t y_rs, int64_t y_cs, int Q, int N, double* mean_x,
                   double* ss_x, double* mean_y, double* ss_y, double* cross, void* stream) {
    const int rc = fn_dis_host::corr_check(X, x_rs, x_cs, P, Y, y_rs, y_cs, Q, N, mean_x, ss_x, mean_y, ss_y, cross);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(corr_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, (long)x_rs, (long)x_cs, P, Y, (long)y_rs,
                       (long)y_cs, Q, N, mean_x, ss_x, mean_y, ss_y, cross);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_mi_scores(const int32_t* counts, int pairs, double* out, int32_t* hits, void* stream) {
    const int rc = fn_dis_host::mi_check(counts, pairs, out, hits);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(mi_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, counts, pairs, out, hits);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
