// attributes.hip - controllability metrics behind the decode (attributes.py): rhythm density and note density of decoded event tokens
// (fn_event_attributes) and the consistency / restrictiveness / monotonicity of a fader sweep (fn_sweep_scores).  include/fadernets.h has the
// definition and says which part is the reference's (the piano-roll fill, the attributes, the scores) and which is ours (tokens -> timed notes).
// Plain HIP: no inline assembly, no hand-counted waits, no atomics, nothing between workgroups.
#include "events.h"

namespace {

// the parameters as the definition clamps them; with these clamps every product below fits 32 unsigned bits (t <= 1024 * 4096)
struct AttrView {
    int on_lo, off_lo, np, shift_lo, ns, eos, vocab;
    uint32_t num, den, bc;
};

__device__ __forceinline__ AttrView attr_view(const FnAttrParams* __restrict__ p) {
    AttrView c;
    c.on_lo = p->on_lo, c.off_lo = p->off_lo, c.shift_lo = p->shift_lo, c.eos = p->eos, c.vocab = p->vocab_size;
    c.np = min(max(p->n_pitch, 0), 128), c.ns = min(max(p->n_shift, 0), 4096);
    c.num = (uint32_t)min(max(p->ticks_num, 1), 32768), c.den = (uint32_t)min(max(p->ticks_den, 1), 256), c.bc = (uint32_t)min(max(p->beat_cells, 1), 64);
    return c;
}

// the fill of one kept note into the lane's own bit column (bit c of word w = cell 32 w + c; the words of a column are 128 apart)
__device__ __forceinline__ void attr_fill(uint32_t* col, const AttrView& c, uint32_t t0, uint32_t t1, int nc) {
    const int a = (int)((2u * c.den * t0 + c.num) / (2u * c.num));
    int b = (int)((c.den * t1) / c.num);
    if (a > 0 && a < nc) col[((a - 1) >> 5) * 128] &= ~(1u << ((a - 1) & 31));
    if (b < nc - 1 && ((col[(b >> 5) * 128] >> (b & 31)) & 1u)) b -= 1;
    const int hi = min(b, nc);
    if (hi <= a) return;
    const int w0 = a >> 5, w1 = (hi - 1) >> 5;
    for (int w = w0; w <= w1; ++w) {
        const int lo_bit = w == w0 ? (a & 31) : 0, hi_bit = w == w1 ? ((hi - 1) & 31) + 1 : 32;
        const uint32_t upto = hi_bit == 32 ? 0xffffffffu : (1u << hi_bit) - 1u;
        col[w * 128] |= upto & ~((1u << lo_bit) - 1u);
    }
}

// One fn_note_walk over the row.  FILL = false: only the largest t1 of a kept note (the first, cheap walk that gives n_cells); FILL = true: the notes
// go into the lane's bit columns as they close.
template <bool FILL>
__device__ __forceinline__ uint32_t attr_walk(const uint32_t* ev, int len, uint32_t t_end, int lane, const AttrView& c, uint32_t* bits, int nc) {
    uint32_t t_last = 0;
    fn_note_walk(ev, len, t_end, lane, [&](int p, uint32_t t0, uint32_t t1, int) {
        t_last = max(t_last, t1);
        if (FILL) attr_fill(bits + (p >> 6) * 64 + lane, c, t0, t1, nc);
    });
    return t_last;
}

extern __shared__ __attribute__((aligned(16))) char attr_smem[];

// One wavefront per row, one row per 64-thread workgroup.  LDS: ev[steps] (fn_event_scan's words: tick << 9 | code) and
// bits[ceil(cells_ld / 32)][128], a bit column per pitch over the cells.  n_cells is needed by the fill's guards, so phase 2 walks the events
// twice: a first walk that only finds t_last, then the walk that fills (the notes are not kept in between).
// Every lane reaches every barrier: no return before the end, and every ballot / shuffle sits in wave-uniform control flow.
__global__ __launch_bounds__(64) void event_raster_kernel(const int32_t* __restrict__ tokens, int tok_ld, int steps, const FnAttrParams* __restrict__ params,
                                                          int32_t* __restrict__ n_cells, int32_t* __restrict__ status, float* __restrict__ r_density,
                                                          float* __restrict__ n_density, int32_t* __restrict__ c_r, int32_t* __restrict__ c_n,
                                                          uint8_t* __restrict__ rhythm, uint8_t* __restrict__ notes, int cells_ld) {
    const int lane = threadIdx.x;
    const long r = blockIdx.x;
    const AttrView c = attr_view(params);
    uint32_t* ev = reinterpret_cast<uint32_t*>(attr_smem);
    uint32_t* bits = ev + steps;
    const int words = (cells_ld + 31) >> 5;
    const int32_t* row = tokens + r * tok_ld;

    // phase 1: the row's end, the clock of every token, the events into LDS
    uint32_t t_end;
    const int len = fn_event_scan<false>(row, steps, lane, c, ev, nullptr, t_end);
    for (int k = lane; k < words * 128; k += 64) bits[k] = 0u;          // lane l zeroes the columns of pitches l and l + 64: its own
    __syncthreads();

    // phase 2: t_last, n_cells, then the fill
    const uint32_t t_last = fn_wave_max_u32(attr_walk<false>(ev, len, t_end, lane, c, nullptr, 0));
    const uint32_t nc_u = t_last > 0u ? c.bc * ((t_last * c.den) / (c.num * c.bc) + 1u) : 0u;          // < 2^31
    const int nc = (int)nc_u;
    const bool fits = nc > 0 && nc <= cells_ld;
    if (fits) attr_walk<true>(ev, len, t_end, lane, c, bits, nc);
    __syncthreads();

    // phase 3: per cell the 128-bit set by two ballots; the per-cell bytes are collected 64 cells at a time in lane c & 63 and stored coalesced
    const int lim = fits ? nc : 0;
    int onsets = 0, total = 0;
    unsigned long long prev0 = 0ull, prev1 = 0ull;
    const int sweep = (rhythm || notes) ? cells_ld : lim;
    for (int base = 0; base < sweep; base += 64) {
        uint8_t my_r = 0, my_n = 0;
        for (int c0 = base; c0 < min(base + 64, lim); c0 += 32) {
            const uint32_t wa = bits[(c0 >> 5) * 128 + lane], wb = bits[(c0 >> 5) * 128 + 64 + lane];
            const int cnt = min(32, lim - c0);
            for (int j = 0; j < cnt; ++j) {
                const unsigned long long s0 = __ballot((wa >> j) & 1u), s1 = __ballot((wb >> j) & 1u);
                const int n = __popcll(s0) + __popcll(s1);
                const int rh = n == 0 ? 0 : (c0 + j == 0 || (s0 & ~prev0) != 0ull || (s1 & ~prev1) != 0ull) ? 1 : 2;
                onsets += rh == 1, total += n;
                prev0 = s0, prev1 = s1;
                if (lane == ((c0 + j) & 63)) my_r = (uint8_t)rh, my_n = (uint8_t)n;
            }
        }
        if (base + lane < cells_ld) {
            if (rhythm) rhythm[r * cells_ld + base + lane] = my_r;
            if (notes) notes[r * cells_ld + base + lane] = my_n;
        }
    }
    if (lane == 0) {
        n_cells[r] = nc;
        status[r] = nc == 0 ? FN_ATTR_EMPTY : fits ? 0 : FN_ATTR_OVERFLOW;
        if (fits) {
            r_density[r] = (float)((double)onsets / (double)nc), n_density[r] = (float)((double)total / (double)nc);
            c_r[r] = 10 * onsets < 3 * nc ? 0 : 2 * onsets < nc ? 1 : 2;
            c_n[r] = total <= 2 * nc ? 0 : 2 * total <= 7 * nc ? 1 : 2;
        } else {
            const float v = nc == 0 ? 0.f : __builtin_nanf("");
            r_density[r] = v, n_density[r] = v, c_r[r] = nc == 0 ? 0 : -1, c_n[r] = nc == 0 ? 0 : -1;
        }
    }
}

// sum over the Vn values, ascending from 0.0, the same in every lane (Vn is wave-uniform; lane v holds the term of value v)
__device__ __forceinline__ double attr_asc(double x, int Vn) {
    double acc = 0.0;
    for (int k = 0; k < Vn; ++k) acc += __shfl(x, k, 64);
    return acc;
}

// a[i] += a[i + h], h = 8, 4, 2, 1 over the 16 wavefronts' partial sums: part (one column per lane), sc (three per-sample sums), cnt (used samples)
__device__ __forceinline__ void attr_tree(double (*part)[64], double (*sc)[4], int* cnt, int wave, int lane) {
    __syncthreads();
    for (int h = 8; h > 0; h >>= 1) {
        if (wave < h) {
            part[wave][lane] += part[wave + h][lane];
            if (lane < 3) sc[wave][lane] += sc[wave + h][lane];
            if (lane == 3) cnt[wave] += cnt[wave + h];
        }
        __syncthreads();
    }
}

// One workgroup of 16 wavefronts; wavefront j takes the samples j, j + 16, ... in turn, lane v the fader value v.  The per-sample statistics are sums
// over the lanes (attr_asc), the per-value ones run down the samples in every lane's registers and meet in LDS (attr_tree).  Two passes over the
// samples: the column means, then the column variances.
__global__ __launch_bounds__(1024) void sweep_scores_kernel(const float* __restrict__ sw, const float* __restrict__ ot, const int32_t* __restrict__ status,
                                                            int S, int Vn, const double* __restrict__ values, double sw_std, double ot_std,
                                                            double* __restrict__ scores, int32_t* __restrict__ n_used) {
    __shared__ double part[16][64];
    __shared__ double sc[16][4];
    __shared__ int cnt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool act = lane < Vn;
    const double val = act ? values[lane] : 0.0;
    const double vbar = attr_asc(val, Vn) / Vn;
    const double dv = val - vbar;
    const double sxx = attr_asc(dv * dv, Vn);

    double colsum = 0.0, rs = 0.0, ms = 0.0, vs = 0.0;
    int used = 0;
    for (int s = wave; s < S; s += 16) {
        const int st = act ? status[(long)s * Vn + lane] : 0;
        if (__ballot(st != 0) != 0ull) continue;
        ++used;
        const double y = act ? (double)sw[(long)s * Vn + lane] : 0.0;
        const double o = act ? (double)ot[(long)s * Vn + lane] / ot_std : 0.0;
        const double x = y / sw_std;
        colsum += x;
        const double mo = attr_asc(o, Vn) / Vn, mx = attr_asc(x, Vn) / Vn, ybar = attr_asc(y, Vn) / Vn;
        rs += sqrt(attr_asc((o - mo) * (o - mo), Vn) / Vn);
        vs += sqrt(attr_asc((x - mx) * (x - mx), Vn) / Vn);
        const double dy = y - ybar;
        const double sxy = attr_asc(dv * dy, Vn), ss_tot = attr_asc(dy * dy, Vn);
        const double slope = sxx != 0.0 ? sxy / sxx : 0.0, icpt = ybar - slope * vbar;
        const double e = y - (icpt + slope * val);
        const double ss_res = attr_asc(e * e, Vn);
        ms += ss_tot == 0.0 ? 1.0 : 1.0 - ss_res / ss_tot;
    }
    part[wave][lane] = colsum;
    if (lane == 0) sc[wave][0] = rs, sc[wave][1] = ms, sc[wave][2] = vs, sc[wave][3] = 0.0, cnt[wave] = used;
    attr_tree(part, sc, cnt, wave, lane);
    const int nu = cnt[0];
    const double mean = part[0][lane] / nu, rs_all = sc[0][0], ms_all = sc[0][1], vs_all = sc[0][2];
    __syncthreads();

    double q = 0.0;
    for (int s = wave; s < S; s += 16) {
        const int st = act ? status[(long)s * Vn + lane] : 0;
        if (__ballot(st != 0) != 0ull) continue;
        const double d = (act ? (double)sw[(long)s * Vn + lane] / sw_std : 0.0) - mean;
        q += d * d;
    }
    part[wave][lane] = q;
    if (lane == 0) sc[wave][0] = 0.0, sc[wave][1] = 0.0, sc[wave][2] = 0.0, cnt[wave] = 0;
    attr_tree(part, sc, cnt, wave, lane);
    if (wave == 0) {
        const double col = attr_asc(sqrt(part[0][lane] / nu), Vn);
        if (lane == 0) {
            const double nan = __builtin_nan("");
            n_used[0] = nu;
            scores[0] = nu ? 1.0 - col / Vn : nan;
            scores[1] = nu ? 1.0 - rs_all / nu : nan;
            scores[2] = nu ? ms_all / nu : nan;
            scores[3] = nu ? vs_all / nu : nan;
        }
    }
}

}  // namespace

extern "C" {

int fn_event_attributes(const int32_t* tokens, int tok_ld, int rows, int steps, const FnAttrParams* params_dev, int32_t* n_cells, int32_t* status,
                        float* r_density, float* n_density, int32_t* c_r, int32_t* c_n, uint8_t* rhythm, uint8_t* notes, int cells_ld, void* stream) {
    if (!tokens || !params_dev || !n_cells || !status || !r_density || !n_density || !c_r || !c_n) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || cells_ld < 1 || cells_ld > FN_ATTR_MAX_CELLS || tok_ld < steps) return FN_E_SHAPE;
    const size_t lds = 4u * (size_t)steps + 512u * (size_t)((cells_ld + 31) / 32);          // <= 36 KB: below what a launch may ask for without an attribute
    hipLaunchKernelGGL(event_raster_kernel, dim3((unsigned)rows), dim3(64), lds, (hipStream_t)stream, tokens, tok_ld, steps, params_dev, n_cells, status,
                       r_density, n_density, c_r, c_n, rhythm, notes, cells_ld);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_sweep_scores(const float* r, const float* n, const int32_t* status, int S, int Vn, const double* values, int which, double r_std,
                    double n_std, double* scores, int32_t* n_used, void* stream) {
    if (!r || !n || !status || !values || !scores || !n_used) return FN_E_NULL;
    if (S < 1 || S > FN_ATTR_MAX_SAMPLES || Vn < 2 || Vn > 64 || which < 0 || which > 1) return FN_E_SHAPE;
    hipLaunchKernelGGL(sweep_scores_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, which == 0 ? r : n, which == 0 ? n : r, status, S, Vn, values,
                       which == 0 ? r_std : n_std, which == 0 ? n_std : r_std, scores, n_used);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
