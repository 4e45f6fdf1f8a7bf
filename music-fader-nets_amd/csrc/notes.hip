// notes.hip - event tokens <-> timed notes (notes.py, midi.py): fn_notes_from_tokens publishes the notes that event_raster_kernel (attributes.hip)
// keeps in registers, with velocity; fn_tokens_from_notes is the tokeniser; fn_notes_stitch joins decoded windows into pieces (transfer.py).
// include/fadernets.h has the definitions.
// Plain HIP: no inline assembly, no atomics, nothing between workgroups; one wavefront per row, every lane reaches every barrier.
#include "events.h"

namespace {

struct NoteView {
    int on_lo, off_lo, np, shift_lo, ns, eos, vocab, vel_lo, nv, vstep, def_vel, pad, add_eos;
};

__device__ __forceinline__ NoteView note_view(const FnNoteParams* __restrict__ p) {
    NoteView c;
    c.on_lo = p->on_lo, c.off_lo = p->off_lo, c.shift_lo = p->shift_lo, c.eos = p->eos, c.vocab = p->vocab_size, c.vel_lo = p->vel_lo;
    c.np = min(max(p->n_pitch, 0), 128), c.ns = min(max(p->n_shift, 0), 4096), c.nv = min(max(p->n_vel, 0), 128);
    c.vstep = c.nv > 0 ? (127 + c.nv - 1) / c.nv : 1;
    c.def_vel = min(max(p->default_vel, 1), 127), c.pad = p->pad, c.add_eos = p->add_eos;
    return c;
}

// Ascending bitonic sort of n 64-bit keys in LDS by one wavefront; n a power of two (1: nothing to do).  Pair t of a pass is (lo, lo + stride) with
// bit `stride` of lo clear; the direction of a pair is bit `size` of lo.  A barrier in front of every pass and one behind the last.
__device__ __forceinline__ void lds_bitonic_sort(unsigned long long* k, int n, int lane) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = lane; t < (n >> 1); t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == ((lo & size) == 0)) k[lo] = b, k[hi] = a;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

extern __shared__ __attribute__((aligned(16))) char note_smem[];

constexpr unsigned long long NOTE_NO_KEY = ~0ull;

// LDS: key[P] (t0 << 17 | pitch << 10 | index of the note-on token; NOTE_NO_KEY where the token opens no kept note), P = the power of two >= steps;
// ev[steps] and vel[steps], the velocity current at every token (phase 1: fn_event_scan with the velocity track, as event_raster_kernel runs it
// without); t1[steps] by note-on token.  Phase 2: fn_note_walk; a note that closes goes to the slot of its note-on token, which no other note has.
// Phase 3: sort the keys; rank j of the order is note j.
__global__ __launch_bounds__(64) void notes_from_tokens_kernel(const int32_t* __restrict__ tokens, int tok_ld, int steps, const FnNoteParams* __restrict__ params,
                                                               FnNote* __restrict__ notes, int notes_ld, int32_t* __restrict__ n_notes,
                                                               int32_t* __restrict__ t_end_out, int32_t* __restrict__ status) {
    const int lane = threadIdx.x;
    const long r = blockIdx.x;
    const NoteView c = note_view(params);
    const int P = pow2_at_least(steps);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(note_smem);
    uint32_t* ev = reinterpret_cast<uint32_t*>(key + P);
    uint32_t* t1s = ev + steps;
    uint8_t* vel = reinterpret_cast<uint8_t*>(t1s + steps);
    const int32_t* row = tokens + r * tok_ld;

    // phase 1
    uint32_t t_end;
    const int len = fn_event_scan<true>(row, steps, lane, c, ev, vel, t_end);
    for (int k = lane; k < P; k += 64) key[k] = NOTE_NO_KEY;
    __syncthreads();

    // phase 2
    int mine = 0;
    fn_note_walk(ev, len, t_end, lane, [&](int p, uint32_t t0, uint32_t t1, int at) {
        key[at] = ((unsigned long long)t0 << 17) | ((unsigned long long)p << 10) | (unsigned long long)at;
        t1s[at] = t1, ++mine;
    });
    mine = fn_wave_sum_i32(mine);
    const int n = mine;                                 // <= len

    // phase 3
    lds_bitonic_sort(key, P, lane);
    FnNote* out = notes + r * notes_ld;
    for (int j = lane; j < notes_ld; j += 64) {
        FnNote q = {0, 0, 0, 0};
        if (j < n) {
            const unsigned long long k = key[j];
            const int at = (int)(k & 1023ull);
            q.t0 = (int32_t)(k >> 17), q.t1 = (int32_t)t1s[at], q.pitch = (int32_t)((k >> 10) & 127ull), q.vel = (int32_t)vel[at];
        }
        out[j] = q;
    }
    if (lane == 0) n_notes[r] = n, t_end_out[r] = (int32_t)t_end, status[r] = n == 0 ? FN_NOTES_EMPTY : n > notes_ld ? FN_NOTES_OVERFLOW : 0;
}

// LDS: key[1024] (tick << 18 | kind << 17 | pitch << 10 | k; kind 0 = OFF, 1 = ON; NOTE_NO_KEY for no event), bin[512] by k.
// Phase 1: lane l takes the span's notes k = l, l + 64, ...: the kept ones leave their two events in slots 2k, 2k + 1.  Phase 2: the sort.
// Phase 3, 64 events of the order at a time: the gap to the event before, the bin of the ON before (a carry-forward scan), the count of
// tokens (a sum scan), then every lane writes its own event's tokens as far as they lie in front of `steps`.
__global__ __launch_bounds__(64) void tokens_from_notes_kernel(const FnNote* __restrict__ notes, int n_total, const FnNoteSpan* __restrict__ spans,
                                                               const FnNoteParams* __restrict__ params, int32_t* __restrict__ tokens, int tok_ld, int steps,
                                                               int32_t* __restrict__ n_tokens, int32_t* __restrict__ n_kept, int32_t* __restrict__ status) {
    __shared__ unsigned long long key[2 * FN_NOTES_MAX];
    __shared__ uint8_t bin[FN_NOTES_MAX];
    const int lane = threadIdx.x;
    const long r = blockIdx.x;
    const NoteView c = note_view(params);
    const FnNoteSpan sp = spans[r];
    const int count = min(max(sp.count, 0), FN_NOTES_MAX);
    const long t_lo = sp.t_lo, t_hi = min(max((long)sp.t_hi, t_lo), t_lo + FN_NOTES_MAX_TICK);
    const int P = pow2_at_least(2 * count);             // count 0: 1, nothing to sort

    // phase 1
    int kept = 0;
    for (int k = lane; k < (P >> 1); k += 64) {
        unsigned long long on = NOTE_NO_KEY, off = NOTE_NO_KEY;
        const long at = (long)sp.first + k;
        if (k < count && at >= 0 && at < n_total) {
            const FnNote q = notes[at];
            const long t1 = min((long)q.t1, t_hi);
            if (q.pitch >= 0 && q.pitch < c.np && q.t0 >= t_lo && q.t0 < t_hi && t1 > q.t0) {
                const unsigned long long low = ((unsigned long long)q.pitch << 10) | (unsigned long long)k;
                on = ((unsigned long long)(q.t0 - t_lo) << 18) | (1ull << 17) | low;
                off = ((unsigned long long)(t1 - t_lo) << 18) | low;
                bin[k] = c.nv > 0 ? (uint8_t)min((min(max(q.vel, 1), 127) - 1) / c.vstep, c.nv - 1) : (uint8_t)0;
                ++kept;
            }
        }
        key[2 * k] = on, key[2 * k + 1] = off;          // 2k + 1 < P
    }
    kept = fn_wave_sum_i32(kept);

    // phase 2
    lds_bitonic_sort(key, P, lane);

    // phase 3
    const int n_ev = 2 * kept;                          // the events are the first n_ev keys of the order
    int32_t* row = tokens + r * tok_ld;
    const uint32_t ns = (uint32_t)c.ns;
    uint32_t total = 0, prev_bin = 0;                   // prev_bin: 1 + the bin of the last ON so far; 0: none
    for (int base = 0; base < n_ev; base += 64) {
        const int j = base + lane;
        const bool live = j < n_ev;
        const unsigned long long k = live ? key[j] : 0ull;
        const uint32_t tick = (uint32_t)(k >> 18), before = (live && j > 0) ? (uint32_t)(key[j - 1] >> 18) : 0u;
        const bool is_on = live && ((k >> 17) & 1ull);
        const int pitch = (int)((k >> 10) & 127ull);
        const uint32_t g = tick - before;
        const uint32_t full = ns ? g / ns : 0u, rest = ns ? g % ns : 0u;
        const uint32_t b = (is_on && c.nv > 0) ? 1u + (uint32_t)bin[k & 1023ull] : 0u;
        uint32_t last = fn_wave_scan_last(b, lane);     // the last non-zero b at or before the lane ...
        if (last == 0u) last = prev_bin;
        uint32_t seen = __shfl_up(last, 1, 64);         // ... and before it
        if (lane == 0) seen = prev_bin;
        prev_bin = __shfl(last, 63, 64);
        const bool vel_tok = b != 0u && b != seen;
        const uint32_t cnt = live ? full + (rest ? 1u : 0u) + (vel_tok ? 1u : 0u) + 1u : 0u;
        const uint32_t x = fn_wave_scan_add(cnt, lane);
        const uint32_t start = total + x - cnt;         // < 2^23: the gaps of a row sum to at most FN_NOTES_MAX_TICK
        total += __shfl(x, 63, 64);
        if (live) {
            const uint32_t lim = (uint32_t)steps;
            for (uint32_t q = start, stop = min(start + full, lim); q < stop; ++q) row[q] = c.shift_lo + c.ns - 1;
            uint32_t q = start + full;
            if (rest) {
                if (q < lim) row[q] = c.shift_lo + (int)rest - 1;
                ++q;
            }
            if (vel_tok) {
                if (q < lim) row[q] = c.vel_lo + (int)b - 1;
                ++q;
            }
            if (q < lim) row[q] = (is_on ? c.on_lo : c.off_lo) + pitch;
        }
    }
    if (c.add_eos != 0 && c.eos >= 0) {
        if (lane == 0 && total < (uint32_t)steps) row[total] = c.eos;
        total += 1u;
    }
    for (uint32_t q = min(total, (uint32_t)steps) + lane; q < (uint32_t)steps; q += 64) row[q] = c.pad;
    if (lane == 0) n_tokens[r] = (int32_t)total, n_kept[r] = kept, status[r] = total > (uint32_t)steps ? FN_NOTES_OVERFLOW : kept == 0 ? FN_NOTES_EMPTY : 0;
}

// floor(a / b) for b > 0
__device__ __forceinline__ long floor_div(long a, long b) {
    const long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// One window of one piece as fn_notes_stitch walks it: where its notes come from, how many there are, and what clauses 1 to 6 make of note k.
// Everything that steers an address is clamped here: `n` notes starting at `base`, all inside src [n_total] or inside the dec_ld slots of the row.
struct StitchWindow {
    const FnNote* base;
    long t_lo, W, end;          // end: dec_end where mode 2 fits the times, 0 where it does not
    int n, mode;
};

__device__ __forceinline__ StitchWindow stitch_window(const FnNote* __restrict__ dec, int dec_rs, int dec_ld, const int32_t* __restrict__ dec_n,
                                                      const int32_t* __restrict__ dec_end, const FnNote* __restrict__ src, int n_total,
                                                      const FnNoteSpan* __restrict__ spans, const int32_t* __restrict__ mode, long j, long row) {
    const FnNoteSpan sp = spans[j];
    StitchWindow w;
    w.t_lo = sp.t_lo, w.W = min(max((long)sp.t_hi - (long)sp.t_lo, 0l), (long)FN_NOTES_MAX_TICK);
    w.mode = mode[row], w.end = 0, w.n = 0, w.base = src;
    if (w.mode == 0) {
        const long lo = max(0l, -(long)sp.first), hi = min((long)sp.count, (long)n_total - (long)sp.first);          // the k with first + k in [0, n_total)
        if (hi > lo) w.n = (int)(hi - lo), w.base = src + ((long)sp.first + lo);
    } else if (w.mode == 1 || w.mode == 2) {
        w.n = min(max(dec_n[row], 0), dec_ld), w.base = dec + row * dec_rs;
        const long e = dec_end[row];
        if (w.mode == 2 && e > w.W) w.end = e;
    }
    return w;
}

// note k < w.n of the window -> is it kept, and as what
__device__ __forceinline__ bool stitch_note(const StitchWindow& w, long k, int4& q) {
    q = *reinterpret_cast<const int4*>(w.base + k);          // (t0, t1, pitch, vel)
    long t0 = q.x, t1 = q.y;
    if (w.mode == 0) {
        if (!(t0 >= w.t_lo && t0 < w.t_lo + w.W)) return false;
    } else {
        if (w.end > 0) t0 = floor_div(t0 * w.W, w.end), t1 = max(t0 + 1, floor_div(t1 * w.W, w.end));
        if (!(t0 >= 0 && t0 < w.W)) return false;
        t0 += w.t_lo, t1 = w.t_lo + min(t1, w.W);
    }
    if (t1 <= t0 || q.z < 0 || q.z >= 128 || t0 < INT32_MIN || t1 > INT32_MAX) return false;          // t0 < t1: the two bounds cover both times
    q.x = (int)t0, q.y = (int)t1, q.w = min(max(q.w, 1), 127);
    return true;
}

// One wavefront per (window j, piece v), 64 notes of the window at a time.  WRITE false: the count of kept notes goes to win_first[v][j].
// WRITE true (after stitch_scan_kernel): the kept notes go to out[v] from win_first[v][j] on, in input order - a lane's place is the number of kept
// notes in the lanes below it - and the window zeroes its share of [total, out_ld): element total + 64 * j + lane and every 64 * S-th behind it.
template <bool WRITE>
__global__ __launch_bounds__(64) void stitch_walk_kernel(const FnNote* __restrict__ dec, int dec_rs, int dec_ld, const int32_t* __restrict__ dec_n,
                                                         const int32_t* __restrict__ dec_end, const FnNote* __restrict__ src, int n_total,
                                                         const FnNoteSpan* __restrict__ spans, int S, int V, const int32_t* __restrict__ mode,
                                                         FnNote* __restrict__ out, int out_ld, int32_t* __restrict__ win_first) {
    const int lane = threadIdx.x;
    const long j = blockIdx.x, v = blockIdx.y;
    const StitchWindow w = stitch_window(dec, dec_rs, dec_ld, dec_n, dec_end, src, n_total, spans, mode, j, j * V + v);
    int32_t* counts = win_first + v * ((long)S + 1);
    FnNote* piece = out + v * (long)out_ld;
    long at = WRITE ? counts[j] : 0;                    // < 2^31: the entry point refuses sizes at which a count could leave int32
    for (long base = 0; base < w.n; base += 64) {          // long: n reaches 2^31 - 1 when S is 1
        const long k = base + lane;
        int4 q = make_int4(0, 0, 0, 0);
        const bool keep = k < w.n && stitch_note(w, k, q);
        const unsigned long long m = __ballot(keep);
        if (WRITE && keep) {
            const long pos = at + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < out_ld) *reinterpret_cast<int4*>(piece + pos) = q;
        }
        at += __popcll(m);
    }
    if (WRITE) {
        for (long i = (long)counts[S] + 64 * j + lane; i < out_ld; i += 64l * S) *reinterpret_cast<int4*>(piece + i) = make_int4(0, 0, 0, 0);
    } else if (lane == 0) {
        counts[j] = (int32_t)at;
    }
}

constexpr int STITCH_SCAN_PASS = 256;                   // windows per pass of stitch_scan_kernel: 4 per lane

// One wavefront per piece: win_first[v][0 .. S) from counts to the counts in front (an exclusive scan, in place: a lane reads and writes its own four
// entries of a pass), win_first[v][S] the total; out_n and status of the piece.
__global__ __launch_bounds__(64) void stitch_scan_kernel(int32_t* __restrict__ win_first, int S, int out_ld, int32_t* __restrict__ out_n,
                                                         int32_t* __restrict__ status) {
    const int lane = threadIdx.x;
    const long v = blockIdx.x;
    int32_t* row = win_first + v * ((long)S + 1);
    int carry = 0;
    for (int base = 0; base < S; base += STITCH_SCAN_PASS) {
        const int i0 = base + 4 * lane;
        int c[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = i0 + q < S ? row[i0 + q] : 0, sum += c[q];
        const int x = fn_wave_scan_add(sum, lane);
        int before = carry + x - sum;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (i0 + q < S) row[i0 + q] = before;
            before += c[q];
        }
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) row[S] = carry, out_n[v] = min(carry, out_ld), status[v] = carry > out_ld ? FN_NOTES_OVERFLOW : carry == 0 ? FN_NOTES_EMPTY : 0;
}

}  // namespace

extern "C" {

int fn_notes_from_tokens(const int32_t* tokens, int tok_ld, int rows, int steps, const FnNoteParams* params_dev, FnNote* notes, int notes_ld,
                         int32_t* n_notes, int32_t* t_end, int32_t* status, void* stream) {
    if (!tokens || !params_dev || !notes || !n_notes || !t_end || !status) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || tok_ld < steps || notes_ld < 1) return FN_E_SHAPE;
    size_t P = 1;
    while (P < (size_t)steps) P <<= 1;
    const size_t lds = 8u * P + 9u * (size_t)steps;          // <= 17 KB: below what a launch may ask for without an attribute
    hipLaunchKernelGGL(notes_from_tokens_kernel, dim3((unsigned)rows), dim3(64), lds, (hipStream_t)stream, tokens, tok_ld, steps, params_dev, notes,
                       notes_ld, n_notes, t_end, status);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_tokens_from_notes(const FnNote* notes, int n_total, const FnNoteSpan* spans, int rows, const FnNoteParams* params_dev, int32_t* tokens,
                         int tok_ld, int steps, int32_t* n_tokens, int32_t* n_kept, int32_t* status, void* stream) {
    if (!spans || !params_dev || !tokens || !n_tokens || !n_kept || !status || (!notes && n_total > 0)) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || tok_ld < steps || n_total < 0) return FN_E_SHAPE;
    hipLaunchKernelGGL(tokens_from_notes_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, notes, n_total, spans, params_dev, tokens,
                       tok_ld, steps, n_tokens, n_kept, status);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_notes_stitch(const FnNote* dec, int dec_rs, int dec_ld, const int32_t* dec_n, const int32_t* dec_end, const FnNote* src, int n_total,
                    const FnNoteSpan* spans, int S, int V, const int32_t* mode, FnNote* out, int out_ld, int32_t* win_first, int32_t* out_n,
                    int32_t* status, void* stream) {
    if (!dec || !dec_n || !dec_end || !spans || !mode || !out || !win_first || !out_n || !status || (!src && n_total > 0)) return FN_E_NULL;
    if (S < 1 || V < 1 || dec_ld < 1 || dec_rs < dec_ld || out_ld < 1 || n_total < 0) return FN_E_SHAPE;
    if (((uintptr_t)dec | (uintptr_t)src | (uintptr_t)out) & 15u) return FN_E_ALIGN;
    if (S > FN_STITCH_MAX_S || V > FN_STITCH_MAX_V || out_ld > FN_STITCH_MAX_OUT || (int64_t)S * (n_total > dec_ld ? n_total : dec_ld) > INT32_MAX)
        return FN_E_UNSUPPORTED;
    const dim3 grid((unsigned)S, (unsigned)V);
    hipLaunchKernelGGL(stitch_walk_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, dec, dec_rs, dec_ld, dec_n, dec_end, src, n_total, spans, S, V,
                       mode, out, out_ld, win_first);
    FN_CHECK_LAUNCH();
    hipLaunchKernelGGL(stitch_scan_kernel, dim3((unsigned)V), dim3(64), 0, (hipStream_t)stream, win_first, S, out_ld, out_n, status);
    FN_CHECK_LAUNCH();
    hipLaunchKernelGGL(stitch_walk_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, dec, dec_rs, dec_ld, dec_n, dec_end, src, n_total, spans, S, V,
                       mode, out, out_ld, win_first);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
