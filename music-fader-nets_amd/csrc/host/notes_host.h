// notes_host.h - fn_notes_from_tokens / fn_tokens_from_notes / fn_notes_stitch in plain C++ (include/fadernets.h has the definition these follow clause
// by clause, not the kernels).  No dependencies: the stand-alone notes_check.cpp and stitch_check.cpp include it.  Integers only.
#ifndef FADERNETS_NOTES_HOST_H
#define FADERNETS_NOTES_HOST_H

#include <algorithm>
#include <cstdint>
#include <tuple>
#include <vector>

#include "../../../include/fadernets.h"

namespace fn_notes_host {

inline int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

// offset of token e in the range of n tokens that starts at lo, or -1
inline int in_range(int e, int lo, int n) {
    const int64_t d = (int64_t)e - (int64_t)lo;
    return (d >= 0 && d < n) ? (int)d : -1;
}

struct Velocity {
    int nv, vstep;
    explicit Velocity(int n_vel) : nv(clampi(n_vel, 0, 128)), vstep(nv > 0 ? (127 + nv - 1) / nv : 1) {}
    int of_bin(int k) const { return std::min(1 + k * vstep, 127); }
    int bin_of(int v) const { return std::min((v - 1) / vstep, nv - 1); }
};

inline int notes_from_tokens(const int32_t* tokens, int tok_ld, int rows, int steps, const FnNoteParams* params, FnNote* notes, int notes_ld,
                             int32_t* n_notes, int32_t* t_end, int32_t* status) {
    if (!tokens || !params || !notes || !n_notes || !t_end || !status) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || tok_ld < steps || notes_ld < 1) return FN_E_SHAPE;
    const FnNoteParams c = *params;
    const int np = clampi(c.n_pitch, 0, 128), ns = clampi(c.n_shift, 0, 4096);
    const Velocity vel(c.n_vel);
    for (int64_t r = 0; r < rows; ++r) {
        const int32_t* row = tokens + r * tok_ld;
        std::vector<FnNote> kept;
        std::vector<int64_t> open(128, -1);
        std::vector<int> open_vel(128, 0);
        int64_t t = 0;
        int cur = clampi(c.default_vel, 1, 127);
        auto close = [&](int p) {
            if (t > open[p]) kept.push_back(FnNote{(int32_t)open[p], (int32_t)t, p, open_vel[p]});
            open[p] = -1;
        };
        for (int i = 0; i < steps; ++i) {
            const int e = row[i];
            if (c.eos >= 0 && e == c.eos) break;
            if (c.vocab_size > 0 && (e < 0 || e >= c.vocab_size)) continue;
            int p;
            if ((p = in_range(e, c.on_lo, np)) >= 0) {
                if (open[p] >= 0) close(p);
                open[p] = t, open_vel[p] = cur;
            } else if ((p = in_range(e, c.off_lo, np)) >= 0) {
                if (open[p] >= 0) close(p);
            } else if ((p = in_range(e, c.shift_lo, ns)) >= 0) {
                t += p + 1;
            } else if ((p = in_range(e, c.vel_lo, vel.nv)) >= 0) {
                cur = vel.of_bin(p);
            }
        }
        for (int p = 0; p < 128; ++p)
            if (open[p] >= 0) close(p);
        std::sort(kept.begin(), kept.end(), [](const FnNote& a, const FnNote& b) { return std::make_pair(a.t0, a.pitch) < std::make_pair(b.t0, b.pitch); });
        const int64_t n = (int64_t)kept.size();
        FnNote* out = notes + r * notes_ld;
        for (int64_t j = 0; j < notes_ld; ++j) out[j] = j < n ? kept[(size_t)j] : FnNote{0, 0, 0, 0};
        n_notes[r] = (int32_t)n, t_end[r] = (int32_t)t;
        status[r] = n == 0 ? FN_NOTES_EMPTY : n > notes_ld ? FN_NOTES_OVERFLOW : 0;
    }
    return FN_OK;
}

inline int tokens_from_notes(const FnNote* notes, int n_total, const FnNoteSpan* spans, int rows, const FnNoteParams* params, int32_t* tokens, int tok_ld,
                             int steps, int32_t* n_tokens, int32_t* n_kept, int32_t* status) {
    if (!spans || !params || !tokens || !n_tokens || !n_kept || !status || (!notes && n_total > 0)) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || tok_ld < steps || n_total < 0) return FN_E_SHAPE;
    const FnNoteParams c = *params;
    const int np = clampi(c.n_pitch, 0, 128), ns = clampi(c.n_shift, 0, 4096);
    const Velocity vel(c.n_vel);
    for (int64_t r = 0; r < rows; ++r) {
        const FnNoteSpan sp = spans[r];
        const int count = clampi(sp.count, 0, FN_NOTES_MAX);                                                  // 1
        const int64_t t_lo = sp.t_lo, t_hi = std::min(std::max((int64_t)sp.t_hi, t_lo), t_lo + FN_NOTES_MAX_TICK);  // 2
        std::vector<std::tuple<int64_t, int, int, int>> events;                                               // (tick, 0 OFF / 1 ON, pitch, k)
        std::vector<int> bin((size_t)count, 0);
        int kept = 0;
        for (int k = 0; k < count; ++k) {
            const int64_t at = (int64_t)sp.first + k;
            if (at < 0 || at >= n_total) continue;
            const FnNote q = notes[at];
            const int64_t t1 = std::min((int64_t)q.t1, t_hi);
            if (!(q.pitch >= 0 && q.pitch < np && q.t0 >= t_lo && q.t0 < t_hi && t1 > q.t0)) continue;       // 3
            events.emplace_back(q.t0 - t_lo, 1, q.pitch, k), events.emplace_back(t1 - t_lo, 0, q.pitch, k);  // 4
            if (vel.nv > 0) bin[(size_t)k] = vel.bin_of(clampi(q.vel, 1, 127));
            ++kept;
        }
        std::sort(events.begin(), events.end());                                                              // 5
        std::vector<int32_t> stream;                                                                          // the first `steps` tokens
        int64_t length = 0, clock = 0;
        int cur = -1;
        auto emit = [&](int32_t e) {
            if (length < steps) stream.push_back(e);
            ++length;
        };
        for (const auto& [tick, kind, pitch, k] : events) {                                                   // 6
            const int64_t g = tick - clock;
            clock = tick;
            if (ns > 0) {
                const int64_t full = g / ns;
                length += full;
                for (int64_t f = 0; f < full && (int64_t)stream.size() < steps; ++f) stream.push_back(c.shift_lo + ns - 1);
                if (g % ns) emit(c.shift_lo + (int32_t)(g % ns) - 1);
            }
            if (kind == 1 && vel.nv > 0 && bin[(size_t)k] != cur) cur = bin[(size_t)k], emit(c.vel_lo + cur);
            emit((kind == 1 ? c.on_lo : c.off_lo) + pitch);
        }
        if (c.add_eos != 0 && c.eos >= 0) emit(c.eos);
        int32_t* row = tokens + r * tok_ld;
        for (int i = 0; i < steps; ++i) row[i] = i < (int)stream.size() ? stream[(size_t)i] : c.pad;          // 7
        n_tokens[r] = (int32_t)length, n_kept[r] = kept;
        status[r] = length > steps ? FN_NOTES_OVERFLOW : kept == 0 ? FN_NOTES_EMPTY : 0;                      // 8
    }
    return FN_OK;
}

// floor(a / b) for b > 0
inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

inline int notes_stitch(const FnNote* dec, int dec_rs, int dec_ld, const int32_t* dec_n, const int32_t* dec_end, const FnNote* src, int n_total,
                        const FnNoteSpan* spans, int S, int V, const int32_t* mode, FnNote* out, int out_ld, int32_t* win_first, int32_t* out_n,
                        int32_t* status) {
    if (!dec || !dec_n || !dec_end || !spans || !mode || !out || !win_first || !out_n || !status || (!src && n_total > 0)) return FN_E_NULL;
    if (S < 1 || V < 1 || dec_ld < 1 || dec_rs < dec_ld || out_ld < 1 || n_total < 0) return FN_E_SHAPE;
    if (((uintptr_t)dec | (uintptr_t)src | (uintptr_t)out) & 15u) return FN_E_ALIGN;
    if (S > FN_STITCH_MAX_S || V > FN_STITCH_MAX_V || out_ld > FN_STITCH_MAX_OUT || (int64_t)S * std::max(n_total, dec_ld) > INT32_MAX)
        return FN_E_UNSUPPORTED;
    for (int v = 0; v < V; ++v) {
        std::vector<FnNote> piece;
        int32_t* first_of = win_first + (int64_t)v * (S + 1);
        for (int j = 0; j < S; ++j) {
            first_of[j] = (int32_t)piece.size();                                                              // 8
            const FnNoteSpan sp = spans[j];
            const int64_t row = (int64_t)j * V + v, t_lo = sp.t_lo;
            const int64_t W = std::min<int64_t>(std::max<int64_t>((int64_t)sp.t_hi - t_lo, 0), FN_NOTES_MAX_TICK);   // 1
            auto put = [&](int64_t t0, int64_t t1, int pitch, int vel) {                                      // 6
                if (t1 <= t0 || pitch < 0 || pitch >= 128 || t0 < INT32_MIN || t0 > INT32_MAX || t1 < INT32_MIN || t1 > INT32_MAX) return;
                piece.push_back(FnNote{(int32_t)t0, (int32_t)t1, pitch, clampi(vel, 1, 127)});
            };
            if (mode[row] == 0) {                                                                             // 2
                for (int64_t k = std::max<int64_t>(0, -(int64_t)sp.first); k < sp.count; ++k) {          // the k before are in front of the array
                    const int64_t at = (int64_t)sp.first + k;
                    if (at >= n_total) break;
                    const FnNote q = src[at];
                    if (q.t0 >= t_lo && q.t0 < t_lo + W) put(q.t0, q.t1, q.pitch, q.vel);
                }
            } else if (mode[row] == 1 || mode[row] == 2) {                                                    // 3, 4
                const int n = clampi(dec_n[row], 0, dec_ld);
                const int64_t end = dec_end[row];
                for (int k = 0; k < n; ++k) {
                    const FnNote q = dec[row * dec_rs + k];
                    int64_t t0 = q.t0, t1 = q.t1;
                    if (mode[row] == 2 && end > W) t0 = floor_div(t0 * W, end), t1 = std::max(t0 + 1, floor_div(t1 * W, end));
                    if (t0 >= 0 && t0 < W) put(t_lo + t0, t_lo + std::min(t1, W), q.pitch, q.vel);
                }
            }                                                                                                 // 5: nothing
        }
        const int64_t total = (int64_t)piece.size();
        first_of[S] = (int32_t)total;
        FnNote* row_out = out + (int64_t)v * out_ld;
        for (int64_t i = 0; i < out_ld; ++i) row_out[i] = i < total ? piece[(size_t)i] : FnNote{0, 0, 0, 0};
        out_n[v] = (int32_t)std::min<int64_t>(total, out_ld);
        status[v] = total > out_ld ? FN_NOTES_OVERFLOW : total == 0 ? FN_NOTES_EMPTY : 0;
    }
    return FN_OK;
}

}  // namespace fn_notes_host

#endif
