// attr_host.h - fn_event_attributes / fn_sweep_scores in plain C++ (include/fadernets.h has the definition these follow clause by clause, not the
// kernels).  No dependencies: the stand-alone attr_check.cpp includes it.  Integers, one fp64 division rounded to fp32 per density, fp64 scores.
#ifndef FADERNETS_ATTR_HOST_H
#define FADERNETS_ATTR_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../../include/fadernets.h"

namespace fn_attr_host {

struct Note {
    int pitch;
    int64_t t0, t1;
};

inline int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

// offset of token e in the range of n tokens that starts at lo, or -1
inline int in_range(int e, int lo, int n) {
    const int64_t d = (int64_t)e - (int64_t)lo;
    return (d >= 0 && d < n) ? (int)d : -1;
}

inline int event_attributes(const int32_t* tokens, int tok_ld, int rows, int steps, const FnAttrParams* params, int32_t* n_cells, int32_t* status,
                            float* r_density, float* n_density, int32_t* c_r, int32_t* c_n, uint8_t* rhythm, uint8_t* notes, int cells_ld) {
    if (!tokens || !params || !n_cells || !status || !r_density || !n_density || !c_r || !c_n) return FN_E_NULL;
    if (rows < 1 || steps < 1 || steps > FN_ATTR_MAX_STEPS || cells_ld < 1 || cells_ld > FN_ATTR_MAX_CELLS || tok_ld < steps) return FN_E_SHAPE;
    const FnAttrParams c = *params;
    const int np = clampi(c.n_pitch, 0, 128), ns = clampi(c.n_shift, 0, 4096), bc = clampi(c.beat_cells, 1, 64);
    const int64_t num = clampi(c.ticks_num, 1, 32768), den = clampi(c.ticks_den, 1, 256);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t r = 0; r < rows; ++r) {
        const int32_t* row = tokens + r * tok_ld;
        // tokens -> notes
        std::vector<Note> kept;
        std::vector<int64_t> open(128, -1);
        int64_t t = 0;
        auto close = [&](int p) {
            if (t > open[p]) kept.push_back(Note{p, open[p], t});
            open[p] = -1;
        };
        for (int i = 0; i < steps; ++i) {
            const int e = row[i];
            if (c.eos >= 0 && e == c.eos) break;
            if (c.vocab_size > 0 && (e < 0 || e >= c.vocab_size)) continue;
            int p;
            if ((p = in_range(e, c.on_lo, np)) >= 0) {
                if (open[p] >= 0) close(p);
                open[p] = t;
            } else if ((p = in_range(e, c.off_lo, np)) >= 0) {
                if (open[p] >= 0) close(p);
            } else if ((p = in_range(e, c.shift_lo, ns)) >= 0) {
                t += p + 1;
            }
        }
        for (int p = 0; p < 128; ++p)
            if (open[p] >= 0) close(p);
        if (rhythm) std::fill(rhythm + r * cells_ld, rhythm + (r + 1) * cells_ld, (uint8_t)0);
        if (notes) std::fill(notes + r * cells_ld, notes + (r + 1) * cells_ld, (uint8_t)0);
        if (kept.empty()) {
            n_cells[r] = 0, status[r] = FN_ATTR_EMPTY, r_density[r] = 0.f, n_density[r] = 0.f, c_r[r] = 0, c_n[r] = 0;
            continue;
        }
        // notes -> grid
        int64_t t_last = 0;
        for (const Note& k : kept) t_last = std::max(t_last, k.t1);
        const int64_t nc = bc * ((t_last * den) / (num * bc) + 1);
        n_cells[r] = (int32_t)nc;
        if (nc > cells_ld) {
            status[r] = FN_ATTR_OVERFLOW, r_density[r] = nan, n_density[r] = nan, c_r[r] = -1, c_n[r] = -1;
            continue;
        }
        std::vector<uint8_t> grid((size_t)nc * 128, 0);
        for (const Note& k : kept) {
            const int64_t a = (2 * den * k.t0 + num) / (2 * num);
            int64_t b = (den * k.t1) / num;
            if (a > 0 && a < nc && grid[(size_t)(a - 1) * 128 + k.pitch]) grid[(size_t)(a - 1) * 128 + k.pitch] = 0;
            if (b < nc - 1 && grid[(size_t)b * 128 + k.pitch]) b -= 1;
            for (int64_t x = a; x < std::min(b, nc); ++x) grid[(size_t)x * 128 + k.pitch] = 1;
        }
        // grid -> attributes
        int64_t onsets = 0, total = 0;
        for (int64_t x = 0; x < nc; ++x) {
            int count = 0;
            bool subset = true;
            for (int p = 0; p < 128; ++p) {
                if (!grid[(size_t)x * 128 + p]) continue;
                ++count;
                if (x == 0 || !grid[(size_t)(x - 1) * 128 + p]) subset = false;
            }
            const int rh = count == 0 ? 0 : (x == 0 || !subset) ? 1 : 2;
            onsets += rh == 1, total += count;
            if (rhythm) rhythm[r * cells_ld + x] = (uint8_t)rh;
            if (notes) notes[r * cells_ld + x] = (uint8_t)count;
        }
        status[r] = 0;
        r_density[r] = (float)((double)onsets / (double)nc), n_density[r] = (float)((double)total / (double)nc);
        c_r[r] = 10 * onsets < 3 * nc ? 0 : 2 * onsets < nc ? 1 : 2;
        c_n[r] = total <= 2 * nc ? 0 : 2 * total <= 7 * nc ? 1 : 2;
    }
    return FN_OK;
}

// the definition's sum over samples: 16 partial sums, then a[i] += a[i + h]
struct SampleSum {
    double a[16] = {0};
    void add(int s, double x) { a[s % 16] += x; }
    double total() {
        for (int h = 8; h > 0; h /= 2)
            for (int i = 0; i < h; ++i) a[i] += a[i + h];
        return a[0];
    }
};

inline int sweep_scores(const float* r, const float* n, const int32_t* status, int S, int Vn, const double* values, int which, double r_std, double n_std,
                        double* scores, int32_t* n_used) {
    if (!r || !n || !status || !values || !scores || !n_used) return FN_E_NULL;
    if (S < 1 || S > FN_ATTR_MAX_SAMPLES || Vn < 2 || Vn > 64 || which < 0 || which > 1) return FN_E_SHAPE;
    const float* sw = which == 0 ? r : n;
    const float* ot = which == 0 ? n : r;
    const double sw_std = which == 0 ? r_std : n_std, ot_std = which == 0 ? n_std : r_std;
    std::vector<int> used;
    for (int s = 0; s < S; ++s) {
        bool ok = true;
        for (int v = 0; v < Vn; ++v) ok = ok && status[(size_t)s * Vn + v] == 0;
        if (ok) used.push_back(s);
    }
    *n_used = (int32_t)used.size();
    if (used.empty()) {
        for (int k = 0; k < 4; ++k) scores[k] = std::numeric_limits<double>::quiet_NaN();
        return FN_OK;
    }
    const double nu = (double)used.size();
    auto pstd = [&](const float* row, double scale) {
        double m = 0.0, q = 0.0;
        for (int v = 0; v < Vn; ++v) m += (double)row[v] / scale;
        m /= Vn;
        for (int v = 0; v < Vn; ++v) q += ((double)row[v] / scale - m) * ((double)row[v] / scale - m);
        return std::sqrt(q / Vn);
    };
    double vbar = 0.0, sxx = 0.0;
    for (int v = 0; v < Vn; ++v) vbar += values[v];
    vbar /= Vn;
    for (int v = 0; v < Vn; ++v) sxx += (values[v] - vbar) * (values[v] - vbar);
    SampleSum restrict_sum, mono_sum, var_sum;
    for (int s : used) {
        const float* y = sw + (size_t)s * Vn;
        restrict_sum.add(s, pstd(ot + (size_t)s * Vn, ot_std));
        var_sum.add(s, pstd(y, sw_std));
        double ybar = 0.0, sxy = 0.0, ss_tot = 0.0, ss_res = 0.0;
        for (int v = 0; v < Vn; ++v) ybar += (double)y[v];
        ybar /= Vn;
        for (int v = 0; v < Vn; ++v) sxy += (values[v] - vbar) * ((double)y[v] - ybar);
        for (int v = 0; v < Vn; ++v) ss_tot += ((double)y[v] - ybar) * ((double)y[v] - ybar);
        const double slope = sxx != 0.0 ? sxy / sxx : 0.0, icpt = ybar - slope * vbar;
        for (int v = 0; v < Vn; ++v) {
            const double e = (double)y[v] - (icpt + slope * values[v]);
            ss_res += e * e;
        }
        mono_sum.add(s, ss_tot == 0.0 ? 1.0 : 1.0 - ss_res / ss_tot);
    }
    double col = 0.0;
    for (int v = 0; v < Vn; ++v) {
        SampleSum m, q;
        for (int s : used) m.add(s, (double)sw[(size_t)s * Vn + v] / sw_std);
        const double mean = m.total() / nu;
        for (int s : used) {
            const double d = (double)sw[(size_t)s * Vn + v] / sw_std - mean;
            q.add(s, d * d);
        }
        col += std::sqrt(q.total() / nu);
    }
    scores[0] = 1.0 - col / Vn;
    scores[1] = 1.0 - restrict_sum.total() / nu;
    scores[2] = mono_sum.total() / nu;
    scores[3] = var_sum.total() / nu;
    return FN_OK;
}

}  // namespace fn_attr_host

#endif
