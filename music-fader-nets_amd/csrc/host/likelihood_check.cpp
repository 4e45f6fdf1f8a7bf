// likelihood_check.cpp - stand-alone driver of the host twins of fn_posterior_draw / fn_iw_reduce (likelihood_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined likelihood_check.cpp -o likelihood_check  &&  ./likelihood_check in.bin out.bin
// in.bin, draw: 10 int32 {0, n_jobs, B, S, Z, z_ld, col_step, flags, 0, 0} (job e writes at column e*col_step of ONE z buffer; flags 1: eps_out), the
//          32 bytes of FnDrawParams, then per job 2 int32 {K, stream_id}, B*2Z floats pre, K*Z floats mu_lk, K*Z floats lv_lk.
// out.bin, draw: int32 rc, then (rc == 0) the z buffer [(B*S-1)*z_ld + (n_jobs-1)*col_step + Z] (it starts as CANARY), per job eps [B*S][Z] (flag 1),
//          per job logq [B*S] doubles, per job logp [B*S] doubles.
// in.bin, reduce: 10 int32 {1, B, S, T, nll_ld, n_lat, lat_stride, out_ld, flags, 0} (flags 1: spans given), nll [(T-1)*nll_ld + B*S] floats, with
//          flag 1 t0 [B] and t1 [B] int32, logp and logq [(n_lat-1)*lat_stride + B*S] doubles each.
// out.bin, reduce: int32 rc, then (rc == 0) lw [B*S] doubles and out [(B-1)*out_ld + FN_IW_COLS + n_lat] doubles (both start as CANARY).
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "likelihood_host.h"

static const float CANARY = -777.25f;

template <typename T>
static bool get(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static void put(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}
static size_t sz(long v) { return (size_t)(v > 0 ? v : 0); }

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[10];
    if (std::fread(hd, sizeof(int32_t), 10, f) != 10) return 2;
    static_assert(sizeof(FnDrawParams) == 32 && sizeof(FnPostJob) == 64, "the sizes include/fadernets.h states");
    for (int k = 1; k < 10; ++k)
        if (hd[k] < -1 || hd[k] > (1 << 20)) return 2;          // -1 and 0 are let through: the twins answer them
    static float none[1] = {0.0f};                              // an empty vector's data() may be null: that is another answer
    static double none64[1] = {0.0};
    int32_t rc;
    std::FILE* o;
    if (hd[0] == 0) {
        const int n_jobs = hd[1], B = hd[2], S = hd[3], Z = hd[4], z_ld = hd[5], col_step = hd[6], flags = hd[7];
        const int nj = n_jobs < 0 ? 0 : (n_jobs > 8 ? 8 : n_jobs);
        const long rows = (long)sz(B) * (long)sz(S);
        if (sz(rows) * sz(z_ld) > (1u << 24)) return 2;
        std::vector<FnDrawParams> params(1);
        if (!get(f, params)) return 2;
        std::vector<float> z(rows > 0 ? sz((rows - 1) * z_ld + (long)(nj - 1) * col_step + Z) : 0, CANARY);
        std::vector<std::vector<float>> pre(nj), mu(nj), lv(nj), eps(nj);
        std::vector<std::vector<double>> logq(nj), logp(nj);
        std::vector<FnPostJob> jobs(nj ? nj : 1);
        for (int e = 0; e < nj; ++e) {
            std::vector<int32_t> ks(2);
            if (!get(f, ks) || ks[0] < -1 || ks[0] > (1 << 12)) return 2;
            pre[e].resize(sz(B) * 2 * sz(Z)), mu[e].resize(sz(ks[0]) * sz(Z)), lv[e].resize(sz(ks[0]) * sz(Z));
            if (!get(f, pre[e]) || !get(f, mu[e]) || !get(f, lv[e])) return 2;
            if (flags & 1) eps[e].assign(sz(rows) * sz(Z), CANARY);
            logq[e].assign(sz(rows), (double)CANARY), logp[e].assign(sz(rows), (double)CANARY);
            jobs[e] = FnPostJob{pre[e].empty() ? none : pre[e].data(), mu[e].empty() ? none : mu[e].data(), lv[e].empty() ? none : lv[e].data(),
                                (z.empty() ? none : z.data()) + (long)e * col_step, eps[e].empty() ? nullptr : eps[e].data(),
                                logq[e].empty() ? none64 : logq[e].data(), logp[e].empty() ? none64 : logp[e].data(), ks[0], ks[1]};
        }
        std::fclose(f);
        rc = fn_lik_host::posterior_draw(jobs.data(), n_jobs, B, S, Z, z_ld, params.data());
        if (!(o = std::fopen(argv[2], "wb"))) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) {
            put(o, z);
            for (int e = 0; e < nj; ++e) put(o, eps[e]);
            for (int e = 0; e < nj; ++e) put(o, logq[e]);
            for (int e = 0; e < nj; ++e) put(o, logp[e]);
        }
        std::printf("fn_posterior_draw_host rc %d n_jobs %d B %d S %d Z %d z_ld %d\n", (int)rc, n_jobs, B, S, Z, z_ld);
    } else if (hd[0] == 1) {
        const int B = hd[1], S = hd[2], T = hd[3], nll_ld = hd[4], n_lat = hd[5], lat_stride = hd[6], out_ld = hd[7], flags = hd[8];
        const long rows = (long)sz(B) * (long)sz(S);
        const int nl = n_lat < 0 ? 0 : (n_lat > 8 ? 8 : n_lat);
        if (sz(T) * sz(nll_ld) > (1u << 24) || sz(nl) * sz(lat_stride) > (1u << 24) || sz(B) * sz(out_ld) > (1u << 24)) return 2;
        std::vector<float> nll(T > 0 && rows > 0 ? sz((long)(T - 1) * nll_ld + rows) : 0);
        std::vector<int32_t> t0(flags & 1 ? sz(B) : 0), t1(t0.size());
        std::vector<double> lp(nl > 0 && rows > 0 ? sz((long)(nl - 1) * lat_stride + rows) : 0), lq(lp.size());
        if (!get(f, nll) || !get(f, t0) || !get(f, t1) || !get(f, lp) || !get(f, lq)) return 2;
        std::fclose(f);
        std::vector<double> lw(sz(rows), (double)CANARY), out(B > 0 ? sz((long)(B - 1) * out_ld + FN_IW_COLS + nl) : 0, (double)CANARY);
        rc = fn_lik_host::iw_reduce(nll.empty() ? none : nll.data(), T, nll_ld, t0.empty() ? nullptr : t0.data(), t1.empty() ? nullptr : t1.data(),
                                    lp.empty() ? none64 : lp.data(), lq.empty() ? none64 : lq.data(), n_lat, lat_stride, B, S, lw.empty() ? none64 : lw.data(),
                                    out.empty() ? none64 : out.data(), out_ld);
        if (!(o = std::fopen(argv[2], "wb"))) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, lw), put(o, out);
        std::printf("fn_iw_reduce_host rc %d B %d S %d T %d n_lat %d\n", (int)rc, B, S, T, n_lat);
    } else {
        return 2;
    }
    std::fclose(o);
    return 0;
}
