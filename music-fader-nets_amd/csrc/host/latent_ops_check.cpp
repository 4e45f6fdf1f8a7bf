// latent_ops_check.cpp - stand-alone driver of the host twins of fn_latent_draw / fn_latent_mix (latent_ops_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined latent_ops_check.cpp -o latent_ops_check  &&  ./latent_ops_check in.bin out.bin
// in.bin, draw: 8 int32 {0, n_jobs, rows, Z, z_ld, col_step, flags, 0} (job s writes at column s*col_step of ONE z buffer; flags 1: comp given,
//          2: eps_out, 4: comp_out), the 32 bytes of FnDrawParams, then per job 2 int32 {K, stream_id}, K*Z floats mu_lk, K*Z floats lv_lk and,
//          with flag 1, rows int32 comp.
// out.bin, draw: int32 rc, then (rc == 0) the z buffer [(rows-1)*z_ld + (n_jobs-1)*col_step + Z] (it starts as CANARY), per job eps [rows][Z] (flag 2),
//          per job comp_out [rows] (flag 4).
// in.bin, mix: 8 int32 {1, pairs, D, ab_ld, P, t_per_pair, n_segs, out_ld}, n_segs*4 int32 segments, a and b [(pairs-1)*ab_ld + D] floats,
//          t [P or pairs*P] floats.
// out.bin, mix: int32 rc, then (rc == 0) out [(pairs*P-1)*out_ld + D] floats (it starts as CANARY), omega [pairs][n_segs] floats.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "latent_ops_host.h"

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
    int32_t hd[8];
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8) return 2;
    static_assert(sizeof(FnDrawParams) == 32 && sizeof(FnMixSeg) == 16, "the sizes include/fadernets.h states");
    for (int k = 1; k < 8; ++k)
        if (hd[k] < -1 || hd[k] > (1 << 20)) return 2;          // -1 and 0 are let through: the twins answer them
    static float none[1] = {0.0f};                              // an empty vector's data() may be null: that is another answer
    int32_t rc;
    std::FILE* o;
    if (hd[0] == 0) {
        const int n_jobs = hd[1], rows = hd[2], Z = hd[3], z_ld = hd[4], col_step = hd[5], flags = hd[6];
        const int nj = n_jobs < 0 ? 0 : (n_jobs > 8 ? 8 : n_jobs);
        if (sz(rows) * sz(z_ld) > (1u << 24)) return 2;
        std::vector<FnDrawParams> params(1);
        if (!get(f, params)) return 2;
        std::vector<float> z(rows > 0 ? sz((long)(rows - 1) * z_ld + (long)(nj - 1) * col_step + Z) : 0, CANARY);
        std::vector<std::vector<float>> mu(nj), lv(nj), eps(nj);
        std::vector<std::vector<int32_t>> comp(nj), comp_out(nj);
        std::vector<FnDrawJob> jobs(nj ? nj : 1);
        for (int s = 0; s < nj; ++s) {
            std::vector<int32_t> ks(2);
            if (!get(f, ks) || ks[0] < -1 || ks[0] > (1 << 12)) return 2;
            mu[s].resize(sz(ks[0]) * sz(Z)), lv[s].resize(sz(ks[0]) * sz(Z));
            if (!get(f, mu[s]) || !get(f, lv[s])) return 2;
            if (flags & 1) comp[s].resize(sz(rows));
            if (!get(f, comp[s])) return 2;
            if (flags & 2) eps[s].assign(sz(rows) * sz(Z), CANARY);
            if (flags & 4) comp_out[s].assign(sz(rows), -9);
            jobs[s] = FnDrawJob{mu[s].empty() ? none : mu[s].data(), lv[s].empty() ? none : lv[s].data(), comp[s].empty() ? nullptr : comp[s].data(),
                                (z.empty() ? none : z.data()) + (long)s * col_step, eps[s].empty() ? nullptr : eps[s].data(),
                                comp_out[s].empty() ? nullptr : comp_out[s].data(), ks[0], ks[1]};
        }
        std::fclose(f);
        rc = fn_latent_host::latent_draw(jobs.data(), n_jobs, rows, Z, z_ld, params.data());
        if (!(o = std::fopen(argv[2], "wb"))) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) {
            put(o, z);
            for (int s = 0; s < nj; ++s) put(o, eps[s]);
            for (int s = 0; s < nj; ++s) put(o, comp_out[s]);
        }
        std::printf("fn_latent_draw_host rc %d n_jobs %d rows %d Z %d z_ld %d\n", (int)rc, n_jobs, rows, Z, z_ld);
    } else if (hd[0] == 1) {
        const int pairs = hd[1], D = hd[2], ab_ld = hd[3], P = hd[4], t_per_pair = hd[5], n_segs = hd[6], out_ld = hd[7];
        if (sz(pairs) * sz(ab_ld) > (1u << 24) || sz(pairs) * sz(P) * sz(out_ld) > (1u << 24)) return 2;
        std::vector<FnMixSeg> segs(sz(n_segs > 8 ? 8 : n_segs));
        std::vector<float> a(pairs > 0 ? sz((long)(pairs - 1) * ab_ld + D) : 0), b(a.size()), t(sz(t_per_pair ? (long)pairs * P : P));
        if (!get(f, segs) || !get(f, a) || !get(f, b) || !get(f, t)) return 2;
        std::fclose(f);
        std::vector<float> out(pairs > 0 && P > 0 ? sz(((long)pairs * P - 1) * out_ld + D) : 0, CANARY), omega(sz(pairs) * segs.size(), CANARY);
        static FnMixSeg no_seg[1] = {{0, 0, 0, 0}};
        rc = fn_latent_host::latent_mix(a.empty() ? none : a.data(), b.empty() ? none : b.data(), ab_ld, pairs, D, t.empty() ? none : t.data(), P, t_per_pair,
                                        segs.empty() ? no_seg : segs.data(), n_segs, out.empty() ? none : out.data(), out_ld,
                                        omega.empty() ? nullptr : omega.data());
        if (!(o = std::fopen(argv[2], "wb"))) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, out), put(o, omega);
        std::printf("fn_latent_mix_host rc %d pairs %d D %d P %d n_segs %d\n", (int)rc, pairs, D, P, n_segs);
    } else {
        return 2;
    }
    std::fclose(o);
    return 0;
}
