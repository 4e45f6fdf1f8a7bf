// attr_check.cpp - stand-alone driver of the host twins of fn_event_attributes / fn_sweep_scores (attr_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined attr_check.cpp -o attr_check  &&  ./attr_check in.bin out.bin
// in.bin : 8 int32; word 0 says which call.
//   0: {0, rows, steps, tok_ld, cells_ld, cells (1: rhythm and notes are wanted), 0, 0}, the 12 int32 words of FnAttrParams, rows*tok_ld int32 tokens.
//   1: {1, S, Vn, which, 0, 0, 0, 0}, doubles {r_std, n_std}, Vn doubles of values, S*Vn floats r, S*Vn floats n, S*Vn int32 status.
// out.bin: int32 rc, then (rc == 0)
//   0: rows int32 n_cells, status, rows floats r_density, n_density, rows int32 c_r, c_n, and when wanted rows*cells_ld bytes rhythm, then notes.
//   1: int32 n_used, 4 doubles.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "attr_host.h"

template <typename T>
static bool get(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static void put(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8) return 2;
    static_assert(sizeof(FnAttrParams) == 48, "FnAttrParams is 48 bytes");
    int32_t rc;
    if (hd[0] == 0) {
        const int rows = hd[1], steps = hd[2], tok_ld = hd[3], cells_ld = hd[4], cells = hd[5];
        FnAttrParams prm;
        if (std::fread(&prm, sizeof(prm), 1, f) != 1) return 2;
        if (!(rows > 0 && rows <= (1 << 16) && tok_ld > 0 && tok_ld <= (1 << 12) && cells_ld > 0 && cells_ld <= FN_ATTR_MAX_CELLS)) return 2;
        const size_t R = (size_t)rows;
        std::vector<int32_t> tok(R * tok_ld), n_cells(R, -9), status(R, -9), c_r(R, -9), c_n(R, -9);
        std::vector<float> rd(R, -9.f), nd(R, -9.f);
        std::vector<uint8_t> rhythm(cells ? R * cells_ld : 0, 0xA5), notes(cells ? R * cells_ld : 0, 0xA5);
        if (!get(f, tok)) return 2;
        std::fclose(f);
        rc = fn_attr_host::event_attributes(tok.data(), tok_ld, rows, steps, &prm, n_cells.data(), status.data(), rd.data(), nd.data(), c_r.data(),
                                            c_n.data(), cells ? rhythm.data() : nullptr, cells ? notes.data() : nullptr, cells_ld);
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, n_cells), put(o, status), put(o, rd), put(o, nd), put(o, c_r), put(o, c_n), put(o, rhythm), put(o, notes);
        std::fclose(o);
        std::printf("fn_event_attributes_host rc %d rows %d steps %d cells_ld %d\n", (int)rc, rows, steps, cells_ld);
    } else if (hd[0] == 1) {
        const int S = hd[1], Vn = hd[2], which = hd[3];
        if (!(S > 0 && S <= FN_ATTR_MAX_SAMPLES && Vn > 0 && Vn <= 64)) return 2;
        std::vector<double> stds(2), values((size_t)Vn), scores(4, -9.0);
        std::vector<float> r((size_t)S * Vn), n((size_t)S * Vn);
        std::vector<int32_t> status((size_t)S * Vn);
        if (!get(f, stds) || !get(f, values) || !get(f, r) || !get(f, n) || !get(f, status)) return 2;
        std::fclose(f);
        int32_t n_used = -9;
        rc = fn_attr_host::sweep_scores(r.data(), n.data(), status.data(), S, Vn, values.data(), which, stds[0], stds[1], scores.data(), &n_used);
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) std::fwrite(&n_used, sizeof(n_used), 1, o), put(o, scores);
        std::fclose(o);
        std::printf("fn_sweep_scores_host rc %d S %d Vn %d which %d\n", (int)rc, S, Vn, which);
    } else {
        return 2;
    }
    return 0;
}
