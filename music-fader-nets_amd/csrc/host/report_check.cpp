// report_check.cpp - stand-alone driver of the host twins of fn_token_score / fn_match_rows (report_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined report_check.cpp -o report_check  &&  ./report_check in.bin out.bin
// in.bin : 16 int32; word 0 says which call.
//   0: {0, B, T, V, stride_b, stride_t, n_x, tgt_ld, out_ld, flags (1: target, 2: pred, 4: nll, 8: rank)}, n_x floats x, with a target B*tgt_ld int32.
//   1: {1, rows, T, trim, pred_ld, tgt_ld, aux_ld, topk, flags (1: nll, 2: rank)}, rows*pred_ld int32 pred, rows*tgt_ld int32 target, with nll
//      rows*aux_ld floats, with rank rows*aux_ld int32.
// out.bin: int32 rc, then (rc == 0)
//   0: of the wanted ones B*out_ld int32 pred, floats nll, int32 rank; the columns behind T keep the sentinel -9.
//   1: rows int32 lead, len, correct, (with rank) correct_topk, status, rows doubles acc, (with nll) rows doubles nll_sum.
// Every buffer has exactly the size the call may touch (n_x = the last row's last valid float + 1), so an access past an end is the sanitizer's
// to report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "report_host.h"

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
    int32_t hd[16];
    if (std::fread(hd, sizeof(int32_t), 16, f) != 16) return 2;
    int32_t rc;
    if (hd[0] == 0) {
        const int B = hd[1], T = hd[2], V = hd[3], stride_b = hd[4], stride_t = hd[5], n_x = hd[6], tgt_ld = hd[7], out_ld = hd[8], flags = hd[9];
        if (!(B >= 0 && B <= (1 << 12) && n_x > 0 && n_x <= (1 << 26) && tgt_ld >= 0 && tgt_ld <= (1 << 12) && out_ld >= 0 && out_ld <= (1 << 12))) return 2;
        const size_t N = (size_t)B * out_ld;
        std::vector<float> x((size_t)n_x), nll(flags & 4 ? N : 0, -9.f);
        std::vector<int32_t> target(flags & 1 ? (size_t)B * tgt_ld : 0), pred(flags & 2 ? N : 0, -9), rank(flags & 8 ? N : 0, -9);
        if (!get(f, x) || !get(f, target)) return 2;
        std::fclose(f);
        rc = fn_report_host::token_score(x.data(), stride_b, stride_t, B, T, V, flags & 1 ? target.data() : nullptr, tgt_ld, flags & 2 ? pred.data() : nullptr,
                                         flags & 4 ? nll.data() : nullptr, flags & 8 ? rank.data() : nullptr, out_ld);
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, pred), put(o, nll), put(o, rank);
        std::fclose(o);
        std::printf("fn_token_score_host rc %d B %d T %d V %d\n", (int)rc, B, T, V);
    } else if (hd[0] == 1) {
        const int rows = hd[1], T = hd[2], trim = hd[3], pred_ld = hd[4], tgt_ld = hd[5], aux_ld = hd[6], topk = hd[7], flags = hd[8];
        if (!(rows >= 0 && rows <= (1 << 12) && pred_ld >= 0 && pred_ld <= (1 << 12) && tgt_ld >= 0 && tgt_ld <= (1 << 12) && aux_ld >= 0 && aux_ld <= (1 << 12)))
            return 2;
        const size_t R = (size_t)rows;
        std::vector<int32_t> pred(R * pred_ld), target(R * tgt_ld), rank(flags & 2 ? R * aux_ld : 0);
        std::vector<float> nll(flags & 1 ? R * aux_ld : 0);
        if (!get(f, pred) || !get(f, target) || !get(f, nll) || !get(f, rank)) return 2;
        std::fclose(f);
        std::vector<int32_t> lead(R, -9), len(R, -9), correct(R, -9), correct_topk(flags & 2 ? R : 0, -9), status(R, -9);
        std::vector<double> acc(R, -9.0), nll_sum(flags & 1 ? R : 0, -9.0);
        rc = fn_report_host::match_rows(pred.data(), pred_ld, target.data(), tgt_ld, rows, T, trim, flags & 1 ? nll.data() : nullptr,
                                        flags & 2 ? rank.data() : nullptr, aux_ld, topk, lead.data(), len.data(), correct.data(),
                                        flags & 2 ? correct_topk.data() : nullptr, acc.data(), flags & 1 ? nll_sum.data() : nullptr, status.data());
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, lead), put(o, len), put(o, correct), put(o, correct_topk), put(o, status), put(o, acc), put(o, nll_sum);
        std::fclose(o);
        std::printf("fn_match_rows_host rc %d rows %d T %d trim %d\n", (int)rc, rows, T, trim);
    } else {
        return 2;
    }
    return 0;
}
