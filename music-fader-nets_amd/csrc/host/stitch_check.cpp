// stitch_check.cpp - stand-alone driver of the host twin of fn_notes_stitch (notes_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined stitch_check.cpp -o stitch_check  &&  ./stitch_check in.bin out.bin
// in.bin : 8 int32 {S, V, dec_rs, dec_ld, n_total, out_ld, 0, 0}; then S*V*dec_rs*4 int32 decoded notes, S*V int32 dec_n, S*V int32 dec_end,
//          n_total*4 int32 source notes, S*4 int32 spans, S*V int32 modes.
// out.bin: int32 rc, then (rc == 0) V*out_ld*4 int32 notes, V*(S+1) int32 win_first, V int32 out_n, V int32 status.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "notes_host.h"

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
    static_assert(sizeof(FnNote) == 16 && sizeof(FnNoteSpan) == 16, "the sizes include/fadernets.h states");
    const int S = hd[0], V = hd[1], dec_rs = hd[2], dec_ld = hd[3], n_total = hd[4], out_ld = hd[5];
    const auto within = [](int v, int hi) { return v >= -1 && v <= hi; };          // -1 and 0 are let through: the twin answers them
    if (!(within(S, 1 << 17) && within(V, 1 << 7) && within(dec_rs, 1 << 12) && within(dec_ld, 1 << 12) && within(n_total, 1 << 20) && within(out_ld, 1 << 20)))
        return 2;
    const auto sz = [](int v) { return (size_t)(v > 0 ? v : 0); };
    const size_t rows = sz(S) * sz(V);
    if (rows > (1u << 20) || rows * sz(dec_rs) > (1u << 24) || sz(V) * sz(out_ld) > (1u << 24)) return 2;
    std::vector<FnNote> dec(rows * sz(dec_rs)), src(sz(n_total)), out(sz(V) * sz(out_ld), FnNote{-9, -9, -9, -9});
    std::vector<int32_t> dec_n(rows), dec_end(rows), mode(rows), win_first(sz(V) * (sz(S) + 1), -9), out_n(sz(V), -9), status(sz(V), -9);
    std::vector<FnNoteSpan> spans(sz(S));
    if (!get(f, dec) || !get(f, dec_n) || !get(f, dec_end) || !get(f, src) || !get(f, spans) || !get(f, mode)) return 2;
    std::fclose(f);
    alignas(16) static FnNote none[1] = {{0, 0, 0, 0}};                             // an empty vector's data() may be null: that is another answer
    static FnNoteSpan no_span[1] = {{0, 0, 0, 0}};
    static int32_t sink[4] = {0, 0, 0, 0};
    const int32_t rc = fn_notes_host::notes_stitch(dec.empty() ? none : dec.data(), dec_rs, dec_ld, rows ? dec_n.data() : sink, rows ? dec_end.data() : sink,
                                                   src.data(), n_total, spans.empty() ? no_span : spans.data(), S, V, rows ? mode.data() : sink,
                                                   out.empty() ? none : out.data(), out_ld, win_first.empty() ? sink : win_first.data(),
                                                   out_n.empty() ? sink : out_n.data(), status.empty() ? sink : status.data());
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, out), put(o, win_first), put(o, out_n), put(o, status);
    std::fclose(o);
    std::printf("fn_notes_stitch_host rc %d S %d V %d dec_ld %d n_total %d out_ld %d\n", (int)rc, S, V, dec_ld, n_total, out_ld);
    return 0;
}
