// constrain_check.cpp - stand-alone driver of the host twins of fn_constrain_apply / fn_constrain_advance (constrain_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined constrain_check.cpp -o constrain_check  &&  ./constrain_check in.bin out.bin
// in.bin : int32 {rows, V, ld, step, bias (0 none, 1 shared [V], 2 per row [rows][V]), held (0 / 1), fixup (0: advance without logits / 1), alias
//          (1: held_out is held_in)}, the 8 int32 words of FnConstrainParams, rows*ld floats of logits, the bias floats, rows*4 uint32 of held (when
//          given), rows int32 tokens, rows int32 fallback tokens.
// out.bin: int32 rc of the apply, then (rc == 0) rows*ld floats of logits and rows int32 stuck; int32 rc of the advance on those logits, then
//          (rc == 0) rows int32 tokens, rows*4 uint32 held_out (when held is given) and rows int32 fixed.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "constrain_host.h"

template <typename T>
static bool get(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static void put(std::FILE* f, const std::vector<T>& v) { std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    FnConstrainParams prm;
    static_assert(sizeof(FnConstrainParams) == 32, "FnConstrainParams is 32 bytes");
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8 || std::fread(&prm, sizeof(prm), 1, f) != 1) return 2;
    const int rows = hd[0], V = hd[1], ld = hd[2], step = hd[3], bias_mode = hd[4], has_held = hd[5], fixup = hd[6], alias = hd[7];
    if (!(rows > 0 && rows <= (1 << 16) && V >= 1 && V <= FN_SAMPLE_MAX_V && ld >= V && ld <= (1 << 16) && bias_mode >= 0 && bias_mode <= 2)) return 2;
    const size_t R = (size_t)rows;
    std::vector<float> x(R * ld), bias(bias_mode == 0 ? 0 : bias_mode == 1 ? (size_t)V : R * V);
    std::vector<uint32_t> held(has_held ? R * 4 : 0);
    std::vector<int32_t> tok(R), fb(R);
    if (!get(f, x) || !get(f, bias) || !get(f, held) || !get(f, tok) || !get(f, fb)) return 2;
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    std::vector<int32_t> stuck(R, 0), fixed(R, 0);
    int32_t rc = fn_constrain_host::constrain_apply(x.data(), rows, V, ld, step, &prm, bias_mode ? bias.data() : nullptr, bias_mode == 2 ? V : 0,
                                                    has_held ? held.data() : nullptr, stuck.data());
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, x), put(o, stuck);
    const int32_t rc_apply = rc;

    std::vector<uint32_t> held_out(has_held && !alias ? R * 4 : 0);
    uint32_t* ho = !has_held ? nullptr : alias ? held.data() : held_out.data();
    rc = fn_constrain_host::constrain_advance(tok.data(), 1, rows, V, &prm, fixup ? x.data() : nullptr, ld, fb.data(), 1, has_held ? held.data() : nullptr,
                                              ho, fixed.data());
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) {
        put(o, tok);
        if (has_held) put(o, alias ? held : held_out);
        put(o, fixed);
    }
    std::fclose(o);
    std::printf("fn_constrain_*_host rc %d %d rows %d V %d step %d\n", (int)rc_apply, (int)rc, rows, V, step);
    return 0;
}
