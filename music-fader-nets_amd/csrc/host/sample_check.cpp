// sample_check.cpp - stand-alone driver of the host twin of fn_vocab_sample (sample_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined sample_check.cpp -o sample_check  &&  ./sample_check in.bin out.bin
// in.bin : int32 {B, V, ld, step}, the 32 bytes of FnSampleParams, then B*ld floats of logits.
// out.bin: int32 rc, then (rc == 0) B int32 tokens, B int32 first-index argmaxes, B floats u, B*V floats of log-probs.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sample_host.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[4];
    FnSampleParams p;
    static_assert(sizeof(FnSampleParams) == 32, "FnSampleParams is 32 bytes");
    if (std::fread(hd, sizeof(int32_t), 4, f) != 4 || std::fread(&p, sizeof(p), 1, f) != 1) return 2;
    const int B = hd[0], V = hd[1], ld = hd[2], step = hd[3];
    const bool sane = B > 0 && B <= (1 << 20) && V >= 1 && V <= FN_SAMPLE_MAX_V && ld >= V && ld <= (1 << 16);
    std::vector<float> x(sane ? (size_t)B * ld : 1);
    if (sane && std::fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 2;
    std::fclose(f);
    std::vector<int32_t> tok(sane ? (size_t)B : 1), own(sane ? (size_t)B : 1);
    std::vector<float> u(sane ? (size_t)B : 1), lp(sane ? (size_t)B * V : 1);
    const int32_t rc = fn_sample_host::vocab_sample(x.data(), B, V, ld, &p, step, lp.data(), V, own.data(), 1, tok.data(), 1, u.data());
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) {
        std::fwrite(tok.data(), sizeof(int32_t), tok.size(), o);
        std::fwrite(own.data(), sizeof(int32_t), own.size(), o);
        std::fwrite(u.data(), sizeof(float), u.size(), o);
        std::fwrite(lp.data(), sizeof(float), lp.size(), o);
    }
    std::fclose(o);
    std::printf("fn_vocab_sample_host rc %d B %d V %d step %d\n", (int)rc, B, V, step);
    return 0;
}
