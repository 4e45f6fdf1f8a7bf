// beam_check.cpp - stand-alone driver of the host twins of fn_beam_step / fn_beam_gather / fn_beam_backtrack (beam_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined beam_check.cpp -o beam_check  &&  ./beam_check in.bin out.bin
// in.bin : int32 {B, W, V, ld, step, eos, cols, steps}, B*W*ld floats of logits, B*W floats score_prev, B*W int32 token_prev, B*W*cols floats of
//          state rows, then the slabs of the backtrack: steps*B*W int32 parent, steps*B*W int32 token, steps*B*W floats score.
// out.bin: int32 rc of the step, then (rc == 0) B*W floats score, B*W int32 parent, B*W int32 token, B*W*V floats of log-probs;
//          int32 rc of the gather by the step's parents, then (rc == 0) B*W*cols floats;
//          int32 rc of the backtrack, then (rc == 0) B*W*steps int32 tokens, B*W*steps int32 beams, B*W*steps floats cum, B*W int32 lengths,
//          B*W floats final scores.
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "beam_host.h"

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
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8) return 2;
    const int B = hd[0], W = hd[1], V = hd[2], ld = hd[3], step = hd[4], eos = hd[5], cols = hd[6], steps = hd[7];
    if (!(B > 0 && B <= (1 << 16) && W >= 1 && W <= FN_BEAM_MAX_W && V >= 1 && V <= FN_SAMPLE_MAX_V && ld >= V && ld <= (1 << 16) && cols >= 1 &&
          cols <= (1 << 12) && steps >= 1 && steps <= (1 << 12)))
        return 2;
    const size_t R = (size_t)B * W;
    std::vector<float> x(R * ld), sprev(R), src(R * cols), sc(steps * R);
    std::vector<int32_t> tprev(R), par(steps * R), tok(steps * R);
    if (!get(f, x) || !get(f, sprev) || !get(f, tprev) || !get(f, src) || !get(f, par) || !get(f, tok) || !get(f, sc)) return 2;
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    std::vector<float> score(R), lp(R * V);
    std::vector<int32_t> parent(R), token(R);
    int32_t rc = fn_beam_host::beam_step(x.data(), B, W, V, ld, step, eos, sprev.data(), tprev.data(), W, score.data(), parent.data(), token.data(), W,
                                         lp.data(), V);
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, score), put(o, parent), put(o, token), put(o, lp);
    const int32_t rc_step = rc;

    std::vector<float> dst(R * cols);
    const FnBeamGatherJob job = {src.data(), cols, dst.data(), cols, cols};
    rc = rc_step == 0 ? fn_beam_host::beam_gather(&job, 1, (int)R, W, parent.data()) : rc_step;
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, dst);

    std::vector<int32_t> tokens_out(R * steps), beam_out(R * steps), len_out(R);
    std::vector<float> cum_out(R * steps), score_out(R);
    rc = fn_beam_host::beam_backtrack(par.data(), tok.data(), sc.data(), steps, B, W, eos, tokens_out.data(), beam_out.data(), cum_out.data(),
                                      len_out.data(), score_out.data());
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, tokens_out), put(o, beam_out), put(o, cum_out), put(o, len_out), put(o, score_out);
    std::fclose(o);
    std::printf("fn_beam_*_host rc %d B %d W %d V %d step %d eos %d\n", (int)rc_step, B, W, V, step, eos);
    return 0;
}
