// notes_check.cpp - stand-alone driver of the host twins of fn_notes_from_tokens / fn_tokens_from_notes (notes_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined notes_check.cpp -o notes_check  &&  ./notes_check in.bin out.bin
// in.bin : 8 int32; word 0 says which call; then the 16 int32 words of FnNoteParams.
//   0: {0, rows, steps, tok_ld, notes_ld, 0, 0, 0}, params, rows*tok_ld int32 tokens.
//   1: {1, rows, steps, tok_ld, n_total, 0, 0, 0}, params, n_total*4 int32 notes, rows*4 int32 spans.
// out.bin: int32 rc, then (rc == 0)
//   0: rows*notes_ld*4 int32 notes, rows int32 n_notes, t_end, status.
//   1: rows*tok_ld int32 tokens (columns behind `steps` keep the value -9 they start with), rows int32 n_tokens, n_kept, status.
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
    static_assert(sizeof(FnNoteParams) == 64 && sizeof(FnNote) == 16 && sizeof(FnNoteSpan) == 16, "the sizes include/fadernets.h states");
    FnNoteParams prm;
    if (std::fread(&prm, sizeof(prm), 1, f) != 1) return 2;
    const int rows = hd[1], steps = hd[2], tok_ld = hd[3];
    if (!(rows >= 0 && rows <= (1 << 16) && tok_ld >= 0 && tok_ld <= (1 << 12))) return 2;
    const size_t R = (size_t)rows;
    int32_t rc;
    if (hd[0] == 0) {
        const int notes_ld = hd[4];
        if (!(notes_ld >= 0 && notes_ld <= (1 << 12))) return 2;
        std::vector<int32_t> tok(R * tok_ld), n_notes(R, -9), t_end(R, -9), status(R, -9);
        std::vector<FnNote> notes(R * notes_ld, FnNote{-9, -9, -9, -9});
        if (!get(f, tok)) return 2;
        std::fclose(f);
        rc = fn_notes_host::notes_from_tokens(tok.data(), tok_ld, rows, steps, &prm, notes.data(), notes_ld, n_notes.data(), t_end.data(), status.data());
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, notes), put(o, n_notes), put(o, t_end), put(o, status);
        std::fclose(o);
        std::printf("fn_notes_from_tokens_host rc %d rows %d steps %d notes_ld %d\n", (int)rc, rows, steps, notes_ld);
    } else if (hd[0] == 1) {
        const int n_total = hd[4];
        if (!(n_total >= -1 && n_total <= (1 << 20))) return 2;
        std::vector<FnNote> notes((size_t)std::max(n_total, 0));
        std::vector<FnNoteSpan> spans(R);
        std::vector<int32_t> tok(R * tok_ld, -9), n_tokens(R, -9), n_kept(R, -9), status(R, -9);
        if (!get(f, notes) || !get(f, spans)) return 2;
        std::fclose(f);
        rc = fn_notes_host::tokens_from_notes(notes.data(), n_total, spans.data(), rows, &prm, tok.data(), tok_ld, steps, n_tokens.data(), n_kept.data(),
                                              status.data());
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(&rc, sizeof(rc), 1, o);
        if (rc == 0) put(o, tok), put(o, n_tokens), put(o, n_kept), put(o, status);
        std::fclose(o);
        std::printf("fn_tokens_from_notes_host rc %d rows %d steps %d n_total %d\n", (int)rc, rows, steps, n_total);
    } else {
        return 2;
    }
    return 0;
}
