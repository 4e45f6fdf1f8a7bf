"""Test-side restatement of fn_notes_stitch (include/fadernets.h; notes.stitch_notes, transfer.py), from the clauses and not from the kernels:

  stitch_of        statement 1: plain Python, lists that are appended to
  stitch_of_np     statement 2: numpy, boolean masks per window and a cumsum for win_first
  stitch_ref       either statement over a case, in the shapes the entry point writes
  stitch_cases     the case list the statements, the host twin and the kernels are held to
  transfer_ref     what transfer_piece must return for the tokens and `used` it reports
  hand_midi, check_transfer   the hand piece of the transfer tests and the checks both the CPU and the GPU test make on a result
  stitch_fake_ops  helpers_notes.notes_fake_ops() + fn_notes_stitch as statement 2: transfer_piece on the CPU

Every check is an exact integer comparison."""
import numpy as np
import torch

import helpers_notes as hn

MAX_TICK, EMPTY, OVERFLOW = hn.MAX_TICK, hn.EMPTY, hn.OVERFLOW
PASS, CLIP, FIT = 0, 1, 2
SCAN_PASS = 256                 # the windows one pass of the scan launch takes (STITCH_SCAN_PASS in csrc/notes.hip)
MAX_S, MAX_V, MAX_OUT = 1 << 16, 64, 1 << 24          # FN_STITCH_MAX_S, FN_STITCH_MAX_V, FN_STITCH_MAX_OUT
I32_MIN, I32_MAX = -2**31, 2**31 - 1
SENTINEL = (5, 50, 60, 100)     # a note every window of the cases would keep: a slot behind dec_n that is read changes the result
KEYS = ("notes", "n_notes", "win_first", "status")


def _finish(pieces, firsts, out_ld):
    V = len(pieces)
    notes = np.zeros((V, out_ld, 4), np.int32)
    for v, p in enumerate(pieces):
        n = min(len(p), out_ld)
        if n:
            notes[v, :n] = np.array(p[:n], dtype=np.int64).reshape(-1, 4)
    total = np.array([len(p) for p in pieces], dtype=np.int64)
    status = np.where(total > out_ld, OVERFLOW, np.where(total == 0, EMPTY, 0)).astype(np.int32)
    return dict(notes=notes, n_notes=np.minimum(total, out_ld).astype(np.int32), win_first=np.array(firsts, dtype=np.int32).reshape(V, -1), status=status)


def stitch_of(dec, dec_ld, dec_n, dec_end, src, spans, V, mode, out_ld):
    """statement 1.  dec (S*V, >= dec_ld, 4), row = j*V + v; dec_n, dec_end, mode (S*V,); src (n_total, 4); spans (S, 4)"""
    S, n_total = len(spans), len(src)
    pieces, firsts = [], []
    for v in range(V):
        piece, first_of = [], []
        for j in range(S):
            first_of.append(len(piece))
            first, count, t_lo, t_hi = (int(x) for x in spans[j])
            W = min(max(t_hi - t_lo, 0), MAX_TICK)                                                          # 1
            row = j * V + v
            m = int(mode[row])
            cand = []
            if m == PASS:                                                                                   # 2
                for k in range(max(0, -first), max(0, min(count, n_total - first))):
                    t0, t1, pitch, vel = (int(x) for x in src[first + k])
                    if t_lo <= t0 < t_lo + W:
                        cand.append((t0, t1, pitch, vel))
            elif m in (CLIP, FIT):
                for k in range(min(max(int(dec_n[row]), 0), dec_ld)):
                    t0, t1, pitch, vel = (int(x) for x in dec[row][k])
                    end = int(dec_end[row])
                    if m == FIT and end > W:                                                                # 4
                        t0 = t0 * W // end
                        t1 = max(t0 + 1, t1 * W // end)
                    if 0 <= t0 < W:                                                                         # 3
                        cand.append((t_lo + t0, t_lo + min(t1, W), pitch, vel))
            for t0, t1, pitch, vel in cand:                                                                 # 6
                if t1 > t0 and 0 <= pitch < 128 and I32_MIN <= t0 and t1 <= I32_MAX:
                    piece.append((t0, t1, pitch, min(max(vel, 1), 127)))
        first_of.append(len(piece))
        pieces.append(piece), firsts.append(first_of)
    return _finish(pieces, firsts, out_ld)


def stitch_of_np(dec, dec_ld, dec_n, dec_end, src, spans, V, mode, out_ld):
    """statement 2: every window is a (candidates, 4) int64 array and a mask; win_first is the cumsum of the masks' sums"""
    dec, src, spans = np.asarray(dec, np.int64), np.asarray(src, np.int64).reshape(-1, 4), np.asarray(spans, np.int64)
    S, n_total = len(spans), len(src)
    t_lo = spans[:, 2]
    W = np.clip(spans[:, 3] - t_lo, 0, MAX_TICK)
    n_dec = np.clip(np.asarray(dec_n, np.int64), 0, dec_ld)
    pieces, firsts = [], []
    for v in range(V):
        kept = []
        for j in range(S):
            row = j * V + v
            m = int(mode[row])
            if m == PASS:
                at = np.arange(n_total)
                q = src[(at >= spans[j, 0]) & (at - spans[j, 0] < spans[j, 1])]          # the span as a mask over the source
                t0, t1 = q[:, 0], q[:, 1]
                inside = (t0 >= t_lo[j]) & (t0 < t_lo[j] + W[j])
            elif m in (CLIP, FIT):
                q = dec[row, :n_dec[row]]
                t0, t1, end = q[:, 0], q[:, 1], int(dec_end[row])
                if m == FIT and end > W[j]:
                    t0 = np.floor_divide(t0 * W[j], end)
                    t1 = np.maximum(t0 + 1, np.floor_divide(t1 * W[j], end))
                inside = (t0 >= 0) & (t0 < W[j])
                t0, t1 = t_lo[j] + t0, t_lo[j] + np.minimum(t1, W[j])
            else:
                q = np.zeros((0, 4), np.int64)
                t0 = t1 = q[:, 0]
                inside = np.zeros(0, bool)
            good = inside & (t1 > t0) & (q[:, 2] >= 0) & (q[:, 2] < 128) & (t0 >= I32_MIN) & (t1 <= I32_MAX)
            kept.append(np.stack([t0, t1, q[:, 2], np.clip(q[:, 3], 1, 127)], 1)[good])
        firsts.append(np.r_[0, np.cumsum([len(k) for k in kept])])
        pieces.append(np.concatenate(kept).tolist())
    return _finish(pieces, firsts, out_ld)


def stitch_ref(c, statement=stitch_of_np, out_ld=None):
    return statement(c["dec"], c["dec_ld"], c["dec_n"], c["dec_end"], c["src"], c["spans"], c["V"], c["mode"], c["out_ld"] if out_ld is None else out_ld)


def same(got, ref, tag=""):
    hn.same(got, ref, KEYS, tag)


# ------------------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------------------
def _case(tag, V, dec, dec_ld, dec_n, dec_end, src, spans, mode, out_ld=None):
    """the arrays in the types the entry point takes; dec (S*V, rs, 4) gets SENTINEL in every slot behind dec_n"""
    dec = np.array(dec, dtype=np.int64)
    spans = np.array(spans, dtype=np.int64).reshape(-1, 4)
    for r in range(dec.shape[0]):
        dec[r, min(max(int(dec_n[r]), 0), dec_ld):] = SENTINEL
    src = np.array(src, dtype=np.int64).reshape(-1, 4)
    c = dict(tag=tag, S=len(spans), V=V, dec=dec.astype(np.int32), dec_ld=dec_ld, dec_n=np.array(dec_n, np.int32), dec_end=np.array(dec_end, np.int32),
             src=src.astype(np.int32), spans=spans.astype(np.int32), mode=np.array(mode, np.int32))
    assert c["dec"].shape[0] == c["S"] * V == len(c["dec_n"]) == len(c["dec_end"]) == len(c["mode"]) and dec_ld <= dec.shape[1]
    c["out_ld"] = len(src) + c["S"] * dec_ld if out_ld is None else out_ld
    return c


def _random_case(tag, S, V, dec_ld=8, rs=11, seed=0, width=200):
    """S windows of `width` ticks, a handful of source notes in each, V decoded rows per window with every kind of note: in and out of the window, of
    length 0, pitches -1 and 128, velocities 0 and 200; dec_n from -3 to dec_ld + 5; modes 0, 1, 2 and an invalid 7; dec_end around W"""
    g = np.random.RandomState(seed)
    src, spans = [], []
    for j in range(S):
        n = (0, 1, 3, 5)[j % 4]
        t0 = np.sort(g.randint(0, width, n)) + width * j
        spans.append([len(src), n, width * j, width * (j + 1)])
        for a in t0:
            src.append([a, a + g.randint(0, 150), g.choice([-1, 0, 40, 60, 127, 128], p=[.05, .1, .35, .35, .1, .05]), g.choice([0, 64, 100, 127, 200])])
    rows = S * V
    dec = np.zeros((rows, rs, 4), np.int64)
    dec[:, :, 0] = g.randint(-5, width + 30, (rows, rs))
    dec[:, :, 1] = dec[:, :, 0] + g.randint(0, 90, (rows, rs))
    dec[:, :, 2] = g.choice([-1, 0, 33, 50, 127, 128], (rows, rs), p=[.05, .1, .35, .35, .1, .05])
    dec[:, :, 3] = g.choice([0, 1, 64, 100, 127, 200], (rows, rs))
    dec_n = g.choice([-3, 0, 1, dec_ld - 1, dec_ld, dec_ld + 5], rows)
    dec_end = g.choice([0, width - 1, width, width + 1, 2 * width, 3 * width + 1], rows)
    mode = g.choice([PASS, CLIP, FIT, 7], rows, p=[.3, .3, .3, .1])
    return _case(tag, V, dec, dec_ld, dec_n, dec_end, src, spans, mode)


def _counts_case():
    """per-window kept counts 0, 1, 63, 64, 65 and dec_ld = 130 across the ballot chunk, and a window of 70 notes every one of which is dropped"""
    dec_ld, rs, W = 130, 132, 1000
    wanted = (0, 1, 63, 64, 65, dec_ld, 0)
    dec = np.zeros((len(wanted), rs, 4), np.int64)
    dec_n = []
    for r, n in enumerate(wanted):
        dec[r, :, 0] = np.arange(rs) * 3
        dec[r, :, 1] = dec[r, :, 0] + 2
        dec[r, :, 2:] = (40 + r, 90)
        dec_n.append(n)
    dec_n[-1] = 70
    dec[-1, :70:2, 2], dec[-1, 1:70:2, 0] = 128, W + 5          # a bad pitch or a start behind the window: nothing is kept
    spans = [[0, 0, W * j, W * (j + 1)] for j in range(len(wanted))]
    return _case("kept counts 0 1 63 64 65 dec_ld and an all-dropped window", 1, dec, dec_ld, dec_n, [500] * len(wanted), np.zeros((0, 4)), spans,
                 [CLIP] * len(wanted))


def _interleaved_counts_case():
    """the same counts with kept and dropped notes alternating, so that a lane's place is not its index; V = 3 with the counts rotated per piece"""
    dec_ld, rs, W, V = 130, 130, 1000, 3
    wanted = (0, 1, 63, 64, 65, dec_ld)
    S = len(wanted)
    dec = np.zeros((S * V, rs, 4), np.int64)
    dec_n = np.zeros(S * V, np.int64)
    for j in range(S):
        for v in range(V):
            r, n = j * V + v, wanted[(j + v) % S]
            dec[r, :, 0] = np.arange(rs) * 3
            dec[r, :, 1] = dec[r, :, 0] + 2
            dec[r, :, 2:] = (10 + r, 70 + v)
            if n <= 65:
                dec[r, 1::2, 2] = -1                         # every other note has a bad pitch
                dec_n[r] = min(2 * n, dec_ld)
            else:
                dec_n[r] = n
    spans = [[0, 0, W * j, W * (j + 1)] for j in range(S)]
    return _case("interleaved kept counts, V 3", V, dec, dec_ld, dec_n, [0] * (S * V), np.zeros((0, 4)), spans, [CLIP, FIT, CLIP] * S)


def _source_case():
    """mode 0: a span whose first + count reaches past n_total, one that starts in front of the array, a count of 600 (above FN_NOTES_MAX) all of which
    pass, t1 not cut at the window's end, a span of count 2^31 - 1"""
    src = [[i, i + 500, 30 + i % 50, 1 + i % 127] for i in range(700)]
    spans = [[0, 600, 0, 600], [600, 500, 600, 650], [-5, 20, 0, 10], [650, I32_MAX, 650, 700], [3, 4, 0, 0], [10, -4, 0, 700]]
    S = len(spans)
    return _case("source spans: count 600, past n_total, in front of the array", 1, np.zeros((S, 4, 4)), 4, [0] * S, [0] * S, src, spans, [PASS] * S)


def _fit_case():
    """W = 0; dec_end = W, W + 1 and 2W; W = FN_NOTES_MAX_TICK (t_hi further away: clamped) with times near it, so that t * W reaches 2^44; negative
    decoded times (floor, not truncation); t_lo at both ends of int32"""
    M = MAX_TICK
    rows = [  # (t_lo, t_hi, dec_end, mode, notes)
        (100, 100, 50, FIT, [(0, 10, 40, 80)]),                                                    # W = 0: nothing
        (100, 90, 50, CLIP, [(0, 10, 40, 80)]),                                                    # t_hi < t_lo: W = 0
        (0, 100, 100, FIT, [(0, 10, 40, 80), (99, 150, 41, 80), (100, 120, 42, 80)]),               # dec_end = W: clause 3
        (0, 100, 101, FIT, [(0, 10, 40, 80), (99, 150, 41, 80), (100, 101, 42, 80), (50, 50, 43, 80)]),          # W + 1
        (0, 100, 200, FIT, [(0, 1, 40, 80), (1, 2, 41, 80), (199, 200, 42, 80), (-1, 5, 43, 80), (-3, -1, 44, 80)]),          # 2W; floor(-1/2) = -1: dropped
        (0, 100, 200, CLIP, [(0, 1, 40, 80), (150, 160, 41, 80), (99, 300, 42, 80)]),               # mode 1 ignores dec_end
        (5, 5 + M + 50, 2 * M, FIT, [(M - 1, M, 40, 80), (2 * M - 2, 2 * M - 1, 41, 80), (M + 3, 2 * M - 1, 42, 80), (2 * M, 2 * M + 1, 43, 80)]),          # 2^44
        (5, 5 + M + 50, I32_MAX, FIT, [(I32_MAX - 1, I32_MAX, 40, 80), (1 << 30, I32_MAX, 41, 80), (I32_MIN, -1, 42, 80)]),
        (5, 5 + M + 50, 0, CLIP, [(M - 1, M + 9, 40, 80), (M, M + 9, 41, 80)]),                     # the clamped W cuts
        (I32_MAX - 100, I32_MAX, 0, CLIP, [(0, 50, 40, 80), (99, 200, 41, 80), (100, 200, 42, 80)]),               # t_lo near 2^31
        (I32_MIN, I32_MIN + 100, 150, FIT, [(0, 50, 40, 80), (149, 150, 41, 80)]),                  # t_lo at the other end
        (I32_MIN, I32_MAX, 0, CLIP, [(M - 1, M, 40, 80), (M, M + 1, 41, 80)]),                      # t_hi - t_lo needs 64 bits
    ]
    S, dec_ld = len(rows), 5
    dec = np.zeros((S, dec_ld, 4), np.int64)
    for r, (_, _, _, _, notes) in enumerate(rows):
        dec[r, :len(notes)] = notes
    return _case("window lengths and fitting", 1, dec, dec_ld, [len(r[4]) for r in rows], [r[2] for r in rows], np.zeros((0, 4)),
                 [[0, 0, r[0], r[1]] for r in rows], [r[3] for r in rows])


def stitch_cases():
    """-> [dict(tag, S, V, dec (S*V, rs, 4), dec_ld, dec_n, dec_end, src (n_total, 4), spans (S, 4), mode (S*V,), out_ld)]"""
    cases = [_random_case("S %d V %d" % (S, V), S, V, seed=10 * S + V) for S in (1, 2, 63, 64, 65, SCAN_PASS + 1) for V in (1, 3)]
    cases += [_counts_case(), _interleaved_counts_case(), _source_case(), _fit_case()]
    base = _random_case("S 7 V 3 dec_ld = the row stride", 7, 3, dec_ld=9, rs=9, seed=5)
    cases.append(base)
    total = int(stitch_ref(base)["win_first"][0, -1])
    assert total > 2
    for out_ld, name in ((total, "the total of piece 0"), (total - 1, "one less"), (1, "1")):
        cases.append(dict(base, tag="out_ld %s" % name, out_ld=out_ld))
    edge = _random_case("the source at int32's ends", 3, 2, seed=9)
    edge["src"][:2] = [[I32_MAX - 1, I32_MAX, 40, 80], [0, I32_MIN, 41, 80]]
    edge["spans"][0] = [0, 2, I32_MAX - 10, I32_MAX]
    edge["mode"][:2] = PASS
    cases.append(edge)
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# transfer_piece
# ------------------------------------------------------------------------------------------------------------------------------
def transfer_ref(src, spans, tokens, used, fit, statement=stitch_of_np):
    """src (n_total, 4), spans (S, 4) of midi_segments, tokens (S, V, steps) and used (S, V) as transfer_piece returned them, fit "clip" / "scale" ->
    the Piece it must have returned: the notes of every row by statement 1 of helpers_notes, the tail span, the modes, then a statement from above"""
    src, spans, tokens, used = np.asarray(src), np.asarray(spans, np.int64), np.asarray(tokens), np.asarray(used)
    S, V, steps = tokens.shape
    dec = np.zeros(((S + 1) * V, steps, 4), np.int32)
    dec_n, dec_end = np.zeros((S + 1) * V, np.int32), np.zeros((S + 1) * V, np.int32)
    for j in range(S):
        for v in range(V):
            r = hn.notes_of(tokens[j, v], hn.DEFAULT)
            dec[j * V + v], dec_n[j * V + v], dec_end[j * V + v] = r["notes"], r["n_notes"], r["t_end"]
    first = int(spans[-1, 0] + spans[-1, 1])
    tail = [first, len(src) - first, int(spans[-1, 3]), min(int(spans[-1, 3]) + MAX_TICK, I32_MAX)]
    mode = np.r_[np.where(used, dict(clip=CLIP, scale=FIT)[fit], PASS).reshape(-1), np.zeros(V, np.int64)]
    return statement(dec, steps, dec_n, dec_end, src, np.vstack([spans, tail]), V, mode, len(src) + (S + 1) * steps)


def hand_midi(pkg):
    """helpers_notes.piece() - 3 windows and a tail - and behind it: window 3 empty, window 4 with more notes than 100 tokens take, window 5 as window 0,
    then a tail of two notes: 6 windows of 200 ticks (4 beats at 120 qpm)"""
    base = hn.piece()[:-1]
    crowd = [(800 + 4 * i, 800 + 4 * i + 3, 30 + i % 40, 60 + i % 30) for i in range(45)]
    w5 = [(1000, 1080, 39, 80), (1000, 1100, 43, 70), (1090, 1300, 46, 90)]          # one note rings into the tail
    tail = [(1200, 1230, 50, 80), (1210, 1225, 52, 64)]
    notes = np.array(base.tolist() + crowd + w5 + tail, np.int32)
    return pkg.MidiNotes(torch.from_numpy(notes), torch.arange(0, 1201, 50, dtype=torch.int32), 0)


def tuples(t, n=None):
    return [tuple(x) for x in (t if n is None else t[:int(n)]).tolist()]


def check_transfer(pkg, midi, res, fit, spans, status, ok=None):
    """res against the restatement applied to the tokens and `used` it reports, `used` against the rule, the passed windows against the source"""
    S, V = res.used.shape
    src = midi.notes.numpy()
    ref = transfer_ref(src, spans, res.tokens.cpu().numpy(), res.used.cpu().numpy(), fit)
    same(dict(notes=res.notes.cpu().numpy(), n_notes=res.n_notes.cpu().numpy(), win_first=res.win_first.cpu().numpy(), status=res.status.cpu().numpy()),
            ref, "transfer " + fit)
    ok = (status == 0) if ok is None else ok
    sounds = np.array([[hn.notes_of(res.tokens[j, v].cpu().numpy(), hn.DEFAULT)["n_notes"] > 0 for v in range(V)] for j in range(S)])
    assert np.array_equal(res.used.cpu().numpy(), ok[:, None] & sounds)
    wf = res.win_first.cpu().numpy()
    bounds = np.r_[spans[:, 0], spans[-1, 0] + spans[-1, 1], len(src)]
    for v in range(V):
        for j in range(S + 1):
            if j == S or not res.used[j, v]:
                assert np.array_equal(res.notes[v, wf[v, j]:wf[v, j + 1]].cpu().numpy(), src[bounds[j]:bounds[j + 1]]), (j, v)
        assert wf[v, S + 1] == int(res.n_notes[v]) and int(res.status[v]) == 0
    return ref


def events(notes):
    """what a MIDI file holds of a list of notes: the note-ons and the note-offs (overlapping notes of one pitch are paired anew on reading)"""
    return sorted((t0, p, v) for t0, _, p, v in notes), sorted((t1, p) for _, t1, p, _ in notes)


def stitch_fake_ops():
    base = type(hn.notes_fake_ops())

    class StitchFakeOps(base):
        def notes_stitch(self, dec, dec_ld, dec_n, dec_end, src, spans, mode, out, win_first, out_n, status):
            self.calls.append("notes_stitch")
            ref = stitch_of_np(dec.numpy(), dec_ld, dec_n.numpy(), dec_end.numpy(), src.numpy(), spans.numpy(), out.shape[0], mode.numpy(), out.shape[1])
            for k, t in zip(KEYS, (out, out_n, win_first, status)):
                t.copy_(torch.from_numpy(ref[k]).view(t.shape))

    return StitchFakeOps()
