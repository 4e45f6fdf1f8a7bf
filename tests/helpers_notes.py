"""Test-side restatement of event tokens <-> timed notes (include/fadernets.h, fn_notes_from_tokens / fn_tokens_from_notes; notes.py), from the
definition and not from the kernels:

  notes_of / tokens_of             statement 1: plain Python, dicts and sorted
  notes_of_np / tokens_of_np       statement 2: numpy, cumulative sums for the clock and the token offsets, an explicit sort of packed keys
  notes_from_tokens_ref / tokens_from_notes_ref   statement 2 over a batch, in the shapes the entry points write
  token_cases / span_cases         the case lists the statements, the host twin and the kernels are held to
  piece                            a hand-built piece for midi_segments

A note is (t0, t1, pitch, vel), as FnNote.  The stand-ins at the end (notes_fake_ops) let notes.py / midi.py run on the CPU."""
import numpy as np
import torch

import helpers_attributes as ha

NOTES_MAX, MAX_TICK, MAX_STEPS = 512, 1 << 22, 1024          # FN_NOTES_MAX, FN_NOTES_MAX_TICK, FN_ATTR_MAX_STEPS
EMPTY, OVERFLOW = 1, 2                                        # FN_NOTES_EMPTY, FN_NOTES_OVERFLOW
FIELDS = ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "vocab_size", "vel_lo", "n_vel", "default_vel", "pad", "add_eos")
PARAMS_DTYPE = np.dtype([(k, "<i4") for k in FIELDS] + [("reserved", "<i4", (4,))])          # FnNoteParams, 64 bytes
DEFAULT = dict(on_lo=2, off_lo=90, n_pitch=88, shift_lo=178, n_shift=100, eos=1, vocab_size=342, vel_lo=278, n_vel=64, default_vel=100, pad=0, add_eos=1)
WIDE = dict(DEFAULT, on_lo=2, off_lo=130, n_pitch=128, shift_lo=258, n_shift=100, vocab_size=400, vel_lo=358, n_vel=42)
SENTINEL_TOK = 2 + 40          # a note-on in the default vocabulary: a sentinel column that is read changes the result


def params_bytes(p):
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    for k in FIELDS:
        raw[k] = p[k]
    return raw.view(np.uint8).copy()


def params_from_bytes(b):
    raw = np.asarray(b, dtype=np.uint8).view(PARAMS_DTYPE)[0]
    return {k: int(raw[k]) for k in FIELDS}


def from_attr_params(p):
    """the FnAttrParams dict of helpers_attributes -> FnNoteParams with the velocity range of the same vocabulary"""
    base = WIDE if p["n_pitch"] > 88 else DEFAULT
    return dict(base, **{k: p[k] for k in ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "vocab_size")})


def to_attr_params(p):
    return dict(ha.DEFAULT, **{k: p[k] for k in ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "vocab_size")})


def clamped(p):
    q = dict(p)
    for k, lo, hi in (("n_pitch", 0, 128), ("n_shift", 0, 4096), ("n_vel", 0, 128), ("default_vel", 1, 127)):
        q[k] = min(max(int(p[k]), lo), hi)
    q["vstep"] = (127 + q["n_vel"] - 1) // q["n_vel"] if q["n_vel"] else 1
    return q


def vel_of_bin(k, p):
    return min(1 + k * p["vstep"], 127)


def bin_of_vel(v, p):
    return min((v - 1) // p["vstep"], p["n_vel"] - 1)


def snapped(notes, p):
    """the notes with velocities clamped and snapped to their bins (n_vel 0: the default velocity)"""
    p = clamped(p)
    if p["n_vel"] == 0:
        return [(t0, t1, q, p["default_vel"]) for t0, t1, q, v in notes]
    return [(t0, t1, q, vel_of_bin(bin_of_vel(min(max(v, 1), 127), p), p)) for t0, t1, q, v in notes]


# ------------------------------------------------------------------------------------------------------------------------------
# tokens -> notes
# ------------------------------------------------------------------------------------------------------------------------------
def _finish_notes(kept, t, notes_ld):
    n = len(kept)
    out = np.zeros((notes_ld, 4), np.int32)
    if min(n, notes_ld):
        out[:min(n, notes_ld)] = kept[:notes_ld]
    return dict(notes=out, n_notes=n, t_end=t, status=EMPTY if n == 0 else OVERFLOW if n > notes_ld else 0, kept=kept)


def notes_of(row, p, notes_ld=None):
    """statement 1: the walk with a dict of open notes; -> dict(notes (notes_ld, 4), n_notes, t_end, status, kept = every kept note in order)"""
    p = clamped(p)
    t, vel, held, kept = 0, p["default_vel"], {}, []

    def close(pitch):
        t0, v = held.pop(pitch)
        if t > t0:
            kept.append((t0, t, pitch, v))

    for e in row:
        e = int(e)
        if p["eos"] >= 0 and e == p["eos"]:
            break
        if p["vocab_size"] > 0 and not 0 <= e < p["vocab_size"]:
            continue
        if 0 <= e - p["on_lo"] < p["n_pitch"]:
            pitch = e - p["on_lo"]
            if pitch in held:
                close(pitch)
            held[pitch] = (t, vel)
        elif 0 <= e - p["off_lo"] < p["n_pitch"]:
            if e - p["off_lo"] in held:
                close(e - p["off_lo"])
        elif 0 <= e - p["shift_lo"] < p["n_shift"]:
            t += e - p["shift_lo"] + 1
        elif 0 <= e - p["vel_lo"] < p["n_vel"]:
            vel = vel_of_bin(e - p["vel_lo"], p)
    for pitch in sorted(held):
        close(pitch)
    kept = sorted(kept, key=lambda n: (n[0], n[2]))
    return _finish_notes(kept, t, len(row) if notes_ld is None else notes_ld)


def notes_of_np(row, p, notes_ld=None):
    """statement 2: the clock is a cumulative sum, the velocity the last velocity token before the note-on, and the note of a note-on token ends at
    the next token of its pitch (a note-off closes it, a note-on re-strikes it) or at the row's end; the order is a sort of t0 << 7 | pitch"""
    p = clamped(p)
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    notes_ld = len(row) if notes_ld is None else notes_ld
    if p["eos"] >= 0:
        hit = np.flatnonzero(row == p["eos"])
        if len(hit):
            row = row[:hit[0]]
    ok = (row >= 0) & (row < p["vocab_size"]) if p["vocab_size"] > 0 else np.ones(len(row), bool)
    rng = lambda lo, n: ok & (row >= lo) & (row < lo + n)
    is_on = rng(p["on_lo"], p["n_pitch"])
    is_off = rng(p["off_lo"], p["n_pitch"]) & ~is_on
    is_sh = rng(p["shift_lo"], p["n_shift"]) & ~is_on & ~is_off
    is_vel = rng(p["vel_lo"], p["n_vel"]) & ~is_on & ~is_off & ~is_sh
    clock = np.cumsum(np.where(is_sh, row - p["shift_lo"] + 1, 0))          # after the token; a note token's own time as well
    t_end = int(clock[-1]) if len(row) else 0
    last_vel = np.maximum.accumulate(np.where(is_vel, np.arange(len(row)), -1)) if len(row) else np.zeros(0, np.int64)
    vel = np.where(last_vel >= 0, np.minimum(1 + (row[np.maximum(last_vel, 0)] - p["vel_lo"]) * p["vstep"], 127), p["default_vel"])
    idx = np.flatnonzero(is_on | is_off)
    pitch = np.where(is_on[idx], row[idx] - p["on_lo"], row[idx] - p["off_lo"])
    order = np.argsort(pitch * (len(row) + 1) + idx, kind="stable")          # by pitch, then by position
    idx, pitch = idx[order], pitch[order]
    nxt_same = np.r_[pitch[1:] == pitch[:-1], False] if len(idx) else np.zeros(0, bool)
    t1 = np.where(nxt_same, clock[np.r_[idx[1:], 0]] if len(idx) else 0, t_end)
    t0 = clock[idx]
    keep = is_on[idx] & (t1 > t0)
    key = np.sort((t0[keep] << 7) | pitch[keep])
    by_key = {int((a << 7) | b): (int(a), int(c), int(b), int(d)) for a, b, c, d in zip(t0[keep], pitch[keep], t1[keep], vel[idx][keep])}
    assert len(by_key) == len(key)                                           # (t0, pitch) is unique
    return _finish_notes([by_key[int(k)] for k in key], t_end, notes_ld)


def notes_from_tokens_ref(tokens, steps, p, notes_ld, statement=notes_of_np):
    """tokens (rows, >= steps) -> dict(notes (rows, notes_ld, 4) int32, n_notes, t_end, status (rows,) int32)"""
    rows = [statement(r[:steps], p, notes_ld) for r in np.asarray(tokens)]
    out = {k: np.array([r[k] for r in rows], dtype=np.int32) for k in ("n_notes", "t_end", "status")}
    out["notes"] = np.stack([r["notes"] for r in rows])
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# notes -> tokens
# ------------------------------------------------------------------------------------------------------------------------------
def _window(span):
    first, count, t_lo, t_hi = (int(x) for x in span)
    return first, min(max(count, 0), NOTES_MAX), t_lo, min(max(t_hi, t_lo), t_lo + MAX_TICK)


def tokens_of(notes, span, p, steps):
    """statement 1: a sorted list of event tuples and a stream that is appended to; -> dict(tokens (steps,), n_tokens, n_kept, status)"""
    p = clamped(p)
    first, count, t_lo, t_hi = _window(span)
    events, n_kept = [], 0
    for k in range(count):
        if not 0 <= first + k < len(notes):
            continue
        t0, t1, pitch, vel = (int(x) for x in notes[first + k])
        t1 = min(t1, t_hi)
        if not (0 <= pitch < p["n_pitch"] and t_lo <= t0 < t_hi and t1 > t0):
            continue
        b = bin_of_vel(min(max(vel, 1), 127), p) if p["n_vel"] else None
        events += [(t0 - t_lo, 1, pitch, k, b), (t1 - t_lo, 0, pitch, k, b)]
        n_kept += 1
    stream, length, clock, cur = [], 0, 0, None

    def emit(e, times=1):
        nonlocal length
        stream.extend([e] * min(times, max(0, steps - length)))
        length += times

    for tick, kind, pitch, k, b in sorted(events):
        g, clock = tick - clock, tick
        if p["n_shift"]:
            emit(p["shift_lo"] + p["n_shift"] - 1, g // p["n_shift"])
            if g % p["n_shift"]:
                emit(p["shift_lo"] + g % p["n_shift"] - 1)
        if kind == 1 and b is not None and b != cur:
            cur = b
            emit(p["vel_lo"] + b)
        emit((p["on_lo"] if kind == 1 else p["off_lo"]) + pitch)
    if p["add_eos"] != 0 and p["eos"] >= 0:
        emit(p["eos"])
    tok = np.full(steps, p["pad"], np.int32)
    tok[:len(stream)] = stream
    return dict(tokens=tok, n_tokens=length, n_kept=n_kept, status=OVERFLOW if length > steps else EMPTY if n_kept == 0 else 0)


def tokens_of_np(notes, span, p, steps):
    """statement 2: keys tick << 18 | kind << 17 | pitch << 10 | k sorted by numpy; gaps by a difference, the bin before by a running maximum of
    positions, offsets by a cumulative sum, the tokens scattered to their offsets"""
    p = clamped(p)
    first, count, t_lo, t_hi = _window(span)
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    k = np.arange(count)
    at = first + k
    inside = (at >= 0) & (at < len(notes))
    k, q = k[inside], notes[at[inside]]
    t0, t1, pitch, vel = q[:, 0], np.minimum(q[:, 1], t_hi), q[:, 2], np.clip(q[:, 3], 1, 127)
    keep = (pitch >= 0) & (pitch < p["n_pitch"]) & (t0 >= t_lo) & (t0 < t_hi) & (t1 > t0)
    k, t0, t1, pitch, vel = k[keep], t0[keep], t1[keep], pitch[keep], vel[keep]
    bins = np.zeros(NOTES_MAX, np.int64)
    if p["n_vel"]:
        bins[k] = np.minimum((vel - 1) // p["vstep"], p["n_vel"] - 1)
    key = np.sort(np.concatenate([((t0 - t_lo) << 18) | (1 << 17) | (pitch << 10) | k, ((t1 - t_lo) << 18) | (pitch << 10) | k]))
    n = len(key)
    tick, is_on, pitch, k = key >> 18, ((key >> 17) & 1).astype(bool), (key >> 10) & 127, key & 1023
    g = np.diff(np.r_[0, tick])
    ns = p["n_shift"]
    full, rest = (g // ns, g % ns) if ns else (np.zeros(n, np.int64), np.zeros(n, np.int64))
    b = bins[k]
    pos_on = np.where(is_on, np.arange(n), -1)
    before = np.r_[-1, np.maximum.accumulate(pos_on)[:-1]] if n else np.zeros(0, np.int64)          # the position of the ON before
    velf = is_on & (p["n_vel"] > 0) & ((before < 0) | (b != b[np.maximum(before, 0)]))
    cnt = full + (rest > 0) + velf + 1
    start = np.cumsum(cnt) - cnt
    length = int(cnt.sum())
    tok = np.full(steps, p["pad"], np.int64)

    def scatter(pos, val, mask):
        m = mask & (pos < steps)
        tok[pos[m]] = val[m] if isinstance(val, np.ndarray) else val

    runs = np.clip(steps - start, 0, full)                                   # the long shifts that lie in front of `steps`
    where = np.repeat(start, runs) + np.arange(int(runs.sum())) - np.repeat(np.cumsum(runs) - runs, runs)
    tok[where] = p["shift_lo"] + ns - 1
    everything = np.ones(n, bool)
    scatter(start + full, p["shift_lo"] + rest - 1, rest > 0)
    scatter(start + full + (rest > 0), p["vel_lo"] + b, velf)
    scatter(start + cnt - 1, np.where(is_on, p["on_lo"], p["off_lo"]) + pitch, everything)
    if p["add_eos"] != 0 and p["eos"] >= 0:
        if length < steps:
            tok[length] = p["eos"]
        length += 1
    n_kept = n // 2
    return dict(tokens=tok.astype(np.int32), n_tokens=length, n_kept=n_kept, status=OVERFLOW if length > steps else EMPTY if n_kept == 0 else 0)


def tokens_from_notes_ref(notes, spans, steps, p, statement=tokens_of_np):
    """notes (n_total, 4), spans (rows, 4) -> dict(tokens (rows, steps) int32, n_tokens, n_kept, status (rows,) int32)"""
    rows = [statement(notes, s, p, steps) for s in np.asarray(spans)]
    out = {k: np.array([r[k] for r in rows], dtype=np.int32) for k in ("n_tokens", "n_kept", "status")}
    out["tokens"] = np.stack([r["tokens"] for r in rows])
    return out


def same(got, ref, keys, tag=""):
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, k, g.dtype, r.dtype, g.shape, r.shape)
        assert np.array_equal(g, r), (tag, k, np.argwhere(g != r)[:4].tolist(), g[g != r][:4], r[g != r][:4])


NOTE_KEYS = ("notes", "n_notes", "t_end", "status")
TOKEN_KEYS = ("tokens", "n_tokens", "n_kept", "status")


# ------------------------------------------------------------------------------------------------------------------------------
# the case lists
# ------------------------------------------------------------------------------------------------------------------------------
TOKEN_SHAPES = [(7, 1), (1, 63), (7, 64), (300, 65), (7, 100), (300, 100), (1, 1024), (7, 1024)]          # rows 1 / 7 / 300, steps 1 ... 1024


def token_cases():
    """-> [dict(tag, p, tok (rows, tok_ld) int32, steps, notes_ld)]: the fixture rows of helpers_attributes (its hand rows are among them), rows x steps
    of random_row in both grammar modes with eos mid-row in some, tok_ld = steps + 3 with sentinel columns, notes_ld = steps and 5 (which some rows
    overflow beside rows that fit), the WIDE parameters, parameters to clamp"""
    cases = []
    for g, p, names, tok in ha.fixture_streams():
        cases.append(dict(tag="fixture " + g, p=from_attr_params(p), tok=tok, steps=tok.shape[1], notes_ld=tok.shape[1]))
    for rows, steps in TOKEN_SHAPES:
        rs = np.random.RandomState(2000 * rows + steps)
        tok = np.full((rows, steps + 3), SENTINEL_TOK, dtype=np.int32)
        for i in range(rows):
            tok[i, :steps] = ha.random_row(rs, ha.DEFAULT, steps, i % 3 == 0, eos_at=(steps // 2 if i % 5 == 4 else None))
        for notes_ld in (steps, 5):
            cases.append(dict(tag="%dx%d notes_ld %d" % (rows, steps, notes_ld), p=DEFAULT, tok=tok, steps=steps, notes_ld=notes_ld))
    rs = np.random.RandomState(77)
    tok = np.stack([ha.random_row(rs, ha.WIDE, 100, i % 2 == 0) for i in range(7)]).astype(np.int32)
    tok[:, 3::11] = WIDE["vel_lo"] + rs.randint(0, 42, tok[:, 3::11].shape)
    tok[0, 10], tok[1, 20] = 100000, -7
    cases.append(dict(tag="wide", p=WIDE, tok=tok, steps=100, notes_ld=100))
    cases.append(dict(tag="to clamp: n_pitch 200, n_vel 300, default_vel 0, no vocabulary cut", p=dict(WIDE, n_pitch=200, n_vel=300, default_vel=0, vocab_size=0),
                      tok=tok, steps=100, notes_ld=100))
    cases.append(dict(tag="n_vel 0, no eos, default_vel 500", p=dict(DEFAULT, n_vel=0, eos=-1, default_vel=500), tok=cases[0]["tok"], steps=100, notes_ld=7))
    return cases


SPAN_COUNTS = (0, 1, 31, 32, 33, 64, 65, 511, 512)
SPAN_SHAPES = [(1, 1), (7, 100), (300, 100), (7, 1024), (1, 1024)]


def _span_case(rs, rows, steps, p, tok_ld):
    notes, spans = [], []
    for r in range(rows):
        count = SPAN_COUNTS[(r + steps) % len(SPAN_COUNTS)] if rows > 1 else 33
        if rows == 300 and count > 65:
            count = (r * 7) % 40                                             # 300 rows of 512 notes are a long test: most rows are small
        width = [400, 400, 800, 3000, MAX_TICK, MAX_TICK + 50][r % 6]
        t_lo = [0, 1000, -300, 2**31 - 1 - MAX_TICK, 5, -2**31][r % 6]
        n = max(count, 1)
        t0 = t_lo + (rs.randint(-20, width + 20, n) if width < MAX_TICK else rs.randint(0, 30, n) * (width // 29) - 7)
        if r % 4 == 1:
            t0 = t_lo + np.sort(rs.randint(0, min(width, 2000), n)) // 25 * 25          # on a grid: simultaneous events
        if r % 8 == 2:
            t0[0] = t_lo                                                     # a note at the window's start
        dur = rs.randint(0, 300, n) // (1 + r % 3) * (1 + r % 3)
        pitch = rs.randint(-1, clamped(p)["n_pitch"] + 1, n) if r % 5 == 0 else rs.randint(30, 30 + 3 + r % 20, n)
        vel = rs.randint(-5, 140, n) if r % 2 else rs.randint(60, 70, n)
        rowsn = np.stack([t0, t0 + dur, pitch, vel], 1).astype(np.int64)
        if r % 7 == 3 and n > 2:
            rowsn[1] = rowsn[0]                                               # a duplicated note
        spans.append([len(notes), count, t_lo, min(t_lo + width, 2**31 - 1)])
        notes.extend(rowsn.tolist())
    notes = np.clip(np.array(notes, dtype=np.int64).reshape(-1, 4), -2**31, 2**31 - 1).astype(np.int32)
    spans = np.array(spans, dtype=np.int32).reshape(-1, 4)
    if rows > 2:
        spans[-1, 1] = 600                                                   # count above FN_NOTES_MAX, reaching past n_total
        spans[1, 0] = -3                                                     # reaching in front of the array
        spans[2, 3] = spans[2, 2] - 10                                       # t_hi < t_lo: an empty window
    return dict(tag="%d spans, %d steps" % (rows, steps), p=p, notes=notes, spans=spans, steps=steps, tok_ld=tok_ld)


def span_cases():
    """-> [dict(tag, p, notes (n_total, 4) int32, spans (rows, 4) int32, steps, tok_ld)]: counts 0 ... 512, windows up to FN_NOTES_MAX_TICK at both ends
    of the int32 range, notes on a grid, out of the window and of the pitch range, velocities to clamp, spans that leave the array"""
    rs = np.random.RandomState(4242)
    cases = [_span_case(rs, rows, steps, DEFAULT, steps + 3) for rows, steps in SPAN_SHAPES]
    cases.append(dict(_span_case(rs, 7, 100, WIDE, 100), tag="wide spans"))
    cases.append(dict(_span_case(rs, 7, 100, dict(DEFAULT, n_vel=0, add_eos=0, pad=7), 103), tag="n_vel 0, no eos, pad 7"))
    cases.append(dict(_span_case(rs, 7, 100, dict(DEFAULT, n_shift=0), 103), tag="n_shift 0 stays in bounds", unspecified=True))
    cases.append(dict(_span_case(rs, 7, 100, dict(DEFAULT, n_shift=1, eos=-1), 103), tag="n_shift 1: long runs of shifts"))
    cases.append(dict(tag="no notes at all", p=DEFAULT, notes=np.zeros((0, 4), np.int32), spans=np.array([[0, 5, 0, 100]], np.int32), steps=10, tok_ld=13))
    return cases


def piece():
    """3 windows of 4 beats at 120 qpm (200 ticks each) and a tail: window 0 begins with a chord at its start, window 1 begins late, window 2 holds more
    notes than 20 tokens take"""
    w0 = [(0, 50, 39, 80), (0, 100, 43, 80), (50, 100, 46, 90), (100, 250, 51, 90), (150, 200, 39, 60)]          # one note leaves the window: cut at 200
    w1 = [(210, 300, 40, 80), (300, 390, 44, 80)]
    w2 = [(400 + 12 * i, 400 + 12 * i + 10, 30 + 2 * (i % 7), 70) for i in range(12)]
    tail = [(600, 650, 39, 80)]
    return np.array(w0 + w1 + w2 + tail, np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def notes_fake_ops():
    """the decode / attribute stand-ins + fn_notes_from_tokens / fn_tokens_from_notes as their restatement"""
    base = type(ha.attr_fake_ops())

    class NotesFakeOps(base):
        def notes_from_tokens(self, tokens, steps, params, notes, n_notes, t_end, status):
            self.calls.append("notes_from_tokens")
            ref = notes_from_tokens_ref(tokens.numpy(), steps, params_from_bytes(params.numpy()), notes.shape[1])
            for k, t in zip(NOTE_KEYS, (notes, n_notes, t_end, status)):
                t.copy_(torch.from_numpy(ref[k]))

        def tokens_from_notes(self, notes, spans, params, tokens, steps, n_tokens, n_kept, status):
            self.calls.append("tokens_from_notes")
            self.last_spans = spans.clone()
            ref = tokens_from_notes_ref(notes.numpy(), spans.numpy(), steps, params_from_bytes(params.numpy()))
            tokens[:, :steps].copy_(torch.from_numpy(ref["tokens"]))
            for k, t in zip(TOKEN_KEYS[1:], (n_tokens, n_kept, status)):
                t.copy_(torch.from_numpy(ref[k]))

    return NotesFakeOps()
