"""Event tokens <-> timed notes on the device: tokens_to_notes publishes the notes event_attributes rasters (fn_notes_from_tokens), notes_to_tokens is the
tokeniser (fn_tokens_from_notes; magenta_encode_midi over windows, ptb_v2.py:217-273); include/fadernets.h has the definition.  The walk from tokens to
notes, the order of simultaneous events and the velocity bins are OURS and pinned against nothing of Magenta's; the window cut is the reference's
slice_midi (ptb_v2.py:60-92) made half-open.  midi.py puts Standard MIDI Files on top."""
import collections

import numpy as np
import torch

from . import _lib
from .attributes import MAX_STEPS, _ops_of
from .constrain import MAX_PITCH, _int
from .engine import E_VOCAB

NoteVocab = collections.namedtuple("NoteVocab", ["on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "vel_lo", "n_vel", "midi_lo"],
                                   defaults=(2, 90, 88, 178, 100, 278, 64, 21))
NoteVocab.__doc__ = """The event vocabulary: note-on of pitch p = on_lo + p, note-off = off_lo + p (p < n_pitch <= 128), shift_lo + k = k + 1 ticks of
10 ms (k < n_shift), vel_lo + k = velocity bin k of n_vel (0: no velocity tokens; bin k is velocity min(1 + k * ceil(127 / n_vel), 127)); pitch p is MIDI
note midi_lo + p (21: the piano's lowest A).  The defaults are the 342-token vocabulary of the reference's data (trainer_glsr.py:125,133)."""
Notes = collections.namedtuple("Notes", ["notes", "n_notes", "t_end", "status"])
Notes.__doc__ = """notes (..., notes_ld, 4) int32 rows of (t0, t1, pitch, vel), ascending by (t0, pitch), zeros behind n_notes; n_notes, t_end (the final
clock), status (0, EMPTY, OVERFLOW) int32 (...)."""
NOTES_MAX, MAX_TICK = _lib.FN_NOTES_MAX, _lib.FN_NOTES_MAX_TICK
EMPTY, OVERFLOW = _lib.FN_NOTES_EMPTY, _lib.FN_NOTES_OVERFLOW
PARAMS_DTYPE = np.dtype([(k, "<i4") for k in ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "vocab_size", "vel_lo", "n_vel", "default_vel",
                                              "pad", "add_eos")] + [("reserved", "<i4", (4,))])          # FnNoteParams


def _note_vocab(vocab):
    """the checked NoteVocab; ValueError in the style of _attr_params"""
    V = E_VOCAB
    try:
        on_lo, off_lo, n_pitch, shift_lo, n_shift, vel_lo, n_vel, midi_lo = vocab
    except (TypeError, ValueError):
        raise ValueError("vocab: NoteVocab(on_lo, off_lo, n_pitch, shift_lo, n_shift, vel_lo, n_vel, midi_lo), got %r" % (vocab,))
    n = _int("vocab.n_pitch", n_pitch, 1, MAX_PITCH + 1)
    on, off = _int("vocab.on_lo", on_lo, 0, V + 1), _int("vocab.off_lo", off_lo, 0, V + 1)
    ns, sh = _int("vocab.n_shift", n_shift, 1, 4096 + 1), _int("vocab.shift_lo", shift_lo, 0, V + 1)
    nv, vl = _int("vocab.n_vel", n_vel, 0, 128 + 1), _int("vocab.vel_lo", vel_lo, 0, V + 1)
    ml = _int("vocab.midi_lo", midi_lo, 0, 128 - n + 1)
    ranges = sorted([(on, on + n, "note-on"), (off, off + n, "note-off"), (sh, sh + ns, "time-shift")] + ([(vl, vl + nv, "velocity")] if nv else []))
    if ranges[-1][1] > V:
        raise ValueError("vocab: the token ranges lie inside [0, %d), got %r" % (V, ranges))
    for (_, hi, a), (lo, _, b) in zip(ranges, ranges[1:]):
        if lo < hi:
            raise ValueError("vocab: the %s and %s ranges are disjoint, got %r" % (a, b, ranges))
    return NoteVocab(on, off, n, sh, ns, vl, nv, ml), ranges


def _note_params(vocab, eos, default_vel=100, pad=0, add_eos=False):
    """the checked arguments -> (the 64 bytes of FnNoteParams as a CPU uint8 tensor, NoteVocab)"""
    v, ranges = _note_vocab(vocab)
    eos = -1 if eos is None else _int("eos", eos, 0, E_VOCAB)
    if eos >= 0 and any(lo <= eos < hi for lo, hi, _ in ranges):
        raise ValueError("eos: outside the note, time-shift and velocity ranges, got %d" % eos)
    dv, pad = _int("default_vel", default_vel, 1, 128), _int("pad", pad, 0, E_VOCAB)
    if not isinstance(add_eos, (bool, np.bool_)):
        raise ValueError("add_eos: a bool, got %r" % (add_eos,))
    if add_eos and eos < 0:
        raise ValueError("add_eos: needs an eos")
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    for k, x in zip(PARAMS_DTYPE.names, (v.on_lo, v.off_lo, v.n_pitch, v.shift_lo, v.n_shift, eos, E_VOCAB, v.vel_lo, v.n_vel, dv, pad, int(add_eos))):
        raw[k] = x
    return torch.from_numpy(raw.view(np.uint8).copy()), v


def _what(t):
    return "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__


def tokens_to_notes(tokens, eos=1, vocab=NoteVocab(), default_vel=100, ops=None):
    """The timed notes of event-token rows: what event_attributes rasters, with velocity.

    tokens       (rows, steps) or (n, V, steps) int32 on the device, steps <= 1024.
    eos          a row is read up to the first `eos`; None: to its end.
    default_vel  the velocity before the first velocity token.

    -> Notes(notes (..., steps, 4) int32 rows of (t0, t1, pitch, vel) in ticks of 10 ms, ascending by (t0, pitch), zeros behind n_notes; n_notes, t_end,
    status int32 of tokens.shape[:-1]); device tensors, nothing is copied to the host.  status 0 or EMPTY (no note); `steps` note slots never overflow.
    ValueError for anything that is not as described, before anything is launched.  `ops`: the kernel table (tests); default HipOps(tokens.device)."""
    params, _ = _note_params(vocab, eos, default_vel)
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int32 or tokens.dim() not in (2, 3) or tokens.numel() == 0:
        raise ValueError("tokens: an int32 tensor (rows, steps) or (n, V, steps), got %s" % _what(tokens))
    steps = tokens.shape[-1]
    if steps > MAX_STEPS:
        raise ValueError("tokens: at most %d steps, got %d" % (MAX_STEPS, steps))
    lead = tuple(tokens.shape[:-1])
    tok = tokens.reshape(-1, steps)
    if tok.stride(1) != 1 and steps > 1:
        tok = tok.contiguous()
    rows, dev = tok.shape[0], tok.device
    notes = torch.empty(rows, steps, 4, dtype=torch.int32, device=dev)
    out = [torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3)]
    _ops_of(tok, ops).notes_from_tokens(tok, steps, params.to(dev), notes, *out)
    return Notes(notes.view(lead + (steps, 4)), *(t.view(lead) for t in out))


def notes_to_tokens(notes, spans=None, steps=100, add_eos=True, eos=1, pad=0, vocab=NoteVocab(), n_notes=None, ops=None):
    """The tokeniser: one row of event tokens per span of notes.

    notes    (rows, N, 4) int32 with n_notes (rows,) int32, as tokens_to_notes returns them (N <= 512; every row's window is [0, 2^22) ticks), or flat
             (n_total, 4) int32 with spans (rows, 4) int32 rows of (first, count, t_lo, t_hi): the notes first .. first + count - 1 (count <= 512 is
             used) that start in [t_lo, t_hi), cut at t_hi, times relative to t_lo.  Device tensors; the notes of a span in any order.
    steps    the columns of a row, <= 1024.  add_eos: end every row with eos.  pad: what follows a row's end.

    -> (tokens (rows, steps) int32, n_tokens, n_kept, status (rows,) int32): n_tokens the true length of the row's stream, n_kept the notes of the span
    that lie in the window, status 0, EMPTY (no note) or OVERFLOW (n_tokens > steps: the row holds the first `steps` tokens; the reference drops such
    a segment, ptb_v2.py:264).  Simultaneous events go note-offs first, then by pitch; a velocity token only where the bin changes.
    ValueError for anything that is not as described, before anything is launched."""
    params, _ = _note_params(vocab, eos, 100, pad, add_eos)
    steps = _int("steps", steps, 1, MAX_STEPS + 1)
    if not torch.is_tensor(notes) or notes.dtype != torch.int32 or notes.dim() not in (2, 3) or notes.shape[-1] != 4:
        raise ValueError("notes: an int32 tensor (rows, N, 4) or (n_total, 4), got %s" % _what(notes))
    dev = notes.device
    if notes.dim() == 3:
        rows, N = notes.shape[:2]
        if spans is not None:
            raise ValueError("spans: only with flat notes (n_total, 4)")
        if rows < 1 or not 1 <= N <= NOTES_MAX:
            raise ValueError("notes: at least one row of 1..%d notes, got %s" % (NOTES_MAX, tuple(notes.shape)))
        if not torch.is_tensor(n_notes) or n_notes.dtype != torch.int32 or tuple(n_notes.shape) != (rows,) or n_notes.device != dev:
            raise ValueError("n_notes: an int32 tensor (%d,) beside notes (rows, N, 4), got %s" % (rows, _what(n_notes)))
        spans = torch.stack([torch.arange(rows, dtype=torch.int32, device=dev) * N, n_notes.clamp(0, N), torch.zeros_like(n_notes),
                             torch.full_like(n_notes, MAX_TICK)], 1)
    else:
        if n_notes is not None:
            raise ValueError("n_notes: only with notes (rows, N, 4)")
        if not torch.is_tensor(spans) or spans.dtype != torch.int32 or spans.dim() != 2 or spans.shape[1] != 4 or spans.shape[0] < 1 or spans.device != dev:
            raise ValueError("spans: an int32 tensor (rows, 4) beside flat notes, got %s" % _what(spans))
        rows = spans.shape[0]
    flat, spans = notes.reshape(-1, 4).contiguous(), spans.contiguous()
    tokens = torch.empty(rows, steps, dtype=torch.int32, device=dev)
    out = [torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3)]
    _ops_of(flat, ops).tokens_from_notes(flat, spans, params.to(dev), tokens, steps, *out)
    return (tokens, *out)


Piece = collections.namedtuple("Piece", ["notes", "n_notes", "win_first", "status"])
Piece.__doc__ = """notes (V, out_ld, 4) int32 rows of (t0, t1, pitch, vel) in absolute ticks, the windows in order, zeros behind n_notes; n_notes (V,) int32;
win_first (V, S + 1) int32: the notes in front of window j, the total at S (true counts); status (V,) int32 (0, EMPTY, OVERFLOW)."""
STITCH_MAX_S, STITCH_MAX_V, STITCH_MAX_OUT = _lib.FN_STITCH_MAX_S, _lib.FN_STITCH_MAX_V, _lib.FN_STITCH_MAX_OUT
PASS, CLIP, FIT = 0, 1, 2          # the modes of fn_notes_stitch


def stitch_notes(dec, src_notes, spans, mode, out_ld=None, ops=None):
    """Decoded windows back into pieces (fn_notes_stitch; include/fadernets.h has the clauses): window j of piece v is placed at its span's start, cut
    to its span's length and joined to the windows before it, in one call and without a copy to the host.

    dec        Notes of an (S, V, steps) token tensor, as tokens_to_notes returns them: notes (S, V, dec_ld, 4), n_notes, t_end (S, V) int32.
    src_notes  (n_total, 4) int32, the piece the windows were cut from; spans (S, 4) int32 rows of (first, count, t_lo, t_hi), as midi_segments returns
               them (count is not capped).
    mode       (S, V) int32 on the device: PASS (0) the span's source notes that start in the window, unchanged; CLIP (1) the decoded notes that start
               in [0, W), W = t_hi - t_lo at most 2^22, ends cut at W, moved to t_lo; FIT (2) as CLIP after the decoded times were scaled by W / t_end
               where t_end > W; anything else: the window holds nothing.
    out_ld     the note slots of a piece; None: n_total + S * dec_ld, which cannot overflow.

    -> Piece(notes (V, out_ld, 4), n_notes (V,), win_first (V, S + 1), status (V,)) on the device.  A note that ends up with t1 <= t0, a pitch
    outside [0, 128) or a time outside int32 is dropped, velocities are clamped to [1, 127]: midi_bytes takes every stitched piece.
    ValueError for anything that is not as described, before anything is launched."""
    if not isinstance(dec, Notes) or not all(torch.is_tensor(t) and t.dtype == torch.int32 for t in dec) or dec.notes.dim() != 4 or dec.notes.shape[3] != 4 \
            or dec.notes.numel() == 0 or any(tuple(t.shape) != tuple(dec.notes.shape[:2]) for t in dec[1:]):
        raise ValueError("dec: Notes of an (S, V, steps) token tensor - notes (S, V, dec_ld, 4), n_notes, t_end, status (S, V), int32 - got %s" % (
            ", ".join(_what(t) for t in dec) if isinstance(dec, Notes) else type(dec).__name__))
    S, V, dec_ld = dec.notes.shape[:3]
    dev = dec.notes.device
    if S > STITCH_MAX_S or V > STITCH_MAX_V:
        raise ValueError("dec: at most %d windows of %d pieces, got %d of %d" % (STITCH_MAX_S, STITCH_MAX_V, S, V))
    if not torch.is_tensor(src_notes) or src_notes.dtype != torch.int32 or src_notes.dim() != 2 or src_notes.shape[1] != 4 or src_notes.device != dev:
        raise ValueError("src_notes: an int32 tensor (n_total, 4) beside dec, got %s" % _what(src_notes))
    n_total = src_notes.shape[0]
    if S * max(n_total, dec_ld) >= 2**31:
        raise ValueError("src_notes: S * max(n_total, dec_ld) below 2^31 (a count could leave int32), got %d * %d" % (S, max(n_total, dec_ld)))
    if not torch.is_tensor(spans) or spans.dtype != torch.int32 or tuple(spans.shape) != (S, 4) or spans.device != dev:
        raise ValueError("spans: an int32 tensor (%d, 4) beside dec, got %s" % (S, _what(spans)))
    if not torch.is_tensor(mode) or mode.dtype != torch.int32 or tuple(mode.shape) != (S, V) or mode.device != dev:
        raise ValueError("mode: an int32 tensor (%d, %d) beside dec, got %s" % (S, V, _what(mode)))
    out_ld = n_total + S * dec_ld if out_ld is None else _int("out_ld", out_ld, 1, STITCH_MAX_OUT + 1)
    if out_ld > STITCH_MAX_OUT:
        raise ValueError("out_ld: at most %d note slots, got n_total + S * dec_ld = %d" % (STITCH_MAX_OUT, out_ld))
    rows = dec.notes.reshape(S * V, dec_ld, 4).contiguous()
    out = torch.empty(V, out_ld, 4, dtype=torch.int32, device=dev)
    win_first = torch.empty(V, S + 1, dtype=torch.int32, device=dev)
    out_n, status = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(2))
    _ops_of(rows, ops).notes_stitch(rows, dec_ld, dec.n_notes.reshape(-1).contiguous(), dec.t_end.reshape(-1).contiguous(), src_notes.contiguous(),
                                    spans.contiguous(), mode.reshape(-1).contiguous(), out, win_first, out_n, status)
    return Piece(out, out_n, win_first, status)


KK_MAJOR = (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)          # Krumhansl & Kessler (1982), probe-tone ratings
KK_MINOR = (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)


def key_profiles(device=None):
    """(24, 12) fp64: row tonic + 12 * minor is the Krumhansl-Kessler profile rotated to that tonic"""
    rows = [np.roll(prof, k) for prof in (KK_MAJOR, KK_MINOR) for k in range(12)]
    return torch.tensor(np.array(rows), dtype=torch.float64, device=device)


def estimate_chroma(notes, n_notes=None, vocab=NoteVocab(), one_hot=False):
    """The key vector of get_harmony_vector (ptb_v2.py:95-129) from notes: the duration-weighted pitch-class histogram (pitch class (midi_lo + pitch) %
    12) is correlated (Pearson, fp64) with the 12 rotations of the Krumhansl-Kessler major and minor profiles; index tonic + 12 * minor.  OURS and pinned
    against nothing: it stands in for music21's analyze('key'), which the reference calls.

    notes    (..., N, 4) int32 rows of (t0, t1, pitch, vel); n_notes (...) int32: the rows in use (None: all N; rows with t1 <= t0 weigh nothing).
    one_hot  False: the 24 correlations with everything below 0.1 zeroed (:120); True: 1.0 at the largest correlation (the first on ties).
    -> (..., 24) fp64 on the notes' device; zeros for an empty (or flat) histogram.  A few lines of torch, no kernel."""
    v, _ = _note_vocab(vocab)
    if not isinstance(one_hot, (bool, np.bool_)):
        raise ValueError("one_hot: a bool, got %r" % (one_hot,))
    if not torch.is_tensor(notes):
        notes = torch.as_tensor(np.asarray(notes, dtype=np.int32))
    if notes.dim() < 2 or notes.shape[-1] != 4 or notes.dtype not in (torch.int32, torch.int64):
        raise ValueError("notes: an integer tensor (..., N, 4), got %s" % _what(notes))
    N = notes.shape[-2]
    w = (notes[..., 1].to(torch.int64) - notes[..., 0].to(torch.int64)).clamp(min=0).to(torch.float64)
    if n_notes is not None:
        if not torch.is_tensor(n_notes) or tuple(n_notes.shape) != tuple(notes.shape[:-2]):
            raise ValueError("n_notes: a tensor %s, got %s" % (tuple(notes.shape[:-2]), _what(n_notes)))
        w = w * (torch.arange(N, device=notes.device) < n_notes.to(notes.device).unsqueeze(-1))
    pc = (notes[..., 2].to(torch.int64) + v.midi_lo).remainder(12)
    hist = torch.zeros(notes.shape[:-2] + (12,), dtype=torch.float64, device=notes.device).scatter_add_(-1, pc, w)
    return chroma_of_histogram(hist, one_hot)


def chroma_of_histogram(hist, one_hot=False):
    """(..., 12) fp64 pitch-class weights -> (..., 24) fp64, as estimate_chroma describes"""
    prof = key_profiles(hist.device)
    h, q = hist - hist.mean(-1, keepdim=True), prof - prof.mean(-1, keepdim=True)
    den = h.norm(dim=-1, keepdim=True) * q.norm(dim=-1)
    corr = torch.where(den > 0, (h @ q.T) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    if one_hot:
        best = torch.nn.functional.one_hot(corr.argmax(-1), 24).to(torch.float64)
        return best * (den.amax(-1, keepdim=True) > 0)
    return torch.where(corr < 0.1, torch.zeros_like(corr), corr)
