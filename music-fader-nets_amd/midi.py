"""Standard MIDI Files on top of notes.py: decoded tokens to a .mid a user can open (write_midi, write_midis - what the reference does with
magenta_decode_midi, test_class.py:124-139), and a .mid to the rows the model encodes (read_midi, midi_segments - magenta_encode_midi over 4-beat slices,
ptb_v2.py:217-273).  The file format is host Python, ours (neither mido nor pretty_midi is needed); the two batch steps are the kernels of notes.py.
Control changes are ignored on reading, so a sustain pedal lengthens nothing, as in the reference's loader."""
import bisect
import collections
import os

import numpy as np
import torch

from .attributes import EventGrid, event_attributes
from .constrain import EventVocab, _int
from .notes import NoteVocab, _note_vocab, _what, chroma_of_histogram, notes_to_tokens, tokens_to_notes

MidiNotes = collections.namedtuple("MidiNotes", ["notes", "beats", "n_dropped"])
MidiNotes.__doc__ = """notes (N, 4) int32 rows of (t0, t1, pitch, vel) in ticks of 10 ms, sorted by (t0, pitch); beats: int32 ticks of every quarter-note
beat up to the file's last event, the first at 0; n_dropped: notes left out (pitch outside the vocabulary, channel 10).  CPU tensors."""


# ------------------------------------------------------------------------------------------------------------------------------
# writing
# ------------------------------------------------------------------------------------------------------------------------------
def _varlen(n):
    if not 0 <= n < 1 << 28:
        raise ValueError("a delta time of %d MIDI ticks does not fit a variable-length quantity" % n)
    out = [n & 0x7F]
    while n > 0x7F:
        n >>= 7
        out.append(0x80 | (n & 0x7F))
    return bytes(reversed(out))


def _timing(qpm):
    """-> (division, microseconds per quarter, MIDI ticks per 10 ms): the smallest division under which 10 ms is a whole number of MIDI ticks"""
    if isinstance(qpm, (bool, np.bool_)) or not isinstance(qpm, (int, float, np.integer, np.floating)) or not 4 <= qpm <= 6000:
        raise ValueError("qpm: a number in [4, 6000], got %r" % (qpm,))
    tempo = int(round(60e6 / qpm))
    g = np.gcd(tempo, 10000)
    division = tempo // int(g)
    if division > 0x7FFF:
        raise ValueError("qpm %r: no division below 32768 makes 10 ms a whole number of MIDI ticks (120, 100, 60 ... work)" % (qpm,))
    return division, tempo, 10000 // int(g)


def midi_bytes(notes, vocab=NoteVocab(), qpm=120):
    """(N, 4) integers (t0, t1, pitch, vel) -> the bytes of a format-0 file: one tempo event, note-ons and note-offs at pitch midi_lo + pitch, end of track"""
    v, _ = _note_vocab(vocab)
    division, tempo, per_tick = _timing(qpm)
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    if len(notes) and (notes[:, 0].min() < 0 or (notes[:, 1] <= notes[:, 0]).any() or notes[:, 2].min() < 0 or notes[:, 2].max() >= v.n_pitch
                       or notes[:, 3].min() < 1 or notes[:, 3].max() > 127):
        raise ValueError("notes: rows of (t0 >= 0, t1 > t0, 0 <= pitch < %d, 1 <= vel <= 127)" % v.n_pitch)
    events = sorted([(int(t0), 1, int(p), int(vel)) for t0, _, p, vel in notes] + [(int(t1), 0, int(p), 0) for _, t1, p, _ in notes])
    track, clock = bytearray(b"\x00\xff\x51\x03" + tempo.to_bytes(3, "big")), 0
    for t, on, p, vel in events:
        track += _varlen((t - clock) * per_tick) + bytes([0x90 if on else 0x80, v.midi_lo + p, vel])
        clock = t
    track += b"\x00\xff\x2f\x00"
    return b"MThd" + (6).to_bytes(4, "big") + (0).to_bytes(2, "big") + (1).to_bytes(2, "big") + division.to_bytes(2, "big") + b"MTrk" + len(track).to_bytes(
        4, "big") + bytes(track)


def _put(path_or_file, data):
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as f:
            f.write(data)


def write_midi(path_or_file, notes, n_notes=None, vocab=NoteVocab(), qpm=120, eos=1, default_vel=100, ops=None):
    """One row of notes as a format-0 Standard MIDI File.

    notes    (N, 4) array / tensor of (t0, t1, pitch, vel) with n_notes (None: all N), or a token row: a 1-D int32 device tensor, decoded first by
             tokens_to_notes(eos, vocab, default_vel).
    qpm      the tempo written; one under which 10 ms is a whole number of MIDI ticks (at 120: division 50, one tick each), so every time is exact.
    The file holds one tempo event, note-on / note-off events on channel 1 at pitch midi_lo + pitch, and the end of the track."""
    if torch.is_tensor(notes) and notes.dim() == 1:
        res = tokens_to_notes(notes.unsqueeze(0), eos=eos, vocab=vocab, default_vel=default_vel, ops=ops)
        notes, n_notes = res.notes[0], res.n_notes[0]
    arr = notes.detach().cpu().numpy() if torch.is_tensor(notes) else np.asarray(notes)
    if arr.ndim != 2 or arr.shape[1] != 4 or arr.dtype.kind not in "iu":
        raise ValueError("notes: integers (N, 4) or a 1-D token row, got %s %s" % (arr.dtype, arr.shape))
    if n_notes is not None:
        arr = arr[:_int("n_notes", int(n_notes), 0, len(arr) + 1)]
    _put(path_or_file, midi_bytes(arr, vocab, qpm))


def write_midis(dir, tokens, names=None, eos=1, vocab=NoteVocab(), default_vel=100, qpm=120, ops=None):
    """A whole sweep to files: ONE tokens_to_notes call and one device-to-host copy, then a file per row.

    tokens   (rows, steps) or (n, V, steps) int32 on the device.
    names    a file name per row (row-major); None: 00000.mid ... or, for (n, V, steps), 000_00.mid = sample_value.
    -> the paths written, row-major.  A row without a note gives a file without one."""
    _timing(qpm)
    if torch.is_tensor(tokens) and tokens.dim() in (2, 3) and tokens.numel():
        rows = tokens.numel() // tokens.shape[-1]
        if names is None:
            names = ["%05d.mid" % r for r in range(rows)] if tokens.dim() == 2 else ["%03d_%02d.mid" % divmod(r, tokens.shape[1]) for r in range(rows)]
        names = list(names)
        if len(names) != rows or not all(isinstance(n, str) and n for n in names):
            raise ValueError("names: %d file names, got %r" % (rows, names[:4]))
    res = tokens_to_notes(tokens, eos=eos, vocab=vocab, default_vel=default_vel, ops=ops)          # raises for any other `tokens`
    steps = res.notes.shape[-2]
    host = torch.cat([res.notes.reshape(rows, steps * 4), res.n_notes.reshape(rows, 1)], 1).cpu().numpy()
    os.makedirs(dir, exist_ok=True)
    paths = []
    for r, name in enumerate(names):
        paths.append(os.path.join(dir, name))
        _put(paths[-1], midi_bytes(host[r, :steps * 4].reshape(steps, 4)[:host[r, -1]], vocab, qpm))
    return paths


# ------------------------------------------------------------------------------------------------------------------------------
# reading
# ------------------------------------------------------------------------------------------------------------------------------
class _Bytes:
    """a cursor that answers a read past the end with ValueError"""

    def __init__(self, data, pos=0, end=None):
        self.data, self.pos, self.end = data, pos, len(data) if end is None else end

    def take(self, n):
        if n < 0 or self.pos + n > self.end:
            raise ValueError("MIDI file: it ends inside an event or a chunk (at byte %d)" % self.pos)
        self.pos += n
        return self.data[self.pos - n:self.pos]

    def byte(self):
        return self.take(1)[0]

    def varlen(self):
        n = 0
        for _ in range(4):
            b = self.byte()
            n = (n << 7) | (b & 0x7F)
            if b < 0x80:
                return n
        raise ValueError("MIDI file: a variable-length quantity of more than 4 bytes (at byte %d)" % self.pos)


def _track_events(cur, track):
    """-> ([(tick, track, order, kind, a, b, c)], last tick): kind 'on' / 'off' (channel, pitch, velocity) or 'tempo' (microseconds, 0, 0)"""
    events, tick, status, order = [], 0, None, 0
    while cur.pos < cur.end:
        tick += cur.varlen()
        b = cur.byte()
        if b == 0xFF:                                   # meta: type, length, data
            kind, data = cur.byte(), cur.take(cur.varlen())
            if kind == 0x2F:
                break
            if kind == 0x51:
                if len(data) != 3:
                    raise ValueError("MIDI file: a set-tempo event of %d bytes" % len(data))
                events.append((tick, track, order, "tempo", int.from_bytes(data, "big"), 0, 0))
        elif b in (0xF0, 0xF7):                         # sysex: length, data
            cur.take(cur.varlen())
        elif b >= 0xF0:
            raise ValueError("MIDI file: status byte 0x%02X inside a track" % b)
        else:
            if b >= 0x80:
                status, first = b, cur.byte()
            elif status is None:
                raise ValueError("MIDI file: a data byte without a running status (at byte %d)" % cur.pos)
            else:
                first = b                               # running status
            second = cur.byte() if status & 0xF0 not in (0xC0, 0xD0) else 0
            if first >= 0x80 or second >= 0x80:
                raise ValueError("MIDI file: a data byte above 127 (at byte %d)" % cur.pos)
            if status & 0xF0 == 0x90 and second > 0:
                events.append((tick, track, order, "on", status & 0x0F, first, second))
            elif status & 0xF0 in (0x80, 0x90):         # a note-on of velocity 0 is a note-off
                events.append((tick, track, order, "off", status & 0x0F, first, 0))
        order += 1
    return events, tick


def read_midi(path_or_file, vocab=NoteVocab(), drums=False):
    """A Standard MIDI File (format 0 or 1) as notes in ticks of 10 ms.  Pure Python.

    Running status, note-on with velocity 0 as note-off, any meta / sysex event (skipped by its length) and a set-tempo event anywhere in any track are
    handled.  The events of all tracks are merged by time (then track, then order); per (channel, pitch) a note-off closes the OLDEST open note; notes
    still open at the end close at the last event's time.  Times go through the tempo map in exact integer arithmetic to floor(seconds * 100 + 1/2); a
    note whose quantised length is 0 gets length 1.  Pitches outside [midi_lo, midi_lo + n_pitch) and, unless `drums`, channel 10 are dropped and counted.
    Control changes (the pedal) are ignored, as the reference's loader ignores them.
    -> MidiNotes(notes (N, 4) int32 sorted by (t0, pitch), beats, n_dropped).  ValueError (never IndexError / struct.error) for SMPTE division, a bad
    chunk tag, format 2, and a file that ends inside an event."""
    v, _ = _note_vocab(vocab)
    if not isinstance(drums, (bool, np.bool_)):
        raise ValueError("drums: a bool, got %r" % (drums,))
    if hasattr(path_or_file, "read"):
        data = path_or_file.read()
    else:
        with open(path_or_file, "rb") as f:
            data = f.read()
    if not isinstance(data, (bytes, bytearray)):
        raise ValueError("read_midi: a path or a binary file, got %s" % type(data).__name__)
    cur = _Bytes(bytes(data))
    if cur.take(4) != b"MThd":
        raise ValueError("MIDI file: it does not start with MThd")
    hlen = int.from_bytes(cur.take(4), "big")
    if hlen < 6:
        raise ValueError("MIDI file: a header of %d bytes" % hlen)
    head = cur.take(hlen)
    fmt, ntrks, division = (int.from_bytes(head[i:i + 2], "big") for i in (0, 2, 4))
    if fmt not in (0, 1):
        raise ValueError("MIDI file: format %d (0 and 1 are read)" % fmt)
    if division & 0x8000 or division == 0:
        raise ValueError("MIDI file: SMPTE division 0x%04X (ticks per quarter note are read)" % division)
    events, last = [], 0
    for track in range(ntrks):
        tag = cur.take(4)
        if tag != b"MTrk":
            raise ValueError("MIDI file: chunk tag %r where MTrk is expected" % tag)
        n = int.from_bytes(cur.take(4), "big")
        start = cur.pos
        cur.take(n)
        ev, end = _track_events(_Bytes(cur.data, start, start + n), track)
        events += ev
        last = max(last, end)
    events.sort(key=lambda e: e[:3])
    # the tempo map: (MIDI tick, microseconds per quarter, microsecond-ticks elapsed at that tick); seconds = elapsed / (division * 10^6)
    tempo_map = [(0, 500000, 0)]
    for tick, _, _, kind, us, _, _ in events:
        if kind == "tempo":
            at, tempo, elapsed = tempo_map[-1]
            if tick == at:
                tempo_map[-1] = (at, us, elapsed)
            else:
                tempo_map.append((tick, us, elapsed + (tick - at) * tempo))
    starts = [m[0] for m in tempo_map]

    def ticks10(tick):
        at, tempo, elapsed = tempo_map[bisect.bisect_right(starts, tick) - 1]
        return ((elapsed + (tick - at) * tempo) * 200 + division * 10**6) // (2 * division * 10**6)

    open_notes, notes, dropped = collections.defaultdict(collections.deque), [], 0

    def close(ch, key, on_tick, vel, off_tick):
        nonlocal dropped
        if not v.midi_lo <= key < v.midi_lo + v.n_pitch or (ch == 9 and not drums):
            dropped += 1
            return
        t0, t1 = ticks10(on_tick), ticks10(off_tick)
        notes.append((t0, max(t1, t0 + 1), key - v.midi_lo, vel))

    for tick, _, _, kind, ch, key, vel in events:
        if kind == "on":
            open_notes[(ch, key)].append((tick, vel))
        elif kind == "off" and open_notes[(ch, key)]:
            close(ch, key, *open_notes[(ch, key)].popleft(), tick)
    for (ch, key), q in sorted(open_notes.items()):
        for on_tick, vel in q:
            close(ch, key, on_tick, vel, last)
    notes.sort(key=lambda n: (n[0], n[2], n[1], n[3]))
    if notes and max(n[1] for n in notes) >= 2**31:
        raise ValueError("MIDI file: it lasts longer than 2^31 ticks of 10 ms")
    beats = [ticks10(k * division) for k in range(last // division + 1)]
    return MidiNotes(torch.tensor(notes, dtype=torch.int32).reshape(-1, 4), torch.tensor(beats, dtype=torch.int32), dropped)


# ------------------------------------------------------------------------------------------------------------------------------
# a piece -> the rows of a data set
# ------------------------------------------------------------------------------------------------------------------------------
def midi_segments(midi, beats_per_segment=4, max_tokens=100, vocab=NoteVocab(), labels=False, ops=None, device=None):
    """One piece sliced into windows of `beats_per_segment` beats and tokenised, as process_data does (ptb_v2.py:217-273): window j runs from beat
    bps * j to beat bps * (j + 1) of midi.beats; only whole windows are kept.  The spans come from torch.searchsorted on the sorted t0, then ONE
    notes_to_tokens call (eos = 1 closes every row, pad 0).

    midi     MidiNotes (read_midi); the work happens on `device` (None: where midi.notes lives, or cuda if that is the CPU and no `ops` is given).
    -> dict(tokens (S, max_tokens) float32 ids, as the data sets yield them; n_tokens, status (S,) int32; keep (S,) bool: status 0 (so the row fits) and
    the row does not begin with a time shift - the first note starts at the window's start, the reference's rhythm[0] == 1 and len(events) <=
    max_tokens, :264; chroma (S, 24) fp64: estimate_chroma of the window's notes, cut at its end; spans (S, 4) int32).
    labels=True (every window must last the same W ticks - one tempo - else ValueError; W <= 32768) adds rhythm, note_density (S, 4 * bps) uint8 - cells
    [0, 4 * bps) of event_attributes(tokens, want_cells=True, grid=EventGrid(shift_lo, n_shift, W, 4 * bps, 4)) - and r_density (the share of 1s in rhythm),
    n_density (the mean of note_density), fp64, as datasets._densities computes them (ptb_v2.py:421-422): the arrays YamahaDataset takes.
    Not kept from process_data: the len(np.unique(ms)) > 2 filter and the 75 % filter (they need a velocity roll), and pretty_midi's estimated beats
    (the beats here are the file's own quarter notes)."""
    v, _ = _note_vocab(vocab)
    bps, steps = _int("beats_per_segment", beats_per_segment, 1, 65), _int("max_tokens", max_tokens, 1, 1025)
    if not isinstance(labels, (bool, np.bool_)):
        raise ValueError("labels: a bool, got %r" % (labels,))
    if not isinstance(midi, MidiNotes) or not torch.is_tensor(midi.notes) or midi.notes.dtype != torch.int32 or midi.notes.dim() != 2 or midi.notes.shape[1] != 4:
        raise ValueError("midi: MidiNotes with notes (N, 4) int32, got %s" % (_what(midi.notes) if isinstance(midi, MidiNotes) else type(midi).__name__))
    beats = midi.beats.detach().cpu().to(torch.int64)
    S = (beats.numel() - 1) // bps
    if beats.dim() != 1 or S < 1:
        raise ValueError("midi: not one whole window of %d beats (%d beats)" % (bps, beats.numel()))
    bounds = beats[:S * bps + 1:bps].contiguous()
    if bool((bounds[1:] <= bounds[:-1]).any()):
        raise ValueError("midi.beats: ascending ticks")
    if labels:
        W = int(bounds[1] - bounds[0])
        if bool((bounds[1:] - bounds[:-1] != W).any()) or W > 32768:
            raise ValueError("labels=True: every window must last the same number of ticks, at most 32768 (one tempo); got %s" % sorted(
                set((bounds[1:] - bounds[:-1]).tolist()))[:4])
    dev = torch.device(device) if device is not None else midi.notes.device if (ops is not None or midi.notes.is_cuda) else torch.device("cuda")
    notes = midi.notes.to(dev)
    t0 = notes[:, 0].contiguous()
    if notes.shape[0] > 1 and bool((t0[1:] < t0[:-1]).any()):
        raise ValueError("midi.notes: sorted by t0")
    edge = torch.searchsorted(t0, bounds.to(dev).to(torch.int32))
    lo, hi = bounds[:-1].to(dev), bounds[1:].to(dev)
    spans = torch.stack([edge[:-1], edge[1:] - edge[:-1], lo, hi], 1).to(torch.int32)
    tokens, n_tokens, n_kept, status = notes_to_tokens(notes, spans, steps=steps, add_eos=True, eos=1, pad=0, vocab=v, ops=ops)
    first = tokens[:, 0]
    keep = (status == 0) & ~((first >= v.shift_lo) & (first < v.shift_lo + v.n_shift))
    # the window of every note, its length inside it, and the histogram per window
    j = torch.searchsorted(bounds.to(dev), notes[:, 0].to(torch.int64), right=True) - 1
    inside = (j >= 0) & (j < S)
    jc = j.clamp(0, S - 1)
    w = ((torch.minimum(notes[:, 1].to(torch.int64), hi[jc]) - notes[:, 0]).clamp(min=0) * inside).to(torch.float64)
    pc = (notes[:, 2].to(torch.int64) + v.midi_lo).remainder(12)
    hist = torch.zeros(S * 12, dtype=torch.float64, device=dev).scatter_add_(0, jc * 12 + pc, w).view(S, 12)
    out = dict(tokens=tokens.to(torch.float32), n_tokens=n_tokens, status=status, keep=keep, chroma=chroma_of_histogram(hist), spans=spans)
    if labels:
        cells = 4 * bps
        at = event_attributes(tokens, eos=1, vocab=EventVocab(v.on_lo, v.off_lo, v.n_pitch), grid=EventGrid(v.shift_lo, v.n_shift, W, cells, 4),
                              want_cells=True, ops=ops)
        rhythm, dens = (torch.nn.functional.pad(c, (0, max(0, cells - c.shape[1])))[:, :cells] for c in (at.rhythm, at.notes))
        out.update(rhythm=rhythm, note_density=dens, r_density=(rhythm == 1).to(torch.float64).mean(1), n_density=dens.to(torch.float64).mean(1))
    return out
