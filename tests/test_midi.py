"""Standard MIDI Files (midi.py), CPU side: write_midi -> read_midi gives the notes back, read_midi on byte strings built here (two tracks with a tempo
change, running status, velocity-0 note-offs, sysex and unknown meta events, channel 10, a pitch outside the vocabulary, a note never closed, a
zero-length note) against ticks computed by hand, every malformed file as ValueError, the beats at one tempo and across a tempo change, estimate_chroma
against a numpy restatement, and midi_segments over stand-in ops."""
import io
from collections import Counter

import numpy as np
import pytest
import torch

import helpers_attributes as ha
import helpers_notes as hn
from mfn_import import load_package


def vl(n):
    out = [n & 0x7F]
    while n > 0x7F:
        n >>= 7
        out.append(0x80 | (n & 0x7F))
    return bytes(reversed(out))


def header(fmt, ntrks, division):
    return b"MThd" + (6).to_bytes(4, "big") + fmt.to_bytes(2, "big") + ntrks.to_bytes(2, "big") + division.to_bytes(2, "big")


def track(*events, end=0):
    """events: (delta, bytes); the end of the track `end` ticks after the last"""
    body = b"".join(vl(d) + bytes(e) for d, e in events) + vl(end) + b"\xff\x2f\x00"
    return b"MTrk" + len(body).to_bytes(4, "big") + body


def tempo(us):
    return b"\xff\x51\x03" + us.to_bytes(3, "big")


def _read(pkg, data, **kw):
    return pkg.read_midi(io.BytesIO(data), **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the file codec
# ------------------------------------------------------------------------------------------------------------------------------
def test_write_then_read_gives_the_notes_back(tmp_path):
    pkg = load_package()
    T = hn.MAX_TICK
    notes = np.array([(0, 1, 0, 1), (0, T, 87, 127), (5, 6, 40, 64), (5, 700, 41, 100), (T - 1, T, 0, 2), (300, 300 + 16384, 12, 99)], np.int32)
    order = np.lexsort((notes[:, 2], notes[:, 0]))
    path = str(tmp_path / "a.mid")
    pkg.write_midi(path, notes[::-1].copy())                                  # any order in
    m = pkg.read_midi(path)
    assert m.notes.dtype == torch.int32 and np.array_equal(m.notes.numpy(), notes[order]) and m.n_dropped == 0
    assert m.beats[0] == 0 and m.beats.tolist() == list(range(0, T + 1, 50))   # 120 qpm: a beat is 50 ticks; the last event is at T
    data = open(path, "rb").read()
    assert data[:14] == header(0, 1, 50) and data[14:18] == b"MTrk" and data[22:29] == b"\x00" + tempo(500000) and data[-4:] == b"\x00\xff\x2f\x00"
    assert data.count(b"\xff\x51") == 1
    # a tensor with n_notes, a file object, another tempo, a vocabulary with another lowest pitch
    f = io.BytesIO()
    pkg.write_midi(f, torch.from_numpy(notes[order]), n_notes=3, qpm=100, vocab=pkg.NoteVocab(midi_lo=30))
    assert f.getvalue()[12:14] == (60).to_bytes(2, "big")                      # 600000 us per quarter: division 60, one MIDI tick per 10 ms
    back = _read(pkg, f.getvalue(), vocab=pkg.NoteVocab(midi_lo=30))
    assert np.array_equal(back.notes.numpy(), notes[order][:3]) and back.beats[:3].tolist() == [0, 60, 120]
    for bad in (dict(qpm=97), dict(qpm=0), dict(qpm="120")):
        with pytest.raises(ValueError):
            pkg.write_midi(io.BytesIO(), notes, **bad)
    for bad in ([(0, 0, 1, 64)], [(0, 5, 88, 64)], [(0, 5, 1, 0)], [(0, 5, 1, 128)], [(-1, 5, 1, 64)], np.zeros((2, 3), np.int32), np.zeros((2, 4))):
        with pytest.raises(ValueError):
            pkg.write_midi(io.BytesIO(), np.asarray(bad))


def test_two_tracks_and_a_tempo_change_in_the_first_that_moves_the_notes_of_the_second():
    pkg = load_package()
    # division 480.  Track 0: 120 qpm, and from tick 960 (1 s) 60 qpm.  Track 1: a note over ticks 480-960 (0.5 s - 1 s) and one over 1440-1920:
    # 960 ticks at 500000 us = 1 s, then 480 and 960 ticks at 1000000 us = 1 s and 2 s more
    second = track((480, [0x90, 60, 80]), (480, [0x80, 60, 0]), (480, [0x90, 62, 90]), (480, [0x80, 62, 64]))
    m = _read(pkg, header(1, 2, 480) + track((0, tempo(500000)), (960, tempo(1000000))) + second)
    assert m.notes.tolist() == [[50, 100, 39, 80], [200, 300, 41, 90]] and m.n_dropped == 0
    assert m.beats.tolist() == [0, 50, 100, 200, 300]                         # the quarter notes 0 ... 4 through the same map
    # without the change the second note sits at 1.5 s - 2 s
    one = _read(pkg, header(1, 2, 480) + track((0, tempo(500000))) + second)
    assert one.notes.tolist() == [[50, 100, 39, 80], [150, 200, 41, 90]] and one.beats.tolist() == [0, 50, 100, 150, 200]
    # no tempo event at all: 120 qpm; and the change in the SECOND track moves the notes as well
    assert _read(pkg, header(0, 1, 480) + second).notes.tolist() == one.notes.tolist()
    late = _read(pkg, header(1, 2, 480) + second + track((960, tempo(1000000))))
    assert late.notes.tolist() == m.notes.tolist()


def test_running_status_velocity_0_sysex_and_unknown_meta_events():
    pkg = load_package()
    data = header(0, 1, 100) + track(                                          # division 100 at 120 qpm: a MIDI tick is 5 ms
        (0, [0x90, 60, 64]), (20, [61, 70]),                                   # running status: a second note-on at 100 ms
        (0, [0xF0, 3, 1, 2, 0xF7]), (20, [0xFF, 0x7E, 2, 9, 9]),               # a sysex and an unknown meta event, skipped by their lengths
        (0, [0x90, 60, 0]), (40, [61, 0]),                                     # velocity 0: note-offs at 200 ms and 400 ms (the second by running status)
        (0, [0xB0, 64, 127]), (0, [0xC0, 5]), (0, [0xE0, 0, 64]), (10, [0xD0, 3]))
    m = _read(pkg, data)
    assert m.notes.tolist() == [[0, 20, 39, 64], [10, 40, 40, 70]]
    # half a tick of 10 ms rounds up: MIDI tick 1 = 5 ms -> 1, and a note of 5 ms quantised to nothing gets length 1
    m = _read(pkg, header(0, 1, 100) + track((1, [0x90, 60, 64]), (1, [0x80, 60, 0]), (1, [0x90, 62, 64]), (4, [0x80, 62, 0])))
    assert m.notes.tolist() == [[1, 2, 39, 64], [2, 4, 41, 64]]


def test_channel_10_a_pitch_outside_the_vocabulary_an_open_note_and_a_zero_length_note():
    pkg = load_package()
    data = header(0, 1, 50) + track(
        (0, [0x99, 40, 100]), (0, [0x90, 20, 100]), (0, [0x90, 109, 100]), (0, [0x90, 21, 1]), (0, [0x91, 108, 127]),
        (10, [0x89, 40, 0]), (0, [0x80, 20, 0]), (0, [0x80, 109, 0]), (0, [0x80, 21, 0]),
        (5, [0x90, 64, 50]), (0, [0x80, 64, 0]),                               # a zero-length note at 15: length 1
        (5, [0x80, 70, 0]),                                                    # a note-off without a note-on
        (0, [0x90, 72, 60]), (10, [0x90, 72, 61]), (10, [0x80, 72, 0]),        # two note-ons of one pitch: the note-off closes the OLDEST
        end=30)                                                                # ... and the other, like the one on channel 2, closes at the last event: 70
    m = _read(pkg, data)
    assert m.notes.tolist() == [[0, 10, 0, 1], [0, 70, 87, 127], [15, 16, 43, 50], [20, 40, 51, 60], [30, 70, 51, 61]] and m.n_dropped == 3
    d = _read(pkg, data, drums=True)
    assert d.n_dropped == 2 and [0, 10, 19, 100] in d.notes.tolist() and len(d.notes) == 6
    assert m.beats.tolist() == [0, 50]                                         # the last event is at tick 70


def test_malformed_files_raise_value_error():
    pkg = load_package()
    good = header(0, 1, 480) + track((0, [0x90, 60, 64]), (10, [0x80, 60, 0]))
    assert len(_read(pkg, good).notes) == 1
    bad = dict(
        smpte=header(0, 1, 0xE728) + good[14:],
        zero_division=header(0, 1, 0) + good[14:],
        chunk_tag=good[:14] + b"MTrx" + good[18:],
        not_midi=b"RIFF" + good[4:],
        empty=b"",
        short_header=good[:10],
        format_2=header(2, 1, 480) + good[14:],
        missing_track=header(1, 2, 480) + good[14:],
        ends_inside_a_chunk=good[:-3],
        ends_inside_an_event=header(0, 1, 480) + b"MTrk" + (3).to_bytes(4, "big") + b"\x00\x90\x3c",
        ends_inside_a_delta=header(0, 1, 480) + b"MTrk" + (1).to_bytes(4, "big") + b"\x81",
        meta_longer_than_the_chunk=header(0, 1, 480) + b"MTrk" + (4).to_bytes(4, "big") + b"\x00\xff\x01\x7f",
        data_byte_without_status=header(0, 1, 480) + track((0, [60, 64])),
        real_time_status=header(0, 1, 480) + track((0, [0xF8])),
        tempo_of_two_bytes=header(0, 1, 480) + track((0, [0xFF, 0x51, 2, 1, 2])),
        long_delta=header(0, 1, 480) + b"MTrk" + (8).to_bytes(4, "big") + b"\x81\x81\x81\x81\x01\x90\x3c\x40",
    )
    for name, data in bad.items():
        with pytest.raises(ValueError):
            _read(pkg, data)
    for kw in (dict(vocab=None), dict(vocab=pkg.NoteVocab(midi_lo=60)), dict(drums=1)):
        with pytest.raises(ValueError):
            _read(pkg, good, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. estimate_chroma
# ------------------------------------------------------------------------------------------------------------------------------
def _chroma_np(hist, one_hot=False):
    """the restatement: np.corrcoef against the 24 rotated profiles"""
    from music_fader_nets_amd.notes import KK_MAJOR, KK_MINOR
    out = np.zeros(24)
    if hist.std() == 0:
        return out
    for minor, prof in enumerate((KK_MAJOR, KK_MINOR)):
        for k in range(12):
            out[k + 12 * minor] = np.corrcoef(hist, np.roll(np.array(prof, np.float64), k))[0, 1]
    if one_hot:
        return np.eye(24)[int(np.argmax(out))]
    return np.where(out < 0.1, 0.0, out)


def _notes_of_histogram(hist):
    """a note per pitch class c whose length is hist[c]: pitch (c - 21) % 12 is class c with midi_lo 21"""
    return np.array([(7 * c, 7 * c + int(h), (c - 21) % 12 + 12 * (c % 3), 80) for c, h in enumerate(hist)], np.int32)


def test_estimate_chroma():
    pkg = load_package()
    from music_fader_nets_amd.notes import KK_MAJOR, KK_MINOR
    for minor, prof in enumerate((KK_MAJOR, KK_MINOR)):
        for k in range(12):
            hist = np.roll(np.round(np.array(prof) * 100).astype(int), k)
            notes = torch.from_numpy(_notes_of_histogram(hist))
            c = pkg.estimate_chroma(notes)
            assert c.dtype == torch.float64 and c.shape == (24,) and int(c.argmax()) == k + 12 * minor and abs(float(c.max()) - 1.0) < 1e-12
            assert pkg.estimate_chroma(notes, one_hot=True).tolist() == np.eye(24)[k + 12 * minor].tolist()
    rs = np.random.RandomState(3)
    hists = rs.randint(0, 1000, (40, 12))
    hists[5:8, rs.randint(0, 12, 6)] = 0
    batch = torch.from_numpy(np.stack([_notes_of_histogram(h) for h in hists]))
    for one_hot in (False, True):
        got = pkg.estimate_chroma(batch, one_hot=one_hot).numpy()
        ref = np.stack([_chroma_np(h.astype(np.float64), one_hot) for h in hists])
        assert got.shape == (40, 24) and np.abs(got - ref).max() <= 1e-12      # fp64 sums of 12 terms of magnitude below 10 (after the division)
    assert (got.sum(1) == 1).all() and ((pkg.estimate_chroma(batch).numpy() == 0) | (pkg.estimate_chroma(batch).numpy() >= 0.1)).all()
    # n_notes cuts the rows in use; nothing in use, no notes at all and a flat histogram give zeros
    n = torch.tensor([12] * 39 + [0], dtype=torch.int32)
    cut = pkg.estimate_chroma(batch, n_notes=n)
    assert torch.equal(cut[:39], pkg.estimate_chroma(batch)[:39]) and not cut[39].any()
    assert not pkg.estimate_chroma(torch.zeros(0, 4, dtype=torch.int32)).any() and not pkg.estimate_chroma(batch, n_notes=n, one_hot=True)[39].any()
    assert not pkg.estimate_chroma(torch.from_numpy(_notes_of_histogram([5] * 12))).any()
    for bad in (dict(notes=torch.zeros(3, 5, dtype=torch.int32)), dict(notes=torch.zeros(3, 4)), dict(notes=batch, n_notes=n[:3]), dict(notes=batch, one_hot=1),
                dict(notes=batch, vocab=(1, 2))):
        with pytest.raises(ValueError):
            pkg.estimate_chroma(**bad)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. midi_segments over stand-in ops
# ------------------------------------------------------------------------------------------------------------------------------
def test_midi_segments_on_stand_ins():
    pkg = load_package()
    f = io.BytesIO()
    pkg.write_midi(f, hn.piece())
    midi = _read(pkg, f.getvalue())
    assert midi.beats.tolist() == list(range(0, 651, 50)) and len(midi.notes) == 20
    ops = hn.notes_fake_ops()
    seg = pkg.midi_segments(midi, max_tokens=20, ops=ops)
    assert ops.calls == ["tokens_from_notes"]                                  # ONE call for the piece
    assert seg["spans"].tolist() == [[0, 5, 0, 200], [5, 2, 200, 400], [7, 12, 400, 600]] and torch.equal(ops.last_spans, seg["spans"])
    assert seg["tokens"].dtype == torch.float32 and seg["tokens"].shape == (3, 20)
    ref = hn.tokens_from_notes_ref(midi.notes.numpy(), seg["spans"].numpy(), 20, hn.DEFAULT, hn.tokens_of)
    assert np.array_equal(seg["tokens"].numpy(), ref["tokens"].astype(np.float32)) and np.array_equal(seg["n_tokens"].numpy(), ref["n_tokens"])
    assert seg["status"].tolist() == [0, 0, hn.OVERFLOW] and seg["n_tokens"].tolist()[:2] == [18, 9] and seg["n_tokens"][2] > 20
    assert seg["keep"].tolist() == [True, False, False]                        # window 1 begins with a time shift, window 2 does not fit
    for j, (lo, hi) in enumerate(((0, 200), (200, 400), (400, 600))):
        inside = [(t0, min(t1, hi), p, v) for t0, t1, p, v in midi.notes.tolist() if lo <= t0 < hi]
        own = pkg.estimate_chroma(torch.tensor(inside, dtype=torch.int32))          # the same histogram; a batched product may round differently
        assert float((seg["chroma"][j] - own).abs().max()) <= 1e-12 and bool(own.any()), j
    # labels: the cells of event_attributes on the 16-cell grid of the window
    ops = hn.notes_fake_ops()
    lab = pkg.midi_segments(midi, max_tokens=100, labels=True, ops=ops)
    assert ops.calls == ["tokens_from_notes", "event_attributes"] and lab["keep"].tolist() == [True, False, True]
    p = dict(ha.DEFAULT, ticks_num=200, ticks_den=16, beat_cells=4)
    for j in range(3):
        a = ha.attributes_sets(lab["tokens"][j].numpy().astype(np.int32), p)
        assert lab["rhythm"].shape == (3, 16) and np.array_equal(lab["rhythm"][j].numpy(), a["rhythm"][:16]), j
        assert np.array_equal(lab["note_density"][j].numpy(), a["notes"][:16]) and a["status"] == 0
        assert float(lab["r_density"][j]) == Counter(a["rhythm"][:16].tolist())[1] / 16 and float(lab["n_density"][j]) == sum(a["notes"][:16].tolist()) / 16
    assert lab["rhythm"][0].tolist() == [1, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 2]
    # other window lengths; two tempi only without labels
    assert pkg.midi_segments(midi, beats_per_segment=6, ops=ops)["spans"].tolist() == [[0, 6, 0, 300], [6, 13, 300, 600]]
    two = midi._replace(beats=torch.tensor([0, 50, 100, 150, 200, 260, 320, 380, 440], dtype=torch.int32))
    assert pkg.midi_segments(two, ops=ops)["spans"][:, 2:].tolist() == [[0, 200], [200, 440]]
    calls = list(ops.calls)
    with pytest.raises(ValueError):
        pkg.midi_segments(two, labels=True, ops=ops)
    for kw in (dict(beats_per_segment=0), dict(max_tokens=1025), dict(max_tokens=0), dict(labels=1), dict(vocab=None), dict(beats_per_segment=14)):
        with pytest.raises(ValueError):
            pkg.midi_segments(midi, ops=ops, **kw)
    for bad in (None, midi.notes, midi._replace(notes=midi.notes.long()), midi._replace(notes=midi.notes.flip(0)), midi._replace(beats=midi.beats.flip(0))):
        with pytest.raises(ValueError):
            pkg.midi_segments(bad, ops=ops)
    assert ops.calls == calls                                                  # every ValueError came before a launch
