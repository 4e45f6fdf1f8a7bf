"""Whole-piece transfer: a .mid in, the same piece with its faders moved out.  The reference's notebook (arousal_transfer.ipynb cells 11, 15, 17) moves
one 4-beat window; here every window of a piece is one row of ONE encode and every (window, amount) pair one row of ONE decode, and stitch_notes
(fn_notes_stitch) puts the decoded windows back at their places - ours, the reference stops at the window.  The windows that cannot be transferred
(they do not fit the tokeniser's row, they are empty, their decode sounds nothing) pass the source through, so the output covers the whole file."""
import argparse
import collections
import os

import numpy as np
import torch

from .constrain import _int
from .decode import _check_beam, _decode_rows, fader_latents
from .midi import MidiNotes, _timing, midi_bytes, midi_segments, read_midi, _put
from .notes import CLIP, FIT, MAX_TICK, PASS, STITCH_MAX_V, stitch_notes, tokens_to_notes

Transferred = collections.namedtuple("Transferred", ["notes", "n_notes", "win_first", "status", "used", "tokens"])
Transferred.__doc__ = """notes (V, out_ld, 4) int32 rows of (t0, t1, pitch, vel) in ticks of 10 ms, zeros behind n_notes; n_notes (V,) int32; win_first
(V, S + 2) int32: the notes in front of window j, of the tail (at S) and the total (at S + 1); status (V,) int32; used (S, V) bool: the window holds
the decode (False: the source passed through); tokens (S, V, steps) int32, the decode of every window.  Device tensors."""
FITS = {"clip": CLIP, "scale": FIT}


def _amounts(lmbda):
    """lmbda -> the V amounts as a list of floats"""
    seq = [lmbda] if isinstance(lmbda, (int, float, np.integer, np.floating)) and not isinstance(lmbda, (bool, np.bool_)) else lmbda
    try:
        seq = list(seq)
    except TypeError:
        raise ValueError("lmbda: a number or a sequence of 1..%d numbers, got %r" % (STITCH_MAX_V, lmbda))
    if not 1 <= len(seq) <= STITCH_MAX_V or not all(
            isinstance(a, (int, float, np.integer, np.floating)) and not isinstance(a, (bool, np.bool_)) and np.isfinite(a) for a in seq):
        raise ValueError("lmbda: a finite number or a sequence of 1..%d of them, got %r" % (STITCH_MAX_V, lmbda))
    return [float(a) for a in seq]


@torch.no_grad()
def transfer_piece(model, midi, lmbda=1.0, curve=None, which="both", mode="shift", fit="clip", steps=None, beats_per_segment=4, max_tokens=100,
                   only_kept=False, eps=None, sample=None, beam=None, constraints=None):
    """One piece through the faders of a GM-VAE, window by window, in one batch.

    midi       MidiNotes (read_midi).  It is cut into S windows of `beats_per_segment` beats and tokenised to `max_tokens` columns by midi_segments.
    lmbda      a number, or a sequence of V amounts: V pieces.  curve: None or S numbers, a multiplier per window - the amount of window j in piece v
               is lmbda[v] * curve[j]: fader automation across the piece.  Negative amounts go from high to low.
    which, mode  fader_sweep's: mode="shift" adds amount * (mu_lookup[1] - mu_lookup[0]) to z_r, z_n or both; mode="set" sets z_which[0].
    fit        "clip": a decoded window is cut at its window's length; "scale": a decode that runs longer is first scaled down to it.
    steps      the tokens decoded per window (None: max_tokens).  only_kept: transfer only the windows midi_segments marks `keep`
               (False: every window of status 0).
    eps        (eps_r, eps_n), each (S, Z) or (S, V, Z); None: drawn here.  sample, beam, constraints: as fader_sweep takes them (a per-row bias has
               S * V rows).

    A window that is not transferred, and one whose decode holds no note, passes its source notes through; the choice is made on the device.  The
    notes behind the last whole window pass through by one more span (it reaches 2^22 ticks past that window).
    -> Transferred(notes, n_notes, win_first, status, used, tokens).  One midi_segments, one encode of S rows, one decode of S * V rows, one
    tokens_to_notes and one stitch_notes; nothing is copied to the host here (midi_segments looks once whether the notes are sorted).
    ValueError for anything that is not as described, before anything is launched."""
    if which not in ("r", "n", "both") or mode not in ("set", "shift") or (which == "both" and mode == "set"):
        raise ValueError("which in {r, n, both}, mode in {set, shift}; 'both' only with mode='shift'")
    if fit not in FITS:
        raise ValueError("fit: 'clip' or 'scale', got %r" % (fit,))
    if not isinstance(only_kept, (bool, np.bool_)):
        raise ValueError("only_kept: a bool, got %r" % (only_kept,))
    amounts = _amounts(lmbda)
    V = len(amounts)
    bps, max_tokens = _int("beats_per_segment", beats_per_segment, 1, 65), _int("max_tokens", max_tokens, 1, 1025)
    steps = max_tokens if steps is None else _int("steps", steps, 1, 1025)
    if not isinstance(midi, MidiNotes) or not torch.is_tensor(midi.beats) or midi.beats.dim() != 1:
        raise ValueError("midi: MidiNotes (read_midi), got %s" % type(midi).__name__)
    S = (midi.beats.numel() - 1) // bps
    if S < 1:
        raise ValueError("midi: not one whole window of %d beats (%d beats)" % (bps, midi.beats.numel()))
    if curve is None:
        curve = np.ones(S)
    try:
        curve = np.asarray(curve, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("curve: %d numbers, one per window, got %r" % (S, curve))
    if curve.shape != (S,) or not np.isfinite(curve).all():
        raise ValueError("curve: %d finite numbers, one per window, got shape %s" % (S, curve.shape))
    if eps is not None and (len(eps) != 2 or not all(torch.is_tensor(e) and e.dim() in (2, 3) and e.shape[0] == S and (e.dim() == 2 or e.shape[1] == V)
                                                    for e in eps) or eps[0].dim() != eps[1].dim()):
        raise ValueError("eps: (eps_r, eps_n), each (%d, Z) or (%d, %d, Z)" % (S, S, V))
    _check_beam(steps, None, sample, beam)
    was_training = model.training
    model.eval()
    try:
        ops, dev = model.engine().ops, model._device()
        seg = midi_segments(midi, bps, max_tokens, ops=ops, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        dis_r, dis_n = model.encode(seg["tokens"].to(torch.int32))
        amt = torch.tensor(curve, dtype=torch.float32, device=dev).view(S, 1) * torch.tensor(amounts, dtype=torch.float32, device=dev).view(1, V)
        zr, zn, _ = fader_latents(model, dis_r, dis_n, amt, eps, which, mode)
        c = seg["chroma"].float().unsqueeze(1).expand(S, V, seg["chroma"].shape[-1])
        tokens = _decode_rows(model, torch.cat([zr, zn, c], dim=2).reshape(S * V, -1), steps, None, sample, beam, constraints).view(S, V, steps)
        # one more row of pad tokens and one more span: the tail behind the last whole window
        dec = tokens_to_notes(torch.cat([tokens, torch.zeros(1, V, steps, **i32)]), ops=ops)
        src, spans = midi.notes.to(dev), seg["spans"]
        first = spans[-1, 0] + spans[-1, 1]
        end = spans[-1, 3].to(torch.int64)
        tail = torch.stack([first, src.shape[0] - first, spans[-1, 3], (end + MAX_TICK).clamp(max=2**31 - 1).to(torch.int32)]).to(torch.int32).view(1, 4)
        ok = seg["keep"] if only_kept else seg["status"] == 0
        used = ok.view(S, 1) & (dec.n_notes[:S] > 0)
        how = torch.where(used, torch.full((S, V), FITS[fit], **i32), torch.full((S, V), PASS, **i32))
        piece = stitch_notes(dec, src, torch.cat([spans, tail]), torch.cat([how, torch.full((1, V), PASS, **i32)]), ops=ops)
        return Transferred(piece.notes, piece.n_notes, piece.win_first, piece.status, used, tokens)
    finally:
        model.train(was_training)


def _destinations(dst, V):
    if V == 1 and isinstance(dst, (str, os.PathLike)):
        return None, [os.fspath(dst)]
    if isinstance(dst, (str, os.PathLike)):
        return os.fspath(dst), [os.path.join(os.fspath(dst), "%02d.mid" % v) for v in range(V)]
    paths = list(dst) if isinstance(dst, (list, tuple)) else None
    if paths is None or len(paths) != V or not all(isinstance(p, (str, os.PathLike)) and os.fspath(p) for p in paths):
        raise ValueError("dst: %s, got %r" % ("a path" if V == 1 else "a directory or a list of %d paths" % V, dst))
    return None, [os.fspath(p) for p in paths]


def transfer_midi(model, src, dst, qpm=120, **transfer):
    """A file through transfer_piece: read_midi(src), the transfer, ONE copy to the host, then a file per amount.

    dst        a path when lmbda is one amount; otherwise a directory (00.mid, 01.mid ... are written into it) or a list of V paths.
    qpm        the tempo written (write_midi's).  transfer: the keywords of transfer_piece.
    -> the paths written."""
    _timing(qpm)
    V = len(_amounts(transfer.get("lmbda", 1.0)))
    folder, paths = _destinations(dst, V)
    res = transfer_piece(model, read_midi(src), **transfer)
    out_ld = res.notes.shape[1]
    host = torch.cat([res.notes.reshape(V, out_ld * 4), res.n_notes.view(V, 1)], 1).cpu().numpy()
    if folder is not None:
        os.makedirs(folder, exist_ok=True)
    for v, path in enumerate(paths):
        _put(path, midi_bytes(host[v, :out_ld * 4].reshape(out_ld, 4)[:host[v, -1]], qpm=qpm))
    return paths


def main(argv=None):
    """``python transfer_midi.py --config gmm_model_config.json [--params model.pt] in.mid out.mid``"""
    from .gmm_model import MusicAttrRegGMVAE
    from .train import CHROMA_DIMS, EVENT_DIMS, NOTE_DIMS, RHYTHM_DIMS, read_config
    ap = argparse.ArgumentParser(prog="transfer_midi", description="move the arousal faders of a whole MIDI file with a trained GM-VAE")
    ap.add_argument("--config", required=True, help="the reference's JSON config (gmm_model_config.json)")
    ap.add_argument("--params", help="a state_dict saved by the trainer; without it seeded initial weights are used (a smoke path)")
    ap.add_argument("src", metavar="in.mid")
    ap.add_argument("dst", metavar="out.mid")
    ap.add_argument("--lmbda", type=float, default=1.0, help="how far the latents move along the low-to-high direction (default 1.0)")
    ap.add_argument("--high-to-low", action="store_true", help="move the other way (the amount is negated)")
    ap.add_argument("--fit", choices=sorted(FITS), default="clip", help="cut a decoded window at its length, or scale a longer one down to it")
    ap.add_argument("--temperature", type=float, default=None, help="sample the decode at this temperature (default: greedy)")
    ap.add_argument("--seed", type=int, default=0, help="the seed of the sampled decode and of the initial weights")
    ap.add_argument("--beam", type=int, default=None, help="beam search of this width (not with --temperature)")
    opts = ap.parse_args(argv)
    if opts.beam is not None and opts.temperature is not None:
        raise SystemExit("transfer_midi: --beam goes without --temperature")
    args = read_config(opts.config, "gmm")
    if not torch.cuda.is_available():
        raise SystemExit("transfer_midi: no GPU visible - this package runs on the MI355X HIP kernels only (there is deliberately no CPU fallback)")
    torch.manual_seed(opts.seed)
    model = MusicAttrRegGMVAE(roll_dims=EVENT_DIMS, rhythm_dims=RHYTHM_DIMS, note_dims=NOTE_DIMS, chroma_dims=CHROMA_DIMS, hidden_dims=args["hidden_dim"],
                              z_dims=args["z_dim"], n_step=args["time_step"], n_component=args["num_clusters"])
    if opts.params:
        model.load_state_dict(torch.load(opts.params, map_location="cpu"))
    else:
        print("transfer_midi: no --params given - seeded initial weights (seed %d), the output shows the path and not a model" % opts.seed)
    model = model.cuda()
    kw = dict(lmbda=-opts.lmbda if opts.high_to_low else opts.lmbda, fit=opts.fit)
    if opts.temperature is not None:
        kw["sample"] = dict(temperature=opts.temperature, seed=opts.seed)
    if opts.beam is not None:
        kw["beam"] = dict(width=opts.beam, eos=1)
    paths = transfer_midi(model, opts.src, opts.dst, **kw)
    print("transfer_midi: %s -> %s" % (opts.src, paths[0]))
