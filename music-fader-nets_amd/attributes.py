"""Controllability metrics behind the decode: rhythm density and note density of decoded event tokens, and the consistency / restrictiveness /
monotonicity of a fader sweep (BaseEvaluator.evaluate, test_class.py:79-194), on the device next to the decode that feeds them - fn_event_attributes
and fn_sweep_scores (include/fadernets.h has the definition).  The reference measures through a MIDI file on disk; its piano-roll fill, attributes and
scores are kept, the step from tokens to timed notes is ours (Magenta's performance decoder was not at hand), and the beat grid is fixed to a first beat
at 0 and 120 qpm where pretty_midi estimates it."""
import collections

import numpy as np
import torch

from . import _lib
from .constrain import MAX_PITCH, EventVocab, _int
from .decode import fader_sweep
from .engine import E_VOCAB

EventGrid = collections.namedtuple("EventGrid", ["shift_lo", "n_shift", "ticks_num", "ticks_den", "beat_cells"], defaults=(178, 100, 25, 2, 4))
EventGrid.__doc__ = """Time in the token vocabulary and on the grid: token shift_lo + k moves the clock by k + 1 ticks of 10 ms (k < n_shift; the default
178-277 follows the reference's trainer_glsr.py:125,133), one cell is ticks_num / ticks_den ticks (25/2: sixteenth notes at 120 qpm), beat_cells cells
make a beat (the grid ends on a whole beat)."""
EventAttributes = collections.namedtuple("EventAttributes", ["r_density", "n_density", "c_r", "c_n", "n_cells", "status"])
EventAttributesCells = collections.namedtuple("EventAttributesCells", EventAttributes._fields + ("rhythm", "notes"))
MAX_STEPS, MAX_CELLS, MAX_SAMPLES = _lib.FN_ATTR_MAX_STEPS, _lib.FN_ATTR_MAX_CELLS, _lib.FN_ATTR_MAX_SAMPLES
EMPTY, OVERFLOW = _lib.FN_ATTR_EMPTY, _lib.FN_ATTR_OVERFLOW
PARAMS_DTYPE = np.dtype([(k, "<i4") for k in ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "ticks_num", "ticks_den", "beat_cells",
                                              "vocab_size")] + [("reserved", "<i4", (2,))])          # FnAttrParams
SCORES = ("consistency", "restrictiveness", "monotonicity", "variance")


def _attr_params(eos, vocab, grid):
    """the checked arguments -> (the 48 bytes of FnAttrParams as a CPU uint8 tensor, EventGrid); ValueError in the style of Constraints"""
    V = E_VOCAB
    eos = -1 if eos is None else _int("eos", eos, 0, V)
    try:
        on_lo, off_lo, n_pitch = vocab
    except (TypeError, ValueError):
        raise ValueError("vocab: EventVocab(on_lo, off_lo, n_pitch), got %r" % (vocab,))
    try:
        shift_lo, n_shift, num, den, bc = grid
    except (TypeError, ValueError):
        raise ValueError("grid: EventGrid(shift_lo, n_shift, ticks_num, ticks_den, beat_cells), got %r" % (grid,))
    n = _int("vocab.n_pitch", n_pitch, 1, MAX_PITCH + 1)
    on, off = _int("vocab.on_lo", on_lo, 0, V + 1), _int("vocab.off_lo", off_lo, 0, V + 1)
    ns, sh = _int("grid.n_shift", n_shift, 1, 4096 + 1), _int("grid.shift_lo", shift_lo, 0, V + 1)
    num, den, bc = _int("grid.ticks_num", num, 1, 32768 + 1), _int("grid.ticks_den", den, 1, 256 + 1), _int("grid.beat_cells", bc, 1, 64 + 1)
    ranges = sorted([(on, on + n, "note-on"), (off, off + n, "note-off"), (sh, sh + ns, "time-shift")])
    if ranges[-1][1] > V:
        raise ValueError("vocab / grid: the token ranges lie inside [0, %d), got %r" % (V, ranges))
    for (_, hi, a), (lo, _, b) in zip(ranges, ranges[1:]):
        if lo < hi:
            raise ValueError("vocab / grid: the %s and %s ranges are disjoint, got %r" % (a, b, ranges))
    if eos >= 0 and any(lo <= eos < hi for lo, hi, _ in ranges):
        raise ValueError("eos: outside the note and time-shift ranges, got %d" % eos)
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    for k, v in zip(PARAMS_DTYPE.names, (on, off, n, sh, ns, eos, num, den, bc, V)):
        raw[k] = v
    return torch.from_numpy(raw.view(np.uint8).copy()), EventGrid(sh, ns, num, den, bc)


def _ops_of(t, ops=None):
    if ops is not None:
        return ops
    from .hipops import HipOps
    return HipOps(t.device)


def event_attributes(tokens, eos=1, vocab=EventVocab(2, 90, 88), grid=EventGrid(), want_cells=False, ops=None):
    """Rhythm density, note density and their classes (get_classes, test_class.py:59-70) of event-token rows.

    tokens      (rows, steps) or (n, V, steps) int32 on the device, steps <= 1024.
    eos         a row is read up to the first `eos`; None: to its end.
    vocab, grid EventVocab / EventGrid: where notes and time shifts sit among the tokens, and the cell grid.
    want_cells  also the per-cell rhythm (0 rest, 1 onset, 2 hold) and notes (sounding pitches), uint8 (..., cells_ld).

    -> EventAttributes(r_density, n_density fp32, c_r, c_n, n_cells, status int32), each of tokens.shape[:-1]; device tensors, nothing is copied to the
    host.  status 0, EMPTY (no note: densities 0; the reference skips such a track) or OVERFLOW (more cells than the 2048 the kernel keeps: densities
    NaN; cells_ld is sized so that `steps` tokens of the longest shift fit, so only steps * n_shift beyond 2048 cells can overflow).
    ValueError for anything that is not as described, before anything is launched.  `ops`: the kernel table (tests); default HipOps(tokens.device)."""
    if not isinstance(want_cells, (bool, np.bool_)):
        raise ValueError("want_cells: a bool, got %r" % (want_cells,))
    params, g = _attr_params(eos, vocab, grid)
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int32 or tokens.dim() not in (2, 3) or tokens.numel() == 0:
        raise ValueError("tokens: an int32 tensor (rows, steps) or (n, V, steps), got %s" % (
            "%s %s" % (tokens.dtype, tuple(tokens.shape)) if torch.is_tensor(tokens) else type(tokens).__name__))
    steps = tokens.shape[-1]
    if steps > MAX_STEPS:
        raise ValueError("tokens: at most %d steps, got %d" % (MAX_STEPS, steps))
    lead = tuple(tokens.shape[:-1])
    tok = tokens.reshape(-1, steps)
    if tok.stride(1) != 1 and steps > 1:
        tok = tok.contiguous()
    rows, dev = tok.shape[0], tok.device
    cells_ld = min(MAX_CELLS, g.beat_cells * ((steps * g.n_shift * g.ticks_den) // (g.ticks_num * g.beat_cells) + 1))
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    out = dict(r_density=torch.empty(rows, **f32), n_density=torch.empty(rows, **f32), c_r=torch.empty(rows, **i32), c_n=torch.empty(rows, **i32),
               n_cells=torch.empty(rows, **i32), status=torch.empty(rows, **i32))
    cells = [torch.empty(rows, cells_ld, dtype=torch.uint8, device=dev) for _ in range(2)] if want_cells else [None, None]
    _ops_of(tok, ops).event_attributes(tok, steps, params.to(dev), out["n_cells"], out["status"], out["r_density"], out["n_density"], out["c_r"],
                                       out["c_n"], rhythm=cells[0], notes=cells[1], cells_ld=cells_ld)
    res = [out[k].view(lead) for k in EventAttributes._fields]
    if want_cells:
        return EventAttributesCells(*res, *(c.view(lead + (cells_ld,)) for c in cells))
    return EventAttributes(*res)


def _std(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
        raise ValueError("%s: a finite number > 0, got %r" % (name, v))
    return float(v)


def _sweep_scores_device(r, n, status, values, which, r_std, n_std, ops=None):
    """-> (scores (4,) fp64, n_used (1,) int32) on the device"""
    if which not in ("r", "n"):
        raise ValueError("which in {r, n}, got %r" % (which,))
    r_std, n_std = _std("r_std", r_std), _std("n_std", n_std)
    for name, t, dt in (("r", r, torch.float32), ("n", n, torch.float32), ("status", status, torch.int32)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 or tuple(t.shape) != tuple(r.shape):
            raise ValueError("%s: a %s tensor (S, Vn) like r, got %s" % (name, dt, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    S, Vn = r.shape
    if not 1 <= S <= MAX_SAMPLES or not 2 <= Vn <= 64:
        raise ValueError("r: 1..%d samples of 2..64 values, got %s" % (MAX_SAMPLES, (S, Vn)))
    vals = torch.as_tensor(np.asarray(values.detach().cpu() if torch.is_tensor(values) else values, dtype=np.float64))
    if vals.dim() != 1 or vals.numel() != Vn or not bool(torch.isfinite(vals).all()):
        raise ValueError("values: %d finite numbers, got %s" % (Vn, tuple(vals.shape)))
    dev = r.device
    scores, n_used = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    _ops_of(r, ops).sweep_scores(r.contiguous(), n.contiguous(), status.contiguous(), vals.to(dev), 0 if which == "r" else 1, r_std, n_std, scores, n_used)
    return scores, n_used


def sweep_scores(r, n, status, values, which, r_std, n_std, ops=None):
    """The scores of one evaluation round (test_class.py:169-175 with calculate_* of :259-272 / :308-321), in fp64 on the device.

    r, n     (S, Vn) fp32 densities of S samples at Vn fader values; status (S, Vn) int32: a sample with any non-zero entry is left out.
    values   the Vn fader values; which "r" / "n": the swept attribute; r_std, n_std: the data set's density stds the reference divides by.
    -> dict(consistency = 1 - mean_v std_s(x), restrictiveness = 1 - mean_s std_v(o), monotonicity = mean_s R2 of the swept density against the
    values (1.0 for a flat response, as LinearRegression().score gives), variance = mean_s std_v(x) (calculate_variance), n_used); NaN scores when
    no sample is left.  The five scalars are the only thing copied to the host."""
    scores, n_used = _sweep_scores_device(r, n, status, values, which, r_std, n_std, ops)
    out = dict(zip(SCORES, scores.cpu().tolist()))
    out["n_used"] = int(n_used.cpu().item())
    return out


@torch.no_grad()
def controllability(model, x, chroma, which, min_val, max_val, r_std, n_std, steps=100, n_values=8, eps=None, sample=None, beam=None, constraints=None,
                    eos=1, vocab=EventVocab(2, 90, 88), grid=EventGrid()):
    """One round of BaseEvaluator.evaluate (test_class.py:83-175) for the samples x (n, T) / (n, T, 342), chroma (n, 24), as ONE batched decode:
    fader_sweep(mode="set") over the values min + k * (max - min) / n_values, k < n_values (the reference's quirk that max is never reached, :84-85),
    then event_attributes and sweep_scores on the device.

    eps     (eps_r, eps_n), each (n, n_values, Z): a draw per (sample, value), as the reference's separate shift calls consume; None: drawn here (r, n).
    sample, beam, constraints: as fader_sweep takes them.
    -> dict(consistency, restrictiveness, monotonicity, variance, n_used, values (n_values,) float64, r_density, n_density (n, n_values) fp32 and
    status (n, n_values) int32 device tensors, tokens (n, n_values, steps)).  A sample with an empty (or overflowing) decode at any value is left out of
    the scores, as the reference discards it; nothing but the final scalars is copied to the host."""
    if which not in ("r", "n"):
        raise ValueError("which in {r, n}, got %r" % (which,))
    nv = _int("n_values", n_values, 2, 65)
    for name, v in (("min_val", min_val), ("max_val", max_val)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s: a finite number, got %r" % (name, v))
    _std("r_std", r_std), _std("n_std", n_std)
    _attr_params(eos, vocab, grid)
    gap = (max_val - min_val) / nv
    values = np.array([min_val + k * gap for k in range(nv)], dtype=np.float64)
    n = x.shape[0]
    if eps is None:
        Z = model.latent_dim
        eps = (torch.randn(n, nv, Z), torch.randn(n, nv, Z))
    elif len(eps) != 2 or any(e.dim() != 3 or e.shape[1] != nv for e in eps):
        raise ValueError("eps: (eps_r, eps_n), each (n, %d, Z)" % nv)
    tokens, _ = fader_sweep(model, x, chroma, values.astype(np.float32), steps=steps, which=which, eps=eps, mode="set", sample=sample, beam=beam,
                            constraints=constraints)
    ops = model.engine().ops
    at = event_attributes(tokens, eos=eos, vocab=vocab, grid=grid, ops=ops)
    out = sweep_scores(at.r_density, at.n_density, at.status, values, which, r_std, n_std, ops=ops)
    out.update(values=values, r_density=at.r_density, n_density=at.n_density, status=at.status, tokens=tokens)
    return out
