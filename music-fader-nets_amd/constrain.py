"""Constraints of a decode (greedy_decode / sample_decode / beam_decode / fader_sweep, keyword `constraints`): a token bias with bans, a minimum
length before the end token, and the note grammar of the event vocabulary - validated here, applied by fn_constrain_apply / fn_constrain_advance
(include/fadernets.h has the definition) around the unchanged heads.  The reference has no counterpart."""
import collections

import numpy as np
import torch

from .engine import E_VOCAB

EventVocab = collections.namedtuple("EventVocab", ["on_lo", "off_lo", "n_pitch"])
EventVocab.__doc__ = """Where the notes sit in the token vocabulary: note-on of pitch p = on_lo + p, note-off = off_lo + p, p < n_pitch <= 128."""
MAX_PITCH = 128            # FN_CONSTRAIN_MAX_PITCH
OFF_NEEDS_ON, NO_REONSET = 1, 2          # FN_CONSTRAIN_OFF_NEEDS_ON, FN_CONSTRAIN_NO_REONSET
PARAMS_DTYPE = np.dtype([("on_lo", "<i4"), ("off_lo", "<i4"), ("n_pitch", "<i4"), ("max_poly", "<i4"), ("eos", "<i4"), ("min_len", "<i4"),
                         ("flags", "<u4"), ("reserved", "<i4")])          # FnConstrainParams


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < hi:
        raise ValueError("%s: an int in [%d, %d), got %r" % (name, lo, hi, v))
    return int(v)


class Constraints:
    """What a decode may pick, step by step.

    bias            (342,) - one vector for every row - or (Bi, 342) fp32, added to every step's logits before the head; -inf entries are bans.
    ban             tokens folded into the bias as -inf.
    eos, min_length the token `eos` is banned while step < min_length (steps count from 0, the prompt's included).
    off_needs_on    a note-off only for a pitch that sounds.
    no_reonset      no note-on of a pitch that sounds.
    max_polyphony   no new note-on while that many pitches sound (0: off).
    vocab           EventVocab(on_lo, off_lo, n_pitch).  The default note-ons 2 .. 89 follow the reference's trainer_glsr.py:125,133 (note-ons 2-89,
                    time shifts 178-277); the note-offs 90 .. 177 are INFERRED from the class order of the performance encoding (note-on, note-off,
                    time shift, velocity) - the encoder library was not at hand to confirm it, which is why the layout is a parameter.
    want_stats      the decode appends dict(stuck=(rows,), fixed=(rows,)) int32 to its results: how often a row had every token banned (the eos and
                    grammar bans are then dropped for that step) and how often the sampler's token was replaced by the row's argmax.

    A pitch sounds from the step that FEEDS its note-on to the step that feeds its note-off; a prompt's or forced tokens move the state as the
    decoder's own do (they are not checked against the grammar).  The log-probs a constrained decode returns are those of the constrained
    distribution: banned entries are exactly -inf.  ValueError for anything that is not as described, before anything is launched."""

    def __init__(self, bias=None, ban=(), min_length=0, eos=None, off_needs_on=False, no_reonset=False, max_polyphony=0,
                 vocab=EventVocab(on_lo=2, off_lo=90, n_pitch=88), want_stats=False):
        V = E_VOCAB
        for name, v in (("off_needs_on", off_needs_on), ("no_reonset", no_reonset), ("want_stats", want_stats)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("%s: a bool, got %r" % (name, v))
        self.min_length = _int("min_length", min_length, 0, 1 << 31)
        self.eos = None if eos is None else _int("eos", eos, 0, V)
        if self.min_length > 0 and self.eos is None:
            raise ValueError("min_length goes with eos, the token it keeps away")
        self.max_polyphony = _int("max_polyphony", max_polyphony, 0, MAX_PITCH + 1)
        self.off_needs_on, self.no_reonset, self.want_stats = bool(off_needs_on), bool(no_reonset), bool(want_stats)
        if vocab is None:
            vocab = EventVocab(0, 0, 0)
        try:
            on_lo, off_lo, n_pitch = vocab
        except (TypeError, ValueError):
            raise ValueError("vocab: EventVocab(on_lo, off_lo, n_pitch), got %r" % (vocab,))
        n = _int("vocab.n_pitch", n_pitch, 0, MAX_PITCH + 1)
        on, off = _int("vocab.on_lo", on_lo, 0, V + 1), _int("vocab.off_lo", off_lo, 0, V + 1)
        if on + n > V or off + n > V:
            raise ValueError("vocab: the note ranges lie inside [0, %d), got %r" % (V, (on, off, n)))
        if n > 0 and on < off + n and off < on + n:
            raise ValueError("vocab: the note-on and note-off ranges are disjoint, got %r" % ((on, off, n),))
        self.vocab = EventVocab(on, off, n)
        self.stateful = self.off_needs_on or self.no_reonset or self.max_polyphony > 0
        if self.stateful and n == 0:
            raise ValueError("the note grammar needs a vocab with n_pitch > 0")
        bans = [_int("ban", t, 0, V) for t in (ban.tolist() if torch.is_tensor(ban) or isinstance(ban, np.ndarray) else list(ban))]
        if bias is not None:
            bias = bias.detach().cpu() if torch.is_tensor(bias) else torch.as_tensor(np.asarray(bias))
            if not bias.is_floating_point() or bias.dim() not in (1, 2) or bias.shape[-1] != V or bias.shape[0] < 1:
                raise ValueError("bias: a float tensor (%d,) or (Bi, %d), got %s %s" % (V, V, bias.dtype, tuple(bias.shape)))
            bias = bias.float().clone().contiguous()
            if bool(torch.isnan(bias).any()) or bool((bias == float("inf")).any()):
                raise ValueError("bias: finite or -inf entries (no NaN, no +inf)")
        elif bans:
            bias = torch.zeros(V)
        if bans:
            bias[..., bans] = float("-inf")
        if bias is not None and not bool(torch.isfinite(bias).any(-1).all()):
            raise ValueError("bias / ban: every row keeps a finite entry")
        self.bias = bias

    @property
    def bias_mode(self):
        """0: none, 1: one shared vector, 2: a row per decode row"""
        return 0 if self.bias is None else self.bias.dim()

    def key(self):
        """what a captured graph depends on: the bias form and whether the sounding-pitch state is carried (the scalars and the bias values are data)"""
        return (self.bias_mode, self.stateful)

    def params_bytes(self):
        """the 32 bytes of FnConstrainParams as a CPU uint8 tensor"""
        raw = np.zeros(1, dtype=PARAMS_DTYPE)
        raw["on_lo"], raw["off_lo"], raw["n_pitch"] = self.vocab
        raw["max_poly"], raw["eos"], raw["min_len"] = self.max_polyphony, -1 if self.eos is None else self.eos, self.min_length
        raw["flags"] = (OFF_NEEDS_ON if self.off_needs_on else 0) | (NO_REONSET if self.no_reonset else 0)
        return torch.from_numpy(raw.view(np.uint8).copy())

    def bias_rows(self, Bi, repeat=1):
        """the bias as the kernels take it for Bi sequences of `repeat` rows each: None, (342,) or (Bi * repeat, 342); ValueError on a row count"""
        if self.bias_mode < 2:
            return self.bias
        if self.bias.shape[0] != Bi:
            raise ValueError("bias: %d rows for a decode of %d" % (self.bias.shape[0], Bi))
        return self.bias if repeat == 1 else self.bias.repeat_interleave(repeat, dim=0).contiguous()


def constraint_buffers(con, Bi, dev, repeat=1, gather=False):
    """every device tensor a constrained decode of Bi sequences x `repeat` rows keeps: the parameter bytes, the bias, the sounding-pitch words (and
    the copy the beam gather writes), the stuck / fixed counters and the sampler's argmax column - at their final sizes, nothing is allocated later"""
    rows = Bi * repeat
    bias = con.bias_rows(Bi, repeat)
    i32 = dict(dtype=torch.int32, device=dev)
    return dict(params=con.params_bytes().to(dev), bias=None if bias is None else bias.to(dev),
                held=torch.zeros(rows, 4, **i32) if con.stateful else None, held_g=torch.zeros(rows, 4, **i32) if con.stateful and gather else None,
                stuck=torch.zeros(rows, **i32), fixed=torch.zeros(rows, **i32), own=torch.zeros(rows, **i32))


def load_constraints(cb, con, Bi, repeat=1):
    """another setting of the same key() into the static buffers of a captured graph"""
    cb["params"].copy_(con.params_bytes())
    if cb["bias"] is not None:
        cb["bias"].copy_(con.bias_rows(Bi, repeat))


def constraint_stats(cb):
    return dict(stuck=cb["stuck"].clone(), fixed=cb["fixed"].clone())
