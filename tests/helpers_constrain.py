"""Checking tools of the constrained decode (decode.Constraints, fn_constrain_apply / fn_constrain_advance): the definition of include/fadernets.h
restated in numpy on the sounding-pitch bit words, a second statement as a plain-Python automaton over SETS of sounding pitches, the kernel cases both
CPU and GPU tests run, the checker of a fed stream, the fp64 replay of a constrained decode and the FakeOps stand-in."""
import numpy as np
import torch

from helpers import _DECODER_KEYS, REPLAY_CAP, replay_rows
from helpers_beam import BeamFakeOps
from helpers_sampling import SamplingFakeOps
from oracle import gmvae_oracle as orc

OFF_NEEDS_ON, NO_REONSET = 1, 2                                # FN_CONSTRAIN_*
MAX_PITCH = 128
PARAMS_DTYPE = np.dtype([("on_lo", "<i4"), ("off_lo", "<i4"), ("n_pitch", "<i4"), ("max_poly", "<i4"), ("eos", "<i4"), ("min_len", "<i4"),
                         ("flags", "<u4"), ("reserved", "<i4")])          # FnConstrainParams


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def params_of(on_lo=0, off_lo=0, n_pitch=0, max_poly=0, eos=-1, min_len=0, flags=0):
    return dict(on_lo=int(on_lo), off_lo=int(off_lo), n_pitch=int(n_pitch), max_poly=int(max_poly), eos=int(eos), min_len=int(min_len), flags=int(flags))


def params_bytes(p):
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    for k, v in p.items():
        raw[k] = v
    return raw.view(np.uint8).copy()


def params_from_bytes(b):
    raw = _np(b, np.uint8).view(PARAMS_DTYPE)[0]
    return {k: int(raw[k]) for k in PARAMS_DTYPE.names if k != "reserved"}


# ------------------------------------------------------------------------------------------------------------------------------
# statement 1: numpy on bit words
# ------------------------------------------------------------------------------------------------------------------------------
def _pitch_maps(V, p):
    """(on_pitch (V,), off_pitch (V,)): the pitch a token is the note-on / note-off of, or -1; the on range has precedence"""
    n = min(max(p["n_pitch"], 0), MAX_PITCH)
    e = np.arange(V, dtype=np.int64)
    po, pf = e - p["on_lo"], e - p["off_lo"]
    on = np.where((po >= 0) & (po < n), po, -1)
    off = np.where((pf >= 0) & (pf < n) & (on < 0), pf, -1)
    return on, off


def _bits(held, pitch):
    """held (rows, 4) uint32, pitch (V,) with -1 = none -> (rows, V) bool: the pitch sounds"""
    q = np.maximum(pitch, 0)
    return ((held[:, q >> 5] >> (q & 31).astype(np.uint32)) & np.uint32(1)).astype(bool) & (pitch >= 0)[None, :]


def grammar_bans(V, step, p, held, rows):
    """the set G of the definition as a (rows, V) bool"""
    G = np.zeros((rows, V), bool)
    if 0 <= p["eos"] < V and step < p["min_len"]:
        G[:, p["eos"]] = True
    n = min(max(p["n_pitch"], 0), MAX_PITCH)
    if held is not None and n > 0:
        held = as_words(held)
        on, off = _pitch_maps(V, p)
        s_on, s_off = _bits(held, on), _bits(held, off)
        count = np.array([sum(bin(int(w)).count("1") for w in row) for row in held])
        full = (p["max_poly"] > 0) & (count >= p["max_poly"])
        if p["flags"] & OFF_NEEDS_ON:
            G |= (off >= 0)[None, :] & ~s_off
        if p["flags"] & NO_REONSET:
            G |= s_on
        G |= (on >= 0)[None, :] & ~s_on & full[:, None]
    return G


def as_words(held):
    """int32 (as torch keeps them) or uint32 words -> uint32"""
    a = _np(held)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.int32 else np.ascontiguousarray(a, dtype=np.uint32)


def reference_apply(x, V, step, p, bias=None, held=None, dtype=np.float32):
    """x (rows, >= V) -> (out (rows, V) in dtype, stuck (rows,) bool).  One add in dtype, then selects."""
    x = _np(x)[:, :V].astype(dtype)
    rows = x.shape[0]
    y = x
    if bias is not None:
        b = _np(bias).astype(dtype)
        with np.errstate(invalid="ignore"):
            y = (x + (b[None, :] if b.ndim == 1 else b)).astype(dtype)
    G = grammar_bans(V, step, p, None if held is None else as_words(held), rows)
    left = ((y > -np.inf) & ~G).any(1)
    out = np.where(G & left[:, None], dtype(-np.inf), y)
    return out, ~left


def reference_advance(tok, V, p, logits=None, fallback=None, held=None):
    """-> (tok (rows,) int32, held_out (rows, 4) uint32 or None, fixed (rows,) bool)"""
    tok = _np(tok).astype(np.int64).copy()
    rows = tok.shape[0]
    fixed = np.zeros(rows, bool)
    if logits is not None:
        lg = _np(logits)
        inr = (tok >= 0) & (tok < V)
        fixed = ~inr | (lg[np.arange(rows), np.clip(tok, 0, V - 1)] == -np.inf)
        tok = np.where(fixed, np.clip(_np(fallback).astype(np.int64), 0, V - 1), tok)
    out = None
    if held is not None:
        out = as_words(held).copy()
        on, off = _pitch_maps(V, p)
        for r in range(rows):
            t = int(tok[r])
            if 0 <= t < V:
                if on[t] >= 0:
                    out[r, on[t] >> 5] |= np.uint32(1 << (int(on[t]) & 31))
                elif off[t] >= 0:
                    out[r, off[t] >> 5] &= np.uint32(~(1 << (int(off[t]) & 31)) & 0xffffffff)
    return tok.astype(np.int32), out, fixed


# ------------------------------------------------------------------------------------------------------------------------------
# statement 2: a plain-Python automaton over sets of sounding pitches, written without the words
# ------------------------------------------------------------------------------------------------------------------------------
class NoteAutomaton:
    """one row's state: the set of sounding pitches (None: no state is carried, only the eos rule holds)"""

    def __init__(self, V, p, sounding=None):
        self.V, self.p = V, p
        self.n = min(max(p["n_pitch"], 0), MAX_PITCH)
        self.sounding = None if sounding is None else set(sounding)
        self.notes = [(e, ) + self.kind(e) for e in range(V) if self.kind(e) is not None]           # (token, 'on' / 'off', pitch)

    @staticmethod
    def from_words(V, p, words):
        if words is None:
            return NoteAutomaton(V, p, None)
        w = [int(x) & 0xffffffff for x in words]
        return NoteAutomaton(V, p, {q for q in range(MAX_PITCH) if (w[q // 32] >> (q % 32)) & 1})

    def words(self):
        w = [0, 0, 0, 0]
        for q in self.sounding:
            w[q // 32] |= 1 << (q % 32)
        return w

    def kind(self, e):
        """('on', pitch), ('off', pitch) or None"""
        if not 0 <= e < self.V:
            return None
        if 0 <= e - self.p["on_lo"] < self.n:
            return "on", e - self.p["on_lo"]
        if 0 <= e - self.p["off_lo"] < self.n:
            return "off", e - self.p["off_lo"]
        return None

    def bans(self, step):
        out = set()
        if 0 <= self.p["eos"] < self.V and step < self.p["min_len"]:
            out.add(self.p["eos"])
        if self.sounding is None or self.n == 0:
            return out
        full = self.p["max_poly"] > 0 and len(self.sounding) >= self.p["max_poly"]
        for e, what, q in self.notes:
            if what == "off" and (self.p["flags"] & OFF_NEEDS_ON) and q not in self.sounding:
                out.add(e)
            if what == "on" and q in self.sounding and (self.p["flags"] & NO_REONSET):
                out.add(e)
            if what == "on" and q not in self.sounding and full:
                out.add(e)
        return out

    def feed(self, tok):
        if self.sounding is None:
            return
        k = self.kind(int(tok))
        if k is not None:
            (self.sounding.add if k[0] == "on" else self.sounding.discard)(k[1])


def python_apply(x, V, step, p, bias=None, held=None):
    x = _np(x, np.float32)
    rows = x.shape[0]
    b = None if bias is None else _np(bias, np.float32)
    out, stuck = np.zeros((rows, V), np.float32), np.zeros(rows, bool)
    for r in range(rows):
        auto = NoteAutomaton.from_words(V, p, None if held is None else as_words(held)[r])
        with np.errstate(invalid="ignore"):
            y = [np.float32(x[r, e]) if b is None else np.float32(x[r, e] + (b[e] if b.ndim == 1 else b[r, e])) for e in range(V)]
        G = auto.bans(step)
        left = any(y[e] > -np.inf and e not in G for e in range(V))
        stuck[r] = not left
        out[r] = [np.float32(-np.inf) if (left and e in G) else y[e] for e in range(V)]
    return out, stuck


def python_advance(tok, V, p, logits=None, fallback=None, held=None):
    tok = [int(t) for t in _np(tok)]
    rows = len(tok)
    fixed = np.zeros(rows, bool)
    words = None if held is None else np.zeros((rows, 4), np.uint32)
    for r in range(rows):
        if logits is not None and (not 0 <= tok[r] < V or _np(logits)[r, tok[r]] == -np.inf):
            tok[r] = min(max(int(_np(fallback)[r]), 0), V - 1)
            fixed[r] = True
        if held is not None:
            auto = NoteAutomaton.from_words(V, p, as_words(held)[r])
            auto.feed(tok[r])
            words[r] = auto.words()
    return np.array(tok, np.int32), words, fixed


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel cases (CPU: the two statements and the host twin; GPU: the kernels)
# ------------------------------------------------------------------------------------------------------------------------------
CASE_ROWS = (1, 5, 67)                 # one wavefront, a partial quartet of wavefronts, a partial last workgroup
CASE_V = (3, 24, 342, 1024)
CASE_SHAPES = [(r, v) for r in CASE_ROWS for v in CASE_V]


def _layout(V, clipped):
    """(on_lo, off_lo, n_pitch) for a vocabulary of V tokens; clipped: ranges that V and 0 cut (and that overlap where V is tiny)"""
    if clipped:
        return {3: (2, -1, 5), 24: (20, -4, 10), 342: (300, -40, 88), 1024: (1000, -100, 128)}[V]
    return {3: (0, 1, 1), 24: (2, 10, 8), 342: (2, 90, 88), 1024: (100, 300, 128)}[V]


def _held_with(rs, rows, n, counts, extra=False):
    """(rows, 4) uint32 with counts[r] pitches below n sounding (extra: also bit 127 where n < 128 - a bit outside the vocabulary still counts)"""
    h = np.zeros((rows, 4), np.uint32)
    for r in range(rows):
        for q in rs.choice(max(n, 1), size=min(int(counts[r]), n), replace=False) if n else ():
            h[r, q >> 5] |= np.uint32(1 << (int(q) & 31))
        if extra and n < 128 and r % 3 == 0:
            h[r, 3] |= np.uint32(1 << 31)
    return h


def kernel_cases(rows, V):
    """the cases of the issue for one (rows, V): dicts of rows, V, ld, step, p, x (rows, ld) float32, bias, held, tok, fb, fixup, alias"""
    rs = np.random.RandomState(1000 * rows + V)
    ld = V + 5
    cases = []

    def add(tag, p, bias_mode, held_counts=None, step=3, clipped=False, fixup=True, alias=False, extra=False, only=None):
        x = np.full((rows, ld), 7.5, np.float32)                      # sentinels behind column V
        x[:, :V] = (rs.randn(rows, V) * 3).astype(np.float32)
        x[:, :V][rs.rand(rows, V) < 0.05] = -np.inf
        x[:, min(1, V - 1)] = rs.randn(rows).astype(np.float32)       # one finite logit outside the bias bans below
        bias = None
        if bias_mode:
            bias = (rs.randn(*((V,) if bias_mode == 1 else (rows, V)))).astype(np.float32)
            bias[..., rs.rand(V) < 0.2] = -np.inf
            bias[..., min(1, V - 1)] = 0.25
        if only is not None:                                          # a shared bias that leaves `only` alone
            bias = np.full(V, -np.inf, np.float32)
            bias[only] = 0.5
            x[:, only] = 1.0
        n = min(max(p["n_pitch"], 0), MAX_PITCH)
        held = None if held_counts is None else _held_with(rs, rows, n, np.resize(np.asarray(held_counts), rows), extra)
        tok = rs.randint(0, V, rows).astype(np.int32)
        for r in range(rows):                                        # note-ons, note-offs, others, out of range
            kind = r % 5
            if kind == 0 and n:
                tok[r] = min(max(p["on_lo"] + rs.randint(n), 0), V - 1)
            elif kind == 1 and n:
                tok[r] = min(max(p["off_lo"] + rs.randint(n), 0), V - 1)
            elif kind == 3:
                tok[r] = (-3, V, V + 7, -2 ** 31)[rs.randint(4)]
        fb = rs.randint(0, V, rows).astype(np.int32)
        fb[::4] = (V + 3, -1)[rs.randint(2)]                          # a fallback to clamp
        cases.append(dict(tag=tag, rows=rows, V=V, ld=ld, step=step, p=p, x=x, bias=bias, held=held, tok=tok, fb=fb, fixup=fixup, alias=alias))

    on, off, n = _layout(V, False)
    eos = V - 1 if V - 1 not in range(on, on + n) and V - 1 not in range(off, off + n) else -1
    some = [0, 1, 2, 3, min(5, n)]
    add("plain", params_of(), 0)
    add("bias shared", params_of(), 1)
    add("bias per row", params_of(), 2)
    for flags in (OFF_NEEDS_ON, NO_REONSET, OFF_NEEDS_ON | NO_REONSET):
        add("flags %d" % flags, params_of(on, off, n, flags=flags), flags % 3, held_counts=some, alias=bool(flags & 1))
    mp = min(3, n)
    add("max_poly below", params_of(on, off, n, max_poly=mp), 0, held_counts=[mp - 1], fixup=False)
    add("max_poly at", params_of(on, off, n, max_poly=mp), 1, held_counts=[mp - 1, mp, mp + 1 if n > mp else mp], alias=True)
    add("max_poly counts every bit", params_of(on, off, n, max_poly=mp), 0, held_counts=[mp - 1], extra=True)
    for step in (4, 5):
        add("min_len step %d" % step, params_of(on, off, n, eos=max(eos, 0), min_len=5), 2, step=step)
    add("all together", params_of(on, off, n, max_poly=mp, eos=max(eos, 0), min_len=9, flags=3), 2, held_counts=some, step=8, extra=True)
    add("no state given", params_of(on, off, n, max_poly=1, eos=max(eos, 0), min_len=9, flags=3), 1, step=2)
    # stuck beside not stuck: the bias leaves one note-off alone, which OFF_NEEDS_ON bans exactly where its pitch does not sound
    add("stuck by grammar", params_of(on, off, n, flags=OFF_NEEDS_ON), 0, held_counts=[0, n, 0, 1, n], only=off)
    add("stuck by eos", params_of(on, off, n, eos=max(eos, 0), min_len=4), 0, step=0, only=max(eos, 0))
    add("not stuck at min_len", params_of(on, off, n, eos=max(eos, 0), min_len=4), 0, step=4, only=max(eos, 0))
    con, coff, cn = _layout(V, True)
    add("clipped ranges", params_of(con, coff, cn, max_poly=2, flags=3), 1, held_counts=[0, 1, 2, 3, cn])
    add("n_pitch beyond 128", params_of(on, off, 1000, flags=3), 0, held_counts=some)
    add("n_pitch negative", params_of(on, off, -5, max_poly=1, flags=3), 0, held_counts=[0])
    if V == 1024:
        add("bits in all four words", params_of(100, 300, 128, max_poly=60, flags=3), 2, held_counts=[70, 59, 60])
        assert (cases[-1]["held"] != 0).all()
    return cases


def reference_case(c, apply_fn=reference_apply, advance_fn=reference_advance):
    """a case through a statement of the definition: the apply, then the advance on the rows it left (as the decode loop chains them)"""
    out, stuck = apply_fn(c["x"], c["V"], c["step"], c["p"], c["bias"], c["held"])
    full = c["x"].copy()
    full[:, :c["V"]] = out
    tok, held_out, fixed = advance_fn(c["tok"], c["V"], c["p"], full if c["fixup"] else None, c["fb"] if c["fixup"] else None, c["held"])
    return dict(logits=full, stuck=stuck.astype(np.int32), tok=tok, held=held_out, fixed=fixed.astype(np.int32))


def same_result(a, b, what=""):
    assert np.array_equal(_np(a["logits"], np.float32).view(np.uint32), _np(b["logits"], np.float32).view(np.uint32)), "(apply) logits differ %s" % what
    assert np.array_equal(_np(a["stuck"]), _np(b["stuck"])), "(apply) stuck differs %s" % what
    assert np.array_equal(_np(a["tok"]), _np(b["tok"])), "(advance) tokens differ %s" % what
    assert np.array_equal(_np(a["fixed"]), _np(b["fixed"])), "(advance) fixed differs %s" % what
    assert (a["held"] is None) == (b["held"] is None) and (a["held"] is None or np.array_equal(as_words(a["held"]), as_words(b["held"]))), \
        "(advance) held differs %s" % what


# ------------------------------------------------------------------------------------------------------------------------------
# a fed stream against the automaton
# ------------------------------------------------------------------------------------------------------------------------------
def constraint_params(con):
    """the parameter dict of a pkg.Constraints"""
    return params_from_bytes(con.params_bytes().numpy())


def bias_bans(con, Bi):
    """(Bi, 342) bool: the tokens the bias bans"""
    if con.bias is None:
        return np.zeros((Bi, orc.E), bool)
    b = con.bias.numpy() == -np.inf
    return np.broadcast_to(b, (Bi, orc.E)) if b.ndim == 1 else b


def stream_violations(fed, p, stateful=True, banned=None, logp=None, V=orc.E):
    """Walk every row's fed stream (Bi, steps) through the automaton.  Returns a dict of counts: banned = fed tokens the automaton (or `banned`
    (Bi, V) bool, the bias bans) forbids at their step, early_eos, over_poly = steps after which more than max_poly pitches sound, and - with logp
    (Bi, steps, V) - wrong_inf = entries whose being -inf differs from being banned.  No row may be stuck for the counts to be exact."""
    fed = _np(fed)
    Bi, steps = fed.shape
    st = dict(banned=0, early_eos=0, over_poly=0, wrong_inf=0, max_poly_seen=0, note_ons=0)
    lg = None if logp is None else _np(logp)
    for b in range(Bi):
        auto = NoteAutomaton(V, p, set() if stateful else None)
        for i in range(steps):
            G = auto.bans(i)
            if banned is not None:
                G = G | set(np.nonzero(banned[b])[0].tolist())
            t = int(fed[b, i])
            st["banned"] += t in G
            st["early_eos"] += (t == p["eos"] and i < p["min_len"])
            if lg is not None:
                isinf = lg[b, i] == -np.inf
                want = np.zeros(V, bool)
                want[sorted(G)] = True
                st["wrong_inf"] += int((isinf != want).sum())
            k = auto.kind(t)
            st["note_ons"] += bool(k and k[0] == "on")
            auto.feed(t)
            if stateful:
                st["max_poly_seen"] = max(st["max_poly_seen"], len(auto.sounding))
                st["over_poly"] += (p["max_poly"] > 0 and len(auto.sounding) > p["max_poly"])
    return st


def assert_stream_valid(fed, p, stateful=True, banned=None, logp=None):
    st = stream_violations(fed, p, stateful, banned, logp)
    assert st["banned"] == 0, "(fed) %d fed tokens are banned at their step" % st["banned"]
    assert st["early_eos"] == 0, "(eos) eos before min_length at %d positions" % st["early_eos"]
    assert st["over_poly"] == 0, "(poly) more than max_polyphony pitches sound after %d steps (max %d)" % (st["over_poly"], st["max_poly_seen"])
    assert st["wrong_inf"] == 0, "(inf) %d log-prob entries are -inf where nothing bans them, or finite where something does" % st["wrong_inf"]
    return st


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 replay of a constrained decode
# ------------------------------------------------------------------------------------------------------------------------------
def constrained_replay_check(sd, z, fed, logp, p, stateful, bias=None, rows=None, own=None, scores=None, lens=None):
    """helpers_forced.replay_forced_check for a constrained decode: the oracle decoder replays teacher = fed in fp64 and fp32 (e_ref = their distance,
    tol_lp = min(1e-4, 16 e_ref), delta = 2 tol_lp, the cap REPLAY_CAP - that helper's figures), the fp64 log-probs go through the fp64 restatement of
    fn_constrain_apply (bias added in fp64; log_softmax is shift-invariant, so log-probs serve as logits) and log_softmax, and
      (inf) logp is -inf exactly where the constrained fp64 row is;  (a) |logp - lp64c| <= tol_lp on the finite entries;
      own given (the argmax head's tokens, (Bi, steps)): (b) it is the first-index argmax of its logp row, (c) lp64c[own] >= max lp64c - delta, and
      at most REPLAY_CAP of the positions have a constrained fp64 top-2 gap below delta;
      scores given ((Bi,), a beam hypothesis' summed log-probs along fed): |score - sum_i lp64c[fed_i]| <= steps tol_lp + steps 2^-24 |score|, the
      bound of helpers_beam.beam_replay_check (lens (Bi,): a hypothesis that ended sums the positions before its end).
    fed (Bi, steps), logp (Bi, steps, 342), bias None / (342,) / (Bi, 342).  Returns the figures."""
    fed = torch.as_tensor(_np(fed)).long()
    Bi, steps = fed.shape
    rows = np.asarray(replay_rows(Bi) if rows is None else rows)
    rt = torch.as_tensor(rows, dtype=torch.long)
    fd = fed[rt]
    dec = {k: v.detach().cpu() for k, v in sd.items() if k.startswith(_DECODER_KEYS)}
    zr = torch.as_tensor(z).detach().cpu()[rt]
    with torch.no_grad():
        lp64 = orc.global_decoder({k: v.double() for k, v in dec.items()}, zr.double(), steps, teacher=fd).numpy()
        lp32 = orc.global_decoder({k: v.float() for k, v in dec.items()}, zr.float(), steps, teacher=fd).numpy()
    e_ref = float(np.abs(lp32.astype(np.float64) - lp64).max())
    tol = min(1e-4, 16.0 * e_ref)
    delta = 2.0 * tol
    b64 = None if bias is None else (_np(bias).astype(np.float64) if _np(bias).ndim == 1 else _np(bias).astype(np.float64)[rows])
    held = np.zeros((len(rows), 4), np.uint32) if stateful else None
    V = orc.E
    lpc = np.zeros_like(lp64)
    for i in range(steps):
        out, stuck = reference_apply(lp64[:, i], V, i, p, b64, held, dtype=np.float64)
        assert not stuck.any(), "a replayed row is stuck at step %d" % i
        lpc[:, i] = torch.log_softmax(torch.from_numpy(out), dim=-1).numpy()
        if stateful:
            held = reference_advance(fd[:, i].numpy(), V, p, held=held)[1]
    lg = _np(logp)[rows].astype(np.float64)
    assert lg.shape == lpc.shape, (lg.shape, lpc.shape)
    bad = (lg == -np.inf) != (lpc == -np.inf)
    assert not bad.any(), "(inf) %d entries differ in being -inf from the constrained fp64 replay" % int(bad.sum())
    fin = lpc > -np.inf
    err = np.abs(np.where(fin, lg - np.where(fin, lpc, 0.0), 0.0))
    st = dict(Bi=Bi, steps=steps, rows=len(rows), e_ref=e_ref, tol_lp=tol, delta=delta, max_dlp=float(err.max()), banned_share=float((~fin).mean()))
    assert not np.isnan(lg).any() and st["max_dlp"] <= tol, "(a) |logp - lp64c| = %.3e > tol_lp %.3e (e_ref %.3e)" % (st["max_dlp"], tol, e_ref)
    if own is not None:
        tk = _np(own)[rows].astype(np.int64)
        assert np.array_equal(np.argmax(_np(logp)[rows], axis=-1), tk), "(b) a token is not the first-index argmax of its own log-prob row"
        top2 = np.sort(lpc, axis=-1)[..., -2:]
        short = top2[..., 1] - np.take_along_axis(lpc, tk[..., None], axis=-1)[..., 0]
        assert not (short > delta).any(), "(c) lp64c[tok] is %.3e below the constrained fp64 best (delta %.3e)" % (float(short.max()), delta)
        st["share_below_delta"] = float(((top2[..., 1] - top2[..., 0]) < delta).mean())
        assert st["share_below_delta"] <= REPLAY_CAP, "cap: %.2f %% of the positions have a constrained fp64 top-2 gap below delta" % (100 * st["share_below_delta"])
    if scores is not None:
        along = np.take_along_axis(lpc, fd.numpy()[..., None], axis=-1)[..., 0]
        if lens is not None:
            along = along * (np.arange(steps)[None, :] < _np(lens).astype(np.int64)[rows][:, None])
        along = along.sum(1)
        sc = _np(scores).astype(np.float64)[rows]
        derr = np.abs(sc - along)
        st["max_dscore"] = float(derr.max())
        assert (derr <= steps * tol + steps * 2.0 ** -24 * np.abs(sc)).all(), "(sum) |score - sum lp64c[tok]| = %.3e" % st["max_dscore"]
    return st


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-in
# ------------------------------------------------------------------------------------------------------------------------------
class ConstrainFakeOps(BeamFakeOps, SamplingFakeOps):
    """FakeOps + the beam and sampling stand-ins + fn_constrain_apply / fn_constrain_advance as their numpy restatement"""

    def constrain_apply(self, logits, V, step, params, bias=None, held=None, stuck=None):
        self.calls.append("constrain_apply")
        out, st = reference_apply(logits.numpy(), V, step, params_from_bytes(params.numpy()), None if bias is None else bias.numpy(),
                                  None if held is None else held.numpy())
        logits[:, :V] = torch.from_numpy(out)
        if stuck is not None:
            stuck += torch.from_numpy(st.astype(np.int32))

    def constrain_advance(self, tok, V, params, logits=None, fallback=None, held_in=None, held_out=None, fixed=None):
        self.calls.append("constrain_advance")
        t, h, fx = reference_advance(tok.numpy(), V, params_from_bytes(params.numpy()), None if logits is None else logits.numpy(),
                                     None if fallback is None else fallback.numpy(), None if held_in is None else held_in.numpy())
        if logits is not None:
            tok.copy_(torch.from_numpy(t))
            if fixed is not None:
                fixed += torch.from_numpy(fx.astype(np.int32))
        if held_in is not None:
            held_out.copy_(torch.from_numpy(h.view(np.int32)))


def favour_note_offs(amount=6.0, vocab=(2, 90, 88)):
    """a bias that favours the note-off range (and a little the note-ons): an unconstrained decode then writes note-offs of silent pitches"""
    b = torch.zeros(orc.E)
    b[vocab[1]:vocab[1] + vocab[2]] = amount
    b[vocab[0]:vocab[0] + vocab[2]] = amount - 1.0
    return b


def full_constraints(pkg, per_row=0, **kw):
    """the constraint set of the end-to-end tests: a bias that favours the note range (so an unconstrained decode does break the grammar), the pad
    token banned, every grammar rule, a polyphony ceiling of 3, eos = 1 kept away for 10 steps"""
    bias = favour_note_offs()
    if per_row:
        bias = bias.unsqueeze(0).repeat(per_row, 1)
        bias[1::2, 200:260] += 0.5
    args = dict(bias=bias, ban=(0,), min_length=10, eos=1, off_needs_on=True, no_reonset=True, max_polyphony=3, want_stats=True)
    args.update(kw)
    return pkg.Constraints(**args)


def prompt_tokens(Bi):
    return torch.tensor([[2 + 5, 2 + 9, 90 + 5]]).repeat(Bi, 1)          # two note-ons, then the first one's note-off: the state starts from them
