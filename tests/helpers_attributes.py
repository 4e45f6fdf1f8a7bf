"""Test-side restatement of the controllability metrics (include/fadernets.h, fn_event_attributes / fn_sweep_scores; attributes.py), from the
definition and not from the kernels:

  tokens_to_notes                  the step from event tokens to timed notes - OURS, written once, imported by tests/golden/make_golden_attributes.py
  attributes_sets                  statement 1: plain Python, a set of sounding pitches per cell
  attributes_words                 statement 2: a bit column per pitch over the cells (Python integers), then one 128-bit word per cell
  event_attributes_ref             statement 2 over a token matrix, in the shapes the entry point writes
  sweep_scores_ref                 the scores in numpy fp64, sums in the definition's order
  fixture_streams / score_cases    what the golden generator pushes through the reference's code
  kernel_cases                     the case list the host twin and the kernel are held to

The stand-ins at the end (attr_fake_ops) let attributes.controllability / evaluators.evaluate run on the CPU."""
import collections

import numpy as np
import torch

MAX_STEPS, MAX_CELLS, MAX_SAMPLES = 1024, 2048, 4096          # FN_ATTR_MAX_*
EMPTY, OVERFLOW = 1, 2                                          # FN_ATTR_EMPTY, FN_ATTR_OVERFLOW
FIELDS = ("on_lo", "off_lo", "n_pitch", "shift_lo", "n_shift", "eos", "ticks_num", "ticks_den", "beat_cells", "vocab_size")
PARAMS_DTYPE = np.dtype([(k, "<i4") for k in FIELDS] + [("reserved", "<i4", (2,))])          # FnAttrParams, 48 bytes
DEFAULT = dict(on_lo=2, off_lo=90, n_pitch=88, shift_lo=178, n_shift=100, eos=1, ticks_num=25, ticks_den=2, beat_cells=4, vocab_size=342)
WIDE = dict(DEFAULT, on_lo=2, off_lo=130, n_pitch=128, shift_lo=258, n_shift=100, vocab_size=400)          # all four words of the pitch set
PAD, VEL_LO = 0, 278


def params_bytes(p):
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    for k in FIELDS:
        raw[k] = p[k]
    return raw.view(np.uint8).copy()


def clamped(p):
    """the parameters as the definition clamps them"""
    q = dict(p)
    for k, lo, hi in (("n_pitch", 0, 128), ("n_shift", 0, 4096), ("ticks_num", 1, 32768), ("ticks_den", 1, 256), ("beat_cells", 1, 64)):
        q[k] = min(max(int(p[k]), lo), hi)
    return q


# ------------------------------------------------------------------------------------------------------------------------------
# tokens -> notes (ours)
# ------------------------------------------------------------------------------------------------------------------------------
def tokens_to_notes(row, p):
    """row: ints.  -> [(pitch, t0, t1)] of the kept notes in the order they close (the notes the end of the row closes: by pitch)."""
    p = clamped(p)
    t, held, notes = 0, {}, []

    def close(pitch):
        t0 = held.pop(pitch)
        if t > t0:
            notes.append((pitch, t0, t))

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
            held[pitch] = t
        elif 0 <= e - p["off_lo"] < p["n_pitch"]:
            if e - p["off_lo"] in held:
                close(e - p["off_lo"])
        elif 0 <= e - p["shift_lo"] < p["n_shift"]:
            t += e - p["shift_lo"] + 1
    for pitch in sorted(held):
        close(pitch)
    return notes


def grid_of(notes, p):
    """-> (n_cells, [(pitch, a, b)]) in the notes' order"""
    p = clamped(p)
    if not notes:
        return 0, []
    num, den, bc = p["ticks_num"], p["ticks_den"], p["beat_cells"]
    t_last = max(t1 for _, _, t1 in notes)
    n_cells = bc * ((t_last * den) // (num * bc) + 1)
    return n_cells, [(pitch, (2 * den * t0 + num) // (2 * num), (den * t1) // num) for pitch, t0, t1 in notes]


def _finish(n_cells, onsets, total, rhythm, notes, cells_ld, extra):
    out = dict(n_cells=n_cells, status=0, rhythm=np.zeros(cells_ld, np.uint8), notes=np.zeros(cells_ld, np.uint8), **extra)
    if n_cells == 0:
        out.update(status=EMPTY, r_density=np.float32(0), n_density=np.float32(0), c_r=0, c_n=0)
    elif n_cells > cells_ld:
        out.update(status=OVERFLOW, r_density=np.float32(np.nan), n_density=np.float32(np.nan), c_r=-1, c_n=-1)
    else:
        out["rhythm"][:n_cells], out["notes"][:n_cells] = rhythm, notes
        out.update(r_density=np.float32(np.float64(onsets) / n_cells), n_density=np.float32(np.float64(total) / n_cells),
                   c_r=0 if 10 * onsets < 3 * n_cells else 1 if 2 * onsets < n_cells else 2,
                   c_n=0 if total <= 2 * n_cells else 1 if 2 * total <= 7 * n_cells else 2)
    return out


def attributes_sets(row, p, cells_ld=MAX_CELLS):
    """statement 1: a set of pitches per cell; also returns the roll (n_cells, 128) bool"""
    n_cells, placed = grid_of(tokens_to_notes(row, p), p)
    if n_cells > cells_ld:
        return _finish(n_cells, 0, 0, None, None, cells_ld, dict(roll=None))
    cells = [set() for _ in range(n_cells)]
    for pitch, a, b in placed:
        if 0 < a < n_cells and pitch in cells[a - 1]:
            cells[a - 1].discard(pitch)
        if b < n_cells - 1 and pitch in cells[b]:
            b -= 1
        for c in range(a, min(b, n_cells)):
            cells[c].add(pitch)
    rhythm = [0 if not s else 1 if c == 0 or not s <= cells[c - 1] else 2 for c, s in enumerate(cells)]
    notes = [len(s) for s in cells]
    roll = np.zeros((n_cells, 128), bool)
    for c, s in enumerate(cells):
        roll[c, sorted(s)] = True
    return _finish(n_cells, rhythm.count(1), sum(notes), rhythm, notes, cells_ld, dict(roll=roll))


def attributes_words(row, p, cells_ld=MAX_CELLS):
    """statement 2: a bit column per pitch (bit c = cell c), transposed into one word of pitch bits per cell"""
    n_cells, placed = grid_of(tokens_to_notes(row, p), p)
    if n_cells > cells_ld:
        return _finish(n_cells, 0, 0, None, None, cells_ld, dict(roll=None))
    col = [0] * 128
    for pitch, a, b in placed:
        if 0 < a < n_cells:
            col[pitch] &= ~(1 << (a - 1))
        if b < n_cells - 1 and (col[pitch] >> b) & 1:
            b -= 1
        hi = min(b, n_cells)
        if hi > a:
            col[pitch] |= (1 << hi) - (1 << a)
    words = [sum(((col[q] >> c) & 1) << q for q in range(128)) for c in range(n_cells)]
    rhythm, notes, prev = [], [], 0
    for c, w in enumerate(words):
        notes.append(bin(w).count("1"))
        rhythm.append(0 if w == 0 else 1 if c == 0 or w & ~prev else 2)
        prev = w
    roll = np.array([[(w >> q) & 1 for q in range(128)] for w in words], dtype=bool).reshape(n_cells, 128)
    return _finish(n_cells, rhythm.count(1), sum(notes), rhythm, notes, cells_ld, dict(roll=roll))


OUT_KEYS = ("n_cells", "status", "r_density", "n_density", "c_r", "c_n")
OUT_DTYPES = dict(n_cells=np.int32, status=np.int32, r_density=np.float32, n_density=np.float32, c_r=np.int32, c_n=np.int32)


def event_attributes_ref(tokens, steps, p, cells_ld, statement=attributes_words):
    """tokens (rows, >= steps) -> dict of (rows,) arrays + rhythm, notes (rows, cells_ld) uint8"""
    rows = [statement(r[:steps], p, cells_ld) for r in np.asarray(tokens)]
    out = {k: np.array([r[k] for r in rows], dtype=OUT_DTYPES[k]) for k in OUT_KEYS}
    out["rhythm"], out["notes"] = np.stack([r["rhythm"] for r in rows]), np.stack([r["notes"] for r in rows])
    return out


def same_attributes(got, ref, tag="", cells=True):
    for k in OUT_KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, k, g.dtype, r.dtype, g.shape, r.shape)
        same = g.view(np.int32) == r.view(np.int32) if g.dtype == np.float32 else g == r
        if g.dtype == np.float32:
            same = same | (np.isnan(g) & np.isnan(r))
        assert same.all(), (tag, k, np.argwhere(~same)[:4].tolist(), g[~same][:4], r[~same][:4])
    if cells:
        for k in ("rhythm", "notes"):
            assert np.array_equal(got[k], ref[k]), (tag, k, np.argwhere(got[k] != ref[k])[:4].tolist())


# ------------------------------------------------------------------------------------------------------------------------------
# the scores
# ------------------------------------------------------------------------------------------------------------------------------
def _asc(xs):
    acc = np.float64(0.0)
    for x in xs:
        acc = acc + np.float64(x)
    return acc


def _over_samples(terms):
    """terms: [(s, value)] of the used samples, ascending: 16 partial sums by s % 16, then a[i] += a[i + h], h = 8, 4, 2, 1"""
    a = [np.float64(0.0)] * 16
    for s, x in terms:
        a[s % 16] = a[s % 16] + np.float64(x)
    h = 8
    while h:
        for i in range(h):
            a[i] = a[i] + a[i + h]
        h //= 2
    return a[0]


def sweep_scores_ref(r, n, status, values, which, r_std, n_std):
    """-> dict(consistency, restrictiveness, monotonicity, variance, n_used), fp64"""
    r, n, values = np.asarray(r, np.float32).astype(np.float64), np.asarray(n, np.float32).astype(np.float64), np.asarray(values, np.float64)
    S, Vn = r.shape
    used = [s for s in range(S) if not np.asarray(status)[s].any()]
    nan = float("nan")
    if not used:
        return dict(consistency=nan, restrictiveness=nan, monotonicity=nan, variance=nan, n_used=0)
    y = r if which == 0 else n
    x = y / np.float64(r_std if which == 0 else n_std)
    o = (n if which == 0 else r) / np.float64(n_std if which == 0 else r_std)

    def pstd(v):
        m = _asc(v) / len(v)
        return np.sqrt(_asc((v - m) ** 2) / len(v))

    vbar = _asc(values) / Vn
    sxx = _asc((values - vbar) ** 2)
    r2 = {}
    for s in used:
        ybar = _asc(y[s]) / Vn
        sxy, ss_tot = _asc((values - vbar) * (y[s] - ybar)), _asc((y[s] - ybar) ** 2)
        slope = sxy / sxx if sxx != 0 else np.float64(0.0)
        ss_res = _asc((y[s] - ((ybar - slope * vbar) + slope * values)) ** 2)
        r2[s] = np.float64(1.0) if ss_tot == 0 else 1.0 - ss_res / ss_tot
    nu = len(used)
    col = []
    for v in range(Vn):
        m = _over_samples([(s, x[s, v]) for s in used]) / nu
        col.append(np.sqrt(_over_samples([(s, (x[s, v] - m) ** 2) for s in used]) / nu))
    return dict(consistency=float(1.0 - _asc(col) / Vn), restrictiveness=float(1.0 - _over_samples([(s, pstd(o[s])) for s in used]) / nu),
                monotonicity=float(_over_samples([(s, r2[s]) for s in used]) / nu), variance=float(_over_samples([(s, pstd(x[s])) for s in used]) / nu),
                n_used=nu)


SCORE_KEYS = ("consistency", "restrictiveness", "monotonicity", "variance")


def same_scores(got, ref, tol, tag=""):
    assert got["n_used"] == ref["n_used"], (tag, got["n_used"], ref["n_used"])
    for k in SCORE_KEYS:
        g, r = float(got[k]), float(ref[k])
        assert (np.isnan(g) and np.isnan(r)) or abs(g - r) <= tol, (tag, k, g, r, abs(g - r))


# ------------------------------------------------------------------------------------------------------------------------------
# streams
# ------------------------------------------------------------------------------------------------------------------------------
def _tok(p):
    on, off = (lambda q: p["on_lo"] + q), (lambda q: p["off_lo"] + q)
    sh = lambda k: p["shift_lo"] + k - 1          # k ticks
    return on, off, sh


def hand_rows(p=DEFAULT):
    """every row with a kept note lasts a beat (50 ticks) at least: below that the reference's fill raises (one beat time, polyphonic_event_based_v2.py:329)"""
    on, off, sh = _tok(p)
    E = p["eos"]
    return collections.OrderedDict([
        ("empty", []),
        ("eos first", [E, on(40), sh(50), off(40)]),
        ("only shifts", [sh(50)] * 5),
        ("one note never closed", [on(40), sh(100), sh(30)]),
        ("same pitch back to back: the cleared cell", [on(40), sh(25), off(40), on(40), sh(25), off(40)]),
        ("a one-cell note that vanishes", [on(40), sh(13), off(40), on(40), sh(40), off(40)]),
        ("re-strike while sounding", [on(40), sh(30), on(40), sh(30), off(40)]),
        ("a >= b: a kept note that fills nothing", [sh(57), on(40), sh(5), off(40)]),
        ("a == n_cells", [sh(94), on(40), sh(5), off(40)]),
        ("a == n_cells beside a note that fills", [on(30), sh(94), on(40), sh(5), off(40), off(30)]),
        ("note-off without a note-on", [off(50), sh(20), on(40), sh(30), off(40), off(40)]),
        ("zero-length notes are dropped", [on(40), off(40), sh(30), on(41), on(41), off(41), on(42), sh(60), off(42)]),
        ("eos mid-row with notes behind it", [on(40), sh(50), off(40), E, on(60), sh(100), off(60)]),
        ("pad and velocity tokens between", [on(40), VEL_LO + 22, PAD, sh(50), PAD, on(43), VEL_LO + 32, sh(25), off(40), sh(25), off(43)]),
        ("chords: hold, onset, subset", [on(40), on(44), sh(50), off(44), sh(50), on(47), sh(50), off(40), off(47), sh(25), on(40), on(47), sh(25)]),
        ("dense: first and last pitch", [on(0), on(p["n_pitch"] - 1), sh(100), sh(100), off(0), sh(63), off(p["n_pitch"] - 1)]),
        ("rest between notes", [on(20), sh(12), off(20), sh(100), on(21), sh(37), off(21)]),
        ("an onset in every cell: c_r 2", sum(([on(40 + i % 2), sh(13 - i % 2), off(40 + i % 2)] for i in range(30)), [])),
        ("onsets in two cells of five: c_r 1", sum(([on(40 + i % 2), sh(25 if i % 2 == 0 else 38 - (i // 2) % 2), off(40 + i % 2)] for i in range(16)), [])),
    ])


def random_row(rs, p, steps, grammar, eos_at=None):
    """a seeded stream of `steps` tokens: note-ons / note-offs of a handful of pitches, shifts, pad and velocity; with `grammar` a note-on only for a
    silent pitch and a note-off only for a sounding one"""
    on, off, sh = _tok(p)
    pitches = rs.choice(p["n_pitch"], size=rs.randint(3, 12), replace=False)
    if p["n_pitch"] > 96:
        pitches = np.concatenate([pitches, [0, 31, 32, 63, 64, 95, 96, p["n_pitch"] - 1]])
    held, row = set(), []
    for i in range(steps):
        if eos_at is not None and i == eos_at:
            row.append(p["eos"])
            continue
        u = rs.rand()
        q = int(pitches[rs.randint(len(pitches))])
        if u < 0.3:
            if grammar and q in held:
                q = next((int(x) for x in pitches if int(x) not in held), None)
            if q is None:
                row.append(sh(1 + rs.randint(100)))
            else:
                row.append(on(q)), held.add(q)
        elif u < 0.55:
            if grammar and q not in held:
                q = next(iter(sorted(held)), None)
            if q is None:
                row.append(PAD)
            else:
                row.append(off(q)), held.discard(q)
        elif u < 0.9:
            row.append(sh(1 + int(rs.randint(100) * rs.rand())))
        else:
            row.append(PAD if u < 0.93 else VEL_LO + rs.randint(64))
    return row


def fixture_streams(steps=100):
    """-> [(group, params, names, tokens (rows, steps) int32 padded with PAD)]: what tests/golden/attributes.npz holds"""
    groups = []
    hand = hand_rows()
    rs = np.random.RandomState(20261019)
    rows = list(hand.values())
    names = list(hand)
    for i in range(14):
        grammar = i % 2 == 1
        rows.append(random_row(rs, DEFAULT, steps if i != 5 else 37, grammar, eos_at=60 if i == 8 else None))
        names.append("random %d%s" % (i, " grammar" if grammar else ""))
    groups.append(("d", DEFAULT, names, rows))
    rows = [random_row(rs, WIDE, steps, i % 2 == 1) for i in range(8)]
    groups.append(("w", WIDE, ["wide %d%s" % (i, " grammar" if i % 2 else "") for i in range(8)], rows))
    out = []
    for g, p, names, rows in groups:
        tok = np.full((len(rows), steps), PAD, dtype=np.int32)
        for i, r in enumerate(rows):
            assert len(r) <= steps
            tok[i, :len(r)] = r
        out.append((g, p, names, tok))
    return out


def score_cases():
    """-> [(tag, r (S, 8) fp32, n, status, values fp64, which, r_std, n_std)]: S 1 / 5 / 67, flat, linear and decreasing rows, invalid entries"""
    rs = np.random.RandomState(7)
    cases = []
    for S in (1, 5, 67):
        for which in (0, 1):
            values = np.array([-2.0 + k * 0.5 for k in range(8)]) if which == 0 else np.array([-3.0 + k * (5.5 / 8) for k in range(8)])
            r = (rs.randint(0, 129, (S, 8)) / 128.0).astype(np.float32)
            n = (rs.randint(0, 1025, (S, 8)) / 128.0).astype(np.float32)
            sw = r if which == 0 else n
            sw[0] = 0.25                                                  # flat: SS_tot == 0
            if S > 1:
                sw[1] = (0.125 + 0.0625 * np.arange(8)).astype(np.float32)        # a line over equally spaced values
                sw[2] = np.sort(sw[2])[::-1]                                # decreasing
                (n if which == 0 else r)[3] = 1.5                           # the other attribute flat
            status = np.zeros((S, 8), np.int32)
            cases.append(("S%d which%d" % (S, which), r.copy(), n.copy(), status.copy(), values, which, 0.1875, 1.375))
            if S > 1:
                status[4, 3], status[S - 1, 0] = EMPTY, OVERFLOW
                if S > 16:
                    status[16:33:4, 7] = EMPTY
                cases.append(("S%d which%d invalid" % (S, which), r.copy(), n.copy(), status.copy(), values, which, 0.1875, 1.375))
    return cases


def unused_scores_case():
    tag, r, n, status, values, which, r_std, n_std = score_cases()[2]
    status = status.copy()
    status[:, 1] = EMPTY
    return (tag + " nothing used", r, n, status, values, which, r_std, n_std)


# ------------------------------------------------------------------------------------------------------------------------------
# the case list of the host twin and the kernels
# ------------------------------------------------------------------------------------------------------------------------------
CASE_SHAPES = [(rows, steps) for rows in (1, 5, 67) for steps in (1, 7, 100, 300)]
SENTINEL_TOK = 2 + 40          # a note-on in the default vocabulary: a sentinel column that is read changes the result
SENTINEL_CELL = 0xA5


def cells_ld_for(steps, p):
    """what attributes.event_attributes allocates: every row of `steps` tokens fits"""
    p = clamped(p)
    num, den, bc = p["ticks_num"], p["ticks_den"], p["beat_cells"]
    return min(MAX_CELLS, bc * ((steps * p["n_shift"] * den) // (num * bc) + 1))


def kernel_cases():
    """-> [dict(tag, p, tok (rows, tok_ld) int32, steps, cells_ld)]: the fixture rows, rows x steps with tok_ld = steps + 3 and sentinel columns, a cells_ld
    that one row overflows, parameters to clamp"""
    cases = []
    for g, p, names, tok in fixture_streams():
        cases.append(dict(tag="fixture " + g, p=p, tok=tok, steps=tok.shape[1], cells_ld=cells_ld_for(tok.shape[1], p)))
    for rows, steps in CASE_SHAPES:
        rs = np.random.RandomState(1000 * rows + steps)
        tok = np.full((rows, steps + 3), SENTINEL_TOK, dtype=np.int32)
        for i in range(rows):
            tok[i, :steps] = random_row(rs, DEFAULT, steps, i % 3 == 0, eos_at=(steps // 2 if i % 5 == 4 else None))
        cases.append(dict(tag="%dx%d" % (rows, steps), p=DEFAULT, tok=tok, steps=steps, cells_ld=cells_ld_for(steps, DEFAULT)))
    # one row overflows cells_ld = 40 beside rows that fit, and one fills it exactly
    on, off, sh = _tok(DEFAULT)
    rs = np.random.RandomState(5)
    tok = np.full((6, 60 + 3), SENTINEL_TOK, dtype=np.int32)
    tok[:, :60] = PAD
    tok[0, :5] = [on(40), sh(100), sh(100), sh(100), off(40)]                   # 300 ticks: 28 cells
    tok[1, :9] = [on(41)] + [sh(100)] * 7 + [off(41)]                            # 700 ticks: 60 cells > 40
    tok[2, :6] = [on(42), sh(100), sh(100), sh(100), sh(100), sh(99)]           # 499 ticks: 40 cells, never closed
    tok[3, :60] = random_row(rs, DEFAULT, 60, False)                              # long
    tok[4, :7] = [on(43), sh(100), sh(100), sh(100), sh(100), sh(100), off(43)]  # 500 ticks: 44 cells > 40
    cases.append(dict(tag="cells_ld 40 overflows", p=DEFAULT, tok=tok, steps=60, cells_ld=40))
    cases.append(dict(tag="cells_ld 1", p=DEFAULT, tok=tok, steps=60, cells_ld=1))
    # both caps at once (36 KB of LDS): 1024 steps, 2048 cells; one row of the longest shifts under a held note overflows with its true n_cells
    rs = np.random.RandomState(8)
    tok = np.stack([random_row(rs, DEFAULT, MAX_STEPS, i == 1) for i in range(3)]).astype(np.int32)
    tok[2, 0], tok[2, 1:] = on(40), sh(100)
    cases.append(dict(tag="1024 steps, 2048 cells", p=dict(DEFAULT, eos=-1), tok=tok, steps=MAX_STEPS, cells_ld=MAX_CELLS))
    # parameters to clamp: n_pitch 200 counts as 128, the ranges are cut by vocab_size, other grids
    rs = np.random.RandomState(6)
    base = np.stack([random_row(rs, WIDE, 100, i % 2 == 0) for i in range(5)]).astype(np.int32)
    base[0, 10], base[1, 20], base[2, 5] = 100000, -7, 399
    cases.append(dict(tag="n_pitch 200", p=dict(WIDE, n_pitch=200, vocab_size=0), tok=base, steps=100, cells_ld=MAX_CELLS))
    cases.append(dict(tag="vocab_size cuts the ranges", p=dict(WIDE, vocab_size=300), tok=base, steps=100, cells_ld=MAX_CELLS))
    cases.append(dict(tag="vocab_size cuts every shift", p=dict(WIDE, vocab_size=200), tok=base, steps=100, cells_ld=MAX_CELLS))
    cases.append(dict(tag="no eos, n_shift 5000, triplet grid", p=dict(WIDE, eos=-1, n_shift=5000, ticks_num=50, ticks_den=3, beat_cells=3, vocab_size=0),
                      tok=base, steps=100, cells_ld=700))
    cases.append(dict(tag="zeros to clamp", p=dict(DEFAULT, ticks_num=0, ticks_den=-4, beat_cells=0, n_shift=3), tok=base[:, :50].copy() % 342, steps=50,
                      cells_ld=MAX_CELLS))
    cases.append(dict(tag="negative n_pitch", p=dict(DEFAULT, n_pitch=-3), tok=base[:, :50].copy() % 342, steps=50, cells_ld=64))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# CPU stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def params_from_bytes(b):
    raw = np.asarray(b, dtype=np.uint8).view(PARAMS_DTYPE)[0]
    return {k: int(raw[k]) for k in FIELDS}


def attr_fake_ops():
    """the decode stand-ins + fn_event_attributes / fn_sweep_scores as their restatement (imported here: the golden generator takes this module
    without the package)"""
    from helpers_constrain import ConstrainFakeOps

    class AttrFakeOps(ConstrainFakeOps):
        def event_attributes(self, tokens, steps, params, n_cells, status, r_density, n_density, c_r, c_n, rhythm=None, notes=None, cells_ld=MAX_CELLS):
            self.calls.append("event_attributes")
            ref = event_attributes_ref(tokens.numpy(), steps, params_from_bytes(params.numpy()), cells_ld)
            for k, t in zip(OUT_KEYS, (n_cells, status, r_density, n_density, c_r, c_n)):
                t.copy_(torch.from_numpy(ref[k]))
            for k, t in (("rhythm", rhythm), ("notes", notes)):
                if t is not None:
                    t.copy_(torch.from_numpy(ref[k]))

        def sweep_scores(self, r, n, status, values, which, r_std, n_std, scores, n_used):
            self.calls.append("sweep_scores")
            ref = sweep_scores_ref(r.numpy(), n.numpy(), status.numpy(), values.numpy(), which, r_std, n_std)
            scores.copy_(torch.tensor([ref[k] for k in SCORE_KEYS], dtype=torch.float64))
            n_used.fill_(ref["n_used"])

    return AttrFakeOps()
