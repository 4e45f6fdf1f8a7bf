"""Latent-side drivers of a GM-VAE that need no source piece, or two: generation from the mixture prior (prior_latents, generate: a draw from
N(mu_lookup[k], (temperature * exp(logvar_lookup[k] / 2))^2) by fn_latent_draw on the seeded Philox streams sample_decode uses) and morphing between two
pieces (mix_latents, morph: fn_latent_mix along a path of points, the whole path one decode batch), with latent_classes = approx_qy_x on given latents.
OURS: the reference has the prior's tables (gmm_model.py:151-183) and the class posterior (:194-218) and uses neither this way; include/fadernets.h has
the definitions at fn_latent_draw.  The decoders (decode._decode_rows) and the way out (tokens_to_notes, write_midis) are the existing ones."""
import argparse

import numpy as np
import torch

from . import _lib
from .constrain import _int
from .decode import _check_beam, _check_steps, _constraints_arg, _decode_rows, _is_finite, _is_int

LERP, SLERP, STEP = _lib.FN_MIX_LERP, _lib.FN_MIX_SLERP, _lib.FN_MIX_STEP
MODES = {"lerp": LERP, "slerp": SLERP}
CHROMA = 24
MAX_ROWS = 1 << 20


def _component(name, v, rows, K):
    """None (drawn per row), an int (every row) or (rows,) ints -> None or a CPU int32 array (rows,)"""
    if v is None:
        return None
    if _is_int(v):
        return np.full(rows, _int(name, v, 0, K), np.int32)
    arr = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)
    if arr.shape != (rows,) or arr.dtype.kind not in "iu" or (arr < 0).any() or (arr >= K).any():
        raise ValueError("%s: None, an int or (%d,) ints in [0, %d), got %r" % (name, rows, K, v))
    return arr.astype(np.int32)


def _chroma_rows(key, chroma, rows):
    """exactly one of key (an int in [0, 24): one-hot at tonic + 12 * minor) and chroma ((24,) or (rows, 24)) -> a CPU fp32 tensor (24,) or (rows, 24)"""
    if (key is None) == (chroma is None):
        raise ValueError("exactly one of key and chroma, got key=%r chroma=%r" % (key, None if chroma is None else "given"))
    if key is not None:
        c = torch.zeros(CHROMA)
        c[_int("key", key, 0, CHROMA)] = 1.0
        return c
    try:
        c = chroma.detach() if torch.is_tensor(chroma) else torch.as_tensor(np.asarray(chroma, dtype=np.float32))
    except (TypeError, ValueError):
        raise ValueError("chroma: (24,) or (%d, 24) numbers, got %r" % (rows, chroma))
    if tuple(c.shape) not in ((CHROMA,), (rows, CHROMA)) or c.is_complex() or c.dtype == torch.bool:
        raise ValueError("chroma: (24,) or (%d, 24) numbers, got shape %s" % (rows, tuple(c.shape)))
    return c.float()


def _prior_args(model, rows, rhythm, note, key, chroma, temperature, seed, offset):
    """validated (rows, comp_r, comp_n, chroma rows, the 32 bytes of FnDrawParams as a CPU uint8 tensor); ValueError before anything is launched"""
    rows = _int("rows", rows, 1, MAX_ROWS + 1)
    K = model.n_component
    comp = [_component(nm, v, rows, K) for nm, v in (("rhythm", rhythm), ("note", note))]
    c = _chroma_rows(key, chroma, rows)
    if not _is_finite(temperature) or temperature < 0:
        raise ValueError("temperature: a finite number >= 0, got %r" % (temperature,))
    for name, v in (("seed", seed), ("offset", offset)):
        if not _is_int(v) or not 0 <= int(v) < 1 << 64:
            raise ValueError("%s: an int in [0, 2^64), got %r" % (name, v))
    raw = np.zeros(1, dtype=[("seed", "<u8"), ("offset", "<u8"), ("tau", "<f4"), ("reserved", "<i4", (3,))])
    with np.errstate(over="ignore"):
        raw["seed"], raw["offset"], raw["tau"] = int(seed), int(offset), np.float32(temperature)
    return rows, comp[0], comp[1], c, torch.from_numpy(raw.view(np.uint8).copy())


def _draw(model, rows, comp_r, comp_n, c, params):
    eng = model.engine()
    ops, dev, Z, K = eng.ops, model._device(), model.latent_dim, model.n_component
    z = torch.empty(rows, 2 * Z + CHROMA, device=dev)
    z[:, 2 * Z:] = c.to(dev)
    comps = torch.empty(2, rows, dtype=torch.int32, device=dev)
    jobs = []
    for s, (e, comp) in enumerate((("r", comp_r), ("n", comp_n))):
        mu, lv = (getattr(model, "%s_%s_lookup" % (w, e)).weight.data[:K].float().contiguous() for w in ("mu", "logvar"))
        jobs.append(dict(mu_lk=mu, lv_lk=lv, comp=None if comp is None else torch.from_numpy(comp).to(dev), z=z[:, s * Z:(s + 1) * Z], comp_out=comps[s],
                         stream_id=s))
    ops.latent_draw(jobs, params.to(dev))
    return z, comps.t()


@torch.no_grad()
def prior_latents(model, rows, rhythm=None, note=None, key=None, chroma=None, temperature=1.0, seed=0, offset=0):
    """Latents from the mixture prior, no source piece: -> (z (rows, 2Z+24) fp32, comps (rows, 2) int32: the rhythm and note component of every row).

    rhythm, note  the component z_r / z_n is drawn from (with the reference's two classes: 0 = low, 1 = high density): None = drawn uniformly per row,
                  an int = that component for every row, (rows,) ints = one per row.
    key, chroma   exactly one: key, an int in [0, 24), gives a one-hot chroma at tonic + 12 * minor (the layout of estimate_chroma(one_hot=True));
                  chroma is (24,) or (rows, 24).
    temperature   scales the component's sigma; 0 gives the component means.  seed, offset: the Philox key and counter words, as sample_decode takes
                  them; stream 0 is the rhythm latent, stream 1 the note latent.  The same (seed, offset) gives the same row b whatever `rows` is.
    ONE fn_latent_draw call with two jobs writes into the returned tensor; the host sends the 32 parameter bytes, given components and the chroma.
    ValueError for anything that is not as described, before anything is launched."""
    return _draw(model, *_prior_args(model, rows, rhythm, note, key, chroma, temperature, seed, offset))


def _check_decode(rows, steps, prompt, sample, beam, constraints):
    """the decode keywords as fader_sweep checks them, and what else can be said without a launch"""
    _check_steps(steps)
    _check_beam(steps, prompt, sample, beam)
    if sample is not None:
        unknown = set(sample) - {"temperature", "top_k", "top_p", "seed", "offset"}
        if unknown:
            raise ValueError("sample: keys among temperature, top_k, top_p, seed, offset; got %s" % sorted(unknown, key=str))
    _constraints_arg(constraints, rows, None if beam is None else beam.get("eos"), beam=beam is not None)


@torch.no_grad()
def generate(model, rows, steps=100, rhythm=None, note=None, key=None, chroma=None, temperature=1.0, seed=0, offset=0, prompt=None, sample=None,
             beam=None, constraints=None):
    """prior_latents, then the decode fader_sweep's keywords select (prompt, sample, beam, constraints as it takes them; none: greedy)
    -> (tokens (rows, steps) int32, z (rows, 2Z+24), comps (rows, 2) int32).  temperature, seed and offset are the latent draw's; a sampled decode
    has its own in `sample`."""
    args = _prior_args(model, rows, rhythm, note, key, chroma, temperature, seed, offset)
    _check_decode(args[0], steps, prompt, sample, beam, constraints)
    was_training = model.training
    model.eval()
    try:
        z, comps = _draw(model, *args)
        return _decode_rows(model, z, steps, prompt, sample, beam, constraints), z, comps
    finally:
        model.train(was_training)


def _segments(model, mode):
    """the three segments of a (.., 2Z+24) latent row: z_r and z_n in `mode`, the chroma columns as a step"""
    if mode not in MODES:
        raise ValueError("mode: 'slerp' or 'lerp', got %r" % (mode,))
    Z = model.latent_dim
    return [(0, Z, MODES[mode]), (Z, Z, MODES[mode]), (2 * Z, CHROMA, STEP)]


def _path(t, n, per_pair=False):
    """the points of the path as a CPU fp32 tensor (P,), or (n, P) with per_pair; finite, and at most MAX_ROWS mixed rows"""
    try:
        tt = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("t: finite numbers, got %r" % (t,))
    if tt.ndim != (2 if per_pair else 1) or tt.size < 1 or (per_pair and tt.shape[0] != n) or not np.isfinite(tt).all():
        raise ValueError("t: %s finite numbers, got shape %s" % ("(%d, P)" % n if per_pair else "(P,)", tt.shape))
    if n * tt.shape[-1] > MAX_ROWS:
        raise ValueError("at most %d mixed rows, got %d * %d" % (MAX_ROWS, n, tt.shape[-1]))
    return torch.from_numpy(np.ascontiguousarray(tt))


def _mix(model, za, zb, t, segs, per_pair):
    ops, dev = model.engine().ops, model._device()
    za, zb = za.to(dev).float().contiguous(), zb.to(dev).float().contiguous()
    n, D = za.shape
    P = t.shape[-1]
    z = torch.empty(n, P, D, device=dev)
    omega = torch.empty(n, len(segs), device=dev)
    ops.latent_mix(za, zb, t.to(dev), segs, z.view(n * P, D), omega_out=omega, per_pair=bool(per_pair))
    return z, omega[:, :2]


@torch.no_grad()
def mix_latents(model, za, zb, t, mode="slerp", per_pair=False):
    """The path between the latents of two pieces: za, zb (n, 2Z+24) -> (z (n, P, 2Z+24), omega (n, 2)) in ONE fn_latent_mix call.

    t         P finite numbers, shared by the pairs, or (n, P) with per_pair=True; 0 gives za's row, 1 zb's, exactly; outside [0, 1] extrapolates.
    mode      "slerp": z_r and z_n each turn through the angle between the pair's raw vectors (the mix MusicVAE-style models use); "lerp": the
              straight line.  The 24 chroma columns step from za's to zb's at t = 0.5 in both.
    omega     the angles of z_r and z_n in radians; 0 with "lerp", -1 where a pair's vectors are (anti)parallel or zero and its slice went straight.
    ValueError for anything that is not as described, before anything is launched."""
    segs = _segments(model, mode)
    D = 2 * model.latent_dim + CHROMA
    if not isinstance(per_pair, (bool, np.bool_)):
        raise ValueError("per_pair: a bool, got %r" % (per_pair,))
    for name, v in (("za", za), ("zb", zb)):
        if not torch.is_tensor(v) or not v.is_floating_point() or v.dim() != 2 or v.shape[1] != D or v.shape[0] < 1:
            raise ValueError("%s: a float tensor (n, %d), got %s" % (name, D, tuple(v.shape) if torch.is_tensor(v) else type(v).__name__))
    if za.shape != zb.shape:
        raise ValueError("za and zb: the same shape, got %s and %s" % (tuple(za.shape), tuple(zb.shape)))
    return _mix(model, za, zb, _path(t, za.shape[0], per_pair), segs, per_pair)


@torch.no_grad()
def morph(model, xa, ca, xb, cb, points=8, t=None, steps=100, mode="slerp", eps=None, prompt=None, sample=None, beam=None, constraints=None):
    """Morph piece A into piece B: -> (tokens (n, P, steps) int32, z (n, P, 2Z+24), omega (n, 2)).

    xa, xb    (n, T) token ids or (n, T, 342) one-hot, as encode takes them; ca, cb (n, 24) chroma.  ONE encode covers the 2n rows.
    points    P, with t = linspace(0, 1, P); or t: P finite numbers of its own (mix_latents').  mode: mix_latents'.
    eps       None: the latents are the posterior means; else (eps_r, eps_n), each (2n, Z): A's rows first, then B's.
    prompt, sample, beam, constraints: as fader_sweep takes them (a per-row bias has n * P rows).  ONE decode covers the n * P rows.
    ValueError for anything that is not as described, before anything is launched."""
    Z = model.latent_dim
    if not all(torch.is_tensor(v) for v in (xa, xb, ca, cb)) or xa.shape != xb.shape or xa.dim() not in (2, 3) or xa.shape[0] < 1:
        raise ValueError("xa, xb: tensors of one shape (n, T) or (n, T, %d); ca, cb: tensors (n, %d)" % (model.roll_dims, CHROMA))
    n = xa.shape[0]
    if tuple(ca.shape) != (n, CHROMA) or tuple(cb.shape) != (n, CHROMA):
        raise ValueError("ca, cb: (%d, %d), got %s and %s" % (n, CHROMA, tuple(ca.shape), tuple(cb.shape)))
    if t is None:
        t = np.linspace(0.0, 1.0, _int("points", points, 1, MAX_ROWS + 1), dtype=np.float32)
    if eps is not None and (not isinstance(eps, (tuple, list)) or len(eps) != 2 or not all(torch.is_tensor(e) and tuple(e.shape) == (2 * n, Z) for e in eps)):
        raise ValueError("eps: None or (eps_r, eps_n), each (%d, %d)" % (2 * n, Z))
    segs, tt = _segments(model, mode), _path(t, n)
    P = tt.shape[0]
    _check_decode(n * P, steps, prompt, sample, beam, constraints)
    was_training = model.training
    model.eval()
    try:
        dis_r, dis_n = model.encode(torch.cat([xa, xb]))
        zr, zn = dis_r.mean, dis_n.mean
        if eps is not None:
            zr, zn = zr + dis_r.stddev * eps[0].to(zr.device).float(), zn + dis_n.stddev * eps[1].to(zn.device).float()
        c = torch.cat([ca, cb]).to(zr.device).float()
        zab = torch.cat([zr, zn, c], dim=1)
        z, omega = _mix(model, zab[:n], zab[n:], tt, segs, False)
        D = z.shape[2]
        return _decode_rows(model, z.view(n * P, D), steps, prompt, sample, beam, constraints).view(n, P, steps), z, omega
    finally:
        model.train(was_training)


@torch.no_grad()
def latent_classes(model, z):
    """The class posterior of given latents: z (rows, 2Z+24) or (rows, 2Z) -> (qy_r, qy_n (rows, K) fp32, y_r, y_n (rows,) int32: the most likely
    component).  approx_qy_x (gmm_model.py:194-218) through fn_latent_fwd with pre = [z | 0] and eps = 0, which reproduces z exactly; no kernel of its own."""
    Z, K = model.latent_dim, model.n_component
    if not torch.is_tensor(z) or not z.is_floating_point() or z.dim() != 2 or z.shape[1] not in (2 * Z, 2 * Z + CHROMA) or z.shape[0] < 1:
        raise ValueError("z: a float tensor (rows, %d) or (rows, %d), got %s" % (2 * Z + CHROMA, 2 * Z, tuple(z.shape) if torch.is_tensor(z) else type(z).__name__))
    ops, dev = model.engine().ops, model._device()
    z = z.to(dev).float()
    B = z.shape[0]
    out = []
    zero = torch.zeros(B, Z, device=dev)
    for s, e in enumerate("rn"):
        pre = torch.cat([z[:, s * Z:(s + 1) * Z], zero], dim=1).contiguous()          # mu = z, log sigma = 0
        mu, lv = (getattr(model, "%s_%s_lookup" % (w, e)).weight.data[:K].float().contiguous() for w in ("mu", "logvar"))
        sigma, zz = torch.empty(B, Z, device=dev), torch.empty(B, Z, device=dev)
        ll, qy = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
        y = torch.empty(B, dtype=torch.int32, device=dev)
        ops.latent_fwd(pre, zero, mu, lv, None, sigma, zz, ll, qy, y, torch.empty(B, 4, device=dev))
        out.append((qy, y))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def main(argv=None):
    """``python generate_midi.py --config gmm_model_config.json [--params model.pt] OUT_DIR [--rows 8] [--rhythm 1] [--note 0] [--key 0]``"""
    from .gmm_model import MusicAttrRegGMVAE
    from .midi import write_midis
    from .train import CHROMA_DIMS, EVENT_DIMS, NOTE_DIMS, RHYTHM_DIMS, read_config
    ap = argparse.ArgumentParser(prog="generate_midi", description="generate MIDI files from the mixture prior of a trained GM-VAE")
    ap.add_argument("--config", required=True, help="the reference's JSON config (gmm_model_config.json)")
    ap.add_argument("--params", help="a state_dict saved by the trainer; without it seeded initial weights are used (a smoke path)")
    ap.add_argument("dst", metavar="OUT_DIR", help="the directory the files 00000.mid ... are written into")
    ap.add_argument("--rows", type=int, default=8, help="the number of pieces (default 8)")
    ap.add_argument("--steps", type=int, default=100, help="the tokens decoded per piece (default 100)")
    ap.add_argument("--rhythm", type=int, default=None, help="the rhythm-density component (0 low, 1 high); default: drawn per piece")
    ap.add_argument("--note", type=int, default=None, help="the note-density component (0 low, 1 high); default: drawn per piece")
    ap.add_argument("--key", type=int, default=0, help="the key, tonic + 12 * minor in [0, 24) (default 0: C major)")
    ap.add_argument("--temperature", type=float, default=1.0, help="scales the prior's sigma; 0 decodes the component means (default 1.0)")
    ap.add_argument("--seed", type=int, default=0, help="the seed of the latent draw and of the initial weights")
    opts = ap.parse_args(argv)
    args = read_config(opts.config, "gmm")
    if not torch.cuda.is_available():
        raise SystemExit("generate_midi: no GPU visible - this package runs on the MI355X HIP kernels only (there is deliberately no CPU fallback)")
    torch.manual_seed(opts.seed)
    model = MusicAttrRegGMVAE(roll_dims=EVENT_DIMS, rhythm_dims=RHYTHM_DIMS, note_dims=NOTE_DIMS, chroma_dims=CHROMA_DIMS, hidden_dims=args["hidden_dim"],
                              z_dims=args["z_dim"], n_step=args["time_step"], n_component=args["num_clusters"])
    if opts.params:
        model.load_state_dict(torch.load(opts.params, map_location="cpu"))
    else:
        print("generate_midi: no --params given - seeded initial weights (seed %d), the output shows the path and not a model" % opts.seed)
    model = model.cuda()
    try:
        tokens, _, comps = generate(model, opts.rows, opts.steps, rhythm=opts.rhythm, note=opts.note, key=opts.key, temperature=opts.temperature,
                                    seed=opts.seed)
    except ValueError as e:
        raise SystemExit("generate_midi: %s" % e)
    paths = write_midis(opts.dst, tokens)
    print("generate_midi: %d pieces -> %s (components %s)" % (len(paths), opts.dst, comps.tolist()))
