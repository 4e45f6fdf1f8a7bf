"""Shared code of tests/test_cell_reference.py (CPU) and tests/test_gpu_cell_paths.py (MI355X): the large-batch GRU cell fn_gru_cell_f32 - gru_cell_kernel
(staged), gru_cell_direct_kernel, gru_cell_wlds_kernel, gru_cell_wlds_ovl_kernel and gru_cell_x6_kernel of csrc/gru.hip, decided by gru_cell_plan of
csrc/gru_plan.h - per 16 x 16 tile of h_out against float64, on operand views and K tails.

  cell_reference(inp, dtype)   the semantics of FakeOps.gru_cell on dense CPU inputs: float64 = the reference, float32 = the restatement
  cell_x6_restate(inp, hook)   the float32 restatement of the bf16 x 6 cell: batch rows cut truncated, weight rows cut rounded (helpers_gemm_x6.split3), per
                               32-k block - input part first, then the recurrent part - the six piece products in PA / PB order, each one rounding into the
                               accumulators [r | z] (both parts), n_x (input part) and n_h (recurrent part); then the float32 epilogue in the kernels'
                               association ((b_ih + table) + rowbias, (gi + b_hh) + acc).  hook(block, product, dot [B][3H]) -> dot: planted faults
  the passes                   normal (randn) and small / A3 / B3 / AB2: helpers_gemm_x6.x6_operands' integers as [x | h_prev] and [w_ih | w_hh]^T, scaled by
                               powers of two (the pieces do not change) so that |x|, |h_prev| <= 1 and the pre-activations stay of order one; sum |a||b| < 2^24
                               in integer units, so the kernel's float32 sums are exact in any order and only the epilogue's rounding separates the outputs
  metric                       err_tile = max |got - ref64| / max |ref64| over a 16 x 16 tile of h_out;  err_tile <= F x max(e_ref_tile, 2**-23), e_ref_tile the
                               float32 restatement's own error there; NaN fails.  Input conditions (asserted on the reference alone): every tile maximum
                               >= CELL_MIN_REF, no pre-activation beyond +-8, the 2^24 condition of the piece passes
  buffers                      h_out inside a sentinel-filled allocation with 3 rows behind B and the case's ldo: every sentinel bit-identical afterwards;
                               operand views with NaN padding columns, NaN rows behind B of x, h_prev, gx_rowbias, NaN gx_table rows no token selects
  cell_case_plan(case, addr)   gru_cell_plan restated by hand on addresses and strides; compared with fn_gru_cell_plan (CPU: made-up addresses, GPU: real ones)
  CELL_CASES                   the smallest shapes that reach every instance, tile edge, K tail, input form, view, checked load, automatic branch
"""
import zlib

import numpy as np
import torch

from helpers import SCAN_F_CAP
from helpers_gemm_x6 import PA, PB, _mfma, split3, x6_operands
from helpers_head import HEAD_SENTINEL, tile_errors, worst_ratio

CELL_SENTINEL = HEAD_SENTINEL
CELL_PAD_ROWS = 3
CELL_MIN_REF = 2.0 ** -6            # input condition: every 16 x 16 tile of the reference h_out has a maximum of at least this
CELL_SAT = 8.0                      # input condition: no gate pre-activation of the reference beyond +-8
CELL_V = 50                         # rows of the token table; best_v of the packed-argmax cases
PIECE_PASSES = ("small", "A3", "B3", "AB2")
FAMILIES = ("staged", "direct", "wlds", "wlds-overlap", "x6")
GRU_BF16X6 = 0x4000
# bound per family: the smallest power of two >= 1.5 x the worst ratio measured on an MI355X, capped at SCAN_F_CAP (DESIGN 11d's rule; the lines of
# profiles/gru_cell_fp64_errors.txt).  Measured: staged 3.381, direct 3.952, wlds 3.355, wlds-overlap 6.780, x6 3.374
CELL_F = {"staged": 8, "direct": 8, "wlds": 8, "wlds-overlap": SCAN_F_CAP, "x6": 8}
assert all(f <= SCAN_F_CAP for f in CELL_F.values())

# CELL_FORMS of csrc/gru_plan.h: (variant, family, t0, t1, t2), in its order (the first match wins)
CELL_INSTANCES = ((15, "wlds-overlap", 2, 4, 0), (16, "wlds-overlap", 3, 2, 0), (17, "wlds-overlap", 4, 2, 0), (18, "wlds-overlap", 2, 2, 0),
                  (13, "wlds", 3, 4, 0), (14, "wlds", 3, 2, 0), (9, "wlds", 4, 2, 0), (10, "wlds", 2, 4, 0), (11, "wlds", 4, 2, 0), (12, "wlds", 2, 8, 0),
                  (4, "direct", 4, 1, 0), (5, "direct", 2, 4, 0), (6, "direct", 4, 2, 0), (7, "direct", 2, 2, 0),
                  (1, "staged", 128, 4, 1), (2, "staged", 128, 2, 2), (3, "staged", 64, 4, 1), (8, "staged", 64, 2, 2))
BUILT_INSTANCES = sorted({(f, t0, t1, t2) for _, f, t0, t1, t2 in CELL_INSTANCES})        # 17: variants 9 and 11 name the same one
assert len(BUILT_INSTANCES) == 17
GRU_CELL_MAX_LDS = 160 * 1024
WIDTH_OF = dict(x="K1", h="H", wih="K1", whh="H", out="H")


def rows_per_workgroup(family, t0):
    return t0 if family == "staged" else 32 * t0 if family == "direct" else 64 * t0 if family in ("wlds", "wlds-overlap") else 128


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the plan by hand (csrc/gru_plan.h: gru_cell_plan) and the staged kernel's own choice of loads (csrc/mma_core.h: Stage::can_fast)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def case_ld(case, name):
    return case[WIDTH_OF[name]] + case["pad"].get(name, 0)


def nominal_addresses(case):
    """byte addresses of a case's operands as 16-byte aligned allocations plus the case's own offsets (floats); 0 = absent"""
    off = case["off"]
    a = {n: 0x100000 * (i + 1) + 4 * off.get(n, 0) for i, n in enumerate(("x", "wih", "h", "whh", "out", "bhh", "bih", "table", "rb"))}
    if not case["K1"]:
        a["x"] = a["wih"] = 0
    for n, have in (("bih", case["bih"]), ("table", case["tab"]), ("rb", case["rb"])):
        if not have:
            a[n] = 0
    return a


def cell_case_plan(case, addr=None):
    """dict(family, template, has_tab, has_rb, kmax, grid, threads, lds_bytes, forced_honoured) of fn_gru_cell_f32 for the case on these addresses, and for
    the staged family fast_x / fast_h: whether a K phase runs on load_fast (None: no such phase)"""
    addr = nominal_addresses(case) if addr is None else addr
    B, H, K1 = case["B"], case["H"], case["K1"]
    ld = {n: case_ld(case, n) for n in WIDTH_OF}
    al = lambda n: addr[n] % 16 == 0                                    # noqa: E731  (an absent operand has address 0)
    direct = (H % 32 == 0 and al("h") and al("whh") and ld["h"] % 4 == 0 and ld["whh"] % 4 == 0 and al("out") and ld["out"] % 4 == 0 and al("bhh") and al("bih")
              and al("table") and al("rb") and B * ld["h"] * 4 < 2 ** 32 and 3 * H * ld["whh"] * 4 < 2 ** 32)
    if K1:
        direct = (direct and K1 % 16 == 0 and al("x") and al("wih") and ld["x"] % 4 == 0 and ld["wih"] % 4 == 0 and B * ld["x"] * 4 < 2 ** 32
                  and 3 * H * ld["wih"] * 4 < 2 ** 32)
    kmax = max(K1, H)
    lds_wlds = lambda k: 48 * k * 4 + 4 * 4 * 320 * 4                 # noqa: E731
    wlds_ok, ovl_ok = lds_wlds(kmax) <= GRU_CELL_MAX_LDS, H == 512 and K1 in (0, 512)
    x6_ok = (B % 128 == 0 and H % 32 == 0 and H >= 64 and (not K1 or (K1 % 32 == 0 and ld["x"] % 4 == 0 and ld["wih"] % 4 == 0)) and ld["h"] % 4 == 0
             and ld["whh"] % 4 == 0 and ld["out"] % 4 == 0 and all(al(n) for n in ("x", "wih", "h", "whh", "out", "bhh", "bih", "table", "rb")))
    variant, honoured = case["variant"], False
    if case["x6"] and x6_ok:
        form = ("x6", 0, 0, 0)
    elif variant == 0 and 512 < B <= 2048 and direct and ovl_ok:
        form = ("wlds-overlap", 2 if B <= 1024 else 3 if B <= 1536 else 4, 2, 0)
    elif variant == 0 and B > 512 and direct:
        if B > 1536 or not wlds_ok:
            form = ("direct", 4 if B > 1024 else 2, 2 if B > 1024 else 4, 0)
        else:
            form = ("wlds", 3 if B > 1024 else 2, 2 if B > 1024 else 4, 0)
    else:
        form = ("staged", 64, 2, 2)
        for v, fam, t0, t1, t2 in CELL_INSTANCES:
            ok = fam == "staged" or (direct and (fam == "direct" or (wlds_ok if fam == "wlds" else ovl_ok)))
            if v == variant and ok:
                form, honoured = (fam, t0, t1, t2), True
                break
    fam, t0 = form[0], form[1]
    cdiv = lambda a, b: (a + b - 1) // b                                # noqa: E731
    p = dict(family=fam, template=form[1:], has_tab=int(case["tab"]), has_rb=int(case["rb"]), kmax=kmax, threads=256, lds_bytes=0, forced_honoured=honoured,
             fast_x=None, fast_h=None)
    if fam == "staged":
        p.update(grid=cdiv(B, t0) * (H // 32), lds_bytes=2 * (t0 * 36 + 96 * 36) * 4)
        fast = lambda a, w, K: al(a) and ld[a] % 4 == 0 and al(w) and ld[w] % 4 == 0 and K % 32 == 0          # noqa: E731
        p.update(fast_x=fast("x", "wih", K1) if K1 else None, fast_h=fast("h", "whh", H))
    elif fam == "direct":
        p.update(grid=cdiv(B, 32 * t0) * (H // 32))
    elif fam in ("wlds", "wlds-overlap"):
        p.update(grid=cdiv(B, 64 * t0) * (H // 16), lds_bytes=lds_wlds(kmax if fam == "wlds" else 512))
    else:
        p.update(grid=(B // 128) * (H // 32), threads=512, lds_bytes=3 * (4 * (4 * 3 * 64)) * 16)
    return p


PLAN_KEYS = ("family", "template", "has_tab", "has_rb", "kmax", "grid", "threads", "lds_bytes", "forced_honoured")


def assert_plan_is_the_librarys(case, plan, lib_plan):
    for k in PLAN_KEYS:
        assert plan[k] == lib_plan[k], "%s: %s by hand %r, the library %r" % (case["id"], k, plan[k], lib_plan[k])


def assert_plan_is_the_cases(case, plan):
    """the case reaches the family and instance it is named for - and, where a checked-load case asked for another family, the documented fallback"""
    assert (plan["family"], tuple(plan["template"])) == case["want"], (case["id"], plan)
    assert bool(plan["forced_honoured"]) == case["honoured"], (case["id"], plan)
    if case["fast"] is not None:
        assert (plan["fast_x"], plan["fast_h"]) == case["fast"], (case["id"], plan)


def library_plan(case, addr, lib=None):
    """fn_gru_cell_plan (a pure host function) on a descriptor of the case's shapes, strides and these addresses"""
    import ctypes
    from helpers_gemm import _lib
    L = _lib()
    lib = L.load() if lib is None else lib
    c = L.FnGruCell(B=case["B"], H=case["H"], K1=case["K1"], ldx=case_ld(case, "x"), ldw_ih=case_ld(case, "wih"), ldh=case_ld(case, "h"),
                    ldw_hh=case_ld(case, "whh"), ldo=case_ld(case, "out"), variant=case["variant"] | (GRU_BF16X6 if case["x6"] else 0),
                    h_prev=addr["h"], w_hh=addr["whh"], b_hh=addr["bhh"], h_out=addr["out"], x=addr["x"] or None, w_ih=addr["wih"] or None,
                    b_ih=addr["bih"] or None, gx_table=addr["table"] or None, gx_rowbias=addr["rb"] or None)
    if case["tab"] and case["tok"] == "idx":
        c.idx, c.idx_ld = 0x900000, 7
    if case["tab"] and case["tok"] == "best":
        c.idx_best, c.best_v = 0x900000, CELL_V
    plan = L.FnGruCellPlan()
    assert lib.fn_gru_cell_plan(ctypes.byref(c), ctypes.byref(plan)) == 0 and plan.status == 0, (case["id"], plan.status)
    return plan.as_dict()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _pow2_at_most(x):
    return 2.0 ** np.floor(np.log2(x))


# powers of two of the piece passes: (scale of [x | h_prev], scale of the weights as a function of K = K1 + H).  A3: the 8 wide entries of a batch row are
# up to 1 and meet weights of [-4, 4] / 8; B3: batch integers of [-4, 4] / 4 meet the 8 wide entries of a weight row, up to 1; AB2: 9-bit entries up to 1 meet
# 9-bit weights up to 1/2 at 32 values of k; small: K integer products of [-8, 8] / 8 and [-8, 8] scaled to a sum of about 1.5.  Chosen on the CPU
# (test_cell_reference.py): the largest powers of two that keep every pre-activation within +-8, where a dropped low-piece product (2^-16 of a term) still
# moves some h_out of every pass by more than 4 x the bound - and by less than the 2e-5 of the whole-tensor metric
PASS_SCALES = {"small": (2.0 ** -3, lambda K: _pow2_at_most(1.5 / (0.65 * 5.2 * K ** 0.5))), "A3": (2.0 ** -18, lambda K: 2.0 ** -3),
               "B3": (2.0 ** -2, lambda K: 2.0 ** -18), "AB2": (2.0 ** -9, lambda K: 2.0 ** -10)}


def cell_inputs(case):
    """dense CPU float32 inputs of a case from the generator of its data key: x [B][K1] or None, w_ih, h_prev, w_hh, b_ih or None, b_hh, table [V][3H] or None,
    tok [B] (long; the token of every row) or None, rb [B][3H] or None; for the piece passes also ints = (|a|, |b|) in integer units"""
    B, H, K1, mode = case["B"], case["H"], case["K1"], case["mode"]
    gen = _gen(case["data"] + "/" + mode)
    rn = lambda *s: torch.randn(*s, generator=gen)                       # noqa: E731
    inp = dict(x=None, w_ih=None, b_ih=None, table=None, tok=None, rb=None, ints=None)
    if mode == "normal":
        inp.update(h_prev=rn(B, H) * 0.5, w_hh=rn(3 * H, H) / H ** 0.5, b_hh=rn(3 * H) * 0.1)
        if K1:
            inp.update(x=rn(B, K1), w_ih=rn(3 * H, K1) / K1 ** 0.5)
        bih, table, rb = rn(3 * H) * 0.1, rn(CELL_V, 3 * H) * 0.3, rn(B, 3 * H) * 0.3
    else:
        K = K1 + H
        a, b, C0, bias = x6_operands(case["data"], mode, B, 3 * H, K, True)
        sa, sw = PASS_SCALES[mode][0], float(PASS_SCALES[mode][1](K))
        W = b.t().contiguous()
        inp.update(h_prev=(a[:, K1:] * sa).contiguous(), w_hh=(W[:, K1:] * sw).contiguous(), ints=(a.abs().double(), b.abs().double()))
        if K1:
            inp.update(x=(a[:, :K1] * sa).contiguous(), w_ih=(W[:, :K1] * sw).contiguous())
        ri = lambda *s: torch.randint(-8, 9, s, generator=gen).float() / 32                                   # noqa: E731
        b_hh = ri(3 * H)
        b_hh[H:2 * H] -= 1.0                                              # the z gate mostly shut: h' stays close to n, which sees every product of the cell
        inp.update(b_hh=b_hh)
        bih, table, rb = bias / 32, ri(CELL_V, 3 * H), C0 / 32
    if case["bih"]:
        inp["b_ih"] = bih
    if case["tab"]:
        inp["table"] = table
        if case["tok"] == "start":
            tok = torch.full((B,), CELL_V - 1, dtype=torch.long)
        else:                                                             # even tokens, and in rows 0 and 1 the first and the last row of the table
            tok = 2 * torch.randint(0, CELL_V // 2, (B,), generator=gen)
            tok[0], tok[1 % B] = 0, CELL_V - 1
        inp["tok"] = tok
    if case["rb"]:
        inp["rb"] = rb
    return inp


def cell_reference(inp, dtype=torch.float64, x_mm=None, h_mm=None, w_ih=None, w_hh=None, b_ih="given", want_pre=False):
    """h_out [B][H] of FakeOps.gru_cell's semantics in `dtype` on the CPU.  x_mm / h_mm / w_ih / w_hh / b_ih: other operands for the PRODUCTS (the epilogue's
    old state stays inp['h_prev']) - where planted faults edit.  want_pre: also the three pre-activations"""
    c = lambda t: None if t is None else t.detach().cpu().to(dtype)     # noqa: E731
    hp, bhh = c(inp["h_prev"]), c(inp["b_hh"])
    B, H = hp.shape
    x, wih = c(inp["x"] if x_mm is None else x_mm), c(inp["w_ih"] if w_ih is None else w_ih)
    hm, whh = c(hp if h_mm is None else h_mm), c(inp["w_hh"] if w_hh is None else w_hh)
    bih = c(inp["b_ih"] if isinstance(b_ih, str) else b_ih)
    gi = torch.zeros(B, 3 * H, dtype=dtype)
    if x is not None:
        gi = gi + x @ wih.t()
    if bih is not None:
        gi = gi + bih
    if inp["table"] is not None:
        gi = gi + c(inp["table"])[inp["tok"]]
    if inp["rb"] is not None:
        gi = gi + c(inp["rb"])
    gh = hm @ whh.t() + bhh
    pr, pz = gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H]
    r, z = torch.sigmoid(pr), torch.sigmoid(pz)
    pn = gi[:, 2 * H:] + r * gh[:, 2 * H:]
    out = (1.0 - z) * torch.tanh(pn) + z * hp
    assert out.dtype == dtype
    return (out, (pr, pz, pn)) if want_pre else out


def cell_x6_restate(inp, hook=None, w_rounded=True, nh_sees_x=False):
    """the bf16 x 6 cell in float32, see the module text; w_rounded = False and nh_sees_x are planted faults"""
    hp = inp["h_prev"].numpy()
    B, H = hp.shape
    K1 = 0 if inp["x"] is None else inp["x"].shape[1]
    A = hp if not K1 else np.concatenate([inp["x"].numpy(), hp], 1)
    W = inp["w_hh"].numpy() if not K1 else np.concatenate([inp["w_ih"].numpy(), inp["w_hh"].numpy()], 1)
    Ap = [p.astype(np.float64) for p in split3(A, False)]
    Wp = [p.astype(np.float64) for p in split3(W, w_rounded)]
    nbx, nblk = K1 // 32, (K1 + H) // 32
    acc_rz, acc_nx, acc_nh = np.zeros((B, 2 * H), np.float32), np.zeros((B, H), np.float32), np.zeros((B, H), np.float32)
    for blk in range(nblk):
        s = 32 * blk
        for c in range(6):
            dot = Ap[PA[c]][:, s:s + 32] @ Wp[PB[c]][:, s:s + 32].T
            if hook is not None:
                dot = hook(blk, c, dot)
            acc_rz = _mfma(acc_rz, dot[:, :2 * H])
            if blk < nbx:                                                 # (the other accumulator multiplies zeros: it does not move)
                acc_nx = _mfma(acc_nx, dot[:, 2 * H:])
                if nh_sees_x:
                    acc_nh = _mfma(acc_nh, dot[:, 2 * H:])
            else:
                acc_nh = _mfma(acc_nh, dot[:, 2 * H:])
    t = torch.from_numpy
    gi = torch.zeros(B, 3 * H) if inp["b_ih"] is None else inp["b_ih"].expand(B, 3 * H)
    if inp["table"] is not None:
        gi = gi + inp["table"][inp["tok"]]
    if inp["rb"] is not None:
        gi = gi + inp["rb"]
    bh = inp["b_hh"]
    r = torch.sigmoid((gi[:, :H] + bh[:H]) + t(acc_rz[:, :H]))
    z = torch.sigmoid((gi[:, H:2 * H] + bh[H:2 * H]) + t(acc_rz[:, H:]))
    n = torch.tanh((gi[:, 2 * H:] + t(acc_nx)) + r * (t(acc_nh) + bh[2 * H:]))
    out = (1.0 - z) * n + z * inp["h_prev"]
    assert out.dtype == torch.float32
    return out


_REF_CACHE = {}


def cell_references(case):
    """dict(inp, ref64, fake32, e_ref, den) of a case, computed once per (data, mode, shape, form); asserts the input conditions on the reference"""
    key = (case["data"], case["mode"], case["B"], case["H"], case["K1"], case["tab"], case["rb"], case["bih"], case["tok"] == "start")
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    inp = cell_inputs(case)
    ref64, pre = cell_reference(inp, torch.float64, want_pre=True)
    fake32 = cell_reference(inp, torch.float32)
    e_ref, den = tile_errors(fake32, ref64)
    assert den.min() >= CELL_MIN_REF, "input condition: %s has a tile maximum of %.3e < %.3e" % (case["id"], den.min(), CELL_MIN_REF)
    assert np.isfinite(e_ref).all(), case["id"]
    sat = max(float(p.abs().max()) for p in pre)
    assert sat <= CELL_SAT, "input condition: %s has a pre-activation of %.2f" % (case["id"], sat)
    if inp["ints"] is not None:                                           # the 2^24 condition: every float32 partial sum of the products is an exact integer multiple
        a, b = inp["ints"]
        most = float((a @ b).max())
        assert most < 2 ** 24, "input condition: %s sum |a||b| = %g >= 2^24" % (case["id"], most)
    res = dict(inp=inp, ref64=ref64, fake32=fake32, e_ref=e_ref, den=den, sat=sat)
    _REF_CACHE[key] = res
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------------
# buffers and the check
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _alloc(rows, cols, ld, off, extra, fill, src=None):
    """flat CPU tensor of off + (rows + extra) x ld floats filled with `fill`, its [rows][cols] view `off` floats in holding src"""
    flat = torch.full((off + (rows + extra) * ld,), fill, dtype=torch.float32)
    if src is not None:
        flat.as_strided((rows, cols), (ld, 1), off).copy_(src)
    return flat, (rows, cols, ld, off)


def cell_buffers(case, device="cpu"):
    """(launch arguments of HipOps.gru_cell / FakeOps.gru_cell as views on `device`, the whole h_out allocation [B + 3][ldo]).  Padding columns, rows behind B
    of x / h_prev / gx_rowbias and unselected gx_table rows are NaN; the h_out allocation is sentinel-filled"""
    inp = cell_references(case)["inp"]
    B, H, K1, off = case["B"], case["H"], case["K1"], case["off"]
    nan = float("nan")
    view = lambda fs: fs[0].to(device).as_strided(fs[1][:2], (fs[1][2], 1), fs[1][3])              # noqa: E731
    kw = dict(h_prev=view(_alloc(B, H, case_ld(case, "h"), off.get("h", 0), CELL_PAD_ROWS, nan, inp["h_prev"])),
              w_hh=view(_alloc(3 * H, H, case_ld(case, "whh"), off.get("whh", 0), 0, nan, inp["w_hh"])))
    bo = off.get("bhh", 0)
    kw["b_hh"] = torch.cat([torch.full((bo,), nan), inp["b_hh"]]).to(device)[bo:]
    if K1:
        kw.update(x=view(_alloc(B, K1, case_ld(case, "x"), off.get("x", 0), CELL_PAD_ROWS, nan, inp["x"])),
                  w_ih=view(_alloc(3 * H, K1, case_ld(case, "wih"), off.get("wih", 0), 0, nan, inp["w_ih"])))
    if case["bih"]:
        kw["b_ih"] = inp["b_ih"].to(device)
    if case["tab"]:
        table = torch.full((CELL_V, 3 * H), nan)
        used = torch.unique(inp["tok"])
        table[used] = inp["table"][used]
        kw["gx_table"] = table.to(device)
        if case["tok"] == "start":
            kw["start_token"] = CELL_V - 1
        elif case["tok"] == "idx":
            toks = torch.full((B, 7), -(2 ** 30), dtype=torch.int32)      # a strided column; its neighbours would index far outside the table
            toks[:, 3] = inp["tok"].int()
            kw["idx"] = toks.to(device)[:, 3]
        else:                                                             # packed argmax words: (key << 32) | (best_v - 1 - token), the key arbitrary and not zero
            key = torch.arange(B, dtype=torch.int64) * 0x9e3779b1 % (2 ** 31 - 1) + 1
            kw.update(idx_best=((key << 32) | (CELL_V - 1 - inp["tok"])).to(device), best_v=CELL_V)
    if case["rb"]:
        kw["gx_rowbias"] = torch.cat([inp["rb"], torch.full((CELL_PAD_ROWS, 3 * H), nan)]).to(device)[:B]
    ldo = case_ld(case, "out")
    obuf = torch.full((B + CELL_PAD_ROWS, ldo), CELL_SENTINEL, dtype=torch.float32).to(device)
    kw["h_out"] = obuf[:B, :H]
    return kw, obuf


def cell_tile_ratio(case, got, F):
    """(worst err / max(e_ref, 2**-23), tile row, tile column, tiles over F) of got [B][H] (CPU) against the case's float64 reference; NaN counts as inf"""
    ref = cell_references(case)
    err, _ = tile_errors(got, ref["ref64"])
    return worst_ratio(err, ref["e_ref"], F)


def check_cell_vs_f64(case, obuf, F):
    """the whole h_out allocation of one launch (CPU tensor): every sentinel bit-identical, then err <= F x max(e_ref, 2**-23) in every tile"""
    assert F <= SCAN_F_CAP
    B, H = case["B"], case["H"]
    outside = torch.ones_like(obuf, dtype=torch.bool)
    outside[:B, :H] = False
    sent = torch.tensor(CELL_SENTINEL).view(torch.int32)
    assert bool((obuf.view(torch.int32)[outside] == sent).all()), "%s: h_out was written outside [B][H]" % case["id"]
    r, i, j, n = cell_tile_ratio(case, obuf[:B, :H], F)
    ref = cell_references(case)
    assert r <= F, "%s: %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., units %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
        case["id"], r, ref["e_ref"][i, j], 16 * i, 16 * j, ref["den"][i, j], n, ref["e_ref"].size, F)
    return r, i, j


def old_metric_accepts(got, fake32, tol=2e-5):
    """what tests/test_gpu_parity.py asks of the cells: max |got - ref| < 2e-5 of the WHOLE tensor's maximum, against the float32 restatement"""
    e = float((got.double() - fake32.double()).abs().max()) / max(1e-12, float(fake32.double().abs().max()))
    return e < tol


def cell_line(case, plan, worst):
    """one line of profiles/gru_cell_fp64_errors.txt"""
    return "%-66s %-12s %-12s tab %d rb %d grid %4d  %-6s ratio %6.3f tile (%d, %d)" % (
        case["id"], plan["family"], "<%s>" % ", ".join(map(str, plan["template"])), plan["has_tab"], plan["has_rb"], plan["grid"], case["mode"], *worst)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
FORMS4 = ((False, False), (False, True), (True, True), (True, False))          # (token table, row constant)
INSTANCE_OF_VARIANT = {v: (f, (t0, t1, t2)) for v, f, t0, t1, t2 in CELL_INSTANCES}
ONE_PER_FAMILY = (("staged", 8), ("direct", 5), ("wlds", 10), ("wlds-overlap", 18), ("x6", 0))
STAGED = ("staged", (64, 2, 2))


def _cc(cid, group, B, H, K1, variant=0, x6=False, form=(False, False), bih=True, tok="idx", pad=None, off=None, mode="normal", want=None, honoured=None,
        fast=None, data=None):
    """pad: extra floats per row of x / h / wih / whh / out; off: floats an operand (x, h, wih, whh, bhh) starts behind a 16-byte aligned allocation;
    want: (family, template) the case is named for (default: what `variant` / x6 names); honoured: forced_honoured of the plan; fast: for staged cases
    (input phase, recurrent phase) on load_fast; data: the key of the generator (cases that must agree bit for bit share it)"""
    if want is None:
        want = ("x6", (0, 0, 0)) if x6 else INSTANCE_OF_VARIANT[variant] if variant else STAGED
    return dict(id=cid, group=group, B=B, H=H, K1=K1, variant=variant, x6=x6, tab=form[0], rb=form[1], bih=bih, tok=tok, pad=pad or {}, off=off or {}, mode=mode,
                want=want, honoured=(variant != 0 and not x6) if honoured is None else honoured, fast=fast, data=data or cid)


def _shape_of(fam, variant):
    """(B, H, K1) of the one-per-family instances: one full row tile and one of 17 rows; the overlapped fill exists at H = 512 only"""
    rows = rows_per_workgroup(fam, INSTANCE_OF_VARIANT[variant][1][0] if variant else 0)
    return (128, 64, 64) if fam == "x6" else (rows + 17, 512, 512) if fam == "wlds-overlap" else (rows + 17, 64, 64)


CELL_CASES = []
# row and unit tiles: every built instance at rows-per-workgroup + 17 rows and two or four unit tiles, the four input forms in turn
for _i, (_v, _f, _t0, _t1, _t2) in enumerate(CELL_INSTANCES):
    _B = rows_per_workgroup(_f, _t0) + 17
    for _K1 in ((0, 512) if _f == "wlds-overlap" else (64,)):
        CELL_CASES.append(_cc("tiles-v%d-%s-%d-%d-%d-B%d-K%d" % (_v, _f, _t0, _t1, _t2, _B, _K1), "tiles", _B, 512 if _f == "wlds-overlap" else 64, _K1,
                              variant=_v, form=FORMS4[(_i + (_K1 == 0)) % 4]))
CELL_CASES.append(_cc("tiles-v8-staged-4x8-super-tiles-B256-H256", "tiles", 256, 256, 64, variant=8, form=(True, True)))
CELL_CASES.append(_cc("tiles-x6-B128-H64", "tiles", 128, 64, 64, x6=True, form=(True, True)))
# K tails of the shared ring at 70 rows: nks = K / 16 against a ring of PF slots, two or more unit tiles everywhere
for _H, _K1 in [(64, k) for k in (16, 32, 48, 80, 144, 272)] + [(64, 0), (96, 0), (288, 0)]:
    for _i, _v in enumerate((4, 5, 6, 7, 10, 12, 14)):
        CELL_CASES.append(_cc("ktail-v%d-H%d-K%d" % (_v, _H, _K1), "ktails", 70, _H, _K1, variant=_v, form=FORMS4[(_i + _K1 // 16) % 4], data="ktail-H%d-K%d" % (_H, _K1)))
# input forms: the four (table, row constant) forms with and without b_ih in one instance of every family; token sources
for _f, _v in ONE_PER_FAMILY:
    _B, _H, _K1 = _shape_of(_f, _v)
    for _tab, _rb in FORMS4:
        for _bih in (True, False):
            CELL_CASES.append(_cc("form-%s-tab%d-rb%d-bih%d" % (_f, _tab, _rb, _bih), "forms", _B, _H, _K1, variant=_v, x6=_f == "x6", form=(_tab, _rb), bih=_bih))
    for _tok in ("start", "best"):
        CELL_CASES.append(_cc("token-%s-%s" % (_f, _tok), "tokens", _B, _H, _K1, variant=_v, x6=_f == "x6", form=(True, False), tok=_tok))
# views: ld = width + 4 and + 16 on each operand alone and on all together, one instance of every family; the plan still names the family
for _f, _v in ONE_PER_FAMILY:
    _B, _H, _K1 = _shape_of(_f, _v)
    for _p in (4, 16):
        for _n in ("x", "h", "wih", "whh", "out", "all"):
            CELL_CASES.append(_cc("view-%s-%s-ld+%d" % (_f, _n, _p), "views", _B, _H, _K1, variant=_v, x6=_f == "x6", form=(True, True),
                                  pad={k: _p for k in WIDTH_OF} if _n == "all" else {_n: _p}, data="view-%s" % _f))
# staged checked loads (Stage::load_checked): forced 128- and 64-row forms and the automatic plan at B <= 512; then the same inputs with a direct, a
# weight-slice and the bf16 x 6 form asked for: the plan must decline (forced_honoured 0) and run the staged default
_CHECKED = (("K50", 50, {}, {}, (False, True)), ("K75", 75, {}, {}, (False, True)), ("h-offset-one-float", 64, {}, {"h": 1}, (True, False)),
            ("ldh-H+2", 64, {"h": 2}, {}, (True, False)), ("ldwhh-H+1", 64, {"whh": 1}, {}, (True, False)), ("wih-offset-one-float", 64, {}, {"wih": 1}, (False, True)))
for _n, _K1, _pad, _off, _fast in _CHECKED:
    for _i, _v in enumerate((2, 8, 0)):
        CELL_CASES.append(_cc("checked-v%d-%s" % (_v, _n), "checked", (128 if _v == 2 else 64) + 17, 64, _K1, variant=_v, form=FORMS4[(_i + _K1) % 4], pad=_pad, off=_off,
                              fast=_fast, data="checked-%s" % _n))
    for _v, _x6 in ((5, False), (10, False), (0, True)):
        CELL_CASES.append(_cc("checked-%s-%s-declined" % ("x6" if _x6 else "v%d" % _v, _n), "checked", 128, 64, _K1, variant=_v, x6=_x6, form=(True, True), pad=_pad,
                              off=_off, want=STAGED, honoured=False, fast=_fast, data="checked-%s" % _n))
CELL_CASES.append(_cc("checked-v8-aligned-both-phases-fast", "checked", 81, 64, 64, variant=8, fast=(True, True)))
# the automatic plan above 512 rows
CELL_CASES += [
    _cc("auto-B530-H64-K64-wlds-2-4", "auto", 530, 64, 64, form=(True, True), want=("wlds", (2, 4, 0))),
    _cc("auto-B1041-H64-K64-wlds-3-2", "auto", 1041, 64, 64, form=(False, True), want=("wlds", (3, 2, 0))),
    _cc("auto-B1553-H64-K64-direct-4-2", "auto", 1553, 64, 64, form=(True, False), want=("direct", (4, 2, 0))),
    _cc("auto-B530-H64-K1024-slice-over-LDS-direct-2-4", "auto", 530, 64, 1024, form=(False, False), want=("direct", (2, 4, 0))),
    _cc("auto-B530-H512-K512-overlap-2-2", "auto", 530, 512, 512, form=(True, True), want=("wlds-overlap", (2, 2, 0))),
    _cc("auto-B1041-H512-K0-overlap-3-2", "auto", 1041, 512, 0, form=(True, False), want=("wlds-overlap", (3, 2, 0))),
    _cc("auto-B1553-H512-K0-overlap-4-2", "auto", 1553, 512, 0, form=(True, True), want=("wlds-overlap", (4, 2, 0))),
]
# bf16 x 6: every producer trip count nblk = 2 .. 13 at H = 64, then 5 (H = 96, 256 rows) and 32; the piece passes at nblk 2, 3, 4, 32; declined shapes
for _j in range(12):
    CELL_CASES.append(_cc("x6-B128-H64-K%d-nblk%d" % (32 * _j, _j + 2), "x6", 128, 64, 32 * _j, x6=True, form=FORMS4[_j % 4], bih=_j % 3 != 2))
CELL_CASES += [_cc("x6-B256-H96-K64-nblk5", "x6", 256, 96, 64, x6=True, form=(True, True)), _cc("x6-B128-H512-K512-nblk32", "x6", 128, 512, 512, x6=True, form=(False, True))]
for _H, _K1 in ((64, 0), (64, 32), (64, 64), (512, 512)):
    for _m in PIECE_PASSES:
        CELL_CASES.append(_cc("x6-%s-B128-H%d-K%d-nblk%d" % (_m, _H, _K1, (_H + _K1) // 32), "x6-pieces", 128, _H, _K1, x6=True, form=(False, True), mode=_m))
CELL_CASES += [
    _cc("x6-declined-B130", "x6-declined", 130, 64, 64, x6=True, form=(True, True), want=STAGED, honoured=False),
    _cc("x6-declined-K48", "x6-declined", 128, 64, 48, x6=True, form=(False, True), want=STAGED, honoured=False),
    _cc("x6-declined-H32", "x6-declined", 128, 32, 32, x6=True, form=(True, False), want=STAGED, honoured=False),
    _cc("x6-declined-b_hh-offset-4-bytes", "x6-declined", 128, 64, 64, x6=True, off={"bhh": 1}, want=STAGED, honoured=False),
    _cc("x6-declined-B640-runs-the-automatic-weight-slice", "x6-declined", 640 + 2, 64, 64, x6=True, form=(True, True), want=("wlds", (2, 4, 0)), honoured=False),
]
CELL_BY_ID = {c["id"]: c for c in CELL_CASES}
assert len(CELL_BY_ID) == len(CELL_CASES)
CELL_GROUPS = sorted({c["group"] for c in CELL_CASES})
