"""Shared code of tests/test_head_reference.py (CPU) and tests/test_gpu_head_paths.py (MI355X): the fused output head fn_out_head_f32
(out_head_kernel, csrc/gemm.hip) and the LDS-free NT GEMM (gemm_nt_direct_kernel<PF, WGS>) on every K-loop path, against float64.

  head_reference(...)        logits = h W^T + b, log-softmax, nll[row], dlogits[row] = grad_scale (softmax - onehot), rows time-major
                             (row = t B + b, target at [b, t]), plain torch on the CPU in float64 - or, the same lines in float32, the restatement
  head_tile_errors(got, ref) per 16-row x 16-column tile (grid from row 0 / column 0, ragged last tiles; nll = 16-row x 1 tiles)
                             err = max |got - ref| / max |ref| over THAT tile alone - never over the whole tensor
  check_head_vs_f64(...)     layout (padding columns exactly 0, rows >= R and the nll tail of an over-allocated sentinel-filled buffer untouched),
                             then err <= F x max(e_ref, 2**-23) in EVERY tile, e_ref = the float32 restatement's own error in that tile,
                             F = helpers.SCAN_F_CAP.  Returns the worst ratio and where it occurred.
  head_path / nt_direct_instance   the device-side / host-side choice of K loop / kernel instance restated on shapes, so that every case can
                             assert that it reaches the path it names; the host-side one is checked against the library (fn_gemm_plan).

Input condition: every tile maximum of the float64 reference is >= SCAN_MIN_REF.  Two kinds of case have a reference that IS zero, not small:
V = 1 (softmax = 1: nll = 0 and dlogits = 0 in exact arithmetic) and grad_scale = 0 (dlogits = 0).  There the relative error is undefined and the
check is the strictest one there is: the kernel's value must be exactly 0 (a case has to declare this: `zero` in its table entry).
"""
import zlib

import numpy as np
import torch

from helpers import SCAN_EPS, SCAN_F_CAP, SCAN_MIN_REF

HEAD_TILE = 16
HEAD_SENTINEL = -123.25         # fill value of the over-allocated output buffers
HEAD_PAD_ROWS = 3               # rows past R that must stay untouched
HEAD_GRAD_SCALE = 0.37
OH_BM, OH_BN, OH_WN = 64, 384, 4            # out_head_kernel: rows per workgroup, column tile, column groups of a workgroup's four waves


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reference and metric
# ---------------------------------------------------------------------------------------------------------------------------------------------
def head_reference(h, W, bias, target, B, T, grad_scale, dtype=torch.float64):
    """(nll [R], dlogits [R][V]) of the output head in `dtype` on the CPU; h [T*B][H] time-major rows, W [V][H], bias [V], target [B][T]"""
    h, W, bias = h.detach().cpu().to(dtype), W.detach().cpu().to(dtype), bias.detach().cpu().to(dtype)
    R, V = h.shape[0], W.shape[0]
    assert R == B * T and tuple(target.shape) == (B, T)
    lp = torch.log_softmax(h @ W.t() + bias, dim=-1)
    tg = target.detach().cpu().long().t().reshape(R, 1)                 # row t B + b <- target[b, t]
    nll = -lp.gather(1, tg).reshape(R)
    p = lp.exp()
    p.scatter_add_(1, tg, -torch.ones(R, 1, dtype=dtype))
    return nll, grad_scale * p


def head_reference_f64(h, W, bias, target, B, T, grad_scale):
    return head_reference(h, W, bias, target, B, T, grad_scale, torch.float64)


def _tile_max(x, tr=HEAD_TILE, tc=HEAD_TILE):
    """[ceil(R / tr)][ceil(C / tc)] maxima of a non-negative 2-D float64 tensor; a NaN makes its tile NaN"""
    R, Cn = x.shape
    pr, pc = -R % tr, -Cn % tc
    x = torch.nn.functional.pad(x, (0, pc, 0, pr))
    return x.view((R + pr) // tr, tr, (Cn + pc) // tc, tc).amax((1, 3)).numpy()


def tile_errors(got, ref64, tc=HEAD_TILE):
    """(err, den) per 16 x tc tile of one 2-D quantity: den = max |ref| over the tile, err = max |got - ref| / den; where the reference tile is
    identically zero err is 0 if the tile of `got` is exactly zero too and inf otherwise.  NaN in `got` gives NaN."""
    got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    num, den = _tile_max((got - ref64).abs(), tc=tc), _tile_max(ref64.abs(), tc=tc)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(den > 0, num / den, np.where(num == 0, 0.0, np.where(np.isnan(num), np.nan, np.inf)))
    return err, den


def head_tile_errors(got, ref64):
    """{quantity: (err, den)} for the quantities of ref64 ('nll' [R] as 16 x 1 tiles, 'dlogits' [R][V] as 16 x 16 tiles).  A quantity the
    reference has and `got` lacks is an error."""
    res = {}
    for k, ref in ref64.items():
        assert got.get(k) is not None, "output %s missing" % k
        if k == "nll":
            res[k] = tile_errors(got[k].reshape(-1, 1), ref.reshape(-1, 1), tc=1)
        else:
            res[k] = tile_errors(got[k], ref)
    return res


def worst_ratio(err, e_ref, F):
    """(worst err / max(e_ref, 2**-23), tile row, tile column, number of tiles over F); NaN counts as inf"""
    ratio = err / np.maximum(e_ref, SCAN_EPS)
    flat = np.where(np.isnan(ratio), np.inf, ratio)
    i, j = np.unravel_index(int(np.argmax(flat)), flat.shape)
    return float(flat[i, j]), int(i), int(j), int((~(flat <= F)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# which K loop / kernel instance a launch takes (csrc/gemm.hip restated on shapes).  head_path restates a choice the kernel makes on the device;
# nt_direct_instance restates the host's (csrc/gemm_plan.h) and is checked against the library's own answer, fn_gemm_plan: on the CPU for every NT case
# and inside the sweep of test_gemm_reference.py, on the MI355X for every launch on its real addresses
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _aligned16(ptr, ld):
    return ptr % 16 == 0 and ld % 4 == 0


def head_path(ptr_h, ldh, ptr_W, ldw, K, R, V):
    """(path, nks, nmain) of out_head_kernel: 'direct' = the LDS-free loop (nks 16-k steps, nmain of them in the two-deep pipeline, the odd one
    in the tail), 'staged_fast' / 'staged_checked' = the LDS-staged loop with unconditional float4 / bounds-checked loads (nks = nmain = None)"""
    al = _aligned16(ptr_h, ldh) and _aligned16(ptr_W, ldw)
    if al and K % 16 == 0 and R * ldh < (1 << 30) and V * ldw < (1 << 30):
        nks = K >> 4
        return "direct", nks, nks // 2 * 2
    if al and K % 16 == 0:                      # Stage<.., KC = true>::can_fast for both operands
        return "staged_fast", None, None
    return "staged_checked", None, None


def nt_direct_instance(M, N, K, lda, ldb, ldc, ptrs, lean, splitk, a_k=True, b_k=True, x6=False):
    """the gemm_nt_direct_kernel instance fn_gemm_f32 launches for this call, or None when the dispatch goes elsewhere.  ptrs = (A, B, C, bias)
    addresses (bias 0 = none); x6: FN_GEMM_BF16X6 set (then the shapes the bf16 x 6 NT kernel takes go there first)"""
    al = lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and all(p % 16 == 0 for p in ptrs)
    whole = a_k and b_k and splitk <= 1 and M % 128 == 0 and N % 128 == 0
    if x6 and whole and K % 32 == 0 and K >= 128 and al and (M // 128) * (N // 128) >= 128:
        return None
    if whole and K % 16 == 0 and K >= 64 and al and M * lda < (1 << 30) and N * ldb < (1 << 30) and (M // 128) * (N // 128) >= 256:
        return "gemm_nt_direct_kernel<1, 4>" if lean else "gemm_nt_direct_kernel<4, 2>"
    return None


def nt_direct_steps(K, lean):
    """(nks, nmain, steady iterations of the ring loop, unpipelined leftover steps) of gemm_nt_direct_kernel<PF, WGS>, PF = 1 (lean) or 4"""
    PF = 1 if lean else 4
    nks = K >> 4
    nmain = nks // PF * PF
    return nks, nmain, max(0, nmain // PF - 1), nks - nmain


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the head cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _hc(cid, B, T, H, V, ld=None, h_view="dense", w_view="dense", form="both", bias="randn", path="direct", twin=False):
    """h_view: dense | wide (columns [4, 4 + H) of a [R][H + 16] matrix) | off1 (a dense matrix that starts one float into its buffer) |
    ld66 (columns [0, H) of a [R][H + 2] matrix) | span (columns [0, H) of a [R][16384] allocation);  w_view: dense | ld+4;
    form: both | nll | dl | gs0 (both outputs, grad_scale = 0);  bias: randn | lowp (columns 32..47 12 units down, no target among them);
    twin: also run the direct path on a dense copy of h and compare the two nll"""
    return dict(id=cid, B=B, T=T, H=H, V=V, ld=(V + 3) // 4 * 4 if ld is None else ld, h_view=h_view, w_view=w_view, form=form, bias=bias,
                path=path, twin=twin, zero=("dlogits", "nll") if V == 1 else ("dlogits",) if form == "gs0" else ())


HEAD_CASES = []
# direct path, step counts: no main loop / zero steady iterations without and with the tail / steady iterations with an odd tail
for _H, _why in ((16, "tail-only"), (32, "drain-only"), (48, "drain+tail"), (64, "1steady"), (80, "1steady+tail"), (112, "2steady+tail"), (528, "15steady+tail")):
    HEAD_CASES.append(_hc("direct-nks%d-%s" % (_H // 16, _why), 7, 23, _H, 342))
HEAD_CASES.append(_hc("direct-nks33-lowprob-columns", 7, 23, 528, 342, bias="lowp"))
# direct path, operand views
HEAD_CASES.append(_hc("direct-h-column-slice-ldh-H+16", 7, 23, 64, 342, h_view="wide"))
HEAD_CASES.append(_hc("direct-W-ldw-H+4", 7, 23, 64, 342, w_view="ld+4"))
# staged-checked path
HEAD_CASES.append(_hc("checked-K75", 7, 23, 75, 342, path="staged_checked"))
HEAD_CASES.append(_hc("checked-K513", 7, 23, 513, 342, path="staged_checked"))
HEAD_CASES.append(_hc("checked-h-offset-one-float", 7, 23, 64, 342, h_view="off1", path="staged_checked", twin=True))
HEAD_CASES.append(_hc("checked-ldh66", 7, 23, 64, 342, h_view="ld66", path="staged_checked", twin=True))
# staged-fast path: only the 2^30-element span test sends aligned operands with K % 16 == 0 there
HEAD_CASES.append(_hc("fast-span-2^30-ldh16384", 256, 256, 32, 19, h_view="span", path="staged_fast"))
# rows: R % 64 in {1, 31, 33, 63, 0}, B not a divisor of 64 (the rc % B, rc / B target mapping across workgroup edges)
for _B, _T in ((1, 1), (1, 31), (3, 11), (7, 9), (1, 64), (5, 13), (1, 257), (3, 43)):
    HEAD_CASES.append(_hc("direct-rows-R%d-B%d" % (_B * _T, _B), _B, _T, 64, 342))
# columns: whole column groups of a wave empty (V <= 288 leaves group 3 without a column), V not a multiple of 16, V = ld = 384
for _V in (1, 15, 16, 17, 96, 97, 288, 289, 342, 383, 384):
    HEAD_CASES.append(_hc("direct-cols-V%d-ld%d" % (_V, (_V + 3) // 4 * 4), 7, 23, 80, _V))
HEAD_CASES.append(_hc("direct-cols-V289-ld384", 7, 23, 80, 289, ld=384))
# forms, once on a direct and once on a staged-checked case ("both" = every case above)
for _f in ("nll", "dl", "gs0"):
    HEAD_CASES.append(_hc("direct-form-%s" % _f, 7, 23, 64, 342, form=_f))
    HEAD_CASES.append(_hc("checked-form-%s" % _f, 7, 23, 75, 342, form=_f, path="staged_checked"))
HEAD_BY_ID = {c["id"]: c for c in HEAD_CASES}
SPAN_LD = 16384


def head_layout(case):
    """(byte offset of h in its 16-byte aligned allocation, ldh, byte offset of W, ldw): what the operand views of a case look like to the kernel"""
    H = case["H"]
    off_h, ldh = {"dense": (0, H), "wide": (16, H + 16), "off1": (4, H), "ld66": (0, H + 2), "span": (0, SPAN_LD)}[case["h_view"]]
    off_w, ldw = {"dense": (0, H), "ld+4": (0, H + 4)}[case["w_view"]]
    return off_h, ldh, off_w, ldw


def head_case_path(case):
    off_h, ldh, off_w, ldw = head_layout(case)
    return head_path(off_h, ldh, off_w, ldw, case["H"], case["B"] * case["T"], case["V"])


def head_inputs(case):
    """dense CPU fp32 inputs of a case from its own generator: h = randn, W = randn H**-0.5 (logits of a few units), bias, target [B][T] int32 with
    every seventh position pinned to column 0 and the next one to column V - 1"""
    B, T, H, V = case["B"], case["T"], case["H"], case["V"]
    gen = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    h = torch.randn(B * T, H, generator=gen)
    W = torch.randn(V, H, generator=gen) * H ** -0.5
    bias = torch.randn(V, generator=gen)
    tgt = torch.randint(0, V, (B, T), generator=gen, dtype=torch.int32)
    pos = torch.arange(B * T).view(B, T)
    tgt[pos % 7 == 0] = 0
    tgt[pos % 7 == 1] = V - 1
    if case["bias"] == "lowp":
        bias[32:48] -= 12.0
        low = (tgt >= 32) & (tgt < 48)
        tgt[low] += 16
    return dict(h=h, W=W, bias=bias, target=tgt)


def head_wanted(case):
    return {"both": ("nll", "dlogits"), "gs0": ("nll", "dlogits"), "nll": ("nll",), "dl": ("dlogits",)}[case["form"]]


def head_grad_scale(case):
    return 0.0 if case["form"] == "gs0" else HEAD_GRAD_SCALE


_HEAD_REF_CACHE = {}


def head_references(case):
    """dict(inputs, ref64, fake32, e_ref, den) of a case, computed once: ref64 / fake32 = {nll, dlogits} of head_reference in float64 / float32
    (the quantities the case's form produces), e_ref = head_tile_errors(fake32, ref64).  Asserts the input condition."""
    if case["id"] in _HEAD_REF_CACHE:
        return _HEAD_REF_CACHE[case["id"]]
    inp = head_inputs(case)
    gs, want = head_grad_scale(case), head_wanted(case)
    out = {}
    for name, dt in (("ref64", torch.float64), ("fake32", torch.float32)):
        nll, dl = head_reference(inp["h"], inp["W"], inp["bias"], inp["target"], case["B"], case["T"], gs, dt)
        assert nll.dtype == dt and dl.dtype == dt
        out[name] = {k: v for k, v in (("nll", nll), ("dlogits", dl)) if k in want}
    errs = head_tile_errors(out["fake32"], out["ref64"])
    for k, (e, den) in errs.items():
        if k in case["zero"]:
            assert den.max() == 0.0 and e.max() == 0.0, "%s %s: declared exactly zero, but the reference or the restatement is not" % (case["id"], k)
        else:
            assert den.min() >= SCAN_MIN_REF, "input condition: %s %s has a tile maximum of %.3e < 2**-100" % (case["id"], k, den.min())
            assert np.isfinite(e).all(), (case["id"], k)
    res = dict(inputs=inp, ref64=out["ref64"], fake32=out["fake32"], e_ref={k: v[0] for k, v in errs.items()}, den={k: v[1] for k, v in errs.items()})
    _HEAD_REF_CACHE[case["id"]] = res
    return res


def head_buffers(case, device="cpu"):
    """(nll buffer [R + pad] or None, dlogits buffer [R + pad][ld] or None), sentinel-filled; the launch gets their first R rows"""
    R, want = case["B"] * case["T"], head_wanted(case)
    nll = torch.full((R + HEAD_PAD_ROWS,), HEAD_SENTINEL, device=device) if "nll" in want else None
    dl = torch.full((R + HEAD_PAD_ROWS, case["ld"]), HEAD_SENTINEL, device=device) if "dlogits" in want else None
    return nll, dl


def head_fill_from(case, out, nll_buf, dl_buf):
    """write {nll, dlogits} into the buffers the way the kernel does: R rows, V columns, padding columns zero"""
    R, V = case["B"] * case["T"], case["V"]
    if nll_buf is not None:
        nll_buf[:R] = out["nll"].float()
    if dl_buf is not None:
        dl_buf[:R] = 0.0
        dl_buf[:R, :V] = out["dlogits"].float()


def check_head_layout(case, nll_buf, dl_buf):
    R, V = case["B"] * case["T"], case["V"]
    if dl_buf is not None:
        assert tuple(dl_buf.shape) == (R + HEAD_PAD_ROWS, case["ld"])
        pad = dl_buf[:R, V:]
        assert pad.numel() == 0 or float(pad.abs().max()) == 0.0, "%s: padding column %d of dlogits is not zero" % (
            case["id"], V + int(torch.nonzero(pad.abs().amax(0) != 0)[0]))
        assert bool((dl_buf[R:] == HEAD_SENTINEL).all()), "%s: dlogits rows >= R were written" % case["id"]
    if nll_buf is not None:
        assert tuple(nll_buf.shape) == (R + HEAD_PAD_ROWS,)
        assert bool((nll_buf[R:] == HEAD_SENTINEL).all()), "%s: nll rows >= R were written" % case["id"]


def check_head_vs_f64(case, nll_buf, dl_buf, F=SCAN_F_CAP):
    """The buffers of one launch (CPU tensors, head_buffers) against the float64 head: the layout checks, then in EVERY 16 x 16 tile of dlogits and
    every 16-row tile of nll   err <= F x max(e_ref, 2**-23),  err = max |got - ref64| / max |ref64| over that tile alone, e_ref = the float32
    restatement's err there; tiles whose reference is exactly zero (case['zero']) must be exactly zero.  No tile is exempt.
    Returns (worst ratio, quantity, tile row, tile column)."""
    assert F <= SCAN_F_CAP
    ref = head_references(case)
    check_head_layout(case, nll_buf, dl_buf)
    R, V = case["B"] * case["T"], case["V"]
    got = {"nll": None if nll_buf is None else nll_buf[:R], "dlogits": None if dl_buf is None else dl_buf[:R, :V]}
    errs = head_tile_errors(got, ref["ref64"])
    worst, bad = (-1.0, "", 0, 0), []
    for k, (e, den) in errs.items():
        r, i, j, n = worst_ratio(e, ref["e_ref"][k], F)
        if r > worst[0]:
            worst = (r, k, i, j)
        if not r <= F:
            bad.append("%s %s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., columns %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
                case["id"], k, e[i, j], r, ref["e_ref"][k][i, j], 16 * i, 16 * j if k == "dlogits" else 0, den[i, j], n, e.size, F))
    assert not bad, "\n".join(bad)
    return worst


def check_nll_agree(case, nll_a, nll_b, F=SCAN_F_CAP):
    """two kernels' nll of the same values (another k order inside a 16-k step: not bit-equal): per 16-row tile
    max |a - b| / max |ref64| <= F x max(e_ref, 2**-23)"""
    ref = head_references(case)
    num = _tile_max((nll_a.detach().cpu().double() - nll_b.detach().cpu().double()).abs().reshape(-1, 1), tc=1)
    r, i, _, n = worst_ratio(num / ref["den"]["nll"], ref["e_ref"]["nll"], F)
    assert r <= F, "%s: the two paths' nll differ by %.1f x max(e_ref, 2**-23) in rows %d.. (%d tiles over F)" % (case["id"], r, 16 * i, n)
    return r


def old_metric_accepts(got, ref, tol=1e-5):
    """what test_out_head_fused asks of dlogits: max |got - ref| < 1e-5 of the WHOLE tensor's maximum"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(1e-12, float(ref.abs().max())) < tol


def head_line(case, path, worst):
    """one line of profiles/out_head_fp64_errors.txt"""
    p, nks, nmain = path
    steps = "nks %2d nmain %2d" % (nks, nmain) if p == "direct" else "K %d" % case["H"]
    return "%-34s %-15s %-16s R %5d V %3d ld %3d  ratio %6.3f  %-7s tile (%d, %d)" % (
        case["id"], p, steps, case["B"] * case["T"], case["V"], case["ld"], worst[0], worst[1], worst[2], worst[3])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the NT GEMM cases: C = alpha A B^T + bias + beta C, M = N = 2048 (256 tiles of 128 x 128: the least the dispatch sends to the LDS-free kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------------
NT_M = NT_N = 2048
NT_ALPHA = 0.5


def _nc(K, lean, beta=2.0, views=False):
    nks, nmain, steady, rem = nt_direct_steps(K, lean)
    cid = "nt-%s-K%d-nks%d-steady%d-rem%d%s%s" % ("lean-pf1" if lean else "pf4", K, nks, steady, rem, "-beta0" if beta == 0.0 else "", "-lda-K+4-ldc-N+4" if views else "")
    return dict(id=cid, K=K, lean=lean, beta=beta, views=views, key=(K, beta))


NT_CASES = [_nc(K, lean) for lean in (False, True) for K in (64, 80, 96, 112, 128, 144, 160, 176)]
NT_CASES += [_nc(112, lean, beta=0.0) for lean in (False, True)] + [_nc(144, lean, views=True) for lean in (False, True)]
NT_BY_ID = {c["id"]: c for c in NT_CASES}


def nt_layout(case):
    """(lda, ldb, ldc)"""
    K = case["K"]
    return (K + 4 if case["views"] else K), K, (NT_N + 4 if case["views"] else NT_N)


def nt_case_instance(case):
    lda, ldb, ldc = nt_layout(case)
    return nt_direct_instance(NT_M, NT_N, case["K"], lda, ldb, ldc, (0, 0, 0, 0), case["lean"], 1)


_NT_REF_CACHE = {}


def nt_references(case):
    """dict(A, B, C0, bias, ref64, fake32, e_ref, den), shared by the cases of one (K, beta): fake32 = FakeOps.gemm in float32 on the CPU"""
    if case["key"] in _NT_REF_CACHE:
        return _NT_REF_CACHE[case["key"]]
    from fake_ops import FakeOps
    K, beta = case["key"]
    gen = torch.Generator().manual_seed(1000 + K)
    A, Bm = torch.randn(NT_M, K, generator=gen), torch.randn(NT_N, K, generator=gen)
    C0, bias = torch.randn(NT_M, NT_N, generator=gen), torch.randn(NT_N, generator=gen)
    ref64 = NT_ALPHA * (A.double() @ Bm.double().t()) + bias.double() + beta * C0.double()
    fake32 = C0.clone()
    FakeOps().gemm(A, Bm, fake32, alpha=NT_ALPHA, beta=beta, bias=bias)
    assert fake32.dtype == torch.float32
    e_ref, den = tile_errors(fake32, ref64)
    assert den.min() >= SCAN_MIN_REF and np.isfinite(e_ref).all()
    res = dict(A=A, B=Bm, C0=C0, bias=bias, ref64=ref64, fake32=fake32, e_ref=e_ref, den=den)
    _NT_REF_CACHE[case["key"]] = res
    return res


def nt_buffer(case, C0, device="cpu"):
    """sentinel-filled [M + pad][ldc] buffer whose [:M, :N] block holds C0 (the beta C term)"""
    ldc = nt_layout(case)[2]
    buf = torch.full((NT_M + HEAD_PAD_ROWS, ldc), HEAD_SENTINEL, device=device)
    buf[:NT_M, :NT_N] = C0.to(device)
    return buf


def check_nt_vs_f64(case, cbuf, F=SCAN_F_CAP):
    """C of one launch (CPU tensor, nt_buffer) against float64 alpha A B^T + bias + beta C0 per 16 x 16 tile, same bound as the head; rows >= M and
    columns >= N untouched.  Returns (worst ratio, tile row, tile column)."""
    assert F <= SCAN_F_CAP
    ref = nt_references(case)
    assert bool((cbuf[NT_M:] == HEAD_SENTINEL).all()) and bool((cbuf[:, NT_N:] == HEAD_SENTINEL).all()), "%s: C was written outside [M][N]" % case["id"]
    e, den = tile_errors(cbuf[:NT_M, :NT_N], ref["ref64"])
    r, i, j, n = worst_ratio(e, ref["e_ref"], F)
    assert r <= F, "%s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., columns %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
        case["id"], e[i, j], r, ref["e_ref"][i, j], 16 * i, 16 * j, den[i, j], n, e.size, F)
    return r, i, j


def nt_line(case, instance, worst):
    """one line of profiles/out_head_fp64_errors.txt"""
    return "%-46s %-28s ratio %6.3f  tile (%d, %d)" % (case["id"], instance, worst[0], worst[1], worst[2])
