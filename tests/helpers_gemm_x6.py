"""Shared code of tests/test_gemm_x6_reference.py (CPU) and tests/test_gpu_gemm_x6_paths.py (MI355X): the four bf16 x 6 GEMM kernels of csrc/gemm.hip -
gemm_tn_x6_kernel (every wavefront splits its own operands), gemm_tn_x6w_kernel (producer / consumer wavefronts, 128 x 128 tiles), gemm_tn_x6v_kernel
(128 x 256 tiles), all three also behind fn_gru_dwhh_f32, and gemm_nt_x6w_kernel - exactly and per tile against float64.

The dispatch mirror (x6_tn_plan / x6_nt_plan / trip_schedule), make_problem, c_buffer and the checkers are helpers_gemm.py's.  Here:

  split3(x, rounded)         THE split of x6w_core.h (fn_split) on float32 arrays with integer operations: hi = the top 16 bits (truncated) or the top 16
                             bits of bits + 0x8000 (fn_rn16), mid the same of x - hi, lo = the rest; x == hi + mid + lo exactly (asserted)
  x6_cut / x6_accumulate     the float32 restatement of THIS arithmetic: A cut truncated, B cut rounded, per 32-k block the six piece products lo*hi,
                             hi*lo, mid*mid, mid*hi, hi*mid, hi*hi in that order, each one MFMA = a 32-term dot of exact products formed in float64 and
                             added to the float32 accumulator with one rounding; one accumulator per K range, a K tail a zero-padded block (producer /
                             consumer kernels) or fp32 steps of four rows (per-wave kernel); the ranges added in slab order; alpha, bias, beta C.
                             Every product of two bf16 pieces has <= 16 significant bits and the 32 of a dot are added in float64: the sum is exact in ANY
                             order unless the terms span more than 2^32, so the host's BLAS (which forms the dots) cannot move e_ref - the reason given
                             at the end of DESIGN 11b
  the passes                 small / A3 / B3 / AB2 (exact: integers, bit for bit) and normal (per 16 x 16 tile), see x6_operands
  X6_TN_CASES / X6_DWHH_CASES / X6_NT_CASES   the smallest shapes that reach every kernel x grid form x walk x reduction x trip count
"""
import numpy as np
import torch

from helpers import SCAN_F_CAP
from helpers_gemm import (NTX6, PLAN_CUS, X6_TRIPS, X6P, X6V, X6W, _cdiv, _gen, _lib, _r4, dwhh_plan, gemm_instance, k_ranges, make_problem)

EXACT_MODES = ("small", "A3", "B3", "AB2")
X6_MODES = EXACT_MODES + ("normal",)
WIDE_BITS, WIDE_PER_VECTOR = 18, 8          # A3 / B3: odd integers of 18-bit span, at most 8 per row of A^T / column of B (20 bits x 16 leave the 2^24 condition)
AB2_BITS, AB2_K = 9, 32                     # AB2: odd integers of 9-bit span in both operands at a common set of at most 32 values of k
MAX_ABS = {"small": (8, 8), "A3": (2 ** WIDE_BITS, 4), "B3": (4, 2 ** WIDE_BITS), "AB2": (2 ** AB2_BITS, 2 ** AB2_BITS)}
# the six products of a 32-k block in the kernels' order (piece 0 = hi, 1 = mid, 2 = lo): PA / PB of x6w_consume
PA, PB = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)
PRODUCT_NAMES = ("lo*hi", "hi*lo", "mid*mid", "mid*hi", "hi*mid", "hi*hi")
# which exact pass sees which product (the others multiply a piece that is zero there): asserted by the CPU test on the pieces themselves
PASS_OF_PRODUCT = {"lo*hi": "A3", "mid*hi": "A3", "hi*lo": "B3", "hi*mid": "B3", "mid*mid": "AB2", "hi*hi": "small"}
# bound of the normal pass per family: the smallest power of two >= 1.5 x the worst ratio measured on an MI355X, capped at SCAN_F_CAP (DESIGN 11d's rule;
# profiles/gemm_fp64_errors.txt).  Measured: tn-perwave 5.487, tn-128 5.817, tn-256 5.817, nt 6.913, dwhh 5.356 - 1.5 x each lies between 8 and 16
X6_F = {"tn-perwave": SCAN_F_CAP, "tn-128": SCAN_F_CAP, "tn-256": SCAN_F_CAP, "nt": SCAN_F_CAP, "dwhh": SCAN_F_CAP}
assert all(f <= SCAN_F_CAP for f in X6_F.values())
KERNEL_OF = {"perwave": X6P, "128": X6W, "256": X6V}
TN3 = ("perwave", "128", "256")


def x6_flags(kern, pertile=False):
    """the bits of the splitk argument for a kernel choice ('perwave' / '128' / '256' / 'nt')"""
    lib = _lib()
    return (lib.GEMM_BF16X6 | (lib.GEMM_X6_PERWAVE if kern == "perwave" else lib.GEMM_X6_WIDE if kern == "256" else 0)
            | (lib.GEMM_X6_PERTILE if pertile else 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the split and the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _top16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _rn16(x):
    return ((np.ascontiguousarray(x, np.float32).view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(np.float32)


def split3(x, rounded):
    """(hi, mid, lo) float32 arrays, each a bf16 value: fn_split<RN> of x6w_core.h.  The two subtractions are exact in float32 (asserted through the sum)"""
    f = _rn16 if rounded else _top16
    x = np.ascontiguousarray(x, np.float32)
    hi = f(x)
    r1 = x - hi
    mid = f(r1)
    lo = r1 - mid
    assert (_top16(lo) == lo).all(), "the last remainder has more than 8 significant bits"
    assert (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all()
    return hi, mid, lo


def x6_cut(a, b):
    """a [M][K], b [K][N] (torch float32) -> (Ap, Bp): three float64 arrays each, [M][Kp] / [Kp][N] with Kp = K rounded up to whole 32-k blocks and zeros
    behind row K: A truncated, B rounded"""
    K = a.shape[1]
    Kp = _cdiv(K, 32) * 32
    Ap = [np.zeros((a.shape[0], Kp)) for _ in range(3)]
    Bp = [np.zeros((Kp, b.shape[1])) for _ in range(3)]
    for dst, src in zip(Ap, split3(a.numpy(), False)):
        dst[:, :K] = src
    for dst, src in zip(Bp, split3(b.numpy(), True)):
        dst[:K] = src
    return Ap, Bp


def _mfma(acc, dot):
    """one MFMA: the float32 accumulator plus a dot formed in float64, rounded once"""
    return (acc.astype(np.float64) + dot).astype(np.float32)


def x6_accumulate(Ap, Bp, a, b, ranges, perwave, hook=None):
    """the slabs: per K range one float32 accumulator over its 32-k blocks, six products each in the kernels' order.  perwave: the rows behind the last
    whole block of a range run as fp32 MFMA steps of four rows on the uncut operands (a, b: torch float32), not as a zero-padded block.
    hook(range, block, product, dot) -> dot: where planted faults edit a product"""
    M, N = Ap[0].shape[0], Bp[0].shape[1]
    slabs = []
    for ri, (k0, k1) in enumerate(ranges):
        acc = np.zeros((M, N), np.float32)
        whole = (k1 - k0) >> 5
        for blk in range(whole if perwave else _cdiv(k1 - k0, 32)):
            s = k0 + 32 * blk
            for c in range(6):
                dot = Ap[PA[c]][:, s:s + 32] @ Bp[PB[c]][s:s + 32]
                acc = _mfma(acc, dot if hook is None else hook(ri, blk, c, dot))
        if perwave:
            a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
            for s in range(k0 + 32 * whole, k1, 4):
                dot = np.zeros((M, N))
                for k in range(s, min(s + 4, k1)):                       # single float64 operations in ascending k: the same on every host
                    dot = dot + a64[:, k:k + 1] * b64[k:k + 1]
                acc = _mfma(acc, dot)
        slabs.append(acc)
    return slabs


def x6_epilogue(slabs, alpha, bias, beta, C0):
    """the slabs added in order (slab_reduce_kernel / slab_reduce4_kernel: slab 0, 1, ..), then o = alpha s, o += bias, o += beta C0 - in float32"""
    total = slabs[0]
    for s in slabs[1:]:
        total = total + s
    o = np.float32(alpha) * total
    if bias is not None:
        o = o + bias.numpy()
    if beta != 0.0:
        o = o + np.float32(beta) * C0.numpy()
    assert o.dtype == np.float32
    return torch.from_numpy(o)


def x6_restate(a, b, ranges, perwave, alpha, bias, beta, C0, hook=None, cut=None, slab_edit=None):
    """the whole restatement; cut: edited pieces instead of x6_cut(a, b); slab_edit(slabs) -> slabs"""
    Ap, Bp = x6_cut(a, b) if cut is None else cut
    slabs = x6_accumulate(Ap, Bp, a, b, ranges, perwave, hook)
    return x6_epilogue(slabs if slab_edit is None else slab_edit(slabs), alpha, bias, beta, C0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operands of the five passes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def wide_positions(nvec, K, per=WIDE_PER_VECTOR):
    """k [nvec][per]: where vector v (a row of A^T, a column of B) holds its wide values.  The 64 vectors of a producer set have 64 per slots; slot q
    goes to block q mod nblk (every block of every K range gets slots of every set while nblk <= 64 per) at an in-block position that walks all 32"""
    nblk = _cdiv(K, 32)
    v, j = np.arange(nvec)[:, None], np.arange(per)[None, :]
    q = (v % 64) * per + j
    blk = q % nblk
    pos = (13 * (v % 64) + 7 * j + q // nblk + 3 * (v // 64)) % 32
    rows = np.minimum(32, K - 32 * blk)                   # rows the block really has
    return 32 * blk + pos % rows


def _wide_values(shape, bits, gen):
    """odd integers of `bits`-bit span and random sign with bit 9 set where there is one (a non-zero second piece)"""
    mag = torch.randint(0, 2 ** (bits - 1), shape, generator=gen) | (2 ** (bits - 1)) | 1 | (512 if bits > 10 else 0)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def ab2_positions(K):
    """the common k set of the AB2 pass: 32 values (all of K when K < 32), one per in-block position, spread over the blocks"""
    nblk = _cdiv(K, 32)
    ks = set()
    for j in range(AB2_K):
        blk = j * nblk // AB2_K if nblk < AB2_K else j * (nblk // AB2_K)
        if 32 * blk + j >= K:                             # the partial last block has no such row: the block before it
            blk -= 1
        if blk >= 0:
            ks.add(32 * blk + j)
    return sorted(ks)


def x6_operands(cid, mode, M, N, K, bias):
    """(a [M][K], b [K][N], C0 [M][N], bias [N] or None) of one pass:
    small   integers of [-8, 8], one bf16 piece each: dense - dropped, repeated or misplaced blocks, rows, tiles, ranges, K tails, the epilogue
    A3      b integers of [-4, 4]; a integers of [-8, 8] but for <= 8 wide values per row (odd, 18-bit span, random sign: three non-zero pieces under the
            truncating split): lo*hi, mid*hi, hi*hi
    B3      the mirror image, b wide under the rounding split: hi*lo, hi*mid
    AB2     both operands odd integers of 9-bit span (two pieces) at a common set of <= 32 values of k, [-8, 8] elsewhere: mid*mid
    normal  standard normals"""
    gen = _gen(cid, mode)
    if mode == "normal":
        a, b = torch.randn((M, K), generator=gen), torch.randn((K, N), generator=gen)
        return a, b, torch.randn((M, N), generator=gen), (torch.randn((N,), generator=gen) if bias else None)
    ri = lambda shape, m: torch.randint(-m, m + 1, shape, generator=gen).float()                  # noqa: E731
    if mode == "small":
        a, b = ri((M, K), 8), ri((K, N), 8)
    elif mode == "A3":
        a, b = ri((M, K), 8), ri((K, N), 4)
        a.scatter_(1, torch.from_numpy(wide_positions(M, K)), _wide_values((M, WIDE_PER_VECTOR), WIDE_BITS, gen))
    elif mode == "B3":
        a, b = ri((M, K), 4), ri((K, N), 8)
        bt = b.t().contiguous()
        bt.scatter_(1, torch.from_numpy(wide_positions(N, K)), _wide_values((N, WIDE_PER_VECTOR), WIDE_BITS, gen))
        b = bt.t().contiguous()
    else:
        a, b = ri((M, K), 8), ri((K, N), 8)
        ks = ab2_positions(K)
        a[:, ks] = _wide_values((M, len(ks)), AB2_BITS, gen)
        b[ks] = _wide_values((len(ks), N), AB2_BITS, gen)
    return a, b, ri((M, N), 8), (ri((N,), 8) if bias else None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _xc(cid, M, N, K, splitk=1, kernels=TN3, alpha=0.5, beta=2.0, bias=True, a=(0, None), b=(0, None), c=(0, None), bias_off=0, ranges=1, grid="3d",
        reduce=None, walks=(), pertile=False, last=None):
    """a TN case (A [K][M], B [K][N] row-contiguous).  a / b / c as helpers_gemm._gc.  What the id claims: ranges, grid form, reduce, the kernels that
    WALK items at 256 compute units, rows of the last K range; pertile: run again with FN_GEMM_X6_PERTILE and ask for the same bits"""
    return dict(id=cid, kind="tn", a_k=False, b_k=False, M=M, N=N, K=K, splitk=splitk, kernels=kernels, alpha=alpha, beta=beta, bias=bias, a_off=a[0],
                lda=a[1] if a[1] is not None else _r4(M), b_off=b[0], ldb=b[1] if b[1] is not None else _r4(N), c0=c[0],
                ldc=c[1] if c[1] is not None else _r4(c[0] + N) + 4, bias_off=bias_off, ranges=ranges, grid=grid, reduce=reduce, walks=walks, pertile=pertile,
                last=last)


R4, R1 = "slab_reduce4_kernel", "slab_reduce_kernel"
X6_TN_CASES = []
# one K range of nblk = 1 .. 13 whole blocks at 128 x 256: every prologue / steady / tail count of both trip schedules (REST = 7 resp. 4)
for _n in range(1, 14):
    X6_TN_CASES.append(_xc("x-128x256-K%d-nblk%d-whole" % (32 * _n, _n), 128, 256, 32 * _n, beta=0.0 if _n % 3 == 0 else 2.0, bias=_n % 2 == 1))
# ... and a partial last block of 31, 29, 28, 4, 1 rows at the block counts on either side of the boundaries of both schedules (4 | 5, 6 | 7 and 7 | 8, 10 | 11;
# 1 and 2: the per-wave kernel without a whole block and with a single one)
for _n in (1, 2, 4, 5, 6, 7, 8, 10, 11):
    for _r in (1, 3, 4, 28, 31):
        X6_TN_CASES.append(_xc("x-128x256-K%d-nblk%d-last-block-%d-rows" % (32 * _n - _r, _n, 32 - _r), 128, 256, 32 * _n - _r, last=32 * _n - _r,
                               beta=0.0 if _r == 4 else 2.0))
# ragged outputs
X6_TN_CASES += [
    _xc("x-132x128-K75-second-row-tile-of-4-rows", 132, 128, 75),
    _xc("x-64x128-K75-second-A-set-beyond-the-matrix", 64, 128, 75, beta=0.0),
    _xc("x-128x68-K75-ragged-columns", 128, 68, 75),
    _xc("x-128x260-K75-ragged-columns-second-wide-tile", 128, 260, 75),
    _xc("x-128x130-ldb132-K200-split3-scalar-slab-store-scalar-reduce", 128, 130, 200, splitk=3, b=(0, 132), ranges=3, reduce=R1, last=8),
    _xc("x-342x72-lda344-K75-window-clamp", 342, 72, 75, a=(0, 344)),
    # split K: 3 and 5 ranges on the 3-D grid, 8 and 16 on the 1-D grid, a short last range, fewer ranges than asked for, one block per range
    _xc("x-132x260-K300-split3-3d-last-range-44", 132, 260, 300, splitk=3, ranges=3, reduce=R4, last=44),
    _xc("x-132x260-K320-split5-3d", 132, 260, 320, splitk=5, ranges=5, reduce=R4, last=64, beta=0.0),
    _xc("x-132x260-K500-split8-1d-last-range-52", 132, 260, 500, splitk=8, ranges=8, grid="1d", reduce=R4, last=52),
    _xc("x-132x260-K512-split16-1d-one-block-per-range", 132, 260, 512, splitk=16, ranges=16, grid="1d", reduce=R4, last=32),
    _xc("x-132x260-K100-split8-gives-4-ranges-3d", 132, 260, 100, splitk=8, ranges=4, reduce=R4, last=4),
    # 72 ranges of one block (the last: 7 rows) x 4 tiles of 128 x 128 = 288 items on 256 compute units: workgroups walk one or two items; the 128 x 256
    # kernel has 144 items there and walks at 256 x 512 (288)
    _xc("x-256x256-K2279-split72-1d-288-items-walk", 256, 256, 2279, splitk=72, ranges=72, grid="1d", reduce=R4, walks=("128",), pertile=True, last=7),
    _xc("x-256x512-K2279-split72-1d-288-wide-items-walk", 256, 512, 2279, splitk=72, kernels=("256",), ranges=72, grid="1d", reduce=R4, walks=("256",),
        pertile=True, last=7, beta=0.0),
    # the epilogues
    _xc("x-132x72-K300-split3-beta1-bias", 132, 72, 300, splitk=3, alpha=1.0, beta=1.0, ranges=3, reduce=R4, last=44),
    _xc("x-132x72-K500-split8-bias-off1-scalar-reduce", 132, 72, 500, splitk=8, bias_off=1, ranges=8, grid="1d", reduce=R1, last=52),
    _xc("x-342x72-lda344-K500-split8-C-column-342-scalar-reduce", 342, 72, 500, splitk=8, a=(0, 344), c=(342, 416), ranges=8, grid="1d", reduce=R1, last=52),
]

# fn_gru_dwhh_f32 with the bf16 x 6 bit: dW [3H][H] = beta dW + [dgx[:, :2H] | dghn]^T hprev, default (128 x 128 producer / consumer) and per-wave
X6_DWHH_CASES = []
for _H, _form in ((64, "one-launch-msplit128-ragged-dghn-band"), (128, "one-launch-three-tiles"), (96, "two-products")):
    for _rows in (37, 1030):
        for _S in (1, 4, 8):
            for _beta in (0.0, 1.0):
                X6_DWHH_CASES.append(dict(id="xd-H%d-%s-rows%d-split%d-beta%d" % (_H, _form, _rows, _S, _beta), kind="dwhh", H=_H, rows=_rows, splitk=_S,
                                          beta=_beta, form="one-launch" if _H != 96 else "two-products", kernels=("128", "perwave"), M=3 * _H, N=_H, K=_rows,
                                          alpha=1.0, bias=False))

# gemm_nt_x6w_kernel: A [M][K], B [N][K]; 2048 x 1024 = 128 tiles is the least the dispatch sends there; 4096 x 1152 = 288 tiles walk at 256 compute units
def _nc(cid, M, N, K, alpha=1.0, beta=0.0, bias=False, pad=(0, 0, 0), walks=False, pertile=False):
    return dict(id=cid, kind="nt", a_k=True, b_k=True, M=M, N=N, K=K, splitk=1, kernels=("nt",), alpha=alpha, beta=beta, bias=bias, a_off=0, lda=K + pad[0],
                b_off=0, ldb=K + pad[1], c0=0, ldc=N + pad[2], bias_off=0, ranges=1, grid="1d", reduce=None, walks=("nt",) if walks else (), pertile=pertile,
                last=None)


X6_NT_CASES = [_nc("xn-2048x1024-K%d-nblk%d" % (32 * _n, _n), 2048, 1024, 32 * _n, alpha=0.5 if _n % 2 else 1.0, beta=2.0 if _n % 2 else 0.0, bias=_n % 2 == 1,
                   pad=(4, 8, 4) if _n in (5, 10) else (0, 0, 0)) for _n in (4, 5, 6, 7, 8, 10, 11, 13)]
X6_NT_CASES.append(_nc("xn-4096x1152-K256-nblk8-288-tiles-walk-padded-alpha-beta-bias", 4096, 1152, 256, alpha=0.5, beta=2.0, bias=True, pad=(8, 4, 12),
                       walks=True, pertile=True))
# just below each condition of the dispatch: the plan must name an fp32 kernel (nothing is launched: the fp32 kernels have their own suites)
X6_NT_BELOW = [("K96", 2048, 1024, 96), ("K-not-a-multiple-of-32", 2048, 1024, 144), ("127-tiles", 127 * 128, 128, 128)]

X6_CASES = X6_TN_CASES + X6_DWHH_CASES + X6_NT_CASES
X6_BY_ID = {c["id"]: c for c in X6_CASES}
assert len(X6_BY_ID) == len(X6_CASES)


def case_family(case, kern):
    return "dwhh" if case["kind"] == "dwhh" else "nt" if case["kind"] == "nt" else "tn-" + kern


def x6_case_plan(case, kern, ptrs=None, pertile=False, cus=PLAN_CUS):
    """the mirror on the case's nominal layout (16-byte aligned allocations) or on real addresses: a plan (TN, NT) or dict(form, launches) (dwhh)"""
    flags = x6_flags(kern, pertile)
    if case["kind"] == "dwhh":
        return dwhh_plan(case["H"], case["rows"], (0, 0, 0, 0, 0) if ptrs is None else ptrs, case["splitk"], False, flags, cus)
    if ptrs is None:
        ptrs = (4 * case["a_off"], 4 * case["b_off"], 4 * case["c0"], 4 * case["bias_off"] if case["bias"] else 0, 0)
    return gemm_instance(case["a_k"], case["b_k"], case["M"], case["N"], case["K"], case["lda"], case["ldb"], case["ldc"], ptrs, case["splitk"], False, flags, cus)


def assert_x6_plan_matches_case(case, kern, plan, pertile=False, cus=PLAN_CUS):
    """the plan is what the id names: the kernel, the ranges and the rows of the last one, the grid form, whether workgroups walk, the reduction"""
    for p in plan["launches"] if case["kind"] == "dwhh" else [plan]:
        what = (case["id"], kern, p)
        assert p["family"] == "x6" and p["kernel"] == (NTX6 if kern == "nt" else KERNEL_OF[kern]), what
        if case["kind"] == "dwhh":
            assert plan["form"] == case["form"] and p["msplit"] == (2 * case["H"] if case["form"] == "one-launch" else 0), what
            continue
        assert (p["ranges"], p["grid"], p["reduce"]) == (case["ranges"], case["grid"], case["reduce"]), what
        if cus == PLAN_CUS:
            assert p["walks"] == (kern in case["walks"] and not pertile), what
        if case["last"] is not None:
            assert case["K"] - (p["ranges"] - 1) * p["klen"] == case["last"], what


_PROBLEMS = {}


def case_ranges(case):
    """the K ranges of the case - the same for all its kernels (ranges of whole 32-k blocks)"""
    if case["kind"] == "dwhh":
        plan = x6_case_plan(case, "128")["launches"]
        assert len({p["klen"] for p in plan}) == 1
        return k_ranges(case["K"], plan[0]["klen"])
    kl = {x6_case_plan(case, k)["klen"] for k in case["kernels"]}
    assert len(kl) == 1
    return k_ranges(case["K"], kl.pop())


def has_tail(case):
    return any((k1 - k0) & 31 for k0, k1 in case_ranges(case))


def x6_problem(case, mode, perwave=False, defer=True):
    """the problem of one pass.  perwave matters where a K range has a partial last block (the per-wave kernel runs it on the fp32 MFMA): its own
    restatement there, the shared one elsewhere.  Exact problems defer the restatement (prob['restate']())."""
    perwave = perwave and has_tail(case)
    key = (case["id"], mode, perwave, defer and mode != "normal")
    if key not in _PROBLEMS:
        M, N, K = case["M"], case["N"], case["K"]
        a, b, C0, bias = x6_operands(case["id"], mode, M, N, K, case["bias"])
        ranges = case_ranges(case)
        restate = lambda: x6_restate(a, b, ranges, perwave, case["alpha"], bias, case["beta"], C0)                   # noqa: E731
        exact = mode != "normal"
        prob = make_problem("%s/%s%s" % (case["id"], mode, "/perwave" if perwave else ""), "exact" if exact else "normal", M, N, [(a, b)],
                            [[(a, b, k0, k1)] for k0, k1 in ranges], case["alpha"], case["beta"], bias, C0, restate=restate,
                            max_abs=MAX_ABS.get(mode, (8, 8)), defer=exact and defer)
        prob.update(ranges=ranges, perwave=perwave, pass_=mode)
        _PROBLEMS[key] = prob
    return _PROBLEMS[key]


def dwhh_tensors(case, prob):
    """(dgx [rows][3H], dghn, hprev [rows][H]) that hold the problem's a = [dgx[:, :2H] | dghn]^T and b = hprev; the unused columns [2H, 3H) of dgx carry
    other values (the dghn band shifted by one row and negated, plus one: never equal to it), so that a read from the wrong band cannot pass"""
    a, b = prob["pieces"][0]
    H = case["H"]
    at = a.t().contiguous()                                  # [rows][3H]
    other = -at[:, 2 * H:].roll(1, 0) + 1.0
    return torch.cat([at[:, :2 * H], other], 1).contiguous(), at[:, 2 * H:].contiguous(), b


def x6_line(case, kern, plan, res, nexact=None, modes=EXACT_MODES):
    p = plan["launches"][0] if case["kind"] == "dwhh" else plan
    sched = sorted({(n, r) for n, r, _ in p["blocks"]})
    return "%-78s %-20s ranges %2d grid %-11s %-5s %-20s blocks %-22s exact %s  ratio %6.3f tile (%d, %d)" % (
        case["id"], p["kernel"], p["ranges"], "x".join(map(str, p["grid_xyz"])), "walk" if p["walks"] else "-", p["reduce"] or "-",
        ",".join("%d%s" % (n, "+%dr" % r if r else "") for n, r in sched)[:22],
        "/".join(modes) + ("" if nexact is None else " %d/%d" % (nexact, len(modes) * case["M"] * case["N"])), *res)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what the tables must reach
# ---------------------------------------------------------------------------------------------------------------------------------------------
def x6_coverage_wanted():
    want = set()
    for k in (X6P, X6W, X6V):
        want |= {(k, "3d", "one", None), (k, "3d", "one", R4), (k, "3d", "one", R1), (k, "1d", "one", R4), (k, "1d", "one", R1)}
    want |= {(X6W, "1d", "walk", R4), (X6V, "1d", "walk", R4), (NTX6, "1d", "one", None), (NTX6, "1d", "walk", None)}
    want |= {("fn_gru_dwhh_f32", form, k) for form in ("one-launch", "two-products") for k in (X6P, X6W)}
    # every trip count of the schedules: block counts 1 .. 13 whole, and partial last blocks on either side of every boundary
    for k in (X6W, X6V):
        NS, LEAD, PARTIAL = X6_TRIPS[k]
        REST = 2 * NS + LEAD - 2 + PARTIAL
        want |= {(k, "nblk", n, False) for n in range(1, 14)}
        want |= {(k, "nblk", n, True) for n in (1, REST, REST + 1, REST + NS, REST + NS + 1) if n <= 13}
        want |= {(k, "passes", p) for p in (0, 1, 2)} | {(k, "tail", t) for t in range(1, REST + 1)}
    want |= {(NTX6, "nblk", n, False) for n in (4, 5, 6, 7, 8, 10, 11, 13)} | {(NTX6, "passes", p) for p in (0, 1, 2, 3)}
    want |= {(X6P, "pairs-odd-steps", p > 0, o, s) for p in (0, 1) for o in (0, 1) for s in (0, 1, 7, 8) if p or o or s}
    return want


def x6_coverage_reached():
    got = set()
    for c in X6_CASES:
        for kern in c["kernels"]:
            plan = x6_case_plan(c, kern)
            for p in plan["launches"] if c["kind"] == "dwhh" else [plan]:
                got.add((p["kernel"], p["grid"], "walk" if p["walks"] else "one", p["reduce"]))
                if c["kind"] == "dwhh":
                    got.add(("fn_gru_dwhh_f32", plan["form"], p["kernel"]))
                for n, r, s in p["blocks"]:
                    if p["kernel"] == X6P:
                        got.add((X6P, "pairs-odd-steps", s["pairs"] > 0, s["odd"], s["fp32_steps"]))
                    else:
                        got |= {(p["kernel"], "nblk", n, r > 0), (p["kernel"], "passes", s["passes"]), (p["kernel"], "tail", s["tail"])}
    return got
