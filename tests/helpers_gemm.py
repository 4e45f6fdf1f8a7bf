"""Shared code of tests/test_gemm_reference.py (CPU) and tests/test_gpu_gemm_paths.py (MI355X): the fp32 GEMMs of csrc/gemm.hip that are not the
LDS-free NT kernel - the LDS-staged gemm_kernel<BM, BN, BK, ..> in its five tile shapes, gemm_multi_kernel, the weight-gradient kernels
gemm_tn_kernel / gemm_tn_lean_kernel (also behind fn_gru_dwhh_f32) and the two split-K reductions - exactly and per tile against float64.

  gemm_instance / multi_plan / dwhh_plan   the host-side dispatch and the device-side choice of load path restated on shapes, leading dimensions
                             and addresses: which kernel instance a call launches, its K ranges, the grid form of a TN launch, the slab
                             reduction that follows, and per tile and K range whether the staged loop takes load_fast or load_checked;
                             its host-side fields are checked against the library's own answer (fn_gemm_plan / fn_gru_dwhh_plan)
  x6_tn_plan / x6_nt_plan / trip_schedule   the same for a bf16 x 6 launch (the mode bits, 128 x 128 or 128 x 256 tiles, workgroups that walk items, per K
                             range its 32-k blocks and what x6w_trips makes of them); cases, passes and restatement of those kernels: helpers_gemm_x6.py
  lib_gemm_plan / lib_dwhh_plan / assert_mirror_matches_library   that answer, and the comparison
  restate32(prob)            the float32 restatement: every accumulator adds its K range in order, as sequential float32 additions of 8-wide chunk
                             products; the accumulators of a split launch are then added in slab order; alpha, bias, beta C as the epilogue
  check_exact(prob, cbuf)    operands, bias and C0 integers of [-8, 8]: sum |a||b| + |bias| + |beta c| < 2^24 per output element (asserted), so every
                             partial sum is exact in float32 in any order and the result must equal float64 BIT FOR BIT
  check_normal(prob, cbuf)   standard normals: per 16 x 16 tile err = max |got - ref64| / max |ref64| over that tile alone, err <= F x max(e_ref, 2**-23),
                             e_ref = restate32's own error in that tile (helpers_head.tile_errors / worst_ratio)
Both checks first ask that nothing outside the [M][N] view of the sentinel-filled, over-allocated C buffer was written.
"""
import zlib

import numpy as np
import torch

from helpers import SCAN_F_CAP, SCAN_MIN_REF
from helpers_head import nt_direct_instance, tile_errors, worst_ratio

GEMM_SENTINEL = -123.25
GEMM_PAD_ROWS = 3
# bound of the normal pass per family: the smallest power of two >= 1.5 x the worst ratio measured on an MI355X, capped at SCAN_F_CAP (the rule
# of DESIGN 11d; e_ref itself is built from single IEEE operations and is the same on every host).  Measured (profiles/gemm_fp64_errors.txt):
# staged 5.902, multi 4.309, tn 4.190, tn-lean 3.378, dwhh 6.096
GEMM_F = {"staged": 16, "multi": 8, "tn": 8, "tn-lean": 8, "dwhh": 16}
GEMM_FAMILIES = tuple(GEMM_F)
assert all(f <= SCAN_F_CAP for f in GEMM_F.values())

STAGED = {"gemm_kernel<64,16,16>": (64, 16, 16), "gemm_kernel<128,128,32>": (128, 128, 32), "gemm_kernel<32,64,32>": (32, 64, 32),
          "gemm_kernel<64,64,32>": (64, 64, 32), "gemm_kernel<64,64,16>": (64, 64, 16)}
TN_PF = {"gemm_tn_kernel": 8, "gemm_tn_lean_kernel": 4}
# the one combination fn_gemm_f32 cannot reach: both operands row-contiguous AND 16-byte aligned go to gemm_tn_kernel before any staged instance, so the
# staged <.., AKC = false, BKC = false> instances never see operands that pass Stage::can_fast
UNREACHABLE = {("staged", (False, False), "fast"): "aligned TN operands are taken by gemm_tn_kernel first"}


def _cdiv(a, b):
    return (a + b - 1) // b


def _al16(p, ld):
    return p % 16 == 0 and ld % 4 == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the dispatch restated on shapes.  The library decides it in one place (csrc/gemm_plan.h) and hands the decision out (fn_gemm_plan /
# fn_gru_dwhh_plan); this restatement adds what only the device sees (load paths, pipeline steps) and is itself CHECKED AGAINST THE LIBRARY: on the CPU
# for every case and a seeded sweep (test_gemm_reference.py), on the MI355X for every launch on its real addresses (assert_mirror_matches_library)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PLAN_CUS = 256                      # compute units the CPU tests state (an MI355X has 256); a GPU test asks for the device's own


def _lib():
    from mfn_import import load_package
    load_package()
    from music_fader_nets_amd import _lib as lib
    return lib


def _flags(lean, x6):
    """lean / x6 (False, True = FN_GEMM_BF16X6, or the bf16 x 6 bits themselves) as they ride on the splitk argument"""
    lib = _lib()
    return (lib.GEMM_LEAN if lean else 0) | (lib.GEMM_BF16X6 if x6 is True else int(x6))


def lib_gemm_plan(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, lean, x6=False, cus=PLAN_CUS):
    """fn_gemm_plan for the call gemm_instance describes (same arguments), as a dict; no device is touched"""
    import ctypes
    lib = _lib()
    pA, pB, pC, pbias = ptrs[:4]
    pws = ptrs[4] if len(ptrs) > 4 else 0
    plan = lib.FnGemmPlan()
    rc = lib.load().fn_gemm_plan(int(a_k), int(b_k), M, N, K, lda, ldb, ldc, pA, pB, pC, pbias, pws, splitk | _flags(lean, x6), cus, ctypes.byref(plan))
    assert rc == 0, rc
    return plan.as_dict()


def lib_dwhh_plan(H, rows, ptrs, splitk, lean, x6=False, cus=PLAN_CUS):
    """fn_gru_dwhh_plan for the call dwhh_plan describes, as dict(form, launches)"""
    import ctypes
    lib = _lib()
    pws = ptrs[4] if len(ptrs) > 4 else 0
    n, plans = ctypes.c_int32(), (lib.FnGemmPlan * 2)()
    rc = lib.load().fn_gru_dwhh_plan(ptrs[0], ptrs[1], ptrs[2], ptrs[3], pws, rows, H, splitk | _flags(lean, x6), cus, ctypes.byref(n), plans)
    assert rc == 0, rc
    return dict(form="one-launch" if n.value == 1 else "two-products", launches=[plans[i].as_dict() for i in range(n.value)])


def assert_mirror_matches_library(mp, lp, M, N, what=""):
    """the host-side fields of a mirror plan (gemm_instance / tn_plan) against the library's plan of the same call (lib_gemm_plan, HipOps.gemm_plan):
    kernel, klen, ranges, grid form (and, the fp32 kernels have no walking form, the grid itself), reduce kernel and its trips, tiles, msplit"""
    assert lp["kernel"] == mp["kernel"], (what, mp["kernel"], lp)
    if mp["family"] == "x6":                         # the bf16 x 6 kernels: the grid itself (a walking launch is cus x 1 x 1), item count = tiles x ranges
        trips = 0 if lp["reduce"] is None else _cdiv(M * N // 4 if lp["reduce"] == "slab_reduce4_kernel" else M * N, lp["reduce_blocks"] * 256)
        got = (lp["klen"], lp["ranges"], lp["grid"], lp["tiles"], lp["reduce"], trips, lp["msplit"])
        assert got == (mp["klen"], mp["ranges"], mp["grid_xyz"], mp["tiles"], mp["reduce"], mp["reduce_trips"], mp["msplit"]), (what, mp, lp)
        assert mp["items"] == lp["tiles"] * lp["ranges"] and mp["walks"] == (lp["grid"][2] == 1 and lp["grid"][0] < mp["items"]), (what, mp, lp)
        assert (lp["reduce_blocks"] == 0) == (mp["ranges"] == 1) and lp["reduce_blocks"] <= 2048
        return
    if mp["family"] == "nt-direct":
        tiles = (M // 128) * (N // 128)
        assert (lp["klen"] > 0, lp["ranges"], lp["grid"], lp["tiles"], lp["reduce"], lp["reduce_blocks"]) == (True, 1, (tiles, 1, 1), tiles, None, 0), (what, lp)
        return
    S, tiles = mp["ranges"], mp["tiles"]
    grid = (tiles * S, 1, 1) if mp.get("grid") == "1d" else (tiles, 1, S)
    trips = 0 if lp["reduce"] is None else _cdiv(M * N // 4 if lp["reduce"] == "slab_reduce4_kernel" else M * N, lp["reduce_blocks"] * 256)
    got = (lp["klen"], lp["ranges"], lp["grid"], lp["tiles"], lp["reduce"], trips, lp["msplit"])
    assert got == (mp["klen"], S, grid, tiles, mp["reduce"], mp["reduce_trips"], mp.get("msplit", 0)), (what, mp, lp)
    assert (lp["reduce_blocks"] == 0) == (S == 1) and lp["reduce_blocks"] <= 2048


def assert_dwhh_mirror_matches_library(mp, lp, H, what=""):
    assert lp["form"] == mp["form"] and len(lp["launches"]) == len(mp["launches"]), (what, mp["form"], lp)
    for m, l, rows in zip(mp["launches"], lp["launches"], (3 * H,) if mp["form"] == "one-launch" else (2 * H, H)):
        assert_mirror_matches_library(m, l, rows, H, what)


def split_ranges(K, splitk, gran):
    """(klen, number of K ranges) as launch_gemm / launch_tn recompute them: ranges of whole `gran`-k blocks, the last one short"""
    if splitk <= 1:
        return K, 1
    klen = _cdiv(_cdiv(K, splitk), gran) * gran
    return klen, _cdiv(K, klen)


def k_ranges(K, klen):
    return [(k0, min(K, k0 + klen)) for k0 in range(0, K, klen)]


def slab_reduction(S, M, N, ldc, pws, pC, pbias):
    """(kernel, trips of its grid-stride loop) of launch_slab_reduce, (None, 0) for an unsplit launch"""
    if S <= 1:
        return None, 0
    v4 = N % 4 == 0 and ldc % 4 == 0 and (pws | pC | pbias) % 16 == 0
    total = M * N // 4 if v4 else M * N
    blocks = min(_cdiv(total, 256), 2048)
    return ("slab_reduce4_kernel" if v4 else "slab_reduce_kernel"), _cdiv(total, blocks * 256)


def staged_loads(BM, BN, BK, a_k, b_k, M, N, lda, ldb, pA, pB, ranges):
    """{'fast': n, 'checked': n} over (tile, K range) workgroups of gemm_kernel: Stage::can_fast of both operands - 16-byte alignment, a range made
    of whole BK tiles, and for a row-contiguous operand every tile row inside the matrix (a K-contiguous one clamps its rows)"""
    n = {"fast": 0, "checked": 0}
    for k0, k1 in ranges:
        whole = (k1 - k0) % BK == 0 and k0 % 4 == 0
        for tm in range(_cdiv(M, BM)):
            fa = _al16(pA, lda) and whole and (a_k or tm * BM + BM <= M)
            for tn in range(_cdiv(N, BN)):
                fb = _al16(pB, ldb) and whole and (b_k or tn * BN + BN <= N)
                n["fast" if fa and fb else "checked"] += 1
    return n


X6P, X6W, X6V, NTX6 = "gemm_tn_x6_kernel", "gemm_tn_x6w_kernel", "gemm_tn_x6v_kernel", "gemm_nt_x6w_kernel"
# x6w_trips<NS, LEAD, PARTIAL> as each producer / consumer kernel instantiates it (x6w_produce, x6v_produce, x6w_produce_nt)
X6_TRIPS = {X6W: (3, 2, True), X6V: (2, 1, True), NTX6: (3, 2, False)}


def x6_bits(x6):
    """x6 as it reaches the mirror (True = FN_GEMM_BF16X6 alone, or the bits themselves) -> (per-wave, wide, per-tile)"""
    lib = _lib()
    bits = 0 if x6 is True else int(x6)
    perwave = bool(bits & lib.GEMM_X6_PERWAVE)
    return perwave, bool(bits & lib.GEMM_X6_WIDE) and not perwave, bool(bits & lib.GEMM_X6_PERTILE)


def trip_schedule(nblk, NS, LEAD, PARTIAL):
    """x6w_trips(nblk) restated: the prologue requests blocks 0 .. NS + LEAD - 2 and cuts blocks 0 .. LEAD - 1 (those that exist); steady passes of NS
    fused trips run while t + REST < nblk, REST = 2 NS + LEAD - 2 + PARTIAL; the tail runs the trips that are left (<= REST) through the guarded
    request / cut.  prologue_only: every block was cut in the prologue (no trip cuts anything).  One barrier per block and one more."""
    REST = 2 * NS + LEAD - 2 + (1 if PARTIAL else 0)
    t = passes = 0
    while t + REST < nblk:
        t += NS
        passes += 1
    return dict(requested=min(NS + LEAD - 1, nblk), cut=min(LEAD, nblk), prologue_only=nblk <= LEAD, passes=passes, tail=nblk - t, rest=REST,
                barriers=1 + nblk)


def x6_blocks(kernel, ranges):
    """per K range (32-k blocks the kernel's bf16 loop runs, rows of the partial last block, what becomes of it): the producer / consumer kernels count
    a partial block as a block (its missing rows are zeros) and run the trip schedule over them; the per-wave kernel runs whole blocks in pairs plus an
    odd one and the partial rows as fp32 MFMA steps of four"""
    out = []
    for k0, k1 in ranges:
        n, r = (k1 - k0) >> 5, (k1 - k0) & 31
        if kernel == X6P:
            out.append((n, r, dict(pairs=n // 2, odd=n & 1, fp32_steps=_cdiv(r, 4))))
        else:
            out.append((n + (r > 0), r, trip_schedule(n + (r > 0), *X6_TRIPS[kernel])))
    return out


def x6_tn_plan(M, N, K, ldc, pC, pbias, pws, splitk, x6, msplit, cus):
    """a bf16 x 6 TN launch in full: the kernel by the mode bits, K ranges of whole 32-k blocks, 128 x 128 or 128 x 256 tiles, the grid form and the grid
    itself - a 1-D launch of a producer / consumer kernel with more (tile, K range) items than compute units is one workgroup per compute unit WALKING
    items blockIdx.x, + gridDim.x, .. unless FN_GEMM_X6_PERTILE or a CU count that is no multiple of 8 -, msplit, the slab reduction, and per K range
    its blocks and trip schedule"""
    perwave, wide, pertile = x6_bits(x6)
    kernel = X6P if perwave else X6V if wide else X6W
    klen, S = split_ranges(K, splitk, 32)
    tiles = _cdiv(M, 128) * _cdiv(N, 256 if wide else 128)
    one_d = S > 1 and S % 8 == 0
    items = tiles * S
    walks = not perwave and one_d and not pertile and cus >= 8 and cus % 8 == 0 and items > cus
    red, trips = slab_reduction(S, M, N, ldc, pws, pC, pbias)
    return dict(kernel=kernel, family="x6", klen=klen, ranges=S, tiles=tiles, items=items, grid="1d" if one_d else "3d", walks=walks,
                grid_xyz=(cus if walks else items if one_d else tiles, 1, 1 if one_d else S), msplit=msplit, reduce=red, reduce_trips=trips,
                blocks=x6_blocks(kernel, k_ranges(K, klen)), loads=None)


def x6_nt_plan(M, N, K, x6, cus):
    """gemm_nt_x6w_kernel: whole 128 x 128 tiles, K / 32 whole blocks, one workgroup per tile or - more tiles than compute units - one per compute unit
    walking tiles"""
    tiles = (M // 128) * (N // 128)
    walks = tiles > cus and cus >= 8 and cus % 8 == 0 and not x6_bits(x6)[2]
    return dict(kernel=NTX6, family="x6", klen=K, ranges=1, tiles=tiles, items=tiles, grid="1d", walks=walks, grid_xyz=(cus if walks else tiles, 1, 1),
                msplit=0, reduce=None, reduce_trips=0, blocks=x6_blocks(NTX6, [(0, K)]), loads=None)


def tn_plan(M, N, K, ldc, pC, pbias, pws, splitk, lean, x6=False, msplit=0, cus=PLAN_CUS):
    if x6:
        return x6_tn_plan(M, N, K, ldc, pC, pbias, pws, splitk, x6, msplit, cus)
    klen, S = split_ranges(K, splitk, 4)
    kernel = "gemm_tn_lean_kernel" if lean else "gemm_tn_kernel"
    PF = TN_PF[kernel]
    red, trips = slab_reduction(S, M, N, ldc, pws, pC, pbias)
    steps = []
    for k0, k1 in k_ranges(K, klen):
        nfull = (k1 - k0) >> 2
        steps.append((nfull, (k1 - k0) & 3, nfull // PF * PF))          # whole 4-k steps, rows of the partial last step, pipelined steps
    return dict(kernel=kernel, family="tn-lean" if lean else "tn", klen=klen, ranges=S, grid="1d" if S > 1 and S % 8 == 0 else "3d", reduce=red,
                reduce_trips=trips, steps=steps, tiles=_cdiv(M, 128) * _cdiv(N, 128), msplit=msplit, loads=None)


def gemm_instance(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, lean, x6=False, cus=PLAN_CUS):
    """what fn_gemm_f32 launches for this call.  ptrs = (A, B, C, bias[, workspace]) addresses, 0 = none; splitk = the K ranges asked for; x6: False, True
    (FN_GEMM_BF16X6) or the bf16 x 6 bits; cus: compute units (only the bf16 x 6 producer / consumer kernels' grids depend on it).
    dict(kernel, family, klen, ranges, reduce, reduce_trips, and for the TN kernels grid / steps, for the staged kernel loads / nk, for the bf16 x 6
    kernels x6_tn_plan / x6_nt_plan)"""
    pA, pB, pC, pbias = ptrs[:4]
    pws = ptrs[4] if len(ptrs) > 4 else 0
    if not a_k and not b_k and lda % 4 == 0 and ldb % 4 == 0 and lda >= 4 and ldb >= 4 and (pA | pB) % 16 == 0:
        return tn_plan(M, N, K, ldc, pC, pbias, pws, splitk, lean, x6, cus=cus)
    al = lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and (pA | pB | pC | pbias) % 16 == 0
    if x6 and a_k and b_k and splitk <= 1 and M % 128 == 0 and N % 128 == 0 and K % 32 == 0 and K >= 128 and al and (M // 128) * (N // 128) >= 128:
        return x6_nt_plan(M, N, K, x6, cus)
    direct = nt_direct_instance(M, N, K, lda, ldb, ldc, (pA, pB, pC, pbias), lean, splitk, a_k, b_k, x6=False)
    if direct is not None:
        return dict(kernel=direct, family="nt-direct")
    if N <= 16 and a_k and b_k and splitk <= 1 and M >= 64:
        kernel = "gemm_kernel<64,16,16>"
    elif _cdiv(M, 128) * _cdiv(N, 128) * max(splitk, 1) >= 256:
        kernel = "gemm_kernel<128,128,32>"
    elif splitk <= 1 and K % 32 == 0 and K >= 128:
        kernel = "gemm_kernel<32,64,32>" if a_k and b_k and _cdiv(M, 64) * _cdiv(N, 64) < 240 and M >= 64 else "gemm_kernel<64,64,32>"
    else:
        kernel = "gemm_kernel<64,64,16>"
    BM, BN, BK = STAGED[kernel]
    klen, S = split_ranges(K, splitk, BK)
    ranges = k_ranges(K, klen)
    red, trips = slab_reduction(S, M, N, ldc, pws, pC, pbias)
    return dict(kernel=kernel, family="staged", klen=klen, ranges=S, reduce=red, reduce_trips=trips, tiles=_cdiv(M, BM) * _cdiv(N, BN),
                loads=staged_loads(BM, BN, BK, a_k, b_k, M, N, lda, ldb, pA, pB, ranges), nk=sorted({_cdiv(k1 - k0, BK) for k0, k1 in ranges}))


def multi_plan(a_k, b_k, jobs):
    """fn_gemm_multi on jobs = [dict(M, N, segs=[(K, lda, ldb, A address, B address), ..])]: dict(grid = tiles of the widest job, jobs = [dict(tiles,
    idle = workgroups that return at once, segs = [dict(nk, loads = {'fast': tiles on fn_kloop<4> + load_fast, 'checked': tiles on
    fn_kloop<PF_DEPTH> + load_checked})])])"""
    out = []
    for j in jobs:
        M, N = j["M"], j["N"]
        segs = []
        for K, lda, ldb, pA, pB in j["segs"]:
            segs.append(dict(nk=_cdiv(K, 16), loads=staged_loads(64, 64, 16, a_k, b_k, M, N, lda, ldb, pA, pB, [(0, K)])))
        out.append(dict(tiles=_cdiv(M, 64) * _cdiv(N, 64), segs=segs))
    grid = max(j["tiles"] for j in out)
    for j in out:
        j["idle"] = grid - j["tiles"]
    return dict(kernel="gemm_multi_kernel", family="multi", grid=grid, jobs=out)


def dwhh_plan(H, rows, ptrs, splitk, lean, x6=False, cus=PLAN_CUS):
    """fn_gru_dwhh_f32: ptrs = (dgx, dghn, hprev, dW[, workspace]).  One split-A launch of the TN kernel (msplit = 2H, rows >= 2H from dghn) when 2H
    is a multiple of the 128-row tile, else two fn_gemm_f32 products - which do not carry the lean flag on."""
    pgx, pghn, php, pdw = ptrs[:4]
    pws = ptrs[4] if len(ptrs) > 4 else 0
    if (2 * H) % 128 == 0 and H % 4 == 0 and (pgx | pghn | php) % 16 == 0:
        return dict(form="one-launch", launches=[tn_plan(3 * H, H, rows, H, pdw, 0, pws, splitk, lean, x6, msplit=2 * H, cus=cus)])
    return dict(form="two-products", launches=[gemm_instance(False, False, 2 * H, H, rows, 3 * H, H, H, (pgx, php, pdw, 0, pws), splitk, False, x6, cus),
                                               gemm_instance(False, False, H, H, rows, H, H, H, (pghn, php, pdw + 8 * H * H, 0, pws), splitk, False, x6, cus)])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# problems: references, restatement, checkers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _draw(shape, mode, gen):
    if mode == "exact":
        return torch.randint(-8, 9, shape, generator=gen).float()
    return torch.randn(shape, generator=gen)


def _gen(cid, mode):
    return torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (cid, mode)).encode()))


def restate32(chains, alpha, bias, beta, C0, M, N):
    """float32 restatement.  chains = [[(a [M][K], b [K][N], k0, k1), ..], ..]: every chain is ONE accumulator that walks its pieces in order, adding
    8-wide chunk products one after the other in float32 (the K loop of a workgroup: a K range of a split launch, or the segments of a gemm_multi
    job); the chains are then added in order (the slab reduction); then o = alpha s, o += bias, o += beta C0.  A chunk product is itself eight rounded
    products added in ascending k - single IEEE operations, no library matmul - so e_ref is the same on every machine that runs the test (the head
    suite's e_ref comes from the CPU's sgemm and moves one kernel output's ratio between 8.0 and 13.0 from one machine to the next)."""
    total = None
    for chain in chains:
        acc = torch.zeros(M, N, dtype=torch.float32)
        for a, b, k0, k1 in chain:
            assert a.dtype == torch.float32 and b.dtype == torch.float32
            at = a.t().contiguous()
            for c0 in range(k0, k1, 8):
                chunk = at[c0].unsqueeze(1) * b[c0]
                for k in range(c0 + 1, min(k1, c0 + 8)):
                    chunk = chunk + at[k].unsqueeze(1) * b[k]
                acc = acc + chunk
        total = acc if total is None else total + acc
    o = alpha * total
    if bias is not None:
        o = o + bias
    if beta != 0.0:
        o = o + beta * C0
    assert o.dtype == torch.float32
    return o


def reference64(pieces, alpha, bias, beta, C0):
    acc = sum(a.double() @ b.double() for a, b in pieces)
    if bias is not None:
        acc = alpha * acc + bias.double()
    else:
        acc = alpha * acc
    return acc + beta * C0.double() if beta != 0.0 else acc


def assert_exact_condition(pieces, bias, beta, C0, cid, max_abs=(8, 8)):
    """sum |a||b| + |bias| + |beta c| < 2^24 in every output element: every partial sum of the kernel, in any order and across K ranges and slabs, is then
    an integer (or half-integer) that float32 holds exactly.  max_abs: the span of the integers of a and of b ([-8, 8] unless a pass says otherwise)"""
    mag = sum(a.double().abs() @ b.double().abs() for a, b in pieces)
    if bias is not None:
        mag = mag + bias.double().abs()
    mag = mag + abs(beta) * C0.double().abs()
    assert float(mag.max()) < 2.0 ** 24, "%s: exact pass would leave the integers float32 holds (%.0f)" % (cid, float(mag.max()))
    for a, b in pieces:
        assert bool((a == a.round()).all()) and bool((b == b.round()).all()) and float(a.abs().max()) <= max_abs[0] and float(b.abs().max()) <= max_abs[1]


def make_problem(cid, mode, M, N, pieces, chains, alpha, beta, bias, C0, restate=None, max_abs=(8, 8), defer=False):
    """pieces = [(a [M][K], b [K][N])] in logical form; chains index into them (see restate32).  restate: another float32 restatement of the kernel's
    arithmetic than restate32 (a callable without arguments: the bf16 x 6 kernels, helpers_gemm_x6.py).  defer (exact problems only, whose check needs no
    e_ref): the restatement is not run here - prob['restate']() runs it (a CPU test asks that it equals float64; a GPU test has no use for it)"""
    ref64 = reference64(pieces, alpha, bias, beta, C0)
    if mode == "exact":
        assert_exact_condition(pieces, bias, beta, C0, cid, max_abs)
    if restate is None:
        restate = lambda: restate32(chains, alpha, bias, beta, C0, M, N)                         # noqa: E731
    if defer:
        assert mode == "exact"
        return dict(id=cid, mode=mode, M=M, N=N, pieces=pieces, chains=chains, alpha=alpha, beta=beta, bias=bias, C0=C0, ref64=ref64, restate=restate)
    fake32 = restate()
    e_ref, den = tile_errors(fake32, ref64)
    assert den.min() >= SCAN_MIN_REF, "input condition: %s has a tile maximum of %.3e < 2**-100" % (cid, den.min())
    assert np.isfinite(e_ref).all()
    if mode == "exact":
        assert bool((fake32.double() == ref64).all()), "%s: the restatement of the integer pass is not exact" % cid
    return dict(id=cid, mode=mode, M=M, N=N, pieces=pieces, chains=chains, alpha=alpha, beta=beta, bias=bias, C0=C0, ref64=ref64, fake32=fake32, e_ref=e_ref,
                den=den)


def c_buffer(prob, c0, ldc, device="cpu"):
    """sentinel-filled [M + pad][ldc] buffer; its [:M, c0:c0 + N] view holds C0 (beta != 0) or NaN (beta == 0: C must not be read)"""
    M, N = prob["M"], prob["N"]
    assert ldc >= c0 + N
    buf = torch.full((M + GEMM_PAD_ROWS, ldc), GEMM_SENTINEL, device=device)
    buf[:M, c0:c0 + N] = prob["C0"].to(device) if prob["beta"] != 0.0 else float("nan")
    return buf


def _check_layout(prob, cbuf, c0):
    M, N = prob["M"], prob["N"]
    out = cbuf.clone()
    out[:M, c0:c0 + N] = GEMM_SENTINEL
    bad = torch.nonzero(out != GEMM_SENTINEL)
    assert bad.numel() == 0, "%s: C was written outside [M][N]: buffer row %d, column %d (view: rows < %d, columns %d .. %d)" % (
        prob["id"], int(bad[0][0]), int(bad[0][1]), M, c0, c0 + N - 1)
    return cbuf[:M, c0:c0 + N]


def check_exact(prob, cbuf, c0=0):
    """bit for bit against float64; returns the number of elements compared"""
    assert prob["mode"] == "exact"
    got = _check_layout(prob, cbuf, c0).double()
    ne = torch.nonzero(~(got == prob["ref64"]))                 # NaN counts as different
    if ne.numel():
        i, j = int(ne[0][0]), int(ne[0][1])
        tiles = {(int(r) // 16, int(c) // 16) for r, c in ne.tolist()}
        raise AssertionError("%s: exact pass: %d of %d elements differ from float64 in %d of %d tiles, first at (%d, %d) in tile (rows %d.., columns %d..): got %r, want %r" % (
            prob["id"], ne.shape[0], got.numel(), len(tiles), _cdiv(prob["M"], 16) * _cdiv(prob["N"], 16), i, j, i // 16 * 16, j // 16 * 16, float(got[i, j]),
            float(prob["ref64"][i, j])))
    return got.numel()


def check_normal(prob, cbuf, c0=0, F=SCAN_F_CAP):
    """per 16 x 16 tile against float64; returns (worst ratio, tile row, tile column)"""
    assert F <= SCAN_F_CAP
    got = _check_layout(prob, cbuf, c0)
    e, den = tile_errors(got, prob["ref64"])
    r, i, j, n = worst_ratio(e, prob["e_ref"], F)
    assert r <= F, "%s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., columns %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
        prob["id"], e[i, j], r, prob["e_ref"][i, j], 16 * i, 16 * j, den[i, j], n, e.size, F)
    return r, i, j


def check(prob, cbuf, c0=0, F=SCAN_F_CAP):
    return check_exact(prob, cbuf, c0) if prob["mode"] == "exact" else check_normal(prob, cbuf, c0, F)


def old_metric_accepts(got, ref, tol=1e-5):
    """what test_gemm asks: max |got - ref| < 1e-5 of the WHOLE tensor's maximum"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(1e-12, float(ref.abs().max())) < tol


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fn_gemm_f32 cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
NT, NN, TT, TN = (True, True), (True, False), (False, True), (False, False)            # (a_k, b_k): A [M][K] or [K][M], B [N][K] or [K][N]
LAYOUT_NAME = {NT: "nt", NN: "nn", TT: "tt", TN: "tn"}


def _r4(x):
    return (x + 3) // 4 * 4


def _gc(cid, lay, M, N, K, kernel, splitk=1, lean=False, alpha=0.5, beta=2.0, bias=True, a=(0, None), b=(0, None), c=(0, None), bias_off=0,
        loads=None, reduce=None, grid=None, trips=None):
    """a / b = (offset of the operand in floats behind a 16-byte aligned allocation, leading dimension or None = dense); c = (first column of the view,
    ldc or None = the next multiple of 4 above c0 + N, plus 4).  kernel / loads / reduce / grid / trips: what the id claims, checked against the mirror"""
    a_k, b_k = lay
    lda = a[1] if a[1] is not None else (K if a_k else M)
    ldb = b[1] if b[1] is not None else (K if b_k else N)
    ldc = c[1] if c[1] is not None else _r4(c[0] + N) + 4
    return dict(id=cid, a_k=a_k, b_k=b_k, M=M, N=N, K=K, splitk=splitk, lean=lean, alpha=alpha, beta=beta, bias=bias, a_off=a[0], lda=lda, b_off=b[0], ldb=ldb,
                c0=c[0], ldc=ldc, bias_off=bias_off, kernel=kernel, loads=loads, reduce=reduce, grid=grid, trips=trips)


G16, G32, G3264, G6416, G128 = ("gemm_kernel<64,64,16>", "gemm_kernel<64,64,32>", "gemm_kernel<32,64,32>", "gemm_kernel<64,16,16>", "gemm_kernel<128,128,32>")
FAST, CHK, MIX = ("fast",), ("checked",), ("checked", "fast")

STAGED_CASES = []
# <64,64,16>, the default: ragged M, N and K in every layout (dense row-contiguous operands of 70 / 50 / 7 / 3 columns are misaligned: the staged TN instance)
for _lay in (NT, NN, TT, TN):
    STAGED_CASES.append(_gc("s-64x64x16-%s-70x50x75-ragged-nk5-checked" % LAYOUT_NAME[_lay], _lay, 70, 50, 75, G16, loads=CHK))
    STAGED_CASES.append(_gc("s-64x64x16-%s-7x3x513-ragged-nk33-checked" % LAYOUT_NAME[_lay], _lay, 7, 3, 513, G16, loads=CHK, beta=0.0))
# K = 80 aligned: K-contiguous operands fast everywhere; a row-contiguous operand fast inside and checked on the ragged edge tile of the same launch
STAGED_CASES.append(_gc("s-64x64x16-nt-70x130x80-nk5-fast", NT, 70, 130, 80, G16, loads=FAST))
STAGED_CASES.append(_gc("s-64x64x16-nn-70x130x80-ldb132-nk5-fast-inside-checked-edge", NN, 70, 130, 80, G16, b=(0, 132), loads=MIX))
STAGED_CASES.append(_gc("s-64x64x16-tt-70x130x80-lda72-nk5-fast-inside-checked-edge", TT, 70, 130, 80, G16, a=(0, 72), loads=MIX, beta=0.0))
STAGED_CASES.append(_gc("s-64x64x16-tn-70x130x80-lda72-ldb132-B-off1-nk5-checked", TN, 70, 130, 80, G16, a=(0, 72), b=(1, 132), loads=CHK))
# nk in {1, 2, 3} against the two-deep prefetch, on both load paths (nk = 5: above)
for _K, _lay in ((16, NT), (32, NT), (48, NT)):
    STAGED_CASES.append(_gc("s-64x64x16-%s-70x50x%d-nk%d-fast" % (LAYOUT_NAME[_lay], _K, _K // 16), _lay, 70, 50, _K, G16, loads=FAST))
for _K, _lay in ((10, NN), (20, TT), (40, NT)):
    STAGED_CASES.append(_gc("s-64x64x16-%s-70x50x%d-nk%d-checked" % (LAYOUT_NAME[_lay], _K, (_K + 15) // 16), _lay, 70, 50, _K, G16, loads=CHK))
# operands misaligned by one float, ld % 4 != 0
STAGED_CASES.append(_gc("s-64x64x16-nt-70x50x80-A-off1-checked", NT, 70, 50, 80, G16, a=(1, 80), loads=CHK))
STAGED_CASES.append(_gc("s-64x64x16-nt-70x50x80-ldb82-checked", NT, 70, 50, 80, G16, b=(0, 82), loads=CHK, alpha=1.0))
# split-K: 8 ranges of 528, the last one 404 = 25 tiles + 4: checked while the others are fast
STAGED_CASES.append(_gc("s-64x64x16-nt-300x200x4100-split8-last-range-checked", NT, 300, 200, 4100, G16, splitk=8, loads=MIX, reduce="slab_reduce4_kernel"))
STAGED_CASES.append(_gc("s-64x64x16-nn-300x200x4100-split8-edge-and-last-range-checked", NN, 300, 200, 4100, G16, splitk=8, loads=MIX, reduce="slab_reduce4_kernel",
                        beta=0.0))
STAGED_CASES.append(_gc("s-64x64x16-tt-300x202x515-split3-ldc-odd-scalar-reduce", TT, 300, 202, 515, G16, splitk=3, c=(1, 207), loads=CHK, reduce="slab_reduce_kernel"))
# <64,64,32>: K % 32 == 0, K >= 128 in a non-NT layout, or NT with M < 64
STAGED_CASES.append(_gc("s-64x64x32-nn-70x50x128-nk4-checked-edge", NN, 70, 50, 128, G32, loads=CHK))
STAGED_CASES.append(_gc("s-64x64x32-nn-70x128x128-nk4-fast", NN, 70, 128, 128, G32, loads=FAST))
STAGED_CASES.append(_gc("s-64x64x32-tt-70x50x160-lda72-nk5-fast-inside-checked-edge", TT, 70, 50, 160, G32, a=(0, 72), loads=MIX))
STAGED_CASES.append(_gc("s-64x64x32-nt-50x70x128-M-below-64-nk4-fast", NT, 50, 70, 128, G32, loads=FAST))
STAGED_CASES.append(_gc("s-64x64x32-nt-50x70x160-lda162-M-below-64-nk5-checked", NT, 50, 70, 160, G32, a=(0, 162), loads=CHK))
STAGED_CASES.append(_gc("s-64x64x32-tn-70x50x160-misaligned-nk5-checked", TN, 70, 50, 160, G32, loads=CHK, beta=0.0))
# <32,64,32>: NT, M >= 64, fewer than 240 64-tiles
STAGED_CASES.append(_gc("s-32x64x32-nt-70x50x128-nk4-fast", NT, 70, 50, 128, G3264, loads=FAST))
STAGED_CASES.append(_gc("s-32x64x32-nt-70x50x160-nk5-fast", NT, 70, 50, 160, G3264, loads=FAST, beta=0.0))
STAGED_CASES.append(_gc("s-32x64x32-nt-64x130x128-B-off1-nk4-checked", NT, 64, 130, 128, G3264, b=(1, 128), loads=CHK))
# <64,16,16>: NT, N <= 16, M >= 64
for _N in (1, 3, 16):
    STAGED_CASES.append(_gc("s-64x16x16-nt-64x%dx80-nk5-fast" % _N, NT, 64, _N, 80, G6416, loads=FAST, beta=0.0 if _N == 3 else 2.0))
    STAGED_CASES.append(_gc("s-64x16x16-nt-70x%dx75-nk5-checked" % _N, NT, 70, _N, 75, G6416, loads=CHK))
# <128,128,32>: 256 tiles (the NT layout lands here because K % 16 != 0), and through split-K on a 300 x 200 output (6 tiles x 43 ranges)
STAGED_CASES.append(_gc("s-128x128x32-nt-2048x2048x40-nk2-checked", NT, 2048, 2048, 40, G128, loads=CHK))
STAGED_CASES.append(_gc("s-128x128x32-nn-1930x2040x40-ragged-nk2-checked", NN, 1930, 2040, 40, G128, loads=CHK, beta=0.0))
STAGED_CASES.append(_gc("s-128x128x32-nt-300x200x1376-split43-one-tile-per-range-fast", NT, 300, 200, 1376, G128, splitk=43, loads=FAST, reduce="slab_reduce4_kernel"))
STAGED_CASES.append(_gc("s-128x128x32-nt-300x200x4072-split43-nk3-last-range-40-checked", NT, 300, 200, 4072, G128, splitk=43, loads=MIX, reduce="slab_reduce4_kernel"))
STAGED_CASES.append(_gc("s-128x128x32-tt-300x200x4072-split43-lda300-edge-and-last-range-checked", TT, 300, 200, 4072, G128, splitk=43, loads=MIX,
                        reduce="slab_reduce4_kernel", beta=0.0))
STAGED_CASES.append(_gc("s-128x128x32-nn-300x200x1376-split43-fast-inside-checked-edge", NN, 300, 200, 1376, G128, splitk=43, loads=MIX, reduce="slab_reduce4_kernel"))
STAGED_CASES.append(_gc("s-128x128x32-tn-300x200x1376-split43-A-off1-checked", TN, 300, 200, 1376, G128, splitk=43, a=(1, 300), loads=CHK, reduce="slab_reduce4_kernel"))

TNK, TNL = "gemm_tn_kernel", "gemm_tn_lean_kernel"
TN_NFULL = {TNK: (0, 1, 7, 8, 9, 15, 16, 17, 24), TNL: (0, 1, 3, 4, 5, 7, 8, 9, 12)}          # 0, 1, PF - 1, PF, PF + 1, 2 PF - 1, 2 PF, 2 PF + 1, 3 PF
TN_CASES = []
for _kern in (TNK, TNL):
    _p = "t" if _kern == TNK else "tl"
    _lean = _kern == TNL
    # unsplit K = 4 nfull + r at 200 x 130 (ragged 128-tiles; B [K][130] with ldb = 132)
    for _nf in TN_NFULL[_kern]:
        for _r in (0, 1, 3):
            if 4 * _nf + _r:
                TN_CASES.append(_gc("%s-200x130-K%d-nfull%d-r%d" % (_p, 4 * _nf + _r, _nf, _r), TN, 200, 130, 4 * _nf + _r, _kern, lean=_lean, b=(0, 132), grid="3d",
                                    beta=0.0 if _r == 1 else 2.0))
    # M % 4 == 2 behind a [:, :342] view of a 344-wide matrix (the column-window clamp), and 5 x 1
    TN_CASES.append(_gc("%s-342x70-lda344-K37-window-clamp" % _p, TN, 342, 70, 37, _kern, lean=_lean, a=(0, 344), b=(0, 72), grid="3d"))
    TN_CASES.append(_gc("%s-5x1-K37" % _p, TN, 5, 1, 37, _kern, lean=_lean, a=(0, 8), b=(0, 4), grid="3d"))
    TN_CASES.append(_gc("%s-5x1-K515-split4-scalar-reduce" % _p, TN, 5, 1, 515, _kern, lean=_lean, a=(0, 8), b=(0, 4), splitk=4, grid="3d", reduce="slab_reduce_kernel"))
    # K ranges: 4 and 42 of them on the 3-D grid, 8 and 16 on the 1-D grid (dealt to the XCDs); every last range short
    for _K, _S, _g in ((515, 4, "3d"), (999, 42, "3d"), (1031, 8, "1d"), (4104, 16, "1d")):
        TN_CASES.append(_gc("%s-200x130-K%d-split%d-%s-scalar-reduce" % (_p, _K, _S, _g), TN, 200, 130, _K, _kern, lean=_lean, b=(0, 132), splitk=_S, grid=_g,
                            reduce="slab_reduce_kernel", beta=0.0 if _S == 42 else 2.0))
    TN_CASES.append(_gc("%s-342x72-lda344-K1031-split8-1d-float4-reduce" % _p, TN, 342, 72, 1031, _kern, lean=_lean, a=(0, 344), splitk=8, grid="1d",
                        reduce="slab_reduce4_kernel"))
# the float4 reduction at S in {2, 7, 8, 9, 16, 17} (its 8-deep load batch: none, one, one + tail, two, two + tail): K = 12 S - 1, ranges of 12 and a last one of 11
for _S in (2, 7, 8, 9, 16, 17):
    TN_CASES.append(_gc("t-136x72-K%d-split%d-float4-reduce" % (12 * _S - 1, _S), TN, 136, 72, 12 * _S - 1, TNK, splitk=_S, grid="1d" if _S % 8 == 0 else "3d",
                        reduce="slab_reduce4_kernel", beta=0.0 if _S == 9 else 2.0))
# C = dW[:, 342:] (8 bytes off a 16-byte boundary) and a bias one float off: the scalar reduction although N % 4 == 0 and ldc % 4 == 0
TN_CASES.append(_gc("t-342x72-lda344-K95-split8-C-column-342-scalar-reduce", TN, 342, 72, 95, TNK, a=(0, 344), splitk=8, c=(342, 416), grid="1d",
                    reduce="slab_reduce_kernel"))
TN_CASES.append(_gc("t-136x72-K95-split8-bias-off1-scalar-reduce", TN, 136, 72, 95, TNK, splitk=8, bias_off=1, grid="1d", reduce="slab_reduce_kernel"))
# more than 2048 x 256 items: the second trip of each reduction's grid-stride loop
TN_CASES.append(_gc("t-1030x2048-K9-split2-float4-reduce-second-trip", TN, 1030, 2048, 9, TNK, a=(0, 1032), splitk=2, grid="3d", reduce="slab_reduce4_kernel", trips=2))
TN_CASES.append(_gc("t-730x722-K9-split2-scalar-reduce-second-trip", TN, 730, 722, 9, TNK, a=(0, 732), b=(0, 724), splitk=2, grid="3d", reduce="slab_reduce_kernel",
                    trips=2, beta=0.0))

GEMM_CASES = STAGED_CASES + TN_CASES
GEMM_BY_ID = {c["id"]: c for c in GEMM_CASES}
assert len(GEMM_BY_ID) == len(GEMM_CASES)


def case_family(case):
    return {TNK: "tn", TNL: "tn-lean"}.get(case["kernel"], "staged")


def case_plan(case, ptrs=None):
    """the mirror on the case's nominal layout (allocations at 16-byte aligned addresses) or on real addresses"""
    if ptrs is None:
        ptrs = (4 * case["a_off"], 4 * case["b_off"], 4 * case["c0"], 4 * case["bias_off"] if case["bias"] else 0, 0)
    return gemm_instance(case["a_k"], case["b_k"], case["M"], case["N"], case["K"], case["lda"], case["ldb"], case["ldc"], ptrs, case["splitk"], case["lean"])


def assert_plan_matches_case(case, plan):
    """the plan is what the id claims"""
    assert plan["kernel"] == case["kernel"], (case["id"], plan["kernel"])
    assert plan["reduce"] == case["reduce"], (case["id"], plan["reduce"])
    if case["loads"] is not None:
        assert tuple(sorted(k for k, v in plan["loads"].items() if v)) == case["loads"], (case["id"], plan["loads"])
    if case["grid"] is not None:
        assert plan["grid"] == case["grid"], (case["id"], plan["grid"])
    if case["trips"] is not None:
        assert plan["reduce_trips"] == case["trips"], (case["id"], plan["reduce_trips"])


_PROBLEMS = {}


def gemm_operands(case, mode):
    """(a [M][K], b [K][N], C0, bias) in logical form from the case's own generator"""
    gen = _gen(case["id"], mode)
    M, N, K = case["M"], case["N"], case["K"]
    a, b = _draw((M, K), mode, gen), _draw((K, N), mode, gen)
    return a, b, _draw((M, N), mode, gen), (_draw((N,), mode, gen) if case["bias"] else None)


def gemm_problem(case, mode):
    key = (case["id"], mode)
    if key not in _PROBLEMS:
        a, b, C0, bias = gemm_operands(case, mode)
        plan = case_plan(case)
        chains = [[(a, b, k0, k1)] for k0, k1 in k_ranges(case["K"], plan["klen"])]
        assert len(chains) == plan["ranges"]
        _PROBLEMS[key] = make_problem(case["id"], mode, case["M"], case["N"], [(a, b)], chains, case["alpha"], case["beta"], bias, C0)
    return _PROBLEMS[key]


def stored(case, a, b):
    """the operands as the call stores them: A [M][K] or [K][M], B [N][K] or [K][N]"""
    return (a if case["a_k"] else a.t()), (b.t() if case["b_k"] else b)


def gemm_line(case, plan, mode_results):
    extra = ""
    if plan["family"] == "staged":
        extra = "fast %d checked %d nk %s" % (plan["loads"]["fast"], plan["loads"]["checked"], ",".join(map(str, plan["nk"])))
    else:
        extra = "grid %s steps %s" % (plan["grid"], ",".join("%d+%d" % (s[0], s[1]) for s in sorted(set(plan["steps"]))))
    return "%-76s %-24s ranges %2d %-20s %-34s exact %d/%d  ratio %6.3f tile (%d, %d)" % (
        case["id"], plan["kernel"], plan["ranges"], plan["reduce"] or "-", extra, mode_results["exact"], mode_results["exact"], *mode_results["normal"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fn_gru_dwhh_f32 cases: dW [3H][H] = beta dW + [dgx[:, :2H] | dghn]^T hprev
# ---------------------------------------------------------------------------------------------------------------------------------------------
DWHH_CASES = []
for _H, _form in ((64, "one-launch-msplit128-ragged-dghn-band"), (128, "one-launch-three-tiles"), (96, "two-products")):
    for _rows in (37, 1030):
        for _S in (1, 4, 8):
            for _beta, _lean in ((0.0, False), (1.0, True)):
                DWHH_CASES.append(dict(id="d-H%d-%s-rows%d-split%d-beta%d%s" % (_H, _form, _rows, _S, _beta, "-lean" if _lean else ""), H=_H, rows=_rows,
                                       splitk=_S, beta=_beta, lean=_lean, form="one-launch" if _H != 96 else "two-products"))
DWHH_BY_ID = {c["id"]: c for c in DWHH_CASES}


def dwhh_case_plan(case, ptrs=(0, 0, 0, 0, 0)):
    return dwhh_plan(case["H"], case["rows"], ptrs, case["splitk"], case["lean"])


def dwhh_operands(case, mode):
    """dgx [rows][3H] - its unused columns [2H, 3H) hold distinct integers (exact) / their own normals, so that a read from the wrong band cannot cancel -
    dghn, hprev [rows][H], dW0 [3H][H]"""
    gen = _gen(case["id"], mode)
    H, rows = case["H"], case["rows"]
    dgx, dghn, hp, W0 = _draw((rows, 3 * H), mode, gen), _draw((rows, H), mode, gen), _draw((rows, H), mode, gen), _draw((3 * H, H), mode, gen)
    if mode == "exact":
        dgx[:, 2 * H:] = ((torch.arange(rows * H).view(rows, H) * 7 + 3) % 17 - 8).float()
        assert not bool((dgx[:, 2 * H:] == dghn).all())
    return dgx, dghn, hp, W0


def dwhh_problem(case, mode, band_from_dgx=False):
    key = (case["id"], mode, band_from_dgx)
    if key not in _PROBLEMS:
        dgx, dghn, hp, W0 = dwhh_operands(case, mode)
        H, rows = case["H"], case["rows"]
        a = torch.cat([dgx[:, :2 * H], dgx[:, 2 * H:] if band_from_dgx else dghn], 1).t().contiguous()       # [3H][rows]
        plan = dwhh_case_plan(case)
        klen = plan["launches"][0]["klen"]
        assert all(p["klen"] == klen for p in plan["launches"])
        chains = [[(a, hp, k0, k1)] for k0, k1 in k_ranges(rows, klen)]
        _PROBLEMS[key] = make_problem(case["id"], mode, 3 * H, H, [(a, hp)], chains, 1.0, case["beta"], None, W0)
    return _PROBLEMS[key]


def dwhh_line(case, plan, res):
    l0 = plan["launches"][0]
    return "%-76s %-12s %-20s ranges %2d grid %s %-20s exact %d/%d  ratio %6.3f tile (%d, %d)" % (
        case["id"], plan["form"], l0["kernel"], l0["ranges"], l0["grid"], l0["reduce"] or "-", res["exact"], res["exact"], *res["normal"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fn_gemm_multi cases: one launch = a list of jobs, each job the sum of up to four products in ONE accumulator
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mj(M, N, segs, beta=0.0, bias=False, c=(0, None)):
    """segs = [(K, (a_off, lda or None), (b_off, ldb or None), 'fast' | 'checked' | 'mixed')]"""
    return dict(M=M, N=N, segs=segs, beta=beta, bias=bias, c0=c[0], ldc=c[1] if c[1] is not None else _r4(c[0] + N) + 4)


def _seg(K, path, a=(0, None), b=(0, None)):
    return (K, a, b, path)


MULTI_CASES = [
    # segments of nk = 1 .. 5 tiles on the four-deep ring (fast) and on the two-deep checked loop
    dict(id="m-nt-nk1-5-fast", lay=NT, jobs=[_mj(70, 50, [_seg(K, "fast")]) for K in (16, 32, 48, 64, 80)]),
    dict(id="m-nn-nk1-5-checked", lay=NN, jobs=[_mj(70, 50, [_seg(K, "checked")]) for K in (10, 20, 40, 50, 75)]),
    # K = 3 and 16 (the step's own output-layer gradients), row-contiguous operands
    dict(id="m-tn-K3-checked-K16-fast", lay=TN, jobs=[_mj(64, 128, [_seg(3, "checked")]), _mj(64, 128, [_seg(16, "fast")]), _mj(342, 16, [_seg(3, "checked", a=(0, 344))]),
                                                      _mj(342, 16, [_seg(16, "checked", a=(0, 344))])]),
    # a job that mixes fast and checked segments; four segments with beta = 1 and a bias; a one-tile job beside a six-tile one (the early return)
    dict(id="m-nt-four-segments-mixed-paths-beta1-bias-early-return", lay=NT,
         jobs=[_mj(130, 70, [_seg(32, "fast"), _seg(20, "checked"), _seg(64, "fast"), _seg(75, "checked")], beta=1.0, bias=True),
               _mj(7, 3, [_seg(33, "checked")], bias=True), _mj(64, 64, [_seg(16, "fast"), _seg(48, "fast")], beta=1.0)]),
    # ragged 130 x 70 tiles with row-contiguous operands: fast inside, checked on the edge tiles
    dict(id="m-tn-130x70-ragged-row-contiguous", lay=TN, jobs=[_mj(130, 70, [_seg(32, "mixed", a=(0, 132), b=(0, 72)), _seg(80, "mixed", a=(0, 132), b=(0, 72))], beta=1.0)]),
    dict(id="m-tt-130x70-ragged-A-row-contiguous", lay=TT, jobs=[_mj(130, 70, [_seg(48, "mixed", a=(0, 132))], bias=True), _mj(128, 70, [_seg(48, "fast")])]),
    dict(id="m-nn-130x70-ragged-B-row-contiguous", lay=NN, jobs=[_mj(130, 70, [_seg(32, "mixed", b=(0, 72))]), _mj(130, 64, [_seg(32, "fast")])]),
    # strided A, B and C views (aligned: fast; A one float off: checked)
    dict(id="m-nt-strided-views", lay=NT, jobs=[_mj(37, 70, [_seg(64, "fast", a=(4, 72), b=(8, 76))], beta=1.0, bias=True, c=(6, 84)),
                                                _mj(37, 70, [_seg(64, "checked", a=(1, 72), b=(0, 76))], c=(2, 80))]),
    # 12 jobs in one launch (GM_MAX_JOBS), 13 through the wrapper (12 + 1), in the layout the suite never ran
    dict(id="m-tt-12-jobs-one-launch", lay=TT, jobs=[_mj(20 + 9 * j, 70 - 5 * j, [_seg(16 + 4 * j, "mixed" if j == 8 else "checked")]) for j in range(12)]),
    dict(id="m-tt-13-jobs-two-launches", lay=TT, jobs=[_mj(64, 64, [_seg(16 * (1 + j % 3), "fast")], beta=float(j % 2)) for j in range(13)]),
]
MULTI_BY_ID = {c["id"]: c for c in MULTI_CASES}


def _seg_lds(lay, M, N, K, a, b):
    return (a[1] if a[1] is not None else (K if lay[0] else M)), (b[1] if b[1] is not None else (K if lay[1] else N))


def multi_case_plan(case, ptrs=None):
    """ptrs[j][i] = (A address, B address) of segment i of job j, default: the nominal offsets"""
    lay, jobs = case["lay"], []
    for jx, j in enumerate(case["jobs"]):
        segs = []
        for ix, (K, a, b, _) in enumerate(j["segs"]):
            lda, ldb = _seg_lds(lay, j["M"], j["N"], K, a, b)
            pA, pB = (4 * a[0], 4 * b[0]) if ptrs is None else ptrs[jx][ix]
            segs.append((K, lda, ldb, pA, pB))
        jobs.append(dict(M=j["M"], N=j["N"], segs=segs))
    return multi_plan(lay[0], lay[1], jobs)


def seg_path(loads):
    return "mixed" if loads["fast"] and loads["checked"] else "fast" if loads["fast"] else "checked"


def assert_multi_plan_matches_case(case, plan):
    for j, pj in zip(case["jobs"], plan["jobs"]):
        for (K, _, _, path), ps in zip(j["segs"], pj["segs"]):
            assert seg_path(ps["loads"]) == path and ps["nk"] == _cdiv(K, 16), (case["id"], K, ps)


def multi_problems(case, mode):
    """one problem per job; prob['segs'] = [(a [M][K], b [K][N])]"""
    key = (case["id"], mode)
    if key not in _PROBLEMS:
        gen = _gen(case["id"], mode)
        probs = []
        for jx, j in enumerate(case["jobs"]):
            M, N = j["M"], j["N"]
            pieces = [(_draw((M, K), mode, gen), _draw((K, N), mode, gen)) for K, _, _, _ in j["segs"]]
            C0, bias = _draw((M, N), mode, gen), (_draw((N,), mode, gen) if j["bias"] else None)
            chain = [(a, b, 0, a.shape[1]) for a, b in pieces]
            probs.append(make_problem("%s/job%d" % (case["id"], jx), mode, M, N, pieces, [chain], 1.0, j["beta"], bias, C0))
        _PROBLEMS[key] = probs
    return _PROBLEMS[key]


def multi_line(case, plan, res):
    segs = " ".join("[%s]" % ",".join("%s%d" % (seg_path(s["loads"])[0], s["nk"]) for s in j["segs"]) for j in plan["jobs"])
    return "%-76s %-24s grid %d idle %s segs %s exact %d/%d  ratio %6.3f job %d tile (%d, %d)" % (
        case["id"], "gemm_multi_kernel<%d,%d>" % case["lay"], plan["grid"], ",".join(str(j["idle"]) for j in plan["jobs"]), segs, res["exact"], res["exact"],
        *res["normal"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what the tables must reach: every kernel instance x load path x reduction the mirror can name
# ---------------------------------------------------------------------------------------------------------------------------------------------
def coverage_wanted():
    want = set()
    for kern in STAGED:
        for lay in (NT, NN, TT, TN):
            for path in ("fast", "checked"):
                if kern in (G3264, G6416) and lay != NT:
                    continue                                 # the dispatch sends only NT there
                if ("staged", lay, path) in UNREACHABLE:
                    continue
                want.add((kern, lay, path))
        want.add((kern, "any", "unsplit"))
    for kern in (G16, G128):                                 # the instances a split launch can reach
        want |= {(kern, "any", "slab_reduce4_kernel")}
    want.add((G16, "any", "slab_reduce_kernel"))
    for kern in TN_PF:
        want |= {(kern, g, r) for g, r in (("3d", None), ("3d", "slab_reduce_kernel"), ("1d", "slab_reduce_kernel"), ("1d", "slab_reduce4_kernel"))}
    want |= {(TNK, "3d", "slab_reduce4_kernel"), (TNK, "trips2", "slab_reduce4_kernel"), (TNK, "trips2", "slab_reduce_kernel")}
    for lay in (NT, NN, TT, TN):
        want |= {("gemm_multi_kernel", lay, "fast"), ("gemm_multi_kernel", lay, "checked")}
    want |= {("fn_gru_dwhh_f32", form, kern) for form in ("one-launch", "two-products") for kern in TN_PF if not (form == "two-products" and kern == TNL)}
    return want


def coverage_reached():
    got = set()
    for c in GEMM_CASES:
        p = case_plan(c)
        lay = (c["a_k"], c["b_k"])
        if p["family"] == "staged":
            got |= {(p["kernel"], lay, path) for path, n in p["loads"].items() if n}
            got.add((p["kernel"], "any", p["reduce"] or "unsplit"))
        else:
            got.add((p["kernel"], p["grid"], p["reduce"]))
            if p["reduce_trips"] > 1:
                got.add((p["kernel"], "trips%d" % p["reduce_trips"], p["reduce"]))
    for c in MULTI_CASES:
        for j in multi_case_plan(c)["jobs"]:
            for s in j["segs"]:
                got |= {("gemm_multi_kernel", c["lay"], path) for path, n in s["loads"].items() if n}
    for c in DWHH_CASES:
        p = dwhh_case_plan(c)
        got |= {("fn_gru_dwhh_f32", p["form"], l["kernel"]) for l in p["launches"]}
    return got
