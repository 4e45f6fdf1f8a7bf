"""Shared code of tests/test_reduce_reference.py (CPU) and tests/test_gpu_reduce.py (MI355X): the "glue" kernels of the training step - the
embedding gradient (csrc/embed.hip: fn_token_sort, fn_embed_grad_sorted, fn_embed_grad_f32, fn_time_sum_f32), the small reductions at the end of
csrc/gemm.hip (colsum, colsum_multi, sum, axpy, transpose) and the optimiser (csrc/optim.hip: sumsq, step_params, clip_adam) - against float64.
No GPU import: every driver takes the backend (`ops`: HipOps on the GPU, tests/fake_ops.FakeOps on the CPU) and the device as arguments.

Summation kernels (embed_grad, embed_grad_sorted, time_sum, colsum, colsum_multi, sum, sumsq) get two passes:
  "int"   operands are small integers stored as fp32 ([-8, 8]; sumsq {-1, 0, 1}).  Every partial sum stays far below 2**24, so fp32 addition is
          exact in ANY order and the result must equal the float64 reference bit for bit (check_exact; the sign of a zero is not compared).  A row
          that is missed, doubled or taken from the wrong place is a certain mismatch.  assert_int_exact asserts sum |terms| < 2**24 for every output.
  "randn" operands are standard normal.  For an output that is the sum of n fp32 terms   |got - ref64| <= (n + 2) 2**-24 sum |terms|   (check_sum;
          sum |terms| in float64): the order-independent first-order bound of recursive summation (n - 1 additions of relative error 2**-24 each),
          with room for the few other roundings a kernel has (the product of sumsq / the scale of sum / beta out of colsum / the final cast).
          Outputs with no term must be exactly 0.0.
Elementwise kernels: axpy |got - ref64| <= 2**-23 (|y| + |alpha x|) (two roundings, or one fused); transpose bit-exact.
step_params: each output within 2**-23 relative of the reference's formulas in Python floats; exact zeros where the formula gives zero.
clip_adam: three chained steps against clip_grad_norm_ + Adam in float64, per block of 1024 elements err = max |got - ref64| / max |ref64| over that
block, err <= F x max(e_ref, 2**-23), e_ref = the same quantity for FakeOps in fp32 on the same inputs, F = ADAM_F <= helpers.SCAN_F_CAP.

The hyper-parameters of the Adam reference are the values the C ABI carries: lr, beta1, beta2 and eps are `float` arguments of fn_step_params /
fn_clip_adam, so the float64 reference (and torch.optim.Adam in float64, which test_reduce_reference.py shows to be the same thing) runs with
float(np.float32(0.9)) etc.  With the decimal doubles instead, 1 - beta2 would differ by 1.3e-5 relative (1 - 0.999f = 0.99998712e-3) - a property
of the number format of the interface, not of the kernel, which no fp32 kernel behind this ABI could remove.
"""
import math
import zlib

import numpy as np
import torch

from helpers import SCAN_EPS, SCAN_F_CAP, relerr

U24 = 2.0 ** -24
SENTINEL = -123.25
INT_PASS, RANDN_PASS = "int", "randn"
PASSES = (INT_PASS, RANDN_PASS)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def operands(shape, kind, gen, lo=-8, hi=8):
    """fp32 CPU tensor: integers of [lo, hi] (the exact pass) or standard normal"""
    if kind == INT_PASS:
        return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()
    return torch.randn(tuple(shape), generator=gen)


def _np64(x):
    return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def assert_int_exact(cid, sabs):
    """the exactness condition of the integer pass: sum |terms| < 2**24 for every output element (then every partial sum in any order is an integer
    below 2**24 and fp32 addition never rounds)"""
    m = float(np.max(_np64(sabs))) if np.size(_np64(sabs)) else 0.0
    assert m < 2.0 ** 24, "%s: sum |terms| = %g is not below 2**24" % (cid, m)
    return m


def check_exact(cid, got, ref64):
    """got (fp32) equals the float64 reference bit for bit once both are fp32 (x + 0.0 first: the sign of a zero is not compared).  Returns 0.0"""
    g = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got)
    assert g.dtype == np.float32, g.dtype
    r64 = _np64(ref64)
    assert g.shape == r64.shape, (cid, g.shape, r64.shape)
    r = r64.astype(np.float32)
    assert np.array_equal(r.astype(np.float64), r64), "%s: the reference itself is not representable in fp32" % cid
    bad = (g + np.float32(0.0)).view(np.int32) != (r + np.float32(0.0)).view(np.int32)
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError("%s: integer pass not bit-exact in %d of %d outputs, first at %s: got %r, expected %r" % (
            cid, int(bad.sum()), bad.size, tuple(int(x) for x in i), float(g[i]), float(r[i])))
    return 0.0


def check_sum(cid, got, ref64, sabs, n):
    """|got - ref64| <= (n + 2) 2**-24 sabs for every output (n, sabs broadcast against the outputs); outputs with n == 0 exactly 0.0.
    Returns (worst error / bound, index of it).  NaN counts as inf."""
    g, r, s = _np64(got), _np64(ref64), np.broadcast_to(_np64(sabs), _np64(ref64).shape)
    nn = np.broadcast_to(np.asarray(n, np.float64), r.shape)
    assert g.shape == r.shape, (cid, g.shape, r.shape)
    empty = nn == 0
    if empty.any():
        assert (r[empty] == 0).all() and (s[empty] == 0).all(), cid
        nz = empty & ~(g == 0)
        if nz.any():
            i = np.unravel_index(int(np.argmax(nz)), nz.shape)
            raise AssertionError("%s: output %s has no term and must be exactly 0.0, got %r (%d such outputs)" % (cid, tuple(int(x) for x in i), float(g[i]), int(nz.sum())))
    bound = (nn + 2.0) * U24 * s
    err = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    w = float(ratio[i])
    assert w <= 1.0, "%s: |got - ref64| = %.3e is %.3g x the bound (n + 2) 2**-24 sum|terms| = %.3e at output %s (n = %d, got %r, ref %r); %d of %d outputs over the bound" % (
        cid, float(err[i]), w, float(bound[i]), tuple(int(x) for x in i), int(nn[i]), float(g[i]), float(r[i]), int((ratio > 1.0).sum()), ratio.size)
    return w, tuple(int(x) for x in i)


def check_pass(cid, kind, got, ref64, sabs, n):
    """the check of one pass: bit-exact (int) or within the summation bound (randn).  Returns (worst ratio, index)"""
    if kind == INT_PASS:
        assert_int_exact(cid, sabs)
        return check_exact(cid, got, ref64), ()
    return check_sum(cid, got, ref64, sabs, n)


def check_untouched(cid, buf, mask_written, what="output"):
    """every element of the sentinel-filled buffer outside the written view still holds the sentinel"""
    b = buf.detach().cpu().numpy()
    bad = (~mask_written) & (b != np.float32(SENTINEL))
    assert not bad.any(), "%s: %s written outside its view at %s" % (cid, what, tuple(int(x) for x in np.argwhere(bad)[0]))


def old_metric_accepts(got, ref, tol=2e-5):
    """what the one-by-one tests of test_gpu_parity.py ask: max |got - ref| < tol of the WHOLE tensor's maximum (close())"""
    return relerr(_np64(got), _np64(ref)) < tol


def line(kernel, cid, kind, worst, where=""):
    """one line of profiles/reduce_fp64_errors.txt"""
    res = "bit-exact" if kind == INT_PASS else "ratio %8.5f" % worst
    return "[reduce] %-13s %-46s %-6s %s%s" % (kernel, cid, kind, res, ("  at %s" % (where,)) if where != "" and where != () else "")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# embedding gradient: the sort image and the per-token sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
EG_BLK, EG_PIECE, EG_NT, EG_MAX_JOBS = 1024, 256, 384, 8          # csrc/embed.hip
SEG_COUNTS = (0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 512, 513)
SEG_TOKENS = tuple(3 + 11 * k for k in range(len(SEG_COUNTS)))    # token with SEG_COUNTS[k] positions
SEG_FILLER = 341
SEG_STRIDE = 997                                                  # coprime to 37 x 70: position of the i-th list entry = i x 997 mod rows
TOK_ABSENT, TOK_257, TOK_513 = SEG_TOKENS[0], SEG_TOKENS[10], SEG_TOKENS[12]
LASTCOL_TOKEN = 7


def token_sort_ints(rows, V):
    """fn_token_sort_ints restated: seg[V + 1] | pstart[V + 1] | 2 spare ints | order[rows]"""
    return 2 * (V + 1) + 2 + rows


def eg_tokens(case):
    """the token matrix idx [B][T] (int32 numpy) of a case, by construction; position r = tau B + b holds idx[b][tau]"""
    B, T, V, rows = case["B"], case["T"], case["V"], case["B"] * case["T"]
    pos = np.arange(rows, dtype=np.int64)
    if case["tokens"] == "segcounts":
        assert V > SEG_FILLER and rows >= 2 * EG_BLK + 1 and math.gcd(SEG_STRIDE, rows) == 1
        lst = np.concatenate([np.full(c, t) for c, t in zip(SEG_COUNTS, SEG_TOKENS)])
        lst = np.concatenate([lst, np.full(rows - lst.size, SEG_FILLER)])
        tok = np.empty(rows, np.int64)
        tok[(pos * SEG_STRIDE) % rows] = lst
    elif case["tokens"] == "mod":
        tok = (pos * 7 + pos // 5) % V
    elif case["tokens"] == "lastcol":
        tok = 1 + pos % 5
        tok[(T - 1) * B:] = LASTCOL_TOKEN                         # column T - 1 and nowhere else
    else:
        raise KeyError(case["tokens"])
    assert tok.min() >= 0 and tok.max() < V
    return np.ascontiguousarray(tok.reshape(T, B).T.astype(np.int32))


def eg_positions(idx):
    """token of position r = tau B + b"""
    return np.ascontiguousarray(idx.T).reshape(-1).astype(np.int64)


def sort_image_reference(idx, V):
    """(seg [V + 1], pstart [V + 1], order [rows]) of the stable counting sort of the positions by token"""
    tok = eg_positions(idx)
    cnt = np.bincount(tok, minlength=V)
    seg = np.concatenate([[0], np.cumsum(cnt)])
    pstart = np.concatenate([[0], np.cumsum((cnt + EG_PIECE - 1) // EG_PIECE)])
    return seg.astype(np.int64), pstart.astype(np.int64), np.argsort(tok, kind="stable").astype(np.int64)


def split_image(img, V, rows):
    img = np.asarray(img.detach().cpu().numpy() if torch.is_tensor(img) else img)
    assert img.size >= token_sort_ints(rows, V)
    return img[:V + 1], img[V + 1:2 * (V + 1)], img[2 * (V + 1) + 2:2 * (V + 1) + 2 + rows]


def check_sort_image(cid, img, idx, V):
    """the image fn_token_sort wrote against numpy: order = argsort(token of position, stable), seg / pstart = exclusive cumsums"""
    seg, pstart, order = split_image(img, V, idx.size)
    rseg, rpstart, rorder = sort_image_reference(idx, V)
    assert np.array_equal(seg, rseg), "%s: seg differs from the exclusive cumsum of the counts, first at token %d" % (cid, int(np.argmax(seg != rseg)))
    assert np.array_equal(pstart, rpstart), "%s: pstart differs from the exclusive cumsum of ceil(count / 256), first at token %d" % (cid, int(np.argmax(pstart != rpstart)))
    if not np.array_equal(order, rorder):
        i = int(np.argmax(order != rorder))
        raise AssertionError("%s: order[%d] = %d, the stable sort has %d there (%d entries differ)" % (cid, i, int(order[i]), int(rorder[i]), int((order != rorder).sum())))


def eg_row_tokens(idx, reverse, shift, start):
    """[T][B] int64: the input token of row p B + b of dgx_all - processing step p consumes idx[b][(reverse ? T-1-p : p) + shift], the start token
    where that column is < 0"""
    B, T = idx.shape
    out = np.empty((T, B), np.int64)
    for p in range(T):
        tau = (T - 1 - p if reverse else p) + shift
        out[p] = start if tau < 0 else idx[:, tau]
    return out


def eg_reference(dgx, rowtok, V):
    """(ref64 [V][N3], sum |terms| [V][N3], number of terms [V][1]) of out[v] = sum of the rows of dgx whose input token is v"""
    T, B, N3 = dgx.shape
    d, t = dgx.double().reshape(T * B, N3), torch.from_numpy(rowtok.reshape(-1))
    ref = torch.zeros(V, N3, dtype=torch.float64).index_add_(0, t, d)
    sabs = torch.zeros(V, N3, dtype=torch.float64).index_add_(0, t, d.abs())
    return ref.numpy(), sabs.numpy(), np.bincount(rowtok.reshape(-1), minlength=V).reshape(V, 1)


def _job(reverse=0, shift=0, start=0, transposed=False, view="dense", dgx=0):
    assert not (reverse and shift) and not (transposed and view != "dense")
    return dict(reverse=reverse, idx_shift=shift, start_token=start, transposed=transposed, view=view, dgx=dgx)


def _ec(cid, tokens, B, T, V, N3, jobs, n_dgx=1):
    return dict(id=cid, tokens=tokens, B=B, T=T, V=V, N3=N3, jobs=jobs, n_dgx=n_dgx)


def _seg_jobs():
    return [_job(), _job(reverse=1, view="ld"), _job(shift=-1, start=TOK_ABSENT, transposed=True), _job(shift=-1, start=TOK_257)]


EG_CASES = [
    # the segment counts around the 8-row batch, the 32-row trip and the 256-row piece, over three sorting blocks; N3 = 1540: a second column trip
    _ec("segcounts-B37-T70-V342-N3_1540", "segcounts", 37, 70, 342, 1540, _seg_jobs()),
    _ec("segcounts-B37-T70-V342-N3_4", "segcounts", 37, 70, 342, 4, _seg_jobs()),
    # eight jobs in one launch, B = 300: start pieces of 256 + 44 rows; N3 = 1536: exactly one column trip
    _ec("batch8-B300-T9-V342-N3_1536", "mod", 300, 9, 342, 1536, [
        _job(dgx=0), _job(reverse=1, transposed=True, dgx=1), _job(shift=-1, start=341, transposed=True, dgx=0), _job(shift=-1, start=7, dgx=1),
        _job(transposed=True, dgx=1), _job(reverse=1, dgx=0), _job(shift=-1, start=0, view="ld", dgx=1), _job(view="ld", dgx=0)], n_dgx=2),
    _ec("V1-B30-T11-N3_4", "mod", 30, 11, 1, 4, [_job(), _job(reverse=1, transposed=True), _job(shift=-1, start=0, view="ld")]),
    _ec("V2-B256-T5-N3_1536", "mod", 256, 5, 2, 1536, [_job(shift=-1, start=1), _job(transposed=True)]),
    _ec("V1024-B1-T300-N3_4", "mod", 1, 300, 1024, 4, [_job(shift=-1, start=1023, transposed=True), _job(reverse=1), _job(shift=-1, start=14)]),
    # token 7 only in the last column: under shift -1 no step consumes it - a piece made entirely of weight-0 rows, its table row exactly zero
    _ec("lastcol-B9-T13-V342-N3_1536", "lastcol", 9, 13, 342, 1536, [_job(shift=-1, start=2), _job(), _job(shift=-1, start=300, transposed=True)]),
]
EG_BY_ID = {c["id"]: c for c in EG_CASES}

_EG_CACHE = {}


def eg_inputs(case, kind):
    """dict(idx [B][T] int32 tensor, dgx [n_dgx] of [T][B][N3], refs [per job] = (ref64, sabs, n)), computed once per (case, pass)"""
    key = (case["id"], kind)
    if key not in _EG_CACHE:
        idx = eg_tokens(case)
        gen = _gen("eg", case["id"], kind)
        dgx = [operands((case["T"], case["B"], case["N3"]), kind, gen) for _ in range(case["n_dgx"])]
        refs = [eg_reference(dgx[j["dgx"]], eg_row_tokens(idx, j["reverse"], j["idx_shift"], j["start_token"]), case["V"]) for j in case["jobs"]]
        _EG_CACHE[key] = dict(idx=torch.from_numpy(idx), dgx=dgx, refs=refs)
    return _EG_CACHE[key]


def eg_buffer(case, job, device="cpu"):
    """(sentinel-filled buffer, the view the launch writes): transposed = [:N3, :V] of [N3 + 2][V + 10] (a table written in place into a wider
    matrix, dW_ih[:, :V]); 'dense' = the first V rows of [V + 2][N3]; 'ld' = [:V, :N3] of [V + 2][N3 + 8] (out_ld > N3)"""
    V, N3 = case["V"], case["N3"]
    if job["transposed"]:
        buf = torch.full((N3 + 2, V + 10), SENTINEL, device=device)
        return buf, buf[:N3, :V]
    buf = torch.full((V + 2, N3 + (8 if job["view"] == "ld" else 0)), SENTINEL, device=device)
    return buf, buf[:V, :N3]


def eg_table(case, job, buf):
    """the [V][N3] table of a job from its (CPU) buffer, after checking that nothing outside the view was written"""
    V, N3 = case["V"], case["N3"]
    buf = buf.detach().cpu()
    mask = np.zeros(tuple(buf.shape), bool)
    if job["transposed"]:
        mask[:N3, :V] = True
    else:
        mask[:V, :N3] = True
    check_untouched(case["id"], buf, mask, "the table")
    return (buf[:N3, :V].t() if job["transposed"] else buf[:V, :N3]).contiguous()


def run_embed_sorted(ops, case, kind, device="cpu"):
    """one fn_token_sort + ONE fn_embed_grad_sorted launch with all jobs of the case.  Returns (handle, [buffer per job] on the CPU)"""
    inp = eg_inputs(case, kind)
    handle = ops.token_sort(inp["idx"].to(device), case["V"])
    dgx = [d.to(device) for d in inp["dgx"]]
    bufs, jobs = [], []
    for j in case["jobs"]:
        buf, view = eg_buffer(case, j, device)
        bufs.append(buf)
        jobs.append(dict(dgx=dgx[j["dgx"]], out=view, transposed=j["transposed"], reverse=j["reverse"], idx_shift=j["idx_shift"], start_token=j["start_token"]))
    assert len(jobs) <= EG_MAX_JOBS
    ops.embed_grad_sorted(handle, jobs)
    return handle, [b.cpu() for b in bufs]


def run_embed_onecall(ops, case, kind, ji, device="cpu"):
    """fn_embed_grad_f32 (own sort, dense table) on the inputs of job ji.  Returns the [V + 2][N3] buffer on the CPU"""
    inp, j = eg_inputs(case, kind), case["jobs"][ji]
    buf = torch.full((case["V"] + 2, case["N3"]), SENTINEL, device=device)
    ops.embed_grad(inp["dgx"][j["dgx"]].to(device), inp["idx"].to(device), j["idx_shift"], j["start_token"], j["reverse"], case["V"], buf[:case["V"]])
    return buf.cpu()


def job_name(j):
    return "%s%s%s" % ("rev" if j["reverse"] else "shift-start%d" % j["start_token"] if j["idx_shift"] else "fwd",
                       "-T" if j["transposed"] else "", "-ld" if j["view"] == "ld" else "")


def check_embed_tables(case, kind, tables):
    """every job's [V][N3] table against float64.  Returns (worst ratio, job, (token, column))"""
    refs = eg_inputs(case, kind)["refs"]
    assert len(tables) == len(case["jobs"])
    worst = (0.0, 0, ())
    for ji, (j, tab, (ref, sabs, n)) in enumerate(zip(case["jobs"], tables, refs)):
        w, at = check_pass("%s job %d (%s) %s" % (case["id"], ji, job_name(j), kind), kind, tab, ref, sabs, n)
        if w >= worst[0]:
            worst = (w, ji, at)
    return worst


def check_embed_case(case, kind, bufs):
    return check_embed_tables(case, kind, [eg_table(case, j, b) for j, b in zip(case["jobs"], bufs)])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------------------------------
TS_GRID = 4096 * 256                                              # float4 columns one trip of time_sum_kernel's grid-stride loop covers
TIME_SUM_CASES = [dict(id="T%d-M%d" % (T, M), T=T, M=M) for M in (4, 3552) for T in (1, 2, 3, 4, 5, 8, 67)]
TIME_SUM_CASES.append(dict(id="T3-M4x(4096x256+3)-second-trip", T=3, M=4 * (TS_GRID + 3)))


def time_sum_inputs(case, kind):
    X = operands((case["T"], case["M"]), kind, _gen("ts", case["id"], kind))
    Xd = X.double()
    return X, Xd.sum(0).numpy(), Xd.abs().sum(0).numpy()


def run_time_sum(ops, case, kind, device="cpu"):
    X, ref, sabs = time_sum_inputs(case, kind)
    out = torch.full((case["M"] + 4,), SENTINEL, device=device)
    ops.time_sum(X.to(device), out[:case["M"]])
    out = out.cpu()
    assert bool((out[case["M"]:] == SENTINEL).all()), "%s: time_sum wrote past M" % case["id"]
    return check_pass("time_sum " + case["id"] + " " + kind, kind, out[:case["M"]], ref, sabs, case["T"])


def colsum_chunks(M):
    """csrc/gemm.hip colsum_chunks restated: (chunks, rows per chunk, chunks without a row)"""
    chunks = 256 if M >= 16384 else 64 if M >= 4096 else 16 if M >= 256 else 1
    rpc = (M + chunks - 1) // chunks
    return chunks, rpc, sum(1 for c in range(chunks) if c * rpc >= M)


COLSUM_M = (1, 3, 4, 5, 255, 256, 257, 4096, 4097, 16384, 16385)
COLSUM_N = (1, 255, 256, 257)
COLSUM_BETAS = (0.0, 1.0, 0.5)
COLSUM_CASES = [dict(id="M%d-N%d-ld%d" % (M, N, N + (3 if (i + k) % 2 else 0)), M=M, N=N, ld=N + (3 if (i + k) % 2 else 0))
                for i, M in enumerate(COLSUM_M) for k, N in enumerate(COLSUM_N)]


def colsum_reference(X, out0, beta):
    """(ref64, sum |terms|, n) of out = beta out0 + column sums of X; with beta = 0 out0 is not a term (and must not be read: it is NaN)"""
    Xd = X.double()
    ref, sabs, n = Xd.sum(0), Xd.abs().sum(0), X.shape[0]
    if beta != 0.0:
        ref, sabs, n = ref + beta * out0.double(), sabs + abs(beta) * out0.double().abs(), n + 1
    return ref.numpy(), sabs.numpy(), n


def colsum_inputs(case, kind):
    gen = _gen("cs", case["id"], kind)
    X = operands((case["M"], case["N"]), kind, gen)
    out0 = operands((case["N"],), kind, gen) * (2.0 if kind == INT_PASS else 1.0)       # (even integers: beta = 0.5 keeps them integers)
    return X, out0


def _strided(X, ld, device):
    """X as the [:, :N] view of a NaN-filled [M][ld] matrix on `device`"""
    if ld == X.shape[1]:
        return X.to(device)
    v = torch.full((X.shape[0], ld), float("nan"), device=device)[:, :X.shape[1]]
    v.copy_(X)
    return v


def run_colsum(ops, case, kind, device="cpu"):
    """the three betas on one X; beta = 0 on a NaN-filled out.  Returns (worst ratio, (beta, column))"""
    X, out0 = colsum_inputs(case, kind)
    Xv = _strided(X, case["ld"], device)
    worst = (0.0, ())
    for beta in COLSUM_BETAS:
        out = torch.full((case["N"],), float("nan"), device=device) if beta == 0.0 else out0.clone().to(device)
        ops.colsum(Xv, out, beta=beta)
        ref, sabs, n = colsum_reference(X, out0, beta)
        w, at = check_pass("colsum %s beta %g %s" % (case["id"], beta, kind), kind, out.cpu(), ref, sabs, n)
        if w >= worst[0]:
            worst = (w, (beta,) + tuple(at))
    return worst


CM_N = (1, 1536, 63, 342, 64, 65)                                 # the narrowest job beside the widest
CM_M = (1, 2, 3, 4, 5, 13, 16, 17, 29, 4096)
CM_JOBS = [(M, N) for M in CM_M for N in CM_N] + [(100, 1536), (257, 1), (33, 65), (48, 342), (31, 64)]       # 64 in one launch + 1: a second launch
CM_MAX_JOBS = 64


def cm_job(i):
    """(M, N, ld, beta) of job i: every third job through a view with ld > N, odd jobs accumulate (beta = 1), even ones overwrite a NaN out"""
    M, N = CM_JOBS[i]
    return M, N, N + (5 if i % 3 == 0 else 0), float(i % 2)


_CM_CACHE = {}


def cm_inputs(kind):
    if kind not in _CM_CACHE:
        res = []
        for i in range(len(CM_JOBS)):
            M, N, ld, beta = cm_job(i)
            gen = _gen("cm", i, kind)
            X, out0 = operands((M, N), kind, gen), operands((N,), kind, gen)
            res.append((X, out0, beta, colsum_reference(X, out0, beta)))
        _CM_CACHE[kind] = res
    return _CM_CACHE[kind]


def run_colsum_multi(ops, kind, lo, hi, device="cpu"):
    """jobs [lo, hi) of the table in ONE call of ops.colsum_multi.  Returns the list of CPU outputs"""
    inp = cm_inputs(kind)
    jobs = []
    for i in range(lo, hi):
        X, out0, beta, _ = inp[i]
        out = torch.full((X.shape[1],), float("nan"), device=device) if beta == 0.0 else out0.clone().to(device)
        jobs.append((_strided(X, cm_job(i)[2], device), out, beta))
    ops.colsum_multi(jobs)
    return [j[1].cpu() for j in jobs]


def check_colsum_multi(kind, lo, outs):
    """Returns (worst ratio, (job, column))"""
    inp = cm_inputs(kind)
    worst = (0.0, ())
    for k, out in enumerate(outs):
        i = lo + k
        ref, sabs, n = inp[i][3]
        w, at = check_pass("colsum_multi job %d (M %d N %d ld %d beta %g) %s" % ((i,) + cm_job(i) + (kind,)), kind, out, ref, sabs, n)
        if w >= worst[0]:
            worst = (w, (i,) + tuple(at))
    return worst


SUM_N = (1, 63, 64, 1023, 1024, 1025, 100003)
SUM_SCALE = 0.5


def run_sum(ops, n, kind, device="cpu"):
    x = operands((n,), kind, _gen("sum", n, kind))
    out = torch.full((3,), SENTINEL, device=device)
    ops.sum(x.to(device), out[1:2], SUM_SCALE)
    out = out.cpu()
    assert float(out[0]) == SENTINEL and float(out[2]) == SENTINEL, "sum n %d: a neighbour of the output slot was written" % n
    xd = x.double()
    return check_pass("sum n %d %s" % (n, kind), kind, out[1:2], (SUM_SCALE * xd.sum()).reshape(1).numpy(), (SUM_SCALE * xd.abs().sum()).reshape(1).numpy(), n)


SUMSQ_N = (1, 3, 4, 5, 7, 1023, 1048576, 4 * 1048576 + 3)


def run_sumsq(ops, n, kind, device="cpu"):
    g = operands((n,), kind, _gen("sumsq", n, kind), -1, 1)
    out = torch.full((3,), SENTINEL, device=device)
    ops.sumsq(g.to(device), out[1:2])
    out = out.cpu()
    assert float(out[0]) == SENTINEL and float(out[2]) == SENTINEL, "sumsq n %d: a neighbour of the output slot was written" % n
    ss = (g.double() ** 2).sum().reshape(1).numpy()
    return check_pass("sumsq n %d %s" % (n, kind), kind, out[1:2], ss, ss, n)


AXPY_N = (1, 255, 256, 2048 * 256 + 1)
AXPY_ALPHA = (0.0, -1.0, 0.25)


def check_axpy(cid, got, x, y0, alpha):
    """|got - ref64| <= 2**-23 (|y| + |alpha x|): the product rounded (2**-24 |alpha x|), then the sum (2**-24 |y + alpha x|) - or one rounding when
    fused.  Returns (worst ratio, index)"""
    ref = y0.double() + alpha * x.double()
    bound = 2.0 ** -23 * (y0.double().abs() + (alpha * x.double()).abs())
    err = (got.detach().cpu().double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    assert float(ratio[i]) <= 1.0, "%s: |got - ref64| = %.3e is %.3g x 2**-23 (|y| + |alpha x|) at element %d" % (cid, float(err[i]), float(ratio[i]), i)
    return float(ratio[i]), i


def run_axpy(ops, n, alpha, device="cpu"):
    gen = _gen("axpy", n, alpha)
    x, y0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    y = y0.clone().to(device)
    ops.axpy(alpha, x.to(device), y)
    return check_axpy("axpy n %d alpha %g" % (n, alpha), y.cpu(), x, y0, alpha)


TRANSPOSE_SHAPES = [(R, Cc) for R in (1, 31, 32, 33) for Cc in (1, 31, 32, 33)] + [(1000, 342)]


def run_transpose(ops, R, Cc, device="cpu"):
    """both leading dimensions padded (src NaN outside the view, dst sentinel-filled): bit-exact, nothing written outside dst[:C, :R]"""
    X = torch.randn(R, Cc, generator=_gen("tr", R, Cc))
    X[0, 0] = -0.0
    src = _strided(X, Cc + 3, device)
    dst = torch.full((Cc + 2, R + 5), SENTINEL, device=device)
    ops.transpose(src, dst[:Cc, :R])
    dst = dst.cpu()
    mask = np.zeros(tuple(dst.shape), bool)
    mask[:Cc, :R] = True
    check_untouched("transpose %dx%d" % (R, Cc), dst, mask, "dst")
    assert np.array_equal(dst[:Cc, :R].numpy().view(np.int32), X.t().contiguous().numpy().view(np.int32)), "transpose %dx%d: not bit-exact" % (R, Cc)
    return 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# step_params
# ---------------------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    """the value a `float` argument of the C ABI carries"""
    return float(np.float32(x))


SP_STEPS = (0, 999, 1000, 9999, 10000, 15000, 20000, 20001, 1999, 2000, 2 ** 31 + 5)
SP_T = (0, 1, 1000, 10 ** 6)
SP_BETA, SP_LR, SP_B1, SP_B2, SP_INV_BG = f32(0.2), f32(1e-3), f32(0.9), f32(0.999), 1.0 / 256
ADAM_EPS = f32(1e-8)


def step_params_reference(step, t_counter, advance, supervised, beta=SP_BETA, lr=SP_LR, b1=SP_B1, b2=SP_B2, inv_bg=SP_INV_BG):
    """the eight outputs in Python floats (float64) and the counters afterwards.

    beta0 is the reference trainer's annealing as it is written: 0 below step 1000, then min((step - 10000) / 10000 x beta, beta) - which is
    NEGATIVE on steps 1000..9999 (-0.9 beta at step 1000, rising to 0 at step 10000).  That is the reference's behaviour, and the port reproduces
    it; it is not clamped at zero here either.  out[6] is the Fader sibling's min(step / 2000 x 1e-4, 1e-4), out[7] the constant beta / Bg."""
    t = t_counter + (1 if advance else 0)
    beta0 = 0.0 if step < 1000 else min((step - 10000) / 10000 * beta, beta)
    tt = max(t, 1)
    out = [beta0 * inv_bg, 0.0 if supervised else beta0 * inv_bg, inv_bg if supervised else 0.0, lr / (1.0 - b1 ** tt), 1.0 / math.sqrt(1.0 - b2 ** tt),
           beta0, min(step / 2000 * 1e-4, 1e-4), beta * inv_bg]
    return out, ([step + 1, t] if advance else [step, t_counter])


def check_step_params(cid, got, counters, step, t_counter, advance, supervised):
    """got [8] fp32, counters [2] int64 after the launch.  Each output within 2**-23 relative of the float64 formula (one rounding of a double;
    out[7] is a product of two fp32 values formed in fp32); exactly 0.0 where the formula gives zero.  Returns the worst error / (2**-23 |ref|)"""
    ref, cnt = step_params_reference(step, t_counter, advance, supervised)
    assert [int(c) for c in counters] == cnt, "%s: counters %s, expected %s" % (cid, [int(c) for c in counters], cnt)
    worst = 0.0
    for k in range(8):
        g, r = float(got[k]), ref[k]
        if r == 0.0:
            assert g == 0.0, "%s: out[%d] = %r where the formula gives exactly zero" % (cid, k, g)
            continue
        ratio = abs(g - r) / (SCAN_EPS * abs(r))
        assert ratio <= 1.0, "%s: out[%d] = %r, float64 formula %r: %.3g x 2**-23 relative" % (cid, k, g, r, ratio)
        worst = max(worst, ratio)
    return worst


def run_step_params(ops, step, t_counter, advance, supervised, device="cpu"):
    cnt = torch.tensor([step, t_counter], dtype=torch.int64, device=device)
    out = torch.full((10,), SENTINEL, device=device)
    ops.step_params(cnt, SP_BETA, SP_LR, SP_B1, SP_B2, bool(supervised), SP_INV_BG, bool(advance), out[:8])
    out = out.cpu()
    assert float(out[8]) == SENTINEL and float(out[9]) == SENTINEL
    return check_step_params("step_params step %d t %d advance %d supervised %d" % (step, t_counter, advance, supervised), out[:8], cnt.cpu().tolist(),
                             step, t_counter, advance, supervised)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# clip_grad_norm_ + Adam, three chained steps
# ---------------------------------------------------------------------------------------------------------------------------------------------
ADAM_BLOCK = 1024
ADAM_STEPS = 3
ADAM_MAX_NORM = 1.0
ADAM_F = 4                      # smallest power of two above the measured worst ratio, 2.09 (profiles/reduce_fp64_errors.txt); never above SCAN_F_CAP
ADAM_GRID = 4096 * 256          # elements one trip of clip_adam_kernel's grid-stride loop covers


def _ac(cid, n, grad, t_first, moments, zeros=False):
    """grad: clipped (randn x 3: norm >> max_norm) | unclipped (norm = 0.5 < max_norm: coef exactly 1) | zero;  t_first: Adam's t of the first step;
    moments: zero | rand;  zeros: every 13th element has g = m = v = 0 in all three steps - its p must come back bit-unchanged"""
    return dict(id=cid, n=n, grad=grad, t_first=t_first, moments=moments, zeros=zeros)


ADAM_CASES = [
    _ac("n1-clipped-t1-zero-moments", 1, "clipped", 1, "zero"),
    _ac("n255-unclipped-t1-zero-moments", 255, "unclipped", 1, "zero"),
    _ac("n257-clipped-t100000", 257, "clipped", 10 ** 5, "rand"),
    _ac("n100003-clipped-t1-zero-moments-zero-elements", 100003, "clipped", 1, "zero", zeros=True),
    _ac("n100003-unclipped-t100000-zero-elements", 100003, "unclipped", 10 ** 5, "rand", zeros=True),
    _ac("n100003-zero-gradient-t100000", 100003, "zero", 10 ** 5, "rand"),
    _ac("n4096x256+5-clipped-t1-zero-moments", ADAM_GRID + 5, "clipped", 1, "zero"),
    _ac("n4096x256+5-unclipped-t100000-zero-elements", ADAM_GRID + 5, "unclipped", 10 ** 5, "rand", zeros=True),
]
ADAM_BY_ID = {c["id"]: c for c in ADAM_CASES}


def adam_inputs(case):
    """p (randn x 0.01: parameters of the size of ten Adam steps, so that an error in the update is visible against the block maximum of p), the
    three gradients, m, v - fp32 CPU tensors"""
    n, gen = case["n"], _gen("adam", case["id"])
    p = torch.randn(n, generator=gen) * 0.01
    if case["grad"] == "clipped":
        gs = [torch.randn(n, generator=gen) * 3 for _ in range(ADAM_STEPS)]
        if n < 16:                                                # too few elements for the norm to be large by itself
            gs = [g.sign() * (g.abs() + 3.0) for g in gs]
    elif case["grad"] == "unclipped":
        gs = []
        for _ in range(ADAM_STEPS):
            g = torch.randn(n, generator=gen).abs() + 0.5
            gs.append(g * (0.5 / float(g.double().norm())) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0))
    else:
        gs = [torch.zeros(n) for _ in range(ADAM_STEPS)]
    if case["moments"] == "rand":
        m, v = (torch.rand(n, generator=gen) - 0.5) * 0.2, torch.rand(n, generator=gen) * 0.01 + 1e-4
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    if case["zeros"]:
        for t in gs + [m, v]:
            t[::13] = 0.0
    return dict(p=p, gs=gs, m=m, v=v)


def adam_reference_f64(p, gs, m, v, t_first, max_norm=ADAM_MAX_NORM, lr=SP_LR, b1=SP_B1, b2=SP_B2, eps=ADAM_EPS, t_offset=0, clamp=True):
    """[(p, m, v) after each step] in float64 on the fp32 inputs: clip_grad_norm_(max_norm) then Adam.  t_offset / clamp plant faults (Adam's t off by
    one; the clip coefficient not clamped to 1)"""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    res = []
    for s, g in enumerate(gs):
        g = g.double()
        coef = max_norm / (float(g.norm()) + 1e-6)
        if clamp:
            coef = min(coef, 1.0)
        g = g * coef
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        t = t_first + s + t_offset
        p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
        res.append((p.clone(), m.clone(), v.clone()))
    return res


def adam_torch_f64(p, gs, m, v, t_first, max_norm=ADAM_MAX_NORM, lr=SP_LR, b1=SP_B1, b2=SP_B2, eps=ADAM_EPS):
    """the same with torch.nn.utils.clip_grad_norm_ and torch.optim.Adam in float64, its state preloaded with (t_first - 1, m, v)"""
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[w] = dict(step=torch.tensor(float(t_first - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    res = []
    for g in gs:
        w.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
        st = opt.state[w]
        res.append((w.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return res


def run_adam(ops, case, device="cpu", inputs=None):
    """three steps chained on the device: sumsq -> step_params (advance) -> clip_adam, hyper = step_params' out[3:5].  Returns [(p, m, v) per step]
    on the CPU"""
    inp = adam_inputs(case) if inputs is None else inputs
    p, m, v = inp["p"].clone().to(device), inp["m"].clone().to(device), inp["v"].clone().to(device)
    cnt = torch.tensor([20000, case["t_first"] - 1], dtype=torch.int64, device=device)
    ss, sp = torch.zeros(1, device=device), torch.zeros(8, device=device)
    res = []
    for g in inp["gs"]:
        g = g.to(device)
        ops.sumsq(g, ss)
        ops.step_params(cnt, SP_BETA, SP_LR, SP_B1, SP_B2, False, SP_INV_BG, True, sp)
        ops.clip_adam(p, g, m, v, ss, ADAM_MAX_NORM, sp[3:5], SP_B1, SP_B2, ADAM_EPS)
        res.append((p.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
    assert cnt.cpu().tolist() == [20000 + ADAM_STEPS, case["t_first"] - 1 + ADAM_STEPS]
    return res


def block_errors(got, ref64):
    """(err, den) per block of 1024 elements: den = max |ref64| over the block, err = max |got - ref64| / den; where the reference block is identically
    zero err is 0 if `got` is exactly zero there and inf otherwise; NaN -> inf"""
    g, r = _np64(got), _np64(ref64)
    assert g.shape == r.shape and g.ndim == 1
    pad = -g.size % ADAM_BLOCK
    num = np.pad(np.abs(g - r), (0, pad)).reshape(-1, ADAM_BLOCK)
    num = np.where(np.isnan(num), np.inf, num).max(1)
    den = np.pad(np.abs(r), (0, pad)).reshape(-1, ADAM_BLOCK).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num == 0, 0.0, np.inf)), den


_ADAM_CACHE = {}


def adam_references(case):
    """dict(inputs, ref64 [(p, m, v) per step], e_ref [{p, m, v} per step]): e_ref = block_errors of FakeOps in fp32 chained the same way"""
    if case["id"] not in _ADAM_CACHE:
        from fake_ops import FakeOps
        inp = adam_inputs(case)
        ref = adam_reference_f64(inp["p"], inp["gs"], inp["m"], inp["v"], case["t_first"])
        fake = run_adam(FakeOps(), case, "cpu", inp)
        assert all(x.dtype == torch.float32 for st in fake for x in st)
        e_ref = [{k: block_errors(f, r)[0] for k, f, r in zip("pmv", fs, rs)} for fs, rs in zip(fake, ref)]
        _ADAM_CACHE[case["id"]] = dict(inputs=inp, ref64=ref, fake32=fake, e_ref=e_ref)
    return _ADAM_CACHE[case["id"]]


def check_adam(case, got, F=ADAM_F):
    """got = [(p, m, v) per step].  In EVERY block of 1024 elements of p, m and v after EVERY step  err <= F x max(e_ref, 2**-23); elements with
    g = m = v = 0 keep their p bit for bit.  Returns (worst ratio, step, quantity, block)"""
    assert F <= SCAN_F_CAP
    ref = adam_references(case)
    assert len(got) == ADAM_STEPS
    worst, bad = (-1.0, 0, "", 0), []
    for s, (gs, rs) in enumerate(zip(got, ref["ref64"])):
        for k, g, r in zip("pmv", gs, rs):
            assert g.dtype == torch.float32
            e, den = block_errors(g, r)
            ratio = e / np.maximum(ref["e_ref"][s][k], SCAN_EPS)
            b = int(np.argmax(ratio))
            if ratio[b] > worst[0]:
                worst = (float(ratio[b]), s + 1, k, b)
            if not ratio[b] <= F:
                bad.append("%s step %d %s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in block %d (elements %d..), block max of the reference %.3e; %d of %d blocks over F = %g" % (
                    case["id"], s + 1, k, e[b], ratio[b], ref["e_ref"][s][k][b], b, b * ADAM_BLOCK, den[b], int((~(ratio <= F)).sum()), ratio.size, F))
    assert not bad, "\n".join(bad)
    if case["zeros"]:
        p0 = ref["inputs"]["p"]
        for s, gs in enumerate(got):
            same = gs[0][::13].numpy().view(np.int32) == p0[::13].numpy().view(np.int32)
            assert same.all(), "%s step %d: p of element %d (g = m = v = 0) changed" % (case["id"], s + 1, 13 * int(np.argmax(~same)))
    return worst


def adam_line(case, worst):
    return "[reduce] %-13s %-46s ratio %6.3f  step %d %s block %d  (F = %d)" % ("clip_adam", case["id"], worst[0], worst[1], worst[2], worst[3], ADAM_F)
