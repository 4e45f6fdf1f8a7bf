"""Shared code of tests/test_images_reference.py (CPU) and tests/test_gpu_images.py (MI355X): the operand images fn_frag_pack, fn_frag3_pack and
fn_weight_images (csrc/gru.hip: frag_pack_kernel, frag3_pack_kernel / frag3_item, weight_images_kernel) write, stated on the host in numpy and
compared bit for bit.  Nothing here imports the package, and nothing here has a tolerance: fp32 images are compared as uint32, triple images as
uint16, and the one arithmetic statement (decode3 == src, in float64) is exact.

  frag_image(src, rows, K)     the fp32 fragment-major image (csrc/gru_layout.h, frag_off): rows padded to a multiple of 16 with +0.0, the matrix seen as
                               [row tile][16 rows][K/32 chunks][2 halves][4 k-quads][4 k] and stored as [row tile][chunk][half][k-quad][row][4 k]: the 64
                               lanes (k-quad, row) of a wavefront each own 16 contiguous bytes, 1 KB per (tile, chunk, half)
  split3(x)                    hi / mid / lo of float32 values (csrc/mma_core.h, fn_rn16: the bit pattern plus half a bf16 ulp, truncated - ties away
                               from zero), the remainder of each level formed in float32; lo is the top half of the last remainder
  frag3_image(src, rows, K)    the bf16 triple image (the comment above frag3_item): [row tile 16][k block 32][piece hi / mid / lo][64 lanes][8 bf16] as
                               uint16; lane 16 g + i holds row 16 t + i and k = 32 b + 8 g .. + 7 in k order, i.e. the even k in the low half of a dword
  decode3(image, rows, K)      float64 hi + mid + lo per element, [rows16][K]

The exact domain of split3 (X3_MIN, X3_LIMIT; tests/test_images_reference.py sweeps every mantissa at both ends and in the middle).  Let x be a
finite float32 with exponent e (2**e <= |x| < 2**(e+1); e = -126 for subnormals), so x is a multiple of u = ulp(x) = 2**(e-23) with |x| / u < 2**24.
  hi   = x rounded to 8 significant bits (a carry makes it 2**(e+1)): a multiple of 2**(e-7), |x - hi| <= 2**(e-8)
  r1   = x - hi is a multiple of u with |r1| / u <= 2**15: 16 significant bits, exact in float32 (subnormal results included: float32 subtraction of
         two multiples of u whose difference is below 2**24 u never rounds)
  mid  = r1 rounded to 8 significant bits.  With e1 <= e - 8 the exponent of r1, |r1 - mid| <= 2**(e1-8) <= 2**(e-16)
  r2   = r1 - mid is a multiple of u with |r2| / u <= 2**7: 8 significant bits
  lo   = the top 16 bits of r2.  A bf16 has float32's exponent range and 7 fraction bits, subnormals down to 2**-126 x 2**-7 = 2**-133: every multiple
         of u with 8 significant bits is a bf16 when u >= 2**-133, that is e - 23 >= -133, |x| >= 2**-110 (or x == 0).  Below that, r2 can have a bit
         under 2**-133 which the truncation drops (x = 2**-111 (1 + 2**-23): hi = 2**-111, r1 = 2**-134, mid = 2**-133 by the tie rule,
         r2 = -2**-134, lo = -0.0 and hi + mid + lo = x + 2**-134).
  upper limit: the bit pattern of hi must not reach the infinity's: |x| < 2**128 (1 - 2**-9), bits below 0x7f7f8000 (csrc/mma_core.h says the same).
So hi + mid + lo == x exactly for x == 0 and X3_MIN <= |x| < X3_LIMIT, and the lower limit holds for all of [2**-110, ..) only because no
arithmetic on the way flushes subnormals: the float32 remainders of values near 2**-110 are subnormal.

  PACK_CASES / WI_CASES / REFUSALS    the case tables (each id says what the case is for); pack_source / wi_source build a case's source allocation
  check_frag / check_frag3 / check_dense    the checkers: first differing (row, k, piece) and the case id; padding rows +0.0; the documented length;
                               every word of the destination allocation outside the image still the sentinel
"""
import zlib

import numpy as np

SENTINEL = 0x7FA5C3E1               # a NaN payload no packer produces from the padding (+0.0) and no case draws on purpose
LEAD, TAIL = 4, 67                  # sentinel words in front of (16-byte aligned image; LEAD + 1: 4 bytes off) and behind every destination view
X3_MIN = 2.0 ** -110                # smallest |x| != 0 of the exact domain of split3 ...
X3_MIN_BITS = 0x08800000
X3_LIMIT = 2.0 ** 128 * (1 - 2.0 ** -9)     # ... and its (excluded) upper limit: the first float32 whose hi is the infinity
X3_LIMIT_BITS = 0x7F7F8000
FN_OK, FN_E_NULL, FN_E_SHAPE, FN_E_ALIGN, FN_E_COUNT = 0, -1, -2, -3, -5      # include/fadernets.h
WI_MAX_JOBS = 56
WI_KINDS = ("transpose", "frag", "frag_t", "frag3", "frag3_t", "copy")        # kinds 0..5 of fn_weight_images, as HipOps.weight_images names them
PACK_GRID, WI_GRID, BLOCK = 2048, 128, 256                                    # block caps of the single-matrix launches / blocks per job, threads per block


def frag_floats(rows, K):
    """fn_frag_floats: floats of the fp32 image of a [rows][K] matrix (a triple image has 3/2 of it)"""
    return (rows + 15) // 16 * 16 * K


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.uint32, np.int32), a.dtype
    return a.view(np.uint32)


def _padded(src, rows, K):
    """[rows16][K] uint32: the bits of src with +0.0 rows behind it"""
    assert K % 32 == 0 and rows >= 1
    u = _u32(src).reshape(rows, K)
    pad = np.zeros(((rows + 15) // 16 * 16, K), np.uint32)
    pad[:rows] = u
    return pad


def frag_image(src, rows, K):
    """the fp32 fragment-major image of src [rows][K] as uint32 bit patterns, frag_floats(rows, K) words"""
    pad = _padded(src, rows, K)
    v = pad.reshape(-1, 16, K // 32, 2, 4, 4)                    # [row tile][row][chunk][half][k-quad][k]
    return np.ascontiguousarray(v.transpose(0, 2, 3, 4, 1, 5)).reshape(-1)


def unfrag(image, rows, K):
    """an fp32 image (32-bit words) read back as the padded matrix [rows16][K] uint32"""
    rows16 = (rows + 15) // 16 * 16
    where = frag_image(np.arange(rows16 * K, dtype=np.uint32), rows16, K)      # image position -> row * K + k
    back = np.empty(rows16 * K, np.uint32)
    back[where] = _u32(image).reshape(-1)
    return back.reshape(rows16, K)


def split3(x):
    """(hi, mid, lo) float32 arrays, each with zero low 16 bits"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rn16 = lambda v: ((v.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(all="ignore"):
        hi = rn16(x)
        r1 = x - hi
        mid = rn16(r1)
        r2 = r1 - mid
    lo = (r2.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return hi, mid, lo


def _triple_to_image(pieces, K):
    """[3][rows16][K] uint16 pieces -> the image order [row tile][k block][piece][g][i][8 k]"""
    p = np.asarray(pieces).reshape(3, -1, 16, K // 32, 4, 8)     # [piece][row tile][i][k block][g][k]
    return np.ascontiguousarray(p.transpose(1, 3, 0, 4, 2, 5)).reshape(-1)


def frag3_image(src, rows, K):
    """the bf16 triple image of src [rows][K] (float32) as uint16, 3 * frag_floats(rows, K) halves = 3/2 * frag_floats(rows, K) floats"""
    pad = _padded(src, rows, K).view(np.float32)
    top = np.stack([(p.view(np.uint32) >> np.uint32(16)).astype(np.uint16) for p in split3(pad)])
    return _triple_to_image(top, K)


def image_pieces(image, rows, K):
    """a triple image (uint16) back as [3][rows16][K] uint16"""
    rows16 = (rows + 15) // 16 * 16
    v = np.asarray(image, dtype=np.uint16).reshape(rows16 // 16, K // 32, 3, 4, 16, 8)     # [row tile][k block][piece][g][i][k]
    return np.ascontiguousarray(v.transpose(2, 0, 4, 1, 3, 5)).reshape(3, rows16, K)


def decode3(image, rows, K):
    """float64 hi + mid + lo of every element of a triple image, [rows16][K]"""
    p = (image_pieces(image, rows, K).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (p[0] + p[1]) + p[2]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# source values
# ---------------------------------------------------------------------------------------------------------------------------------------------
BITS_SEEDS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                       0x00400000, 0x3F800000, 0x7F7FFFFF, 0xFF7FFFFF, SENTINEL ^ 1], np.uint32)
# the exact domain's corners (the float32 values, as bit patterns): both limits and their negatives, -0.0 / 0.0, hi roundings that carry into the exponent
# (mantissa 0x7f8000 and above), exact ties of the first level (low half 0x8000) and of the second (1 + 2**-9 + 2**-17: r1 = 2**-9 (1 + 2**-8)), values with
# mid == 0 (bf16 values: lo == 0 too), with lo == 0 and mid != 0 (1 + 2**-9), with all three pieces, and the same at the lowest exponent of the domain
DOMAIN_SEEDS = np.array([X3_MIN_BITS, 0x88800000, X3_LIMIT_BITS - 1, 0xFF7F7FFF, 0x80000000, 0x00000000, 0x3FFF8000, 0xBFFFFFFF, 0x3F7F8000, 0x3F808000,
                         0xC0018000, 0x3F804040, 0xBF804040, 0x3FC00000, 0xC1200000, 0x3F804000, 0x3F812345, 0x08FFFFFF, 0x08808000, 0x08804040,
                         0x7EFFFFFF, 0x7F7F0000, 0x7F000001, 0x08800001], np.uint32)


def _rng(cid):
    return np.random.RandomState(zlib.crc32(cid.encode()) & 0x7FFFFFFF)


def source_values(cid, n, pass_):
    """n seeded uint32 bit patterns of float32 values.  "bits": arbitrary patterns - NaN payloads, infinities, -0.0, subnormals - with BITS_SEEDS at
    positions spread over the array; "domain": values of the exact domain of split3, exponents uniform over the WHOLE domain, DOMAIN_SEEDS likewise"""
    rng = _rng(cid + "/" + pass_)
    if pass_ == "bits":
        v = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        seeds = BITS_SEEDS
    else:
        assert pass_ == "domain"
        e = rng.randint(X3_MIN_BITS >> 23, 0xFF, size=n).astype(np.uint32)
        v = (rng.randint(0, 2, size=n).astype(np.uint32) << np.uint32(31)) | (e << np.uint32(23)) | rng.randint(0, 2 ** 23, size=n).astype(np.uint32)
        over = (v & np.uint32(0x7FFFFFFF)) >= X3_LIMIT_BITS
        v[over] -= np.uint32(0x8000)                              # (mantissa 0x7f8000.. at the top exponent: back inside)
        seeds = DOMAIN_SEEDS
    k = min(n, len(seeds))
    v[(np.arange(k) * (n // k)) if n >= 2 * k else np.arange(k)] = seeds[:k]
    return v


def in_domain(bits):
    a = np.asarray(bits, np.uint32) & np.uint32(0x7FFFFFFF)
    return (a == 0) | ((a >= X3_MIN_BITS) & (a < X3_LIMIT_BITS))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _pack_case(rows, K, mode, packers=("frag", "frag3"), tag=""):
    """mode: "dense" ld = K, "pad4" ld = K + 4 (both: 16-byte loads in frag_pack_kernel), "pad1" ld = K + 1 (element-wise loads), "off4" the view starts
    4 bytes behind a 16-byte boundary with ld = K + 4 (ld % 4 == 0: element-wise loads because of the address alone)"""
    ld = {"dense": K, "pad4": K + 4, "pad1": K + 1, "off4": K + 4}[mode]
    return dict(id="%s%dx%d-%s" % (tag, rows, K, mode), rows=rows, K=K, ld=ld, off=int(mode == "off4"), mode=mode, packers=packers,
                vector_loads=mode in ("dense", "pad4"))


# rows {1, 15, 16, 17, 33, 342} x K {32, 64, 96, 512}, thinned: every rows and every K, each load mode at row counts on both sides of a tile edge;
# 17 x 64 in all four modes
PACK_CASES = [_pack_case(r, K, m) for r, K, m in (
    (1, 32, "dense"), (1, 512, "pad1"), (15, 64, "pad4"), (15, 96, "off4"), (16, 32, "pad1"), (16, 512, "dense"), (17, 64, "dense"), (17, 64, "pad4"),
    (17, 64, "pad1"), (17, 64, "off4"), (17, 96, "pad1"), (33, 96, "off4"), (33, 512, "pad4"), (342, 32, "off4"), (342, 64, "pad1"), (342, 512, "dense"))]
# the grid-stride loops wrap (more items than 2048 blocks x 256 threads): 1040 x 2048 has 1040 * 512 16-byte items for frag_pack_kernel but only
# 1040 * 256 eight-k items for frag3_pack_kernel, which needs more than 2048 x 2048 values to wrap: 2064 x 2048 (one row tile over) for that packer
PACK_CASES += [_pack_case(1040, 2048, "dense", packers=("frag",), tag="wrap-"),_pack_case(2064, 2048, "dense", packers=("frag3",), tag="wrap3-")]


def pack_items(case, packer):
    """work items of the packer's grid-stride loop"""
    return (case["rows"] + 15) // 16 * 16 * (case["K"] // (4 if packer == "frag" else 8))


def pack_source(case, pass_):
    """(alloc, view): the uint32 source allocation of a PACK_CASES entry and its [rows][K] view (leading dimension ld, `off` words behind the start)"""
    rows, K, ld, off = case["rows"], case["K"], case["ld"], case["off"]
    alloc = source_values(case["id"], off + rows * ld + 3, "bits")          # what lies between the rows is arbitrary bits in either pass
    view = alloc[off: off + rows * ld].reshape(rows, ld)[:, :K]
    view[...] = source_values(case["id"], rows * K, pass_).reshape(rows, K)
    return alloc, view


def _wi_job(j, kind, R, C, dst_off=0):
    """job j of a launch: src the columns c0 .. c0 + C of an [R][ld] allocation, ld = C + pad with pad cycling over 1, 4, 3, 8, 5, 2, 12, 7"""
    pad = (1, 4, 3, 8, 5, 2, 12, 7)[j % 8]
    return dict(kind=kind, R=R, C=C, ld=C + pad, c0=pad // 2, dst_off=dst_off)


def wi_shape(job):
    """(rows, K) of the matrix whose image a job of kind 1..4 writes"""
    return (job["R"], job["C"]) if job["kind"] in (1, 3) else (job["C"], job["R"])


def wi_need(job):
    """floats of a job's destination"""
    if job["kind"] in (0, 5):
        return job["R"] * job["C"]
    return frag_floats(*wi_shape(job)) * (3 if job["kind"] >= 3 else 2) // 2


def wi_items(job):
    """iterations of the job's grid-stride loop summed over its 128 blocks: 32 x 32 tiles (kind 0), elements (5), 16-byte items (1, 2), 8-k items (3, 4)"""
    if job["kind"] == 0:
        return ((job["R"] + 31) // 32) * ((job["C"] + 31) // 32)
    if job["kind"] == 5:
        return job["R"] * job["C"]
    rows, K = wi_shape(job)
    return (rows + 15) // 16 * 16 * (K // (4 if job["kind"] < 3 else 8))


def wi_wraps(job):
    return wi_items(job) > WI_GRID * (1 if job["kind"] == 0 else BLOCK)


def _wi_limit_jobs():
    shapes = [(0, R, C) for R, C in ((342, 1536), (37, 70), (1, 1), (1, 45), (45, 1), (33, 31), (32, 32), (64, 96), (31, 33), (353, 417))]
    shapes += [(k, R, C) for k in (1, 3) for R in (342, 17, 1536) for C in (32, 96, 512)]
    shapes += [(k, R, C) for k in (2, 4) for R in (32, 96, 512) for C in (17, 342, 1536)]
    shapes += [(5, R, C) for R, C in ((1, 1), (3, 5), (17, 33), (255, 41), (37, 71), (129, 257), (5, 1023), (1, 7), (63, 65), (341, 39))]
    return [_wi_job(j, k, R, C, dst_off=int(k == 0 and (R, C) in ((37, 70), (31, 33)))) for j, (k, R, C) in enumerate(shapes)]


WI_CASES = {
    # exactly 56 jobs, all six kinds: kind 0 with R, C no multiples of 32, more than 128 tiles, degenerate rows / columns and two destinations 4 bytes off
    # alignment; kinds 1 / 3 rows {342, 17, 1536} x cols {32, 96, 512}; kinds 2 / 4 rows {32, 96, 512} x cols {17, 342, 1536}; kind 5 odd R and C
    "limit-56-jobs": _wi_limit_jobs(),
    # one job per kind, each with more items than 128 blocks x 256 threads (kind 0: more than 128 tiles): every branch's loop wraps
    "grid-stride": [_wi_job(j, k, R, C) for j, (k, R, C) in enumerate(((0, 353, 417), (1, 342, 512), (2, 512, 342), (3, 1536, 512), (4, 512, 1536), (5, 257, 129)))],
}


def wi_source(cid, j, job):
    """(alloc [R][ld], view [R][C]) uint32 of job j of launch cid: arbitrary bits for the fp32 kinds, the exact domain inside the view for the triple kinds"""
    R, C, ld, c0 = job["R"], job["C"], job["ld"], job["c0"]
    name = "%s/%d" % (cid, j)
    alloc = source_values(name, R * ld, "bits").reshape(R, ld)
    view = alloc[:, c0: c0 + C]
    if job["kind"] in (3, 4):
        view[...] = source_values(name, R * C, "domain").reshape(R, C)
    return alloc, view


def wi_expected(job, view):
    """the destination of a job as the numpy statement has it: uint32 words"""
    k = job["kind"]
    if k == 0:
        return np.ascontiguousarray(view.T).reshape(-1)
    if k == 5:
        return np.ascontiguousarray(view).reshape(-1)
    rows, K = wi_shape(job)
    m = view if k in (1, 3) else np.ascontiguousarray(view.T)
    return frag_image(m, rows, K) if k < 3 else frag3_image(m.view(np.float32), rows, K).view(np.uint32)


def _refusal(rid, fn, code, **kw):
    """fn "wi": jobs = [(kind, rows, cols, ld, dst_off)] (valid buffers are built from them), then the overrides n_jobs, null = "jobs" / (j, "src" | "dst");
    fn "frag" / "frag3": rows, K, ld, dst_off, null = "src" | "dst" """
    return dict(id=rid, fn=fn, code=code, **kw)


_OK_JOB = (1, 17, 32, 36, 0)
REFUSALS = [
    _refusal("wi-0-jobs", "wi", FN_E_COUNT, jobs=[_OK_JOB], n_jobs=0),
    _refusal("wi-57-jobs", "wi", FN_E_COUNT, jobs=[_OK_JOB] * 57),
    _refusal("wi-jobs-null", "wi", FN_E_NULL, jobs=[_OK_JOB], null="jobs"),
    _refusal("wi-src-null", "wi", FN_E_NULL, jobs=[_OK_JOB], null=(0, "src")),
    _refusal("wi-dst-null-second-job", "wi", FN_E_NULL, jobs=[_OK_JOB, (0, 5, 7, 9, 0)], null=(1, "dst")),
    _refusal("wi-kind-minus-1", "wi", FN_E_SHAPE, jobs=[(-1, 32, 32, 32, 0)]),
    _refusal("wi-kind-6", "wi", FN_E_SHAPE, jobs=[_OK_JOB, (6, 32, 32, 32, 0)]),
    _refusal("wi-kind1-cols-48", "wi", FN_E_SHAPE, jobs=[(1, 32, 48, 48, 0)]),
    _refusal("wi-kind3-cols-33", "wi", FN_E_SHAPE, jobs=[(3, 32, 33, 36, 0)]),
    _refusal("wi-kind2-rows-48", "wi", FN_E_SHAPE, jobs=[(2, 48, 32, 32, 0)]),
    _refusal("wi-kind4-rows-31", "wi", FN_E_SHAPE, jobs=[(4, 31, 32, 32, 0)]),
    _refusal("wi-ld-below-cols", "wi", FN_E_SHAPE, jobs=[_OK_JOB, (5, 9, 7, 6, 0)]),
    _refusal("wi-rows-0", "wi", FN_E_SHAPE, jobs=[(0, 0, 7, 7, 0)]),
] + [_refusal("wi-kind%d-dst-4-bytes-off" % k, "wi", FN_E_ALIGN, jobs=[(0, 5, 7, 9, 1), (k, 32, 32, 33, 1)]) for k in (1, 2, 3, 4, 5)] + [
    r for fn in ("frag", "frag3") for r in (
        _refusal(fn + "-K-48", fn, FN_E_SHAPE, rows=17, K=48, ld=48, dst_off=0),
        _refusal(fn + "-ld-below-K", fn, FN_E_SHAPE, rows=17, K=32, ld=31, dst_off=0),
        _refusal(fn + "-rows-0", fn, FN_E_SHAPE, rows=0, K=32, ld=32, dst_off=0),
        _refusal(fn + "-src-null", fn, FN_E_NULL, rows=17, K=32, ld=32, dst_off=0, null="src"),
        _refusal(fn + "-dst-null", fn, FN_E_NULL, rows=17, K=32, ld=32, dst_off=0, null="dst"),
        _refusal(fn + "-dst-4-bytes-off", fn, FN_E_ALIGN, rows=17, K=32, ld=32, dst_off=1))]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checkers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _first(mask):
    return int(np.flatnonzero(np.asarray(mask).reshape(-1))[0])


def _outside(cid, buf, lead, n):
    """buf: the whole destination allocation (uint32), the image buf[lead : lead + n]: the allocation is lead + n + TAIL words, all others the sentinel"""
    buf = _u32(buf).reshape(-1)
    assert len(buf) == lead + n + TAIL, "%s: the destination allocation has %d words, the case needs %d + %d + %d" % (cid, len(buf), lead, n, TAIL)
    out = np.concatenate([buf[:lead], buf[lead + n:]])
    bad = out != np.uint32(SENTINEL)
    if bad.any():
        p = _first(bad)
        p = p - lead if p < lead else p - lead + n
        raise AssertionError("%s: word %d relative to the image (%d words long) was written: 0x%08x" % (cid, p, n, int(buf[lead + p])))
    return buf[lead: lead + n]


def check_dense(cid, buf, lead, want, what="dst"):
    """kinds 0 and 5: the destination is the dense 2-D uint32 array `want`"""
    want = _u32(want)
    got = _outside(cid, buf, lead, want.size).reshape(want.shape)
    bad = got != want
    if bad.any():
        r, c = divmod(_first(bad), want.shape[1])
        raise AssertionError("%s: %s[%d][%d] is 0x%08x, expected 0x%08x (%d of %d words differ)" % (cid, what, r, c, int(got[r, c]), int(want[r, c]), int(bad.sum()), bad.size))


def check_frag(cid, buf, lead, src, rows, K):
    """the fp32 image of src [rows][K] (any 32-bit view): exact length, sentinels outside, +0.0 padding rows, every element's bits in its place"""
    n = frag_floats(rows, K)
    got = _outside(cid, buf, lead, n)
    back = unfrag(got, rows, K)
    if back[rows:].any():
        r, k = divmod(_first(back[rows:] != 0), K)
        raise AssertionError("%s: padding row %d, k %d is 0x%08x, not +0.0" % (cid, rows + r, k, int(back[rows + r, k])))
    want = _u32(src).reshape(rows, K)
    bad = back[:rows] != want
    if bad.any():
        r, k = divmod(_first(bad), K)
        raise AssertionError("%s: (row %d, k %d) is 0x%08x, expected 0x%08x (%d of %d elements differ)" % (cid, r, k, int(back[r, k]), int(want[r, k]), int(bad.sum()), bad.size))
    assert np.array_equal(got, frag_image(src, rows, K)), cid


def check_frag3(cid, buf, lead, src, rows, K, bitwise=True):
    """the triple image of src [rows][K] (float32 bits, inside the exact domain): exact length, sentinels outside, padding rows zero in all three pieces,
    (bitwise) every piece of every element the bits of split3, and hi + mid + lo == src exactly in float64.  bitwise=False: the pieces may be any exact
    split (an image whose producer promises the sum only)"""
    n = frag_floats(rows, K) * 3 // 2
    got = _outside(cid, buf, lead, n).view(np.uint16)
    rows16 = frag_floats(rows, K) // K
    pieces = image_pieces(got, rows, K)
    names = ("hi", "mid", "lo")
    if pieces[:, rows:].any():
        p, rest = divmod(_first(pieces[:, rows:] != 0), (rows16 - rows) * K)
        r, k = divmod(rest, K)
        raise AssertionError("%s: padding row %d, k %d, piece %s is 0x%04x, not +0.0" % (cid, rows + r, k, names[p], int(pieces[p, rows + r, k])))
    srcf = _u32(src).reshape(rows, K).view(np.float32)
    assert in_domain(srcf.view(np.uint32)).all(), "%s: the source leaves the exact domain of the split" % cid
    if bitwise:
        want = image_pieces(frag3_image(srcf, rows, K), rows, K)
        bad = pieces != want
        if bad.any():
            p, rest = divmod(_first(bad), rows16 * K)
            r, k = divmod(rest, K)
            raise AssertionError("%s: (row %d, k %d, piece %s) is 0x%04x, expected 0x%04x (%d of %d halves differ)"
                                 % (cid, r, k, names[p], int(pieces[p, r, k]), int(want[p, r, k]), int(bad.sum()), bad.size))
    dec = decode3(got, rows, K)[:rows]
    bad = dec != srcf.astype(np.float64)
    if bad.any():
        r, k = divmod(_first(bad), K)
        raise AssertionError("%s: (row %d, k %d) hi + mid + lo = %r, the source is %r (pieces %s)"
                             % (cid, r, k, float(dec[r, k]), float(srcf[r, k]), ["0x%04x" % int(pieces[p, r, k]) for p in range(3)]))


def in_allocation(image, lead=LEAD):
    """an image (uint32 words) inside a sentinel-filled destination allocation, as the GPU tests build them"""
    image = _u32(image).reshape(-1)
    buf = np.full(lead + len(image) + TAIL, SENTINEL, np.uint32)
    buf[lead: lead + len(image)] = image
    return buf
