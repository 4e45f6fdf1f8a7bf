"""CPU side of tests/test_gpu_images.py: the host statements of the operand-image layouts (tests/helpers_images.py) agree with a second, scalar
statement written from the offset formulas; the bf16 triple split is exact on exactly the domain the helper states (every mantissa at the lowest
exponent, at 2**0 and at the highest); the case tables have the properties their ids claim; the checkers accept the statements and reject planted
faults.  No GPU, no package import."""
import numpy as np
import pytest

import helpers_images as hi
from helpers_images import (BLOCK, DOMAIN_SEEDS, LEAD, PACK_CASES, PACK_GRID, REFUSALS, SENTINEL, TAIL, WI_CASES, WI_MAX_JOBS, X3_LIMIT, X3_LIMIT_BITS, X3_MIN,
                            X3_MIN_BITS, check_dense, check_frag, check_frag3, decode3, frag3_image, frag_floats, frag_image, image_pieces, in_allocation,
                            in_domain, pack_items, pack_source, source_values, split3, unfrag, wi_expected, wi_items, wi_need, wi_shape, wi_source, wi_wraps)

SHAPES = ((1, 32), (16, 32), (17, 64), (33, 96))


def _frag_by_loops(src, rows, K):
    """the fp32 image from the offset of one element: row tile, 32-k chunk, 16-k half, then lane = 16 * (k-quad) + row-in-tile, four floats per lane"""
    rows16, NC = (rows + 15) // 16 * 16, K // 32
    out = np.zeros(rows16 * K, np.uint32)
    for row in range(rows):
        for k in range(K):
            lane = 16 * ((k % 16) // 4) + row % 16
            out[((((row // 16) * NC + k // 32) * 2 + (k // 16) % 2) * 64 + lane) * 4 + k % 4] = src[row, k]
    return out


def _frag3_by_loops(src, rows, K):
    """the triple image from the offset of one bf16: row tile, 32-k block, piece, then lane = 16 * (8-k group) + row-in-tile, eight halves per lane"""
    rows16, nb = (rows + 15) // 16 * 16, K // 32
    out = np.zeros(3 * rows16 * K, np.uint16)
    for row in range(rows):
        for k in range(K):
            for p, v in enumerate(split3(src[row:row + 1, k])):
                lane = 16 * ((k % 32) // 8) + row % 16
                out[((((row // 16) * nb + k // 32) * 3 + p) * 64 + lane) * 8 + k % 8] = int(v.view(np.uint32)[0]) >> 16
    return out


@pytest.mark.parametrize("rows,K", SHAPES)
def test_the_two_statements_of_each_layout_agree(rows, K):
    bits = source_values("two-statements-%dx%d" % (rows, K), rows * K, "bits").reshape(rows, K)
    img = frag_image(bits, rows, K)
    assert img.dtype == np.uint32 and img.shape == (frag_floats(rows, K),)
    assert np.array_equal(img, _frag_by_loops(bits, rows, K))
    assert np.array_equal(unfrag(img, rows, K)[:rows], bits) and not unfrag(img, rows, K)[rows:].any()
    dom = source_values("two-statements-%dx%d" % (rows, K), rows * K, "domain").reshape(rows, K).view(np.float32)
    img3 = frag3_image(dom, rows, K)
    assert img3.dtype == np.uint16 and img3.size * 2 == frag_floats(rows, K) * 3 // 2 * 4
    assert np.array_equal(img3, _frag3_by_loops(dom, rows, K))
    # the even k of a pair sits in the low half of the dword (little endian: the lower address)
    dw = img3.view(np.uint32)
    assert np.array_equal(dw & 0xFFFF, img3[0::2]) and np.array_equal(dw >> 16, img3[1::2])
    assert np.array_equal(decode3(img3, rows, K)[:rows], dom.astype(np.float64))


def _sweep(exp_bits, sign):
    """(x, exact?, pieces) of every mantissa at one biased exponent"""
    bits = (np.uint32(sign) << np.uint32(31)) | (np.uint32(exp_bits) << np.uint32(23)) | np.arange(2 ** 23, dtype=np.uint32)
    x = bits.view(np.float32)
    h, m, l = split3(x)
    with np.errstate(all="ignore"):
        s = (h.astype(np.float64) + m.astype(np.float64)) + l.astype(np.float64)
    return bits, s == x.astype(np.float64), (h, m, l)


@pytest.mark.parametrize("sign", (0, 1))
def test_split3_is_exact_on_every_mantissa_at_the_ends_and_the_middle_of_the_domain(sign):
    assert X3_MIN == np.uint32(X3_MIN_BITS).view(np.float32) and X3_LIMIT == float(np.uint32(X3_LIMIT_BITS).view(np.float32))
    for e in (X3_MIN_BITS >> 23, 127, 254):
        bits, exact, pieces = _sweep(e, sign)
        dom = in_domain(bits)
        assert dom.all() == (e != 254)
        assert exact[dom].all(), "exponent %d: 0x%08x is not the sum of its pieces" % (e, int(bits[dom][~exact[dom]][0]))
        for p in pieces:
            assert not (p.view(np.uint32)[dom] & 0xFFFF).any()
        if e == 254:                                             # the upper limit is tight: the first value behind it already has an infinite hi
            assert int(np.flatnonzero(~dom)[0]) == (X3_LIMIT_BITS & 0x7FFFFF)
            assert np.isinf(pieces[0][~dom]).all() and np.isfinite(pieces[0][dom]).all()


def test_the_lower_limit_of_the_split_is_tight():
    """one binade below X3_MIN the split loses a bit: the docstring's example, and how many values of that binade"""
    x = np.array([2.0 ** -111 * (1 + 2.0 ** -23)], np.float32)
    h, m, l = split3(x)
    assert float(h[0]) == 2.0 ** -111 and float(m[0]) == 2.0 ** -133 and l.view(np.uint32)[0] == 0x80000000
    assert float(h[0]) + float(m[0]) + float(l[0]) == float(x[0]) + 2.0 ** -134
    bits, exact, _ = _sweep((X3_MIN_BITS >> 23) - 1, 0)
    assert not in_domain(bits).any() and not exact.all() and exact.any()
    print("\nbinade below X3_MIN: %d of %d values are not the sum of their pieces" % (int((~exact).sum()), exact.size))
    # zero is in the domain, and so are both seeded limits
    assert in_domain(np.array([0, 0x80000000, X3_MIN_BITS, X3_LIMIT_BITS - 1], np.uint32)).all()
    assert not in_domain(np.array([1, X3_MIN_BITS - 1, X3_LIMIT_BITS, 0x7F800000, 0x7FC00000], np.uint32)).any()


def test_the_seeded_domain_values_are_what_their_comment_says():
    assert in_domain(DOMAIN_SEEDS).all()
    x = DOMAIN_SEEDS.view(np.float32)
    h, m, l = split3(x)
    hb, mb, lb = (p.view(np.uint32) for p in (h, m, l))
    assert (x.astype(np.float64) == h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)).all()
    carry = (hb >> 23) != (DOMAIN_SEEDS >> 23)
    assert carry.sum() >= 3 and ((DOMAIN_SEEDS[carry] & 0x7FFFFF) >= 0x7F8000).all()
    assert ((DOMAIN_SEEDS & 0xFFFF) == 0x8000).sum() >= 3                                     # ties of the first level
    r1 = x - h
    assert ((r1.view(np.uint32) & 0xFFFF) == 0x8000).sum() >= 2                               # ties of the second level
    nz = (DOMAIN_SEEDS & 0x7FFFFFFF) != 0
    assert (nz & ((mb << 1) == 0)).sum() >= 2 and (nz & ((mb << 1) != 0) & ((lb << 1) == 0)).sum() >= 2 and (((mb << 1) != 0) & ((lb << 1) != 0)).sum() >= 4
    for pass_ in ("bits", "domain"):                                                          # the seeds reach even the smallest source
        v = source_values("seeded", 32, pass_)
        assert set(v.tolist()) >= set((hi.BITS_SEEDS if pass_ == "bits" else DOMAIN_SEEDS)[:16].tolist())
    v = source_values("spread", 1 << 16, "domain")
    assert in_domain(v).all()
    e = ((v >> 23) & 0xFF)[(v & 0x7FFFFFFF) != 0]
    assert e.min() == X3_MIN_BITS >> 23 and e.max() == 254 and len(np.unique(e)) == 254 - (X3_MIN_BITS >> 23) + 1
    b = source_values("spread", 1 << 16, "bits")
    f = b.view(np.float32)
    assert np.isnan(f).any() and np.isinf(f).any() and (b == 0x80000000).any() and (((b >> 23) & 0xFF) == 0).sum() > 2


def test_the_case_tables_have_the_properties_their_ids_claim():
    ids = [c["id"] for c in PACK_CASES]
    assert len(set(ids)) == len(ids)
    small = [c for c in PACK_CASES if not c["id"].startswith("wrap")]
    assert 12 <= len(small) <= 16
    assert {c["rows"] for c in small} == {1, 15, 16, 17, 33, 342} and {c["K"] for c in small} == {32, 64, 96, 512}
    for c in PACK_CASES:
        rows, K, ld, off = c["rows"], c["K"], c["ld"], c["off"]
        assert K % 32 == 0 and ld >= K and c["id"].endswith(c["mode"])
        # frag_pack_kernel takes 16-byte loads when the source address is 16-byte aligned and ld % 4 == 0 (allocations are 16-byte aligned)
        assert c["vector_loads"] == (off % 4 == 0 and ld % 4 == 0)
        assert {"dense": ld == K and not off, "pad4": ld == K + 4 and not off, "pad1": ld == K + 1 and not off, "off4": off == 1 and ld % 4 == 0}[c["mode"]]
        alloc, view = pack_source(c, "bits")
        assert view.shape == (rows, K) and view.base is not None and (rows == 1 or view.strides[0] == 4 * ld)
        assert (view.__array_interface__["data"][0] - alloc.__array_interface__["data"][0]) == 4 * off
        for packer in c["packers"]:
            assert (pack_items(c, packer) > PACK_GRID * BLOCK) == c["id"].startswith("wrap"), (c["id"], packer)
    for mode in ("dense", "pad4", "pad1", "off4"):                                            # every load mode pads rows; both load paths see whole tiles too
        assert any(c["rows"] % 16 for c in small if c["mode"] == mode)
    assert {c["vector_loads"] for c in small if c["rows"] % 16 == 0} == {True, False}
    assert any(c["id"].startswith("wrap") and "frag" in c["packers"] for c in PACK_CASES) and any(c["id"].startswith("wrap") and "frag3" in c["packers"] for c in PACK_CASES)
    assert max(c["rows"] * c["ld"] for c in PACK_CASES if "frag" in c["packers"]) == 1040 * 2048

    jobs = WI_CASES["limit-56-jobs"]
    assert len(jobs) == WI_MAX_JOBS and {j["kind"] for j in jobs} == set(range(6))
    assert all(j["ld"] > j["C"] and 0 <= j["c0"] <= j["ld"] - j["C"] for js in WI_CASES.values() for j in js)
    for kind in range(6):
        assert any(j["ld"] % 4 for j in jobs if j["kind"] == kind) and any((j["ld"] % 4 or j["c0"] % 4) for j in jobs if j["kind"] == kind)
    k0 = [j for j in jobs if j["kind"] == 0]
    assert any(j["R"] % 32 and j["C"] % 32 and wi_wraps(j) for j in k0) and any(j["R"] % 32 and j["C"] % 32 and not wi_wraps(j) for j in k0)
    assert sum(j["dst_off"] for j in k0) >= 1 and not any(j["dst_off"] for j in jobs if j["kind"] != 0)
    for kinds, rows, cols in (((1, 3), {342, 17, 1536}, {32, 96, 512}), ((2, 4), {32, 96, 512}, {17, 342, 1536})):
        for kind in kinds:
            assert {(j["R"], j["C"]) for j in jobs if j["kind"] == kind} == {(r, c) for r in rows for c in cols}
            assert all(wi_shape(j)[1] % 32 == 0 for j in jobs if j["kind"] == kind) and any(wi_shape(j)[0] % 16 for j in jobs if j["kind"] == kind)
    assert all(j["R"] % 2 and j["C"] % 2 for j in jobs if j["kind"] == 5)
    stride = WI_CASES["grid-stride"]
    assert [j["kind"] for j in stride] == list(range(6)) and all(wi_wraps(j) for j in stride)
    assert all(wi_items(j) > 128 * (1 if j["kind"] == 0 else 256) for j in stride)
    for kind in range(1, 6):                                                                  # ... and the big launch has loops that do not wrap
        assert any(not wi_wraps(j) for j in jobs if j["kind"] == kind)
    assert max(j["R"] * j["ld"] for js in WI_CASES.values() for j in js) <= 1040 * 2048

    rid = [r["id"] for r in REFUSALS]
    assert len(set(rid)) == len(rid)
    by = {r["id"]: r for r in REFUSALS}
    assert by["wi-0-jobs"]["n_jobs"] == 0 and len(by["wi-57-jobs"]["jobs"]) == WI_MAX_JOBS + 1
    assert by["wi-0-jobs"]["code"] == by["wi-57-jobs"]["code"] == hi.FN_E_COUNT
    for r in REFUSALS:
        assert r["code"] in (hi.FN_E_NULL, hi.FN_E_SHAPE, hi.FN_E_ALIGN, hi.FN_E_COUNT)
        if r["fn"] == "wi" and r["code"] == hi.FN_E_ALIGN:
            assert r["jobs"][-1][4] == 1 and r["jobs"][-1][0] in (1, 2, 3, 4, 5)
        if r["fn"] != "wi" and r["code"] == hi.FN_E_ALIGN:
            assert r["dst_off"] == 1
    assert {r["jobs"][-1][0] for r in REFUSALS if r["fn"] == "wi" and r["code"] == hi.FN_E_ALIGN} == {1, 2, 3, 4, 5}
    assert {r["code"] for r in REFUSALS if r["fn"] == "frag"} == {r["code"] for r in REFUSALS if r["fn"] == "frag3"} == {hi.FN_E_NULL, hi.FN_E_SHAPE, hi.FN_E_ALIGN}


def _pack_images(case):
    _, vb = pack_source(case, "bits")
    _, vd = pack_source(case, "domain")
    return vb, vd


@pytest.mark.parametrize("case", [c for c in PACK_CASES if c["rows"] <= 342], ids=lambda c: c["id"])
def test_the_checkers_accept_the_statements(case):
    rows, K = case["rows"], case["K"]
    vb, vd = _pack_images(case)
    check_frag(case["id"], in_allocation(frag_image(vb, rows, K)), LEAD, vb, rows, K)
    check_frag3(case["id"], in_allocation(frag3_image(vd.view(np.float32), rows, K).view(np.uint32), LEAD + 1), LEAD + 1, vd, rows, K)


def test_the_checkers_accept_the_weight_image_statements():
    for cid, jobs in WI_CASES.items():
        for j, job in enumerate(jobs):
            if job["R"] * job["C"] > 342 * 512:
                continue
            _, view = wi_source(cid, j, job)
            want = wi_expected(job, view)
            assert want.size == wi_need(job)
            buf, name = in_allocation(want, LEAD + job["dst_off"]), "%s/%d" % (cid, j)
            if job["kind"] == 0:
                check_dense(name, buf, LEAD + job["dst_off"], view.T)
            elif job["kind"] == 5:
                check_dense(name, buf, LEAD, view)
            else:
                m = view if job["kind"] in (1, 3) else view.T
                (check_frag if job["kind"] < 3 else check_frag3)(name, buf, LEAD, m, *wi_shape(job))


def _trunc_image(x, rows, K):
    """an exact split with TRUNCATED pieces: the sum is the source, the bits are not the rounded split's"""
    pad = np.zeros(((rows + 15) // 16 * 16, K), np.float32)
    pad[:rows] = x
    cut = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = cut(pad)
    m = cut(pad - h)
    l = cut(pad - h - m)
    return hi._triple_to_image(np.stack([(p.view(np.uint32) >> 16).astype(np.uint16) for p in (h, m, l)]), K)


def test_the_checkers_reject_planted_faults():
    rows, K, cid = 17, 64, "planted"
    bits = source_values(cid, rows * K, "bits").reshape(rows, K)
    dom = source_values(cid, rows * K, "domain").reshape(rows, K)
    x = dom.view(np.float32)
    good = frag_image(bits, rows, K)
    good3 = frag3_image(x, rows, K)
    check_frag(cid, in_allocation(good), LEAD, bits, rows, K)
    check_frag3(cid, in_allocation(good3.view(np.uint32)), LEAD, dom, rows, K)

    def bad_frag(img, match):
        with pytest.raises(AssertionError, match=match):
            check_frag(cid, in_allocation(img), LEAD, bits, rows, K)

    def bad_frag3(img, match, bitwise=True):
        with pytest.raises(AssertionError, match=match):
            check_frag3(cid, in_allocation(np.ascontiguousarray(img).view(np.uint32)), LEAD, dom, rows, K, bitwise=bitwise)

    # two lanes swapped
    f = good.reshape(-1, 64, 4).copy()
    f[1, [3, 4]] = f[1, [4, 3]]
    bad_frag(f.reshape(-1), r"planted: \(row 3, k 16\)")
    t = good3.reshape(-1, 3, 64, 8).copy()
    t[0, 1, [5, 21]] = t[0, 1, [21, 5]]
    bad_frag3(t.reshape(-1), r"planted: \(row 5, k 0, piece mid\)")
    # the two k halves swapped: the 16-k halves of the fp32 image, the even / odd k of every dword of the triple image
    f = good.reshape(-1, 2, 256)[:, ::-1]
    bad_frag(np.ascontiguousarray(f).reshape(-1), r"planted: \(row 0, k 0\)")
    t = good3.reshape(-1, 2)[:, ::-1]
    bad_frag3(np.ascontiguousarray(t).reshape(-1), r"planted: \(row 0, k 0, piece hi\)")
    # a non-zero padding row
    f = unfrag(good, rows, K)
    f[rows + 2, 5] = 0x80000000                                   # even -0.0
    bad_frag(frag_image(f, f.shape[0], K), "planted: padding row 19, k 5")
    p = image_pieces(good3, rows, K)
    p[2, 31, 63] = 1
    bad_frag3(hi._triple_to_image(p, K), "planted: padding row 31, k 63, piece lo")
    # pieces in the order mid / hi / lo
    p = image_pieces(good3, rows, K)
    bad_frag3(hi._triple_to_image(p[[1, 0, 2]], K), r"planted: \(row 0, k 0, piece hi\)")
    # truncated pieces in place of rounded ones: still an exact split, so only the bit comparison sees it
    t = _trunc_image(x, rows, K)
    assert np.array_equal(decode3(t, rows, K)[:rows], x.astype(np.float64)) and not np.array_equal(t, good3)
    bad_frag3(t, r"planted: \(row \d+, k \d+, piece (hi|mid|lo)\)")
    check_frag3(cid, in_allocation(t.view(np.uint32)), LEAD, dom, rows, K, bitwise=False)      # (a promise of the sum alone is kept)
    # a dropped lo piece: with and without the bit comparison
    p = image_pieces(good3, rows, K)
    p[2] = 0
    bad_frag3(hi._triple_to_image(p, K), r"planted: \(row \d+, k \d+, piece lo\)")
    bad_frag3(hi._triple_to_image(p, K), r"planted: \(row \d+, k \d+\) hi \+ mid \+ lo", bitwise=False)
    # one element written past the image, one in front of it, an allocation of another length
    for img, chk, src in ((good, check_frag, bits), (good3.view(np.uint32), check_frag3, dom)):
        buf = in_allocation(img)
        buf[LEAD + img.size] = 0
        with pytest.raises(AssertionError, match="planted: word %d relative to the image" % img.size):
            chk(cid, buf, LEAD, src, rows, K)
        buf = in_allocation(img)
        buf[LEAD - 1] ^= 1
        with pytest.raises(AssertionError, match="planted: word -1 relative to the image"):
            chk(cid, buf, LEAD, src, rows, K)
        with pytest.raises(AssertionError, match="planted: the destination allocation"):
            chk(cid, in_allocation(img)[:-1], LEAD, src, rows, K)
    # the dense kinds: a transposed pair of elements, a write behind the matrix
    d = bits.copy()
    d[3, 4], d[4, 3] = bits[4, 3], bits[3, 4]
    with pytest.raises(AssertionError, match=r"planted: dst\[3\]\[4\]"):
        check_dense(cid, in_allocation(d), LEAD, bits)
    buf = in_allocation(bits)
    buf[-1] = 0
    with pytest.raises(AssertionError, match="planted: word"):
        check_dense(cid, buf, LEAD, bits)
    assert buf[0] == SENTINEL and TAIL > 64
