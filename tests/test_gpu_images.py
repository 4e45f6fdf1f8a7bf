"""The operand-image kernels of csrc/gru.hip - frag_pack_kernel (fn_frag_pack), frag3_pack_kernel / frag3_item (fn_frag3_pack) and weight_images_kernel
(fn_weight_images, kinds 0..5) - bit for bit against the host statements of the layouts (tests/helpers_images.py; tests/test_images_reference.py shows on
the CPU that the statements agree with a second one, where the triple split is exact, what the case tables reach and that planted faults are rejected).

Every call goes through HipOps (ops.lib where the wrapper would refuse first).  Sources are views of allocations of arbitrary bit patterns (NaN payloads,
infinities, -0.0, subnormals; the exact domain of the split for the triple images), destinations views of sentinel-filled allocations: the image has
exactly its documented length, padding rows are +0.0 and every word outside the image is the sentinel afterwards.  No comparison here has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import PlanRecorder, chosen_kernels, scan_kernel_candidates
from helpers_images import (LEAD, PACK_CASES, REFUSALS, SENTINEL, TAIL, WI_CASES, WI_KINDS, check_dense, check_frag, check_frag3, decode3, frag3_image,
                            frag_floats, frag_image, pack_source, source_values, unfrag, wi_need, wi_shape, wi_source)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _dev(a):
    """uint32 words -> a float32 device tensor with the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).to(DEV).view(torch.float32)


def _words(t):
    """a float32 device tensor -> its uint32 words on the host"""
    return t.contiguous().view(torch.int32).reshape(-1).cpu().numpy().view(np.uint32)


def _dst(need, off=0):
    """(allocation, view): `need` floats behind LEAD + off sentinel words (off = 1: 4 bytes off a 16-byte boundary) and in front of TAIL more"""
    buf = torch.full((LEAD + off + need + TAIL,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device=DEV).view(torch.float32)
    view = buf[LEAD + off: LEAD + off + need]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return buf, view


def _untouched(buf):
    w = _words(buf)
    assert (w == np.uint32(SENTINEL)).all(), "a refused call wrote word %d of a destination" % int(np.flatnonzero(w != np.uint32(SENTINEL))[0])


def _pack_src(case, pass_):
    alloc, view = pack_source(case, pass_)
    rows, K, ld, off = case["rows"], case["K"], case["ld"], case["off"]
    d = _dev(alloc)
    v = d[off: off + rows * ld].view(rows, ld)[:, :K]
    assert d.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off and (rows == 1 or v.stride(0) == ld)
    return alloc, view, d, v


def _of(packer):
    cases = [c for c in PACK_CASES if packer in c["packers"]]
    return dict(argnames="case", argvalues=cases, ids=[c["id"] for c in cases])


@pytest.mark.parametrize(**_of("frag"))
def test_frag_pack_bit_exact(ops, case):
    """fn_frag_pack on arbitrary bit patterns: the image is the host statement's bit for bit, a second launch gives the same bits, the source is unchanged"""
    rows, K = case["rows"], case["K"]
    alloc, view, d, v = _pack_src(case, "bits")
    assert ops.frag_floats(rows, K) == frag_floats(rows, K)
    buf, dst = _dst(frag_floats(rows, K))
    again, dst2 = _dst(frag_floats(rows, K))
    ops.frag_pack(v, dst)
    ops.frag_pack(v, dst2)
    torch.cuda.synchronize()
    check_frag(case["id"], _words(buf), LEAD, view, rows, K)
    assert np.array_equal(_words(buf), _words(again)), "%s: a second launch differs" % case["id"]
    assert np.array_equal(_words(d), alloc), "%s: the source changed" % case["id"]


@pytest.mark.parametrize(**_of("frag3"))
def test_frag3_pack_bit_exact(ops, case):
    """fn_frag3_pack on the exact domain of the split: every piece is the host statement's bit for bit, hi + mid + lo is the source exactly, padding rows are
    zero in all three pieces, a second launch gives the same bits, the source is unchanged"""
    rows, K = case["rows"], case["K"]
    alloc, view, d, v = _pack_src(case, "domain")
    need = frag_floats(rows, K) * 3 // 2
    buf, dst = _dst(need)
    again, dst2 = _dst(need)
    ops.frag3_pack(v, dst)
    ops.frag3_pack(v, dst2)
    torch.cuda.synchronize()
    check_frag3(case["id"], _words(buf), LEAD, view, rows, K)
    assert np.array_equal(_words(buf), _words(again)), "%s: a second launch differs" % case["id"]
    assert np.array_equal(_words(d), alloc), "%s: the source changed" % case["id"]


def _weight_images(ops, cid):
    """one fn_weight_images launch of WI_CASES[cid]: every destination against the numpy statement and against the single-matrix entry point"""
    jobs = WI_CASES[cid]
    host, dev, call = [], [], []
    for j, job in enumerate(jobs):
        alloc, view = wi_source(cid, j, job)
        d = _dev(alloc).view(job["R"], job["ld"])
        v = d[:, job["c0"]: job["c0"] + job["C"]]
        buf, dst = _dst(wi_need(job), job["dst_off"])
        host.append((alloc, view))
        dev.append((d, v, buf))
        call.append((WI_KINDS[job["kind"]], v, dst))
    ops.weight_images(call)                                  # (HipOps cuts at 56 jobs: the table has no more, so this is ONE launch)
    torch.cuda.synchronize()
    for j, (job, (alloc, view), (d, v, buf)) in enumerate(zip(jobs, host, dev)):
        name, kind, lead = "%s/job %d kind %d %dx%d ld %d" % (cid, j, job["kind"], job["R"], job["C"], job["ld"]), job["kind"], LEAD + job["dst_off"]
        got = _words(buf)
        assert np.array_equal(_words(d), alloc.reshape(-1)), "%s: the source changed" % name
        if kind in (0, 5):
            check_dense(name, got, lead, view.T if kind == 0 else view)
        else:
            rows, K = wi_shape(job)
            (check_frag if kind < 3 else check_frag3)(name, got, lead, view if kind in (1, 3) else view.T, rows, K)
        # ... and what the single-matrix entry point writes for the same matrix (a contiguous transpose for the transposed kinds)
        if kind == 5:
            continue
        single, sdst = _dst(wi_need(job))
        if kind == 0:
            ops.transpose(v, sdst.view(job["C"], job["R"]))
        else:
            m = v if kind in (1, 3) else v.t().contiguous()
            (ops.frag_pack if kind < 3 else ops.frag3_pack)(m, sdst)
        torch.cuda.synchronize()
        assert np.array_equal(_words(single)[LEAD:], got[lead:]), "%s: differs from the single-matrix entry point" % name


def test_weight_images_all_kinds_at_the_job_limit(ops):
    """one launch of exactly 56 jobs, all six kinds, every source a column view with ld > cols, two kind-0 destinations 4 bytes off alignment"""
    assert len(WI_CASES["limit-56-jobs"]) == 56
    _weight_images(ops, "limit-56-jobs")


def test_weight_images_grid_stride(ops):
    """one job per kind, each with more work items than its 128 blocks x 256 threads: every branch's grid-stride loop wraps"""
    _weight_images(ops, "grid-stride")


@pytest.mark.parametrize("case", REFUSALS, ids=[r["id"] for r in REFUSALS])
def test_image_calls_refuse(ops, case):
    """every refusal returns its code and leaves every destination as it was"""
    from music_fader_nets_amd import _lib
    bufs = []
    if case["fn"] == "wi":
        arr = (_lib.FnWeightImage * len(case["jobs"]))()
        keep = []
        for d, (kind, R, Cc, ld, off) in zip(arr, case["jobs"]):
            src = _dev(source_values(case["id"], max(R, 1) * max(ld, Cc), "bits"))
            buf, dst = _dst(2 * (R + 16) * (Cc + 32), off)
            keep.append(src)
            bufs.append(buf)
            d.src, d.dst, d.rows, d.cols, d.ld, d.kind = src.data_ptr(), dst.data_ptr(), R, Cc, ld, kind
        null = case.get("null")
        if isinstance(null, tuple):
            setattr(arr[null[0]], null[1], None)
        rc = ops.lib.fn_weight_images(None if null == "jobs" else arr, case.get("n_jobs", len(case["jobs"])), ops.stream())
    else:
        rows, K, ld = case["rows"], case["K"], case["ld"]
        src = _dev(source_values(case["id"], max(rows, 1) * max(ld, K), "bits"))
        buf, dst = _dst(2 * (rows + 16) * (K + 32), case["dst_off"])
        bufs.append(buf)
        ps = None if case.get("null") == "src" else C.c_void_p(src.data_ptr())
        pd = None if case.get("null") == "dst" else C.c_void_p(dst.data_ptr())
        rc = (ops.lib.fn_frag_pack if case["fn"] == "frag" else ops.lib.fn_frag3_pack)(ps, rows, K, ld, pd, ops.stream())
    torch.cuda.synchronize()
    assert rc == case["code"], "%s: returned %d, expected %d" % (case["id"], rc, case["code"])
    for buf in bufs:
        _untouched(buf)


def test_the_wrappers_refuse_a_short_destination(ops):
    """HipOps.frag_pack, frag3_pack and weight_images raise when dst is one float short, and nothing is written"""
    src = _dev(source_values("short", 17 * 64, "domain")).view(17, 64)
    ff = frag_floats(17, 64)
    for need, call in ((ff, lambda d: ops.frag_pack(src, d)), (ff * 3 // 2, lambda d: ops.frag3_pack(src, d)),
                       (17 * 64, lambda d: ops.weight_images([("transpose", src, d)])), (17 * 64, lambda d: ops.weight_images([("copy", src, d)])),
                       (ff, lambda d: ops.weight_images([("frag", src, d)])), (ff * 3 // 2, lambda d: ops.weight_images([("frag3", src, d)]))):
        buf, dst = _dst(need)
        with pytest.raises(RuntimeError, match="too small"):
            call(dst[:-1])
        torch.cuda.synchronize()
        _untouched(buf)
        call(dst)                                            # the exact size is taken
    wide = _dev(source_values("short-t", 64 * 17, "domain")).view(64, 17)      # the transposed kinds: images of the [17][64] matrix
    for kind, need in (("frag_t", frag_floats(17, 64)), ("frag3_t", frag_floats(17, 64) * 3 // 2)):
        buf, dst = _dst(need)
        with pytest.raises(RuntimeError, match="too small"):
            ops.weight_images([(kind, wide, dst[:-1])])
        torch.cuda.synchronize()
        _untouched(buf)
        ops.weight_images([(kind, wide, dst)])
    torch.cuda.synchronize()


def _scan(B, H, T, reverse, seed, V=50):
    """one forward table scan on the device with an initial state, its weights packed by the single-matrix entry points"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return dict(B=B, T=T, H=H, reverse=reverse, w=rn(3 * H, H) / H ** 0.5, b_hh=rn(3 * H) * 0.1, b_ih=rn(3 * H) * 0.1, h0=rn(B, H) * 0.5,
                gx_table=rn(V, 3 * H) * 0.5, idx=torch.randint(0, V, (B, T), generator=g, dtype=torch.int32).to(DEV))


def _run_handover(ops, scans, x6, h0_frag):
    """the scans in one weight-stationary launch with h_last_frag (h0_frag: the initial states also as images of the single-matrix packer) ->
    per scan (h_all, gates, hand-over allocation), and the kernel the library's plan says it took"""
    out, launch = [], []
    for s in scans:
        B, H, T = s["B"], s["H"], s["T"]
        need = frag_floats(B, H) * (3 if x6 else 2) // 2
        hand, hl = _dst(need)
        d = {k: v for k, v in s.items() if k != "w"}
        d.update(h_all=torch.full((T, B, H), float("nan"), device=DEV), gates=torch.full((T, ops.gates_floats(B, H)), float("nan"), device=DEV), h_last_frag=hl)
        d["w_hh_frag"] = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
        ops.frag_pack(s["w"], d["w_hh_frag"])
        if x6:
            d["w_hh_frag3"] = torch.zeros(ops.frag_floats(3 * H, H) * 3 // 2, device=DEV)
            ops.frag3_pack(s["w"], d["w_hh_frag3"])
        if h0_frag:
            d["h0_frag"] = torch.zeros(need, device=DEV)
            (ops.frag3_pack if x6 else ops.frag_pack)(s["h0"], d["h0_frag"])
        launch.append(d)
        out.append((d["h_all"], d["gates"], hand))
    rec = PlanRecorder(ops)
    rec.gru_seq_fwd(launch, x6=x6)
    torch.cuda.synchronize()
    return out, chosen_kernels(rec.fwd)


@pytest.mark.parametrize("x6", (False, True), ids=("f32-33x64-T3-fwd-and-reverse", "x6-64x512-T2"))
def test_scan_hand_over_images_decode_to_the_state(ops, x6):
    """the image a weight-stationary forward scan leaves in h_last_frag is the state of the step computed last - h_all[T - 1] in processing order, for forward
    and reverse scans alike: the fp32 image bit for bit in the layout of fn_frag_pack (rows below B), the bf16 x 6 triple image with hi + mid + lo equal
    to it exactly; and an initial state handed in as the image of fn_frag_pack / fn_frag3_pack gives the bits of the row-major one"""
    scans = [_scan(64, 512, 2, 0, 641)] if x6 else [_scan(33, 64, 3, 0, 331), _scan(33, 64, 3, 1, 332)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    forward = scan_kernel_candidates(scans, x6=x6, cus=cus)[0]      # (the backward half of the restatement is not asked: 64 rows have no bf16 x 6 backward)
    assert forward, "not eligible for the forward kernels the case is for"
    name = forward[0]
    assert "step" not in name and name.startswith("gru_fwd_x6" if x6 else "gru_fwd_persist_kernel"), name
    found = ops.dw_x6
    try:
        ops.dw_x6 = x6
        plain, k0 = _run_handover(ops, scans, x6, h0_frag=False)
        imaged, k1 = _run_handover(ops, scans, x6, h0_frag=True)
    finally:
        ops.dw_x6 = found
    assert k0 == k1 == [name], (k0, k1, name)
    for i, (s, (h_all, gates, hand), (h_all2, gates2, hand2)) in enumerate(zip(scans, plain, imaged)):
        B, H, T = s["B"], s["H"], s["T"]
        cid = "%s scan %d" % ("x6" if x6 else "f32", i)
        h = _words(h_all).reshape(T, B, H)
        assert not np.isnan(h.view(np.float32)).any(), cid
        assert np.array_equal(h, _words(h_all2).reshape(T, B, H)), "%s: h_all differs when h0 comes as an image" % cid
        assert torch.equal(gates.view(torch.int32), gates2.view(torch.int32)), "%s: the gates differ when h0 comes as an image" % cid
        assert np.array_equal(_words(hand), _words(hand2)), "%s: the hand-over image differs when h0 comes as an image" % cid
        got = _words(hand)
        assert all(not np.array_equal(h[T - 1], h[p]) for p in range(T - 1)), cid
        if not x6:
            n = frag_floats(B, H)
            assert (got[:LEAD] == SENTINEL).all() and (got[LEAD + n:] == SENTINEL).all(), "%s: written outside the image" % cid
            state = unfrag(got[LEAD: LEAD + n], B, H)[:B]
            which = [p for p in range(T) if np.array_equal(state, h[p])]
            assert which == [T - 1], "%s: the image is the state of step(s) %s of %d, not of the last one" % (cid, which, T)
            rows16 = n // H
            live = frag_image((np.arange(rows16 * H, dtype=np.uint32) // H < B).astype(np.uint32), rows16, H).astype(bool)      # image words of rows below B
            assert live.sum() == B * H and np.array_equal(got[LEAD: LEAD + n][live], frag_image(h[T - 1], B, H)[live]), cid
        else:
            assert B % 16 == 0
            # the header promises the sum, not which rounding the in-kernel split uses: pieces are not compared with fn_frag3_pack's
            check_frag3(cid, got, LEAD, h[T - 1], B, H, bitwise=False)
            dec = decode3(got[LEAD: LEAD + frag_floats(B, H) * 3 // 2].view(np.uint16), B, H)
            which = [p for p in range(T) if np.array_equal(dec, h[p].view(np.float32).astype(np.float64))]
            assert which == [T - 1], "%s: the image decodes to the state of step(s) %s of %d" % (cid, which, T)
            same = np.array_equal(got[LEAD: LEAD + frag_floats(B, H) * 3 // 2].view(np.uint16), frag3_image(h[T - 1].view(np.float32), B, H))
            print("\n%s: the kernel-written triple image %s the bits of fn_frag3_pack's split of the same state" % (cid, "has" if same else "does NOT have"))
    assert not ops.gru_sync_error()
