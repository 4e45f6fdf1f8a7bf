"""The decode launch plans (csrc/decode_plan.h) asked through the C ABI without a GPU: fn_decode_plan / fn_out_argmax_plan with the compute units given
touch no device.  The expectations are written down here a second time: the workspace formula fn_decode_ws_bytes had before the layout function
existed, and a table of plans worked out by hand (H = 512, V = 342: 3 x 32 + 22 + 1 = 119 workgroups per role set; H = 64: 35)."""
import ctypes as C

from mfn_import import load_package


def _lib():
    load_package()
    from music_fader_nets_amd import _lib
    return _lib, _lib.load()


def _decode(L, B, H, V=342, steps=8, addr=1 << 20):
    d = L.FnDecode()
    for nm in ("w_hh1_frag", "b_hh1", "b_ih1", "table1", "rowbias1", "h0", "w_ih2_frag", "b_ih2", "w_hh2_frag", "b_hh2", "w_out_frag", "b_out", "tokens", "ws",
               "sync_ws"):
        setattr(d, nm, addr)                                 # made-up 16-byte aligned addresses: inspected, never dereferenced
    d.B, d.steps, d.H, d.V, d.start_token, d.tok_ld = B, steps, H, V, V - 1, steps
    return d


def test_decode_ws_bytes_is_the_formula_it_was():
    _, lib = _lib()
    for H in (64, 512):
        for V in (1, 342, 384):
            vp = (V + 15) // 16 * 16
            for B in range(1, 2049):
                bp = 16 if B <= 16 else (B + 63) // 64 * 64
                assert lib.fn_decode_ws_bytes(B, H, V) == (4 * bp * H + bp * 3 * H + bp * vp) * 4, (B, H, V)
    assert lib.fn_decode_sync_ws_bytes() == (32 * 160 + 32) * 4


# (H, B) -> (mt, nblk, nrep, grid) on 256 compute units
PLAN_TABLE = {
    (512, 16): (1, 1, 1, 119), (512, 17): (2, 1, 1, 119), (512, 33): (2, 2, 2, 238), (512, 352): (2, 11, 2, 238), (512, 353): (4, 6, 2, 238),
    (512, 2048): (4, 32, 2, 238),
    (64, 16): (1, 1, 1, 35), (64, 33): (2, 2, 2, 70), (64, 352): (2, 11, 7, 245), (64, 353): (4, 6, 6, 210), (64, 2048): (4, 32, 7, 245),
}


def test_decode_plan_literal_table_and_answers():
    L, lib = _lib()
    plan = L.FnDecodePlan()
    f = L.FnDecodeForce()
    f.forced, f.forced_ld, f.force = 1 << 20, 8, 1 << 20
    for (H, B), (mt, nblk, nrep, grid) in PLAN_TABLE.items():
        d = _decode(L, B, H)
        for force in (None, C.byref(f)):
            assert lib.fn_decode_plan(C.byref(d), force, 256, C.byref(plan)) == 0 and plan.status == 0, (H, B, plan.status)
            p = plan.as_dict()
            assert (p["mt"], p["nblk"], p["nrep"], p["grid"]) == (mt, nblk, nrep, grid), (H, B, p)
            assert p["block_rows"] == 16 * mt and p["per_rep"] == (119 if H == 512 else 35) and p["threads"] == 256 and p["forced"] == (force is not None)
            assert p["nslices"] == H // 16 and p["nvt"] == 22 and p["lds_bytes"] == (3 * H * 16 + 4 * mt * 3 * 272) * 4 + 272
            rows = nblk * 16 * mt
            assert (p["x1_off"], p["x2_off"], p["g2_off"], p["logits_off"], p["ws_floats"]) == (0, 2 * rows * H, 4 * rows * H, 7 * rows * H, 7 * rows * H + rows * 352)
            assert 4 * p["ws_floats"] <= lib.fn_decode_ws_bytes(B, H, 342)
    # the answers in front of the plan, and the order of the checks
    d = _decode(L, 40, 512)
    assert lib.fn_decode_plan(C.byref(d), None, 256, None) == L.FN_E_NULL
    assert lib.fn_decode_plan(C.byref(d), None, -1, C.byref(plan)) == L.FN_E_SHAPE
    assert lib.fn_decode_plan(None, None, 256, C.byref(plan)) == 0 and plan.status == L.FN_E_NULL
    assert lib.fn_decode_plan(C.byref(d), None, 118, C.byref(plan)) == 0 and plan.status == L.FN_E_UNSUPPORTED
    d.ws = (1 << 20) + 4
    assert lib.fn_decode_plan(C.byref(d), None, 118, C.byref(plan)) == 0 and plan.status == L.FN_E_ALIGN
    d.H = 48
    assert lib.fn_decode_plan(C.byref(d), None, 256, C.byref(plan)) == 0 and plan.status == L.FN_E_SHAPE
    d.h0 = None
    assert lib.fn_decode_plan(C.byref(d), None, 256, C.byref(plan)) == 0 and plan.status == L.FN_E_NULL
    f.forced_ld = 7
    assert lib.fn_decode_plan(C.byref(d), C.byref(f), 256, C.byref(plan)) == 0 and plan.status == L.FN_E_SHAPE
    # the entry points themselves answer the same before they touch a device
    assert lib.fn_decode_greedy(C.byref(d), None) == L.FN_E_NULL and lib.fn_decode_forced(C.byref(d), C.byref(f), None) == L.FN_E_SHAPE
    assert lib.fn_decode_forced(C.byref(d), None, None) == L.FN_E_NULL and lib.fn_decode_greedy(None, None) == L.FN_E_NULL


def test_out_argmax_plan_kernel_by_k():
    L, lib = _lib()
    plan = L.FnOutArgmaxPlan()
    a = 1 << 20
    for B, V, K, kernel, grid, threads, lds in [
            (2048, 342, 512, "out_argmax_lds8_kernel<4>", 32 * 8, 512, 48 * 512 * 4 + 12288), (70, 97, 32, "out_argmax_lds8_kernel<4>", 2 * 3, 512, 48 * 32 * 4 + 12288),
            (70, 97, 16, "out_argmax_lds_kernel<8>", 2 * 3, 256, 48 * 16 * 4), (130, 342, 112, "out_argmax_lds_kernel<8>", 3 * 8, 256, 48 * 112 * 4),
            (70, 60, 672, "out_argmax_lds8_kernel<4>", 2 * 2, 512, 48 * 672 * 4 + 12288), (70, 60, 688, "out_argmax_direct_kernel<4>", 3 * 1, 256, 0),
            (70, 60, 1024, "out_argmax_direct_kernel<4>", 3 * 1, 256, 0)]:
        assert lib.fn_out_argmax_plan(a, K, a, K, a, B, V, K, a, C.byref(plan)) == 0 and plan.status == 0, (B, V, K, plan.status)
        p = plan.as_dict()
        assert (p["kernel"], p["grid"], p["threads"], p["lds_bytes"]) == (kernel, grid, threads, lds), (B, V, K, p)
    assert lib.fn_out_argmax_plan(a, 512, a, 512, a, 8, 342, 512, a, None) == L.FN_E_NULL
    for args, want in [((None, 512, a, 512, a, 0, 342, 512, a), L.FN_E_NULL), ((a + 4, 512, a, 512, a, 8, 342, 40, a), L.FN_E_SHAPE),
                       ((a + 4, 1 << 20, a, 512, a, 1024, 342, 512, a), L.FN_E_SHAPE), ((a + 4, 512, a, 512, a, 8, 342, 512, a), L.FN_E_ALIGN),
                       ((a, 512, a, 512, a, 8, 342, 512, a + 4), L.FN_E_ALIGN)]:
        assert lib.fn_out_argmax_plan(*args, C.byref(plan)) == 0 and plan.status == want, (args, plan.status)
        assert lib.fn_out_argmax_f32(*args, None) == want
