"""Driver of tests/test_decode_forced.py::test_forced_host_twin_under_asan: runs in a subprocess with the AddressSanitizer runtime preloaded
and pushes the three mask shapes through fn_decode_forced_host, every step checked by helpers_forced.replay_forced_check."""
import ctypes as C

import numpy as np

from host_twins_driver import L, P, f32, frag, gemm, lib   # noqa: E402  (sets sys.path, loads the ASAN twin library)
from helpers import replay_inputs, replay_z                 # noqa: E402
from helpers_forced import FORCED_MASKS, fed_stream, forced_line, forced_mask, forced_tokens, replay_forced_check  # noqa: E402


def run(sd, z, steps, forced, force, forced_ld=None, with_force=True):
    H = sd["grucell_g.weight_hh"].shape[1]
    nb = z.shape[0]
    Wih = sd["grucell_g.weight_ih"].numpy()
    zd = f32(z.numpy())
    K = zd.shape[1]
    keep = dict(w1=frag(sd["grucell_g.weight_hh"].numpy()), w2i=frag(sd["grucell_g_2.weight_ih"].numpy()), w2h=frag(sd["grucell_g_2.weight_hh"].numpy()),
                wo=frag(sd["linear_out_g.weight"].numpy()), table=f32(np.ascontiguousarray(Wih[:, :342].T)),
                rb=gemm(1, 1, nb, 3 * H, K, zd, np.ascontiguousarray(Wih[:, 342:])),
                h0=gemm(1, 1, nb, H, K, zd, sd["linear_init_global.weight"].numpy(), bias=sd["linear_init_global.bias"].numpy()),
                tok=np.zeros((nb, steps), np.int32), logp=np.zeros((nb, steps, 342), np.float32),
                ws=np.zeros(lib.fn_decode_ws_bytes_host(nb, H, 342) // 4 + 4, np.float32), sync=np.zeros(8, np.int32),
                b=[f32(sd[k].numpy()) for k in ("grucell_g.bias_hh", "grucell_g.bias_ih", "grucell_g_2.bias_ih", "grucell_g_2.bias_hh", "linear_out_g.bias")],
                forced=np.ascontiguousarray(forced, np.int32), force=np.ascontiguousarray(force, np.uint8))
    d = L.FnDecode()
    d.B, d.steps, d.H, d.V, d.start_token = nb, steps, H, 342, 341
    d.w_hh1_frag, d.b_hh1, d.b_ih1, d.table1, d.rowbias1, d.h0 = P(keep["w1"]), P(keep["b"][0]), P(keep["b"][1]), P(keep["table"]), P(keep["rb"]), P(keep["h0"])
    d.w_ih2_frag, d.b_ih2, d.w_hh2_frag, d.b_hh2 = P(keep["w2i"]), P(keep["b"][2]), P(keep["w2h"]), P(keep["b"][3])
    d.w_out_frag, d.b_out, d.tokens, d.tok_ld, d.logp, d.ws, d.sync_ws = P(keep["wo"]), P(keep["b"][4]), P(keep["tok"]), steps, P(keep["logp"]), P(keep["ws"]), P(keep["sync"])
    f = L.FnDecodeForce()
    f.forced, f.forced_ld = P(keep["forced"]), keep["forced"].shape[1] if forced_ld is None else forced_ld
    f.force = P(keep["force"]) if with_force else None
    rc = lib.fn_decode_forced_host(C.byref(d), C.byref(f), None)
    greedy = None
    if rc == 0 and not force.any():                      # the plain entry point on the same inputs, into buffers of its own
        gt, gl = np.zeros_like(keep["tok"]), np.zeros_like(keep["logp"])
        d.tokens, d.logp = P(gt), P(gl)
        greedy = (lib.fn_decode_greedy_host(C.byref(d), None), gt, gl)
    return rc, keep["tok"], keep["logp"], greedy


if __name__ == "__main__":
    H, Z, sd = replay_inputs("h64")
    nb, steps = 6, 80
    z = replay_z(nb, Z, 21)
    forced = forced_tokens(nb, steps + 2, 21).numpy()                 # forced_ld > steps
    for kind in FORCED_MASKS:
        force = forced_mask(kind, steps, 21)
        # the exact-size mask array: a read of force[steps] would be a heap overflow ASAN reports
        rc, tok, lp, _ = run(sd, z, steps, forced, force)
        assert rc == 0
        st = replay_forced_check(sd, z, tok, forced, force, fed_stream(tok, forced, force), lp)
        print(forced_line("fn_decode_forced_host", kind, H, st))
    # none forced = fn_decode_greedy_host, bit for bit
    rc, tok, lp, (rc0, gtok, glp) = run(sd, z, steps, forced, np.zeros(steps, bool))
    assert rc == 0 and rc0 == 0 and tok.any() and gtok.any() and np.array_equal(tok, gtok) and np.array_equal(lp, glp)
    # an out-of-range forced token is clamped to the table's rows (no read outside it: ASAN watches), the last mask entry is ignored
    wild = forced.copy()
    wild[:, 3], wild[:, 4], wild[:, steps - 1] = 1 << 30, -5, 1 << 30
    rc, tok, lp, _ = run(sd, z, steps, wild, np.ones(steps, bool))
    assert rc == 0
    clamped = np.clip(wild, 0, 341)
    replay_forced_check(sd, z, tok, clamped, np.ones(steps, bool), fed_stream(tok, clamped, np.ones(steps, bool)), lp)
    assert lib.fn_decode_forced_host(None, None, None) == L.FN_E_NULL
    assert run(sd, z, steps, forced, np.ones(steps, bool), with_force=False)[0] == L.FN_E_NULL
    assert run(sd, z, steps, forced, np.ones(steps, bool), forced_ld=steps - 1)[0] == L.FN_E_SHAPE
    print("HOST FORCED DECODE OK")
