"""The latent block of csrc/loss.hip against float64 on an MI355X: fn_latent_fwd and fn_latent_bwd.

The case table, the float64 references, the float32 restatement of the documented formulas, the per-tile bound and the checkers are
tests/helpers_latent.py; tests/test_latent_reference.py shows on the CPU that the table has the properties its ids claim, that the backward reference
is autograd of the documented loss, that the checkers accept the restatement and FakeOps, and that they reject planted faults.  Each launch is checked
for layout, for its exact parts, then for the tile bound; every test prints its line of profiles/latent_fp64_errors.txt."""
import ctypes as C
import types

import pytest
import torch

from helpers_latent import (BWD_CASES, CHAIN_CASES, EXACT_CASES, FWD_CASES, INT_SENTINEL, LATENT_F, LATENT_REFUSALS, SCAN_F_CAP, SENTINEL, bits_equal, chain,
                            check_bwd, check_fwd, exact_line, line, run_bwd, run_exact, run_fwd)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _ids(cases):
    return [c["id"] for c in cases]


def _same(cid, a, b, what):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]) if a[k].dtype == torch.int32 else bits_equal(a[k], b[k]), "%s: %s of %s differs" % (cid, k, what)


@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_latent_fwd_vs_fp64(ops, case):
    """Z in {1, 5, 63, 64, 65, 128, 200} (empty lanes, a full wave, a one-lane tail, two and a bit passes), K in {1, 2, 3, 8}, B in {1, 3, 4, 21},
    unsupervised and with labels, the posterior live, tied between two identical components, saturated and as at initialisation: sigma, z, ll, qy and
    each column of terms in every tile; y the first index of the maximum of the kernel's own qy and, where the reference decides it, the reference's;
    rows >= B untouched, inputs unmodified, a second launch the same bits"""
    bufs = run_fwd(ops, case, DEV)
    worst = check_fwd(case, bufs)
    _same(case["id"], bufs, run_fwd(ops, case, DEV), "a second launch")
    print()
    print(line("fwd", case["id"], worst))


@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_latent_bwd_from_the_reference_vs_fp64(ops, case):
    """z and qy are the float32 rounding of the float64 forward reference, independent of the forward kernel; each upstream gradient alone, all of them,
    none, w3 = NULL, dmu_lk_rows = NULL: dpre and dmu_lk_rows in every 16 x 16 tile, the entries the form makes exactly zero exactly 0.0"""
    bufs = run_bwd(ops, case, DEV)
    worst = check_bwd(case, bufs)
    _same(case["id"], bufs, run_bwd(ops, case, DEV), "a second launch")
    print()
    print(line("bwd", case["id"], worst))


@pytest.mark.parametrize("case", CHAIN_CASES, ids=_ids(CHAIN_CASES))
def test_latent_bwd_chained_vs_fp64(ops, case):
    """the backward on the z and qy the forward kernel wrote; the reference takes those same arrays"""
    z, q = chain(ops, case, DEV)
    worst = check_bwd(case, run_bwd(ops, case, DEV, z_in=z, qy_in=q), z_in=z, qy_in=q)
    print()
    print(line("bwd-chained", case["id"], worst))


@pytest.mark.parametrize("name", EXACT_CASES)
def test_latent_exact(ops, name):
    what = run_exact(ops, name, DEV)
    print()
    print(exact_line("exact", name, what))


def test_latent_refusals_return_their_code_and_write_nothing(ops):
    """every required pointer NULL gives FN_E_NULL - before the shape is looked at -, B, Z, K <= 0 and K = 9 give FN_E_SHAPE, and not one element of the
    buffers handed over is written"""
    f = torch.full((4096,), SENTINEL, device=DEV)
    i = torch.full((4096,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    p = types.SimpleNamespace(f=C.c_void_p(f.data_ptr()), i=C.c_void_p(i.data_ptr()))
    for name, fn, args, code in LATENT_REFUSALS:
        got = getattr(ops.lib, fn)(*args(p))
        assert got == code, "%s: %s returned %d, expected %d" % (name, fn, got, code)
    torch.cuda.synchronize()
    assert bool((f == SENTINEL).all()) and bool((i == INT_SENTINEL).all()), "a refused call wrote to a buffer"
    assert all(0 < F <= SCAN_F_CAP for F in LATENT_F.values())
    print()
    print(exact_line("C ABI", "%d refusals" % len(LATENT_REFUSALS), "error code returned, nothing written"))
