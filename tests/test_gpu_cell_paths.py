"""The large-batch GRU cell fn_gru_cell_f32 - gru_cell_kernel (staged), gru_cell_direct_kernel, gru_cell_wlds_kernel, gru_cell_wlds_ovl_kernel and
gru_cell_x6_kernel of csrc/gru.hip - per 16 x 16 tile of h_out against float64.

The cases, the references, the restatement of the bf16 x 6 arithmetic, the hand plan and the checker are tests/helpers_cell.py; tests/test_cell_reference.py shows
on the CPU that the table reaches what it claims, that the input conditions hold and that planted faults are rejected.  Every case here is one small launch
through HipOps.gru_cell (and a second one for the repeat): operands are views of NaN-filled allocations (padding columns, rows behind the batch, table rows no
token selects), h_out a view of a sentinel-filled one; the hand plan on the real addresses equals the library's own (HipOps.gru_cell_plan) and names the family
and instance of the case's id; every sentinel is bit-identical afterwards; err <= CELL_F x max(e_ref, 2**-23) in every tile; the second launch gives the same
bits; a packed-argmax token source gives the bits of the same tokens through idx.  One line of profiles/gru_cell_fp64_errors.txt is printed per case."""
import pytest
import torch

from helpers_cell import CELL_CASES, CELL_F, assert_plan_is_the_cases, assert_plan_is_the_librarys, cell_buffers, cell_case_plan, cell_line, check_cell_vs_f64
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADDR_OF = dict(x="x", wih="w_ih", h="h_prev", whh="w_hh", out="h_out", bhh="b_hh", bih="b_ih", table="gx_table", rb="gx_rowbias")


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _launch(ops, case):
    """two launches of the case into two sentinel-filled allocations -> (both on the CPU, the plan on the real addresses)"""
    kw, obuf = cell_buffers(case, DEV)
    again = obuf.clone()
    B, H = case["B"], case["H"]
    named = dict(kw)
    args = [kw.pop(k) for k in ("h_prev", "w_hh", "b_hh", "h_out")]
    found = (ops.dw_x6, ops.cell_x6, ops.cell_x6_rows)
    try:
        if case["x6"]:                                   # the wrapper's own switch: FN_GRU_BF16X6 from 0 rows on
            ops.dw_x6, ops.cell_x6, ops.cell_x6_rows = True, True, 0
        else:
            kw["variant"] = case["variant"]
        addr = {n: 0 if named.get(k) is None else named[k].data_ptr() for n, k in ADDR_OF.items()}
        plan = cell_case_plan(case, addr)
        assert_plan_is_the_librarys(case, plan, ops.gru_cell_plan(*args, **kw))
        assert_plan_is_the_cases(case, plan)
        ops.gru_cell(*args, **kw)
        ops.gru_cell(args[0], args[1], args[2], again[:B, :H], **kw)
        torch.cuda.synchronize()
    finally:
        ops.dw_x6, ops.cell_x6, ops.cell_x6_rows = found
    assert (ops.dw_x6, ops.cell_x6, ops.cell_x6_rows) == found
    return obuf.cpu(), again.cpu(), plan


def _case(ops, case):
    obuf, again, plan = _launch(ops, case)
    worst = check_cell_vs_f64(case, obuf, CELL_F[plan["family"]])
    assert torch.equal(obuf.view(torch.int32), again.view(torch.int32)), "%s: a repeated launch differs from the first" % case["id"]
    if case["tab"] and case["tok"] == "best":            # the same tokens through idx: the same bits
        twin, _, tplan = _launch(ops, dict(case, tok="idx"))
        assert (tplan["family"], tplan["template"]) == (plan["family"], plan["template"])
        assert torch.equal(obuf.view(torch.int32), twin.view(torch.int32)), "%s: idx_best and idx differ" % case["id"]
    print()
    print(cell_line(case, plan, worst))


def _of(*groups):
    cases = [c for c in CELL_CASES if c["group"] in groups]
    return dict(argnames="case", argvalues=cases, ids=[c["id"] for c in cases])


@pytest.mark.parametrize(**_of("tiles"))
def test_cell_row_and_unit_tiles_of_every_instance(ops, case):
    """every built instance at rows-per-workgroup + 17 rows (one full row tile, one of a full 16-row fragment plus one row) and two or four unit tiles; the
    overlapped fill at H = 512 with and without a dense input; the 4 x 8 super-tile walk of the staged kernel"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("ktails"))
def test_cell_k_tails_with_more_than_one_unit_tile(ops, case):
    """nks = K / 16 = 1, 2, 3, 5, 9, 17 of the input phase and 4, 6, 18 of the recurrent phase against rings of 1, 2, 4 and 8 slots at 70 rows, u0 > 0"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("forms", "tokens"))
def test_cell_input_forms_and_token_sources(ops, case):
    """the four (token table, row constant) forms with and without b_ih, the start token, and packed argmax words built on the host, in every family"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("views"))
def test_cell_operand_views(ops, case):
    """ld = width + 4 and + 16 on x, h_prev, w_ih, w_hh, h_out, one at a time and all together: padding never read, nothing written outside [B][H]"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("checked"))
def test_cell_staged_checked_loads_and_the_fallback(ops, case):
    """Stage::load_checked in both phases (K1 = 50, 75; h_prev and w_ih one float into their allocations; ldh = H + 2; ldw_hh = H + 1) on the 128- and the
    64-row staged forms and the automatic plan; a direct, weight-slice or bf16 x 6 form asked for on those inputs is declined and runs the staged default"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("auto"))
def test_cell_automatic_plan_above_512_rows(ops, case):
    """variant 0: the weight-slice cells, the LDS-free cells (above 1536 rows, or a slice that does not fit LDS) and the overlapped fill"""
    _case(ops, case)


@pytest.mark.parametrize(**_of("x6", "x6-pieces", "x6-declined"))
def test_cell_bf16x6_trip_counts_piece_passes_and_declined_shapes(ops, case):
    """gru_cell_x6_kernel at every producer trip count nblk = 2 .. 13, 5 at 256 rows and 32; the passes small / A3 / B3 / AB2 (exact pre-activations: only the
    epilogue's rounding is left) at nblk = 2, 3, 4, 32; shapes the kernel declines run the fp32 cells"""
    _case(ops, case)
