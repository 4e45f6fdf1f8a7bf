"""Event tokens <-> timed notes on a real MI355X: fn_notes_from_tokens and fn_tokens_from_notes exactly against statement 2 of tests/helpers_notes.py on
every case the CPU tests run through the two statements and the host twin (1, 7 and 300 rows per launch, sentinel columns, zeroed tails, pad), the device
round trip through event_attributes, a fader sweep to notes to MIDI files and back, and midi_segments on the real ops against the stand-ins."""
import numpy as np
import pytest
import torch

import helpers_attributes as ha
import helpers_notes as hn
from helpers import make_model
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKEN_CASES, SPAN_CASES = hn.token_cases(), hn.span_cases()
_id = lambda c: c["tag"].replace(" ", "_")


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


@pytest.mark.parametrize("case", TOKEN_CASES, ids=[_id(c) for c in TOKEN_CASES])
def test_notes_from_tokens_kernel(case):
    """tokens as a view of a wider matrix whose last columns are sentinels (a note-on: reading one changes the result); outputs that start as sentinels;
    the notes in front of sentinel words: entries [n_notes, notes_ld) zeroed, nothing behind notes_ld"""
    ops = _ops()
    rows, steps, notes_ld = case["tok"].shape[0], case["steps"], case["notes_ld"]
    ref = hn.notes_from_tokens_ref(case["tok"], steps, case["p"], notes_ld)
    tok = torch.from_numpy(case["tok"]).to(DEV)
    prm = torch.from_numpy(hn.params_bytes(case["p"])).to(DEV)
    buf = torch.full((rows * notes_ld * 4 + 64,), -9, dtype=torch.int32, device=DEV)
    notes = buf[:rows * notes_ld * 4].view(rows, notes_ld, 4)
    out = [torch.full((rows,), -9, dtype=torch.int32, device=DEV) for _ in range(3)]
    ops.notes_from_tokens(tok[:, :steps], steps, prm, notes, *out)
    torch.cuda.synchronize()
    got = dict(notes=notes.cpu().numpy(), n_notes=out[0].cpu().numpy(), t_end=out[1].cpu().numpy(), status=out[2].cpu().numpy())
    hn.same(got, ref, hn.NOTE_KEYS, case["tag"])
    assert bool((buf[rows * notes_ld * 4:] == -9).all()) and torch.equal(tok.cpu(), torch.from_numpy(case["tok"]))


@pytest.mark.parametrize("case", SPAN_CASES, ids=[_id(c) for c in SPAN_CASES])
def test_tokens_from_notes_kernel(case):
    """the token matrix is tok_ld wide and starts as sentinels: `steps` columns are written (the stream, then pad), the others keep the sentinel; with
    n_shift 0 the result is unspecified and only the sentinels are looked at"""
    ops = _ops()
    rows, steps, tok_ld = len(case["spans"]), case["steps"], case["tok_ld"]
    notes, spans = torch.from_numpy(case["notes"]).to(DEV), torch.from_numpy(case["spans"]).to(DEV)
    prm = torch.from_numpy(hn.params_bytes(case["p"])).to(DEV)
    buf = torch.full((rows * tok_ld + 64,), -9, dtype=torch.int32, device=DEV)
    tok = buf[:rows * tok_ld].view(rows, tok_ld)
    out = [torch.full((rows,), -9, dtype=torch.int32, device=DEV) for _ in range(3)]
    ops.tokens_from_notes(notes, spans, prm, tok[:, :steps], steps, *out)
    torch.cuda.synchronize()
    assert bool((tok[:, steps:] == -9).all()) and bool((buf[rows * tok_ld:] == -9).all()), case["tag"]
    if not case.get("unspecified"):
        ref = hn.tokens_from_notes_ref(case["notes"], case["spans"], steps, case["p"])
        got = dict(tokens=tok[:, :steps].cpu().numpy(), n_tokens=out[0].cpu().numpy(), n_kept=out[1].cpu().numpy(), status=out[2].cpu().numpy())
        hn.same(got, ref, hn.TOKEN_KEYS, case["tag"])
    assert torch.equal(notes.cpu(), torch.from_numpy(case["notes"])) and torch.equal(spans.cpu(), torch.from_numpy(case["spans"]))


def test_device_round_trip_keeps_the_attributes():
    """tokens -> notes -> tokens (256 columns, every status 0 or EMPTY as before) -> event_attributes equals event_attributes of the input, on the fixture
    rows of both vocabularies through the kernel table, and for the default one through the public calls"""
    ops = _ops()
    pkg = load_package()
    i32 = dict(dtype=torch.int32, device=DEV)
    for g, p, names, tok_np in ha.fixture_streams():
        rows, steps = tok_np.shape
        tok = torch.from_numpy(tok_np).to(DEV)
        prm = torch.from_numpy(hn.params_bytes(dict(hn.from_attr_params(p), add_eos=1))).to(DEV)
        notes = torch.empty(rows, steps, 4, **i32)
        n_notes, t_end, st = (torch.empty(rows, **i32) for _ in range(3))
        ops.notes_from_tokens(tok, steps, prm, notes, n_notes, t_end, st)
        spans = torch.stack([torch.arange(rows, **i32) * steps, n_notes, torch.zeros(rows, **i32), torch.full((rows,), hn.MAX_TICK, **i32)], 1).contiguous()
        back = torch.empty(rows, 256, **i32)
        n_tokens, n_kept, st2 = (torch.empty(rows, **i32) for _ in range(3))
        ops.tokens_from_notes(notes.view(-1, 4), spans, prm, back, 256, n_tokens, n_kept, st2)
        assert torch.equal(st2, st) and int(st2.max()) <= hn.EMPTY and torch.equal(n_kept, n_notes) and int(n_tokens.max()) <= 256

        def attributes(t, cols):
            cells_ld = ha.cells_ld_for(256, p)
            out = dict(n_cells=torch.empty(rows, **i32), status=torch.empty(rows, **i32), r_density=torch.empty(rows, dtype=torch.float32, device=DEV),
                       n_density=torch.empty(rows, dtype=torch.float32, device=DEV), c_r=torch.empty(rows, **i32), c_n=torch.empty(rows, **i32))
            cells = [torch.empty(rows, cells_ld, dtype=torch.uint8, device=DEV) for _ in range(2)]
            ops.event_attributes(t, cols, torch.from_numpy(ha.params_bytes(p)).to(DEV), rhythm=cells[0], notes=cells[1], cells_ld=cells_ld, **out)
            return dict({k: v.cpu().numpy() for k, v in out.items()}, rhythm=cells[0].cpu().numpy(), notes=cells[1].cpu().numpy())

        ha.same_attributes(attributes(back, 256), attributes(tok, steps), "round trip " + g)
        if g == "d":
            res = pkg.tokens_to_notes(tok)
            assert torch.equal(res.notes, notes) and torch.equal(res.n_notes, n_notes) and torch.equal(res.t_end, t_end) and res.notes.is_cuda
            again, _, _, status = pkg.notes_to_tokens(res.notes, n_notes=res.n_notes, steps=256)
            assert torch.equal(again, back) and torch.equal(status, st)
            a, b = pkg.event_attributes(again), pkg.event_attributes(tok)
            assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                       for x, y in zip(a, b))


def _sweep_inputs():
    rs = np.random.RandomState(11)
    x, c = torch.from_numpy(rs.randint(0, 342, (3, 20))).to(DEV), torch.from_numpy(rs.rand(3, 24).astype(np.float32)).to(DEV)
    g = torch.Generator().manual_seed(5)
    return x, c, (torch.randn(3, 4, 32, generator=g), torch.randn(3, 4, 32, generator=g))


def test_sweep_to_notes_to_files_and_back(tmp_path):
    """fader_sweep of the small model, 3 samples x 4 values x 64 steps, sampled so that notes sound: tokens_to_notes equals statement 1 per row;
    write_midis -> read_midi gives the same notes; the tokens controllability returns go the same way"""
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    x, c, eps = _sweep_inputs()
    values = np.array([-1.0, -0.25, 0.5, 1.25], np.float32)
    kw = dict(sample=dict(temperature=1.0, seed=3))
    tok, _ = pkg.fader_sweep(m, x, c, values, steps=64, which="r", eps=eps, **kw)
    ctl = pkg.controllability(m, x, c, "r", -1.0, 2.0, 0.19, 1.4, steps=64, n_values=4, eps=eps, **kw)
    assert tok.shape == (3, 4, 64) and torch.equal(ctl["tokens"], tok)          # min + k * (max - min) / 4: the same four values
    for t, sub in ((tok, "sweep"), (ctl["tokens"], "controllability")):
        res = pkg.tokens_to_notes(t)
        assert res.notes.shape == (3, 4, 64, 4) and res.notes.is_cuda and res.status.shape == (3, 4)
        host, sounding = t.reshape(12, 64).cpu().numpy(), 0
        for r in range(12):
            ref = hn.notes_of(host[r], hn.DEFAULT)
            hn.same({k: getattr(res, k).reshape((12,) + getattr(res, k).shape[2:])[r].cpu().numpy() for k in hn.NOTE_KEYS},
                    {k: np.asarray(ref[k], np.int32) for k in hn.NOTE_KEYS}, hn.NOTE_KEYS, "%s row %d" % (sub, r))
            sounding += ref["n_notes"] > 0
        assert sounding >= 6                                                   # a sampled decode of 64 tokens sounds notes
        paths = pkg.write_midis(str(tmp_path / sub), t)
        assert len(paths) == 12
        for r, path in enumerate(paths):
            n = int(res.n_notes.reshape(-1)[r])
            assert torch.equal(pkg.read_midi(path).notes, res.notes.reshape(12, 64, 4)[r, :n].cpu()), (sub, r)


def test_midi_segments_on_the_device_equals_the_stand_ins(tmp_path):
    pkg = load_package()
    path = str(tmp_path / "piece.mid")
    pkg.write_midi(path, hn.piece())
    midi = pkg.read_midi(path)
    for kw in (dict(max_tokens=20), dict(max_tokens=100, labels=True), dict(beats_per_segment=6)):
        ref = pkg.midi_segments(midi, ops=hn.notes_fake_ops(), **kw)
        got = pkg.midi_segments(midi, device=DEV, **kw)
        assert sorted(got) == sorted(ref)
        for k, v in ref.items():
            assert got[k].is_cuda and got[k].dtype == v.dtype and got[k].shape == v.shape, k
            if k == "chroma":
                assert float((got[k].cpu() - v).abs().max()) <= 1e-12           # the same integer histogram; fp64 products of 12 terms
            else:
                assert torch.equal(got[k].cpu(), v), k
    assert pkg.midi_segments(midi)["tokens"].is_cuda                           # without ops or device the work goes to the GPU
