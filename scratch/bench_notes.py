"""One measured time per kernel of csrc/notes.hip (profiles/notes.txt): fn_notes_from_tokens on 2048 rows x 100 steps of seeded random
event tokens, fn_tokens_from_notes on 2048 spans of 32 notes into 100 and into 256 columns.  Device events around 2000 back-to-back launches through the
kernel table (no allocation, no copy), 7 windows, the launches alternated; the first 64 rows of each are compared with tests/helpers_notes.py."""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import helpers_attributes as ha
import helpers_notes as hn
from mfn_import import load_package
load_package()
from music_fader_nets_amd.hipops import HipOps

DEV = "cuda:0"
ops = HipOps(DEV)
rs = np.random.RandomState(1)
ROWS = 2048
tok_np = np.stack([ha.random_row(rs, ha.DEFAULT, 100, i % 2 == 1) for i in range(ROWS)]).astype(np.int32)
tok = torch.from_numpy(tok_np).to(DEV)
prm = torch.from_numpy(hn.params_bytes(hn.DEFAULT)).to(DEV)
i32 = dict(dtype=torch.int32, device=DEV)
notes = torch.empty(ROWS, 100, 4, **i32)
o1 = [torch.empty(ROWS, **i32) for _ in range(3)]
n = 32
t0 = np.sort(rs.randint(0, 400, (ROWS, n)) // 5 * 5, axis=1)
flat = np.stack([t0, t0 + rs.randint(5, 120, (ROWS, n)), rs.randint(20, 70, (ROWS, n)), rs.randint(40, 110, (ROWS, n))], 2).astype(np.int32).reshape(-1, 4)
spans_np = np.stack([np.arange(ROWS) * n, np.full(ROWS, n), np.zeros(ROWS), np.full(ROWS, 400)], 1).astype(np.int32)
fl, sp = torch.from_numpy(flat).to(DEV), torch.from_numpy(spans_np).to(DEV)
out_tok = torch.empty(ROWS, 100, **i32)
o2 = [torch.empty(ROWS, **i32) for _ in range(3)]
a = lambda: ops.notes_from_tokens(tok, 100, prm, notes, *o1)
b = lambda: ops.tokens_from_notes(fl, sp, prm, out_tok, 100, *o2)
out_tok256 = torch.empty(ROWS, 256, **i32)
o3 = [torch.empty(ROWS, **i32) for _ in range(3)]
c = lambda: ops.tokens_from_notes(fl, sp, prm, out_tok256, 256, *o3)


def window(f, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / launches


lines = ["device %s, %d rows; us per launch, device events around 2000 back-to-back launches, 7 windows, the three launches alternated" % (torch.cuda.get_device_name(0), ROWS)]
for f in (a, b, c):
    for _ in range(50):
        f()
torch.cuda.synchronize()
res = {"a": [], "b": [], "c": []}
for _ in range(7):
    res["a"].append(window(a, 2000)), res["b"].append(window(b, 2000)), res["c"].append(window(c, 2000))
for k, name in (("a", "fn_notes_from_tokens  2048 rows x 100 steps, notes_ld 100"), ("b", "fn_tokens_from_notes  2048 spans of 32 notes, 100 steps  "),
                ("c", "fn_tokens_from_notes  2048 spans of 32 notes, 256 steps  ")):
    v = np.array(res[k])
    lines.append("%s   median %7.2f  min %7.2f  max %7.2f" % (name, np.median(v), v.min(), v.max()))
ref1 = hn.notes_from_tokens_ref(tok_np[:64], 100, hn.DEFAULT, 100)
ref2 = hn.tokens_from_notes_ref(flat, spans_np[:64], 100, hn.DEFAULT)
same = bool(np.array_equal(notes[:64].cpu().numpy(), ref1["notes"]) and np.array_equal(out_tok[:64].cpu().numpy(), ref2["tokens"]))
lines.append("median notes per row %d; median tokens per span %d, spans that overflow 100 steps %d of %d, 256 steps %d; first 64 rows of each equal the restatement: %s" % (
    int(o1[0].median()), int(o2[0].median()), int((o2[2] == hn.OVERFLOW).sum()), ROWS, int((o3[2] == hn.OVERFLOW).sum()), same))
print("\n".join(lines))
