#!/usr/bin/env python3
"""Golden fixture of the reconstruction report (include/fadernets.h, fn_match_rows): ``report.npz``.

Runs ONLY in the build container.  The reference's own code is executed, not restated: ``acc`` is a function nested three levels deep in
``trainer_gmm.py`` (evaluation_phase -> run -> the batch loop, :545-565), whose module trains a model on import, so the FunctionDef is taken by AST
and compiled unmodified.  It is called the way :567-568 call it - ``acc(out, d, "d", trim=True)`` / ``acc(r_out, r, "r")`` - with ``a`` a (B, T, 342)
float tensor whose argmax along the last axis is the prediction and ``b`` the (B, T) integer targets.  B >= 2 and T >= 2 (upstream ``.squeeze()``s) and
no all-zero target row (upstream divides by zero there).

Arrays only.  Per case k of tests/helpers_report.golden_inputs(): c<k>/tag, c<k>/pred, c<k>/target (B, T) int64, c<k>/trim, c<k>/b_acc (the returned
sum of the per-sample accuracies, float64).
"""
import ast
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers_report as hr  # noqa: E402


def extract_nested(path, name, ns):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1, (path, name, len(found))
    exec(compile(ast.Module(body=found, type_ignores=[]), path + "[extract]", "exec"), ns)


def main():
    ns = dict(np=np, torch=torch)
    extract_nested("trainer_gmm.py", "acc", ns)
    out = {}
    for k, (tag, pred, target, trim) in enumerate(hr.golden_inputs()):
        B, T = pred.shape
        assert B >= 2 and T >= 2 and (target != 0).any(1).all()
        a = torch.zeros(B, T, 342)
        a.scatter_(2, torch.from_numpy(pred).unsqueeze(-1), 1.0)
        b_acc = ns["acc"](a, torch.from_numpy(target), "d", trim=trim)
        P = "c%d/" % k
        out[P + "tag"], out[P + "pred"], out[P + "target"], out[P + "trim"], out[P + "b_acc"] = np.array(tag), pred, target, np.array(trim), np.float64(b_acc)
    np.savez_compressed(os.path.join(HERE, "report.npz"), **out)
    print("wrote report.npz: %d cases, %d bytes" % (k + 1, os.path.getsize(os.path.join(HERE, "report.npz"))))


if __name__ == "__main__":
    main()
