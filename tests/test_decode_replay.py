"""CPU self-test of helpers.replay_decode_check, the every-step check of greedy decodes against an fp64 replay of their own tokens.

The fp32 oracle's greedy decode stands in for a kernel: the checker must accept it, reject each of three corruptions of it, and the
inputs of the GPU replay cases (helpers.REPLAY_CASES) must stay under its 2 % near-tie cap (sampled rows of every case)."""
import numpy as np
import pytest
import torch

from helpers import (REPLAY_CASES, REPLAY_CAP, REPLAY_GRAPH_PATHS, replay_decode_check, replay_inputs, replay_line, replay_rows,
                     replay_z)
from oracle import gmvae_oracle as orc


@pytest.fixture(scope="module")
def clean():
    """the fp32 oracle's greedy decode of 24 rows x 300 steps on the seeded H = 64 inputs, and the checker's figures for it"""
    H, Z, sd = replay_inputs("h64")
    z = replay_z(24, Z, 5)
    lp, tk = orc.greedy_decode(sd, z, 300)
    st = replay_decode_check(sd, z, tk, lp)
    return sd, z, tk, lp, st


def test_replay_accepts_the_clean_decode(clean):
    sd, z, tk, lp, st = clean
    assert st["rows"] == 24 and st["positions"] == 24 * 300
    assert st["ratio"] == pytest.approx(1.0)                     # the stand-in IS the fp32 restatement
    assert 0 < st["e_ref"] and st["tol_lp"] == min(1e-4, 16 * st["e_ref"]) and st["delta"] == 2 * st["tol_lp"]
    st2 = replay_decode_check(sd, z, tk)                          # tokens only
    assert st2["share_below_delta"] == st["share_below_delta"]


def test_replay_rejects_a_late_token_off_the_best(clean):
    """one token at step >= 250 replaced by one whose fp64 gap to the best exceeds delta (chosen above 2e-4 >= any delta)"""
    sd, z, tk, lp, st = clean
    r, s = 7, 263
    lp64 = orc.global_decoder({k: v.double() for k, v in sd.items()}, z[r:r + 1].double(), s + 1, teacher=tk[r:r + 1])[0, s]
    short = lp64.max() - lp64
    cand = torch.nonzero(short > 2e-4).flatten()
    v = int(cand[short[cand].argmin()])                           # the closest token that is still clearly not the best
    bad = tk.clone()
    bad[r, s] = v
    with pytest.raises(AssertionError, match=r"\(c\)"):
        replay_decode_check(sd, z, bad)
    with pytest.raises(AssertionError, match=r"\((a|b)\)"):
        replay_decode_check(sd, z, bad, lp)


def test_replay_rejects_one_moved_log_prob(clean):
    """one log-prob entry at a late step moved by 5 tol_lp (a non-argmax entry moved down: the tokens stay right)"""
    sd, z, tk, lp, st = clean
    r, s = 19, 287
    v = int(lp[r, s].argmin())
    bad = lp.clone()
    bad[r, s, v] -= 5 * st["tol_lp"]
    with pytest.raises(AssertionError, match=r"\(a\)"):
        replay_decode_check(sd, z, tk, bad)


def test_replay_rejects_two_swapped_token_streams(clean):
    """the token streams of two rows swapped from step 150 on"""
    sd, z, tk, lp, st = clean
    bad = tk.clone()
    bad[[3, 16], 150:] = tk[[16, 3], 150:]
    assert not torch.equal(bad, tk)
    with pytest.raises(AssertionError, match=r"\(c\)"):
        replay_decode_check(sd, z, bad)
    with pytest.raises(AssertionError, match=r"\((a|b)\)"):
        replay_decode_check(sd, z, bad, lp)


def test_replay_rows_cover_every_block_edge():
    for Bi in (1, 256, 257, 353, 705, 1500, 2048):
        rows = replay_rows(Bi)
        assert len(rows) == min(Bi, 256) and len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() == Bi - 1
        for r0 in range(0, Bi, 32):
            assert r0 in rows and min(r0 + 32, Bi) - 1 in rows
        assert np.array_equal(rows, replay_rows(Bi))


def test_replay_cases_stay_under_the_near_tie_cap():
    """the GPU replay cases' inputs (weights, latent rows, step counts; both latent batches of the graph paths), 8 sampled rows each,
    decoded by the fp32 oracle: every sample passes the checker, whose cap is at most 2 % of the positions below delta"""
    inputs, pooled = {}, {}
    for path, weights, Bi, steps in REPLAY_CASES:
        if weights not in inputs:
            inputs[weights] = replay_inputs(weights)
        H, Z, sd = inputs[weights]
        for seed in ((Bi, Bi + 1) if path in REPLAY_GRAPH_PATHS else (Bi,)):
            z = replay_z(Bi, Z, seed)
            rows = np.sort(np.random.RandomState(seed).choice(Bi, min(Bi, 8), replace=False))
            lp, tk = orc.greedy_decode(sd, z[rows], steps)
            st = replay_decode_check(sd, z[rows], tk, lp)
            n = pooled.setdefault(weights, [0.0, 0])
            n[0] += st["share_below_delta"] * st["positions"]
            n[1] += st["positions"]
            print(replay_line("%s seed %d (oracle)" % (path, seed), H, st))
    for weights, (below, total) in pooled.items():
        assert below / total <= REPLAY_CAP, (weights, below / total)
