"""Time K candidates per chunk on one encoder pass against the replicated call (needs an MI355X).

Shape: one a user would run: B = 32 chunks of T = 512 samples, K = 8 candidates of L = 48 positions each, so
N = 256 decoder sequences.  Form (a) is score_candidates on the 32 chunks; form (b) is score_targets on the
same 256 sequences with each chunk copied 8 times, the only way there was before.  The two alternate in one
process, timed with device events, medians over the rounds, warm-up first; split-fp16 products and exact
fp32, one engine.  Then each form's encode / decode split from nd_last_timing (a timed call runs the same
launches as two pieces).  Writes profiles/score_candidates.json and prints the rows for DESIGN.md section 1.8.

  python tools/bench_candidates.py [--calls 20] [--rounds 5] [--out profiles/score_candidates.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_score import timed  # noqa: E402
from nanodecoder_amd import synth  # noqa: E402
from nanodecoder_amd.engine import Engine  # noqa: E402

B, T, K, L = 32, 512, 8, 48


def inputs(cfg, seed=3):
    """The chunks and their candidates: slot 0 a random row of 40 bases, the other slots the same row with
    k substitutions and lengths 40 - k (an allele window's worth of variation), EOS behind each."""
    sig = torch.from_numpy(synth.synth_chunk_batch(B, T, seed=seed)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    rng = np.random.default_rng(seed)
    cand = np.full((B, K, L), cfg.pad_idx, np.int32)
    cand_len = np.zeros((B, K), np.int32)
    for b in range(B):
        base = rng.integers(4, cfg.vocab, 40)
        for k in range(K):
            row = base[: 40 - k].copy()
            row[rng.integers(0, len(row), k)] = rng.integers(4, cfg.vocab, k)
            cand[b, k, : len(row)] = row
            cand[b, k, len(row)] = cfg.eos_idx
            cand_len[b, k] = len(row) + 1
    return sig, lens, torch.from_numpy(cand).cuda(), torch.from_numpy(cand_len).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_candidates.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_candidates.py needs a GPU: nothing is measured without one")
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=1)
    sig, lens, cand, cand_len = inputs(cfg)
    rep = torch.arange(B).repeat_interleave(K).cuda()
    sig_r, lens_r = sig[rep].contiguous(), lens[rep].contiguous()
    gold_r, gold_len_r = cand.view(B * K, L), cand_len.view(B * K)
    res = dict(shape=dict(B=B, T=T, K=K, L=L, N=B * K), calls=args.calls, rounds=args.rounds,
               device=torch.cuda.get_device_name(0), modes={})
    eng = Engine(cfg, W, device=0, max_batch=B * K, max_steps=L)
    for exact in (False, True):
        eng.set_exact_fp32(exact)

        def shared():
            return eng.score_candidates(sig, lens, lens, cand=cand, cand_len=cand_len)

        def replicated():
            return eng.score_targets(sig_r, lens_r, lens_r, gold=gold_r, gold_len=gold_len_r)

        for fn in (shared, replicated):  # warm-up: workspaces, graphs
            for _ in range(2):
                r = fn()
        torch.cuda.synchronize()
        diff = float((shared()["scores"].view(-1) - replicated()["scores"]).abs().max())
        a_ms, b_ms = [], []
        for _ in range(args.rounds):  # alternated in one process
            a_ms.append(timed(shared, args.calls))
            b_ms.append(timed(replicated, args.calls))
        # the split: a timed call is the same launches as two pieces, an event between them
        eng.set_timing(True)
        split = {}
        for name, fn in (("shared", shared), ("replicated", replicated)):
            fn()  # the two pieces' own graphs
            ts = []
            for _ in range(args.calls):
                fn()
                ts.append(eng.last_timing())
            split[name] = [float(np.median([t[i] for t in ts])) for i in (0, 1)]
        eng.set_timing(False)
        key = "single_exact" if exact else "single_split"
        a, b = float(np.median(a_ms)), float(np.median(b_ms))
        (ae, ad), (be, bd) = split["shared"], split["replicated"]
        res["modes"][key] = dict(candidates_ms=a, replicated_ms=b, candidates_ms_all=a_ms, replicated_ms_all=b_ms,
                                 saved_ms=b - a, speedup=b / a, candidates_encode_ms=ae, candidates_decode_ms=ad,
                                 replicated_encode_ms=be, replicated_decode_ms=bd, encode_saved_ms=be - ae,
                                 max_score_diff=diff)
        print(f"{key}: candidates {a:.3f} ms / call (encode {ae:.3f} + decode {ad:.3f}), replicated {b:.3f} ms "
              f"(encode {be:.3f} + decode {bd:.3f}): {b / a:.2f}x, {b - a:.3f} ms saved against {be - ae:.3f} ms of "
              f"encoder and context K/V no longer run; max |score difference| {diff:.2e}", flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
