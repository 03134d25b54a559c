"""Time the scoring call with and without its attention output (needs an MI355X).

Shape: configs[1] of bench.py with targets of L = 100 positions, as tools/bench_score.py: B = 256 chunks of
T = 512 samples.  score_targets() and score_targets(return_attn=True) alternate in one process, timed with
device events, medians over the rounds; then nd_token_positions on the attention the call returned, alone.
Split-fp16 products and exact fp32, one engine.  The untapped figure is set beside the one recorded in
profiles/score_targets.json (the same kernels: the tap is an instantiation of its own).  Writes
profiles/score_align.json and prints the rows for DESIGN.md section 1.7.

  python tools/bench_align.py [--calls 20] [--rounds 5] [--out profiles/score_align.json]
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

from bench_score import B, L, T, inputs, timed  # noqa: E402
from nanodecoder_amd import synth  # noqa: E402
from nanodecoder_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_align.json"))
    ap.add_argument("--baseline", default=os.path.join(ROOT, "profiles", "score_targets.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_align.py needs a GPU: nothing is measured without one")
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=1)
    sig, lens, gold, gold_len = inputs(cfg)
    base = {}
    if os.path.exists(args.baseline):
        with open(args.baseline) as f:
            base = json.load(f).get("modes", {})
    res = dict(shape=dict(B=B, T=T, L=L), calls=args.calls, rounds=args.rounds, tap_bytes=B * L * T * 4,
               device=torch.cuda.get_device_name(0), modes={})
    eng = Engine(cfg, W, device=0, max_batch=B, max_steps=L)
    for exact in (False, True):
        eng.set_exact_fp32(exact)

        def plain():
            return eng.score_targets(sig, lens, lens, gold=gold, gold_len=gold_len)

        def tapped():
            return eng.score_targets(sig, lens, lens, gold=gold, gold_len=gold_len, return_attn=True)

        for fn in (plain, tapped):  # warm-up: workspaces, graphs
            for _ in range(2):
                r = fn()
        attn = r["attn"]
        eng.token_positions(attn, lens)
        torch.cuda.synchronize()
        p_ms, t_ms, pos_ms = [], [], []
        for _ in range(args.rounds):  # alternated in one process
            p_ms.append(timed(plain, args.calls))
            t_ms.append(timed(tapped, args.calls))
            pos_ms.append(timed(lambda: eng.token_positions(attn, lens), args.calls))
        key = "single_exact" if exact else "single_split"
        p, t, ps = float(np.median(p_ms)), float(np.median(t_ms)), float(np.median(pos_ms))
        m = dict(score_ms=p, score_attn_ms=t, positions_ms=ps, score_ms_all=p_ms, score_attn_ms_all=t_ms,
                 positions_ms_all=pos_ms, attn_cost_ms=t - p, attn_cost_rel=t / p - 1.0)
        if key in base:
            m["recorded_score_ms"] = base[key]["score_ms"]
            m["score_vs_recorded"] = p / base[key]["score_ms"] - 1.0
        res["modes"][key] = m
        line = (f"{key}: score {p:.3f} ms / call, with attention {t:.3f} ms ({100 * m['attn_cost_rel']:+.1f} %), "
                f"token positions {ps:.3f} ms")
        if key in base:
            line += f"; untapped against the recorded {m['recorded_score_ms']:.3f} ms: " \
                    f"{100 * m['score_vs_recorded']:+.1f} %"
        print(line, flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
