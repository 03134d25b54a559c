"""Time nd_score_targets against the step-wise decoder (needs an MI355X).

Shape: configs[1] of bench.py: B = 256 chunks of T = 512 samples, targets of L = 100 positions (99 bases and
EOS).  A scoring call and a translate_greedy call of the same shape (what forcing the tokens through the
step-wise decoder would cost: the only baseline there is) alternate in one process, timed with device
events; one engine, then a pool of 3 lanes; split-fp16 products and exact fp32.  Writes
profiles/score_targets.json and prints the row for DESIGN.md section 0.

  python tools/bench_score.py [--calls 20] [--out profiles/score_targets.json]
  python tools/bench_score.py --trace      # a few scoring calls only (the program for rocprofv3 --kernel-trace)
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

from nanodecoder_amd import synth  # noqa: E402
from nanodecoder_amd.engine import Engine, EnginePool  # noqa: E402

B, T, L = 256, 512, 100


def decoder_flops(cfg, B, T, L):
    """Algorithmic FLOPs of the decoder rows of one scoring call, from the shapes (2 per multiply-add): the
    six projections and the FFN per row and layer, causal self-attention over (L + 1) / 2 keys on average,
    context attention over T keys; QK^T and PV each 2 * d per key."""
    d, F = cfg.d_model, cfg.d_ff
    proj = 2 * d * (3 * d + d + d + d) + 2 * 2 * d * F
    attn = 2 * 2 * d * ((L + 1) / 2 + T)
    return cfg.dec_layers * B * L * (proj + attn)


def inputs(cfg, seed=3):
    sig = torch.from_numpy(synth.synth_chunk_batch(B, T, seed=seed)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    rng = np.random.default_rng(seed)
    gold = rng.integers(4, cfg.vocab, (B, L)).astype(np.int32)
    gold[:, L - 1] = cfg.eos_idx
    return sig, lens, torch.from_numpy(gold).cuda(), torch.full((B,), L, dtype=torch.int32).cuda()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_targets.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--exact", action="store_true", help="--trace in exact fp32")
    args = ap.parse_args()
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=1)
    sig, lens, gold, gold_len = inputs(cfg)
    if args.trace:
        eng = Engine(cfg, W, device=0, max_batch=B, max_steps=L)
        eng.set_exact_fp32(args.exact)
        for _ in range(5):
            eng.score_targets(sig, lens, lens, gold=gold, gold_len=gold_len)
        torch.cuda.synchronize()
        eng.close()
        return
    res = dict(shape=dict(B=B, T=T, L=L), calls=args.calls, rounds=args.rounds,
               decoder_flops=decoder_flops(cfg, B, T, L), device=torch.cuda.get_device_name(0), modes={})
    for lanes in (1, 3):
        eng = Engine(cfg, W, device=0, max_batch=B, max_steps=L) if lanes == 1 else \
            EnginePool(cfg, W, device=0, lanes=3, max_batch=B, max_steps=L)
        for exact in (False, True):
            eng.set_exact_fp32(exact)

            def score():
                return eng.score_targets(sig, lens, lens, gold=gold, gold_len=gold_len)

            def greedy():
                return eng.translate_greedy(sig, lens, lens, max_len=L)

            def run(fn):
                if lanes == 1:
                    return timed(fn, args.calls)
                # a pool call does not join the caller's stream: the calls' last events bound the batch
                def batch():
                    rs = [fn() for _ in range(lanes)]
                    eng.synchronize()
                    return rs
                return timed(batch, max(1, args.calls // lanes)) / lanes

            for fn in (score, greedy):  # warm-up: workspaces, graphs
                for _ in range(2 * lanes):
                    fn()
            if lanes > 1:
                eng.synchronize()
            torch.cuda.synchronize()
            s_ms, g_ms = [], []
            for _ in range(args.rounds):  # alternated in one process
                s_ms.append(run(score))
                g_ms.append(run(greedy))
            key = f"{'pool3' if lanes > 1 else 'single'}_{'exact' if exact else 'split'}"
            s, g = float(np.median(s_ms)), float(np.median(g_ms))
            res["modes"][key] = dict(score_ms=s, greedy_ms=g, score_ms_all=s_ms, greedy_ms_all=g_ms, ratio=g / s,
                                     decoder_tflops=res["decoder_flops"] / (s * 1e-3) / 1e12)
            print(f"{key}: score {s:.3f} ms / call, greedy {g:.3f} ms / call, ratio {g / s:.2f}x, "
                  f"{res['modes'][key]['decoder_tflops']:.1f} TF/s over the whole call", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
