"""Time what per-base signal positions (-moves) cost (needs an MI355X).

1. Assembly, on tools/bench_assembly.py's workload (the same seeded groups), alternating in one process:
     device_p : frontend.assemble_reads(reads, device=0, positions=ps): packing bases and positions, the pinned
                H2D copies, nd_assemble_reads_p, the D2H copies and the decode to (sequence, positions)
     device   : frontend.assemble_reads(reads, device=0), the call without positions (nd_assemble_reads), the
                baseline: this path is the one the parent commit has
     host_p   : [frontend.assemble_read_p(p, q) for p, q in zip(reads, ps)], the host function with positions
   Sequences and positions must be equal.  Host clock around whole calls, medians, µs per chunk.
2. The headline greedy call (bench.py's configs[1]: 256 chunks of 512 samples, max_length 100, min_length 57,
   three calls in flight, and one call alone) as the Translator issues it with moves, return_attn=True followed
   by nd_token_positions on the call's stream, against the call as it is without (the baseline); device events
   around batches of calls, alternated rounds, medians, ms per call.

Writes profiles/moves.json.

  python tools/bench_moves.py [--reps 5] [--calls 18] [--rounds 3] [--out profiles/moves.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanodecoder_amd import frontend, synth  # noqa: E402
from nanodecoder_amd.engine import Engine, EnginePool  # noqa: E402
from tools.bench_assembly import CHUNK_BASES, GROUPS, LENGTH, STRIDE, make_read  # noqa: E402
from tools.bench_quality import timed  # noqa: E402


def positions_for(reads, seed=7):
    """Chunk-relative positions as a decoder gives them: non-decreasing inside a chunk, below the window."""
    rng = np.random.default_rng(seed)
    return [[np.sort(rng.integers(0, LENGTH, len(x[0].replace(" ", "")))).astype(np.int32) for x in p] for p in reads]


def same(got, exp):
    return len(got) == len(exp) and all(g[0] == e[0] and np.array_equal(g[1], e[1]) for g, e in zip(got, exp))


def assembly(args):
    rows = []
    warm = [make_read(np.random.default_rng(0), 4, 30)]
    frontend.assemble_reads(warm, LENGTH, STRIDE, device=0, positions=positions_for(warm))  # library, allocators
    for bases in CHUNK_BASES:
        for n_reads, n_chunks in GROUPS:
            rng = np.random.default_rng(1000 * bases + n_reads)
            reads = [make_read(rng, n_chunks, bases) for _ in range(n_reads)]
            ps = positions_for(reads)
            C = n_reads * n_chunks
            frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, positions=ps)  # this shape's first calls
            frontend.assemble_reads(reads, LENGTH, STRIDE, device=0)
            host_s, p_s, d_s = [], [], []
            for rep in range(max(args.reps, args.host_reps)):  # alternated in one process
                if rep < args.host_reps:
                    t = time.perf_counter()
                    exp = [frontend.assemble_read_p(p, q, LENGTH, STRIDE) for p, q in zip(reads, ps)]
                    host_s.append(time.perf_counter() - t)
                if rep < args.reps:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    got = frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, positions=ps)
                    p_s.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    plain = frontend.assemble_reads(reads, LENGTH, STRIDE, device=0)
                    d_s.append(time.perf_counter() - t)
            assert same(got, exp), f"device and host differ ({bases} bases, {C} chunks)"
            assert plain == [e[0] for e in exp]
            h, q, d = (float(np.median(x)) * 1e6 / C for x in (host_s, p_s, d_s))
            rows.append(dict(chunk_bases=bases, reads=n_reads, chunks=C, bases_out=sum(len(e[0]) for e in exp),
                             host_p_us_per_chunk=h, device_p_us_per_chunk=q, device_us_per_chunk=d,
                             host_p_s_all=host_s, device_p_s_all=p_s, device_s_all=d_s))
            print(f"{bases:4d} bases x {C:5d} chunks: host with positions {h:8.1f}, device with {q:6.2f}, "
                  f"device without {d:6.2f} us/chunk, values equal", flush=True)
    return rows


def greedy(args):
    B, T, S, MIN = 256, 512, 100, 57
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=11, eos_bias=-3.0)
    sig = torch.from_numpy(synth.synth_chunk_batch(B, T, seed=1000, inject_masks=False)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    out = {}
    for lanes in (1, 3):
        eng = Engine(cfg, W, device=0, max_batch=B, max_steps=S) if lanes == 1 else \
            EnginePool(cfg, W, device=0, lanes=lanes, max_batch=B, max_steps=S)

        def plain():
            return eng.translate_greedy(sig, lens, lens, max_len=S, min_len=MIN)

        def with_moves():
            r = eng.translate_greedy(sig, lens, lens, max_len=S, min_len=MIN, return_attn=True)
            r["positions"] = eng.token_positions(r["attn"], lens, **({"lane": r["lane"]} if lanes > 1 else {}))
            r["attn"] = None
            return r

        def run(fn):
            if lanes == 1:
                return timed(fn, args.calls)

            def batch():
                rs = [fn() for _ in range(lanes)]
                eng.synchronize()
                return rs
            return timed(batch, max(1, args.calls // lanes)) / lanes

        for fn in (plain, with_moves):  # warm-up: workspaces, graphs
            for _ in range(2 * lanes):
                fn()
        if lanes > 1:
            eng.synchronize()
        torch.cuda.synchronize()
        p_ms, m_ms = [], []
        for _ in range(args.rounds):  # alternated in one process
            p_ms.append(run(plain))
            m_ms.append(run(with_moves))
        p, m = float(np.median(p_ms)), float(np.median(m_ms))
        key = "pool3" if lanes > 1 else "single"
        out[key] = dict(plain_ms=p, with_moves_ms=m, plain_ms_all=p_ms, with_moves_ms_all=m_ms, ratio=m / p)
        print(f"greedy {key}: {p:.3f} ms / call without, {m:.3f} ms / call with return_attn + token positions "
              f"({(m / p - 1) * 100:+.1f} %)", flush=True)
        eng.close()
    return dict(shape=dict(B=B, T=T, max_length=S, min_length=MIN), calls=args.calls, rounds=args.rounds, modes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed device assembly calls per group")
    ap.add_argument("--host-reps", type=int, default=1, help="timed host passes per group")
    ap.add_argument("--calls", type=int, default=18, help="greedy calls per timed batch")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moves.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moves.py needs a GPU")
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps,
               windowing=dict(src_seq_length=LENGTH, src_seq_stride=STRIDE),
               timing="assembly: host clock around whole calls (packing, H2D, kernels, D2H, decoding; each ends in "
                      "a device synchronise), medians; greedy: device events around batches of calls, medians "
                      "of alternated rounds.  device_us_per_chunk and plain_ms are the baselines: the paths as "
                      "they are without positions",
               assembly=assembly(args), greedy=greedy(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
