"""Time what per-base methylation probabilities (-mod_probs) add to the -fastq path (needs an MI355X).

1. Assembly, on tools/bench_assembly.py's groups with M in the alphabet (ACGTM), alternating in one process:
     device_m : frontend.assemble_reads(reads, device=0, weights=ws, mod_weights=ms): packing bases and both
                weight arrays, the pinned H2D copies, nd_assemble_reads_m, the D2H copies and the decode to
                (sequence, quality string, ml)
     device_q : frontend.assemble_reads(reads, device=0, weights=ws), the -fastq call (nd_assemble_reads_q), the
                baseline: this path is the one the parent commit has
     host_m   : [frontend.assemble_read_m(p, w, m) for ...], the host function
   Sequences, qualities and ML bytes must be equal.  Host clock around whole calls, medians, µs per chunk.
2. The headline greedy call (bench.py's configs[1]: 256 chunks of 512 samples, max_length 100, min_length 57,
   three calls in flight, and one call alone) on a nine-token model, as the Translator issues it with
   mods=True, return_logp=True followed by nd_token_weights and nd_token_mod_weights on the call's stream,
   against the same call with nd_token_weights alone (qualities=True, the baseline); device events around
   batches of calls, alternated rounds, medians, ms per call.

Writes profiles/assembly_mods.json.

  python tools/bench_mods.py [--reps 5] [--calls 18] [--rounds 3] [--out profiles/assembly_mods.json]
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
from tools.bench_assembly import CHUNK_BASES, GROUPS, LENGTH, STRIDE  # noqa: E402
from tools.bench_quality import timed  # noqa: E402


def make_read(rng, n_chunks, bases):
    """tools/bench_assembly.py's make_read over the five letters ACGTM."""
    step = max(1, bases // 5)
    truth = rng.integers(0, 5, n_chunks * step + bases)
    preds = []
    for i in range(n_chunks):
        w = truth[i * step: i * step + bases].copy()
        sub = rng.random(w.size) < 0.07
        w[sub] = rng.integers(0, 5, int(sub.sum()))
        w = w[rng.random(w.size) >= 0.02]
        preds.append([" ".join("ACGTM"[b] for b in w)])
    return preds


def same(got, exp):
    return len(got) == len(exp) and all(g[:2] == e[:2] and g[2].tobytes() == e[2].tobytes() for g, e in zip(got, exp))


def assembly(args):
    rows = []
    warm = [make_read(np.random.default_rng(0), 4, 30)]
    nine = [[np.full(len(x[0].replace(" ", "")), 9, np.uint16) for x in warm[0]]]
    frontend.assemble_reads(warm, LENGTH, STRIDE, device=0, weights=nine, mod_weights=nine)  # load, warm up
    for bases in CHUNK_BASES:
        for n_reads, n_chunks in GROUPS:
            rng = np.random.default_rng(1000 * bases + n_reads)
            reads = [make_read(rng, n_chunks, bases) for _ in range(n_reads)]
            wrng = np.random.default_rng(7)
            ws = [[wrng.integers(0, 65536, len(x[0].replace(" ", ""))).astype(np.uint16) for x in p] for p in reads]
            ms = [[wrng.integers(0, 65536, len(x[0].replace(" ", ""))).astype(np.uint16) for x in p] for p in reads]
            C = n_reads * n_chunks
            frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, weights=ws, mod_weights=ms)  # first calls
            frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, weights=ws)
            host_s, m_s, q_s = [], [], []
            for rep in range(max(args.reps, args.host_reps)):  # alternated in one process
                if rep < args.host_reps:
                    t = time.perf_counter()
                    exp = [frontend.assemble_read_m(p, w, m, LENGTH, STRIDE) for p, w, m in zip(reads, ws, ms)]
                    host_s.append(time.perf_counter() - t)
                if rep < args.reps:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    got = frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, weights=ws, mod_weights=ms)
                    m_s.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    plain = frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, weights=ws)
                    q_s.append(time.perf_counter() - t)
            assert same(got, exp), f"device and host differ ({bases} bases, {C} chunks)"
            assert plain == [e[:2] for e in exp]
            h, m, q = (float(np.median(x)) * 1e6 / C for x in (host_s, m_s, q_s))
            sites = sum(sum(c in "CM" for c in e[0]) for e in exp)
            rows.append(dict(chunk_bases=bases, reads=n_reads, chunks=C, bases_out=sum(len(e[0]) for e in exp),
                             sites=sites, host_m_us_per_chunk=h, device_m_us_per_chunk=m, device_q_us_per_chunk=q,
                             host_m_s_all=host_s, device_m_s_all=m_s, device_q_s_all=q_s))
            print(f"{bases:4d} bases x {C:5d} chunks: host {h:8.1f}, device with ML {m:6.2f}, "
                  f"device with qualities only {q:6.2f} us/chunk, bytes equal, {sites} sites", flush=True)
    return rows


def greedy(args):
    B, T, S, MIN = 256, 512, 100, 57
    cfg = synth.ModelConfig(itos=list(synth.DEFAULT_ITOS) + ["M"])
    c_id, m_id = cfg.itos.index("C"), cfg.itos.index("M")
    W = synth.make_weights(cfg, seed=11, eos_bias=-3.0)
    sig = torch.from_numpy(synth.synth_chunk_batch(B, T, seed=1000, inject_masks=False)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    out = {}
    for lanes in (1, 3):
        eng = Engine(cfg, W, device=0, max_batch=B, max_steps=S) if lanes == 1 else \
            EnginePool(cfg, W, device=0, lanes=lanes, max_batch=B, max_steps=S)

        def with_weights():
            r = eng.translate_greedy(sig, lens, lens, max_len=S, min_len=MIN, return_logp=True)
            r["weights"] = eng.token_weights(r["tokens"], logp=r["logp"], **({"lane": r["lane"]} if lanes > 1 else {}))
            return r

        def with_mods():
            r = with_weights()
            r["mod_weights"] = eng.token_mod_weights(r["tokens"], r["logp"], c_id, m_id,
                                                     **({"lane": r["lane"]} if lanes > 1 else {}))
            return r

        def run(fn):
            if lanes == 1:
                return timed(fn, args.calls)

            def batch():
                rs = [fn() for _ in range(lanes)]
                eng.synchronize()
                return rs
            return timed(batch, max(1, args.calls // lanes)) / lanes

        for fn in (with_weights, with_mods):  # warm-up: workspaces, graphs
            for _ in range(2 * lanes):
                fn()
        if lanes > 1:
            eng.synchronize()
        torch.cuda.synchronize()
        q_ms, m_ms = [], []
        for _ in range(args.rounds):  # alternated in one process
            q_ms.append(run(with_weights))
            m_ms.append(run(with_mods))
        q, m = float(np.median(q_ms)), float(np.median(m_ms))
        key = "pool3" if lanes > 1 else "single"
        out[key] = dict(with_weights_ms=q, with_mods_ms=m, with_weights_ms_all=q_ms, with_mods_ms_all=m_ms, ratio=m / q)
        print(f"greedy {key}: {q:.3f} ms / call with token weights, {m:.3f} ms / call with modification weights too "
              f"({(m / q - 1) * 100:+.2f} %)", flush=True)
        eng.close()
    return dict(shape=dict(B=B, T=T, max_length=S, min_length=MIN, vocab=cfg.vocab), calls=args.calls,
                rounds=args.rounds, modes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed device assembly calls per group")
    ap.add_argument("--host-reps", type=int, default=1, help="timed host passes per group")
    ap.add_argument("--calls", type=int, default=18, help="greedy calls per timed batch")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assembly_mods.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mods.py needs a GPU")
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps,
               windowing=dict(src_seq_length=LENGTH, src_seq_stride=STRIDE),
               timing="assembly: host clock around whole calls (packing, H2D, kernels, D2H, decoding; each ends in "
                      "a device synchronise), medians; greedy: device events around batches of calls, medians "
                      "of alternated rounds.  device_q_us_per_chunk and with_weights_ms are the baselines: the "
                      "-fastq paths of the same build, without modification weights",
               assembly=assembly(args), greedy=greedy(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
