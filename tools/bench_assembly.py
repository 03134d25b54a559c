"""Time read assembly on the host against the device path (needs an MI355X).

Seeded synthetic groups: every read is a run of overlapping noisy windows of
one random truth (80 % overlap, 7 % substitutions, 2 % deletions), at about
30, 90 and 190 bases per chunk, in groups of several hundred and several
thousand chunks.  Per group, alternating in one process:
  host   : [frontend.assemble_read(p) for p in reads]  (difflib + the Python vote loop)
  device : frontend.assemble_reads(reads, device=0): packing, the pinned H2D copies,
           nd_assemble_reads, the D2H copies and the decode to str, by the host
           clock (the call ends in a device synchronise)
The strings must be equal.  Writes µs per chunk for both to profiles/assembly.json.

  python tools/bench_assembly.py [--reps 5] [--host-reps 2] [--out profiles/assembly.json]
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

from nanodecoder_amd import frontend  # noqa: E402

LENGTH, STRIDE = 300, 60  # the overlapping production windowing (any stride < length takes the voting branch)
GROUPS = [(8, 50), (16, 200)]  # (reads, chunks per read): 400 and 3200 chunks
CHUNK_BASES = [30, 90, 190]


def make_read(rng, n_chunks, bases):
    """all_predictions of one read: windows of ``bases`` bases every bases / 5 of a random truth."""
    step = max(1, bases // 5)
    truth = rng.integers(0, 4, n_chunks * step + bases)
    preds = []
    for i in range(n_chunks):
        w = truth[i * step: i * step + bases].copy()
        sub = rng.random(w.size) < 0.07
        w[sub] = rng.integers(0, 4, int(sub.sum()))
        w = w[rng.random(w.size) >= 0.02]
        preds.append([" ".join("ACGT"[b] for b in w)])
    return preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed device calls per group")
    ap.add_argument("--host-reps", type=int, default=2, help="timed host passes per group")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assembly.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_assembly.py needs a GPU: the device path has no host stand-in")
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps,
               windowing=dict(src_seq_length=LENGTH, src_seq_stride=STRIDE),
               timing="host clock around whole calls; the device call includes packing, H2D, kernels, D2H and "
                      "decoding and ends in a device synchronise; medians", groups=[])
    warm = [make_read(np.random.default_rng(0), 4, 30)]
    frontend.assemble_reads(warm, LENGTH, STRIDE, device=0)  # load the library, warm the allocators
    for bases in CHUNK_BASES:
        for n_reads, n_chunks in GROUPS:
            rng = np.random.default_rng(1000 * bases + n_reads)
            reads = [make_read(rng, n_chunks, bases) for _ in range(n_reads)]
            C = n_reads * n_chunks
            frontend.assemble_reads(reads, LENGTH, STRIDE, device=0)  # this shape's first call
            host_s, dev_s, pack_s = [], [], []
            for rep in range(max(args.reps, args.host_reps)):  # alternated in one process
                if rep < args.host_reps:
                    t = time.perf_counter()
                    exp = [frontend.assemble_read(p, LENGTH, STRIDE) for p in reads]
                    host_s.append(time.perf_counter() - t)
                if rep < args.reps:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    stats = {}
                    got = frontend.assemble_reads(reads, LENGTH, STRIDE, device=0, stats=stats)
                    dev_s.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    frontend.pack_assembly_input(reads)
                    pack_s.append(time.perf_counter() - t)
            assert got == exp, f"device and host strings differ ({bases} bases, {C} chunks)"
            assert stats["fallback"] == 0, "a read fell back to the host: the device figure would include it"
            h, d, p = (float(np.median(x)) * 1e6 / C for x in (host_s, dev_s, pack_s))
            row = dict(chunk_bases=bases, reads=n_reads, chunks=C, bases_out=sum(len(s) for s in exp),
                       host_us_per_chunk=h, device_us_per_chunk=d, device_pack_us_per_chunk=p, speedup=h / d,
                       host_s_all=host_s, device_s_all=dev_s)
            res["groups"].append(row)
            print(f"{bases:4d} bases x {C:5d} chunks: host {h:8.1f} us/chunk, device {d:7.2f} us/chunk "
                  f"(packing {p:.2f}), {h / d:.1f}x, strings equal", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
