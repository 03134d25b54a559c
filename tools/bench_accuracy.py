"""Time the alignment of called reads to their known sequences: the device call against the host rule (needs an
MI355X).

Input, from a fixed seed: 64 pairs, each truth 4000 random ACGT bases, each call its truth with 10 % errors, equal
parts substitution, insertion and deletion.  Measured in one process:
  kernels : nd_align_seqs alone on inputs already on the device (the offsets launch and the alignment launch),
            between two device events; one warm-up call, then the median of --reps calls
  device  : accuracy.align_reads(calls, truths, device=0, want_ops=True): packing, the H2D copies, the call, the
            D2H copies, by the host clock (the call ends in a device synchronise); median of --reps
  host    : accuracy.align_reads(calls, truths, want_ops=True), the numpy rule pair by pair; --host-reps passes
Counts and ops of the two must be equal.  The kernels' LDS and VGPR use come from the build's objects
(tools/kernel_meta.py); where the objects are not at hand (a machine that received the built library only), run
`python tools/bench_accuracy.py --meta-only` where the library was built: it adds them to the file.

  python tools/bench_accuracy.py [--reps 7] [--host-reps 1] [--out profiles/accuracy.json]
"""
from __future__ import annotations

import argparse
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nanodecoder_amd import accuracy  # noqa: E402

PAIRS, TRUTH_BASES, ERROR_RATE, SEED = 64, 4000, 0.10, 20261020


def make_pairs():
    rng = np.random.default_rng(SEED)
    calls, truths = [], []
    for _ in range(PAIRS):
        t = rng.integers(0, 4, TRUTH_BASES)
        x = rng.random(TRUTH_BASES)
        out = []
        for b, u in zip(t.tolist(), x.tolist()):
            if u < ERROR_RATE / 3:
                out.append((b + 1 + int(rng.integers(0, 3))) % 4)  # another base
            elif u < 2 * ERROR_RATE / 3:
                out += [b, int(rng.integers(0, 4))]                # an inserted base behind it
            elif u >= ERROR_RATE:
                out.append(b)                                      # (else: deleted)
        calls.append("".join("ACGT"[b] for b in out))
        truths.append("".join("ACGT"[b] for b in t))
    return calls, truths


def kernel_meta_rows():
    """LDS and VGPR use of align.hip's kernels from the build's objects; None without them."""
    import kernel_meta
    if not glob.glob(os.path.join(kernel_meta.BUILD, "align.o")):
        return None
    rows = [r for r in kernel_meta.collect() if r["object"] == "align.o"]
    return [dict(kernel=r["name"].split("(")[0], lds_bytes=r.get("lds", 0), vgpr=r.get("vgpr", 0),
                 agpr=r.get("agpr", 0), vgpr_spill=r.get("vgpr_spill", 0), scratch_bytes=r.get("private", 0))
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed device calls (at least 5)")
    ap.add_argument("--host-reps", type=int, default=1, help="timed host passes")
    ap.add_argument("--meta-only", action="store_true", help="only add the kernels' LDS / VGPR use to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuracy.json"))
    args = ap.parse_args()
    if args.meta_only:
        with open(args.out) as f:
            res = json.load(f)
        res["kernels"] = kernel_meta_rows()
        if res["kernels"] is None:
            sys.exit("no build objects here: build the library first")
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print("added the kernels' metadata to", args.out)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_accuracy.py needs a GPU: the device path has no host stand-in")
    from nanodecoder_amd import _lib
    reps = max(5, args.reps)
    calls, truths = make_pairs()
    call, call_off, truth, truth_off, cells = accuracy.pack_align_input(calls, truths)
    accuracy.align_reads(calls[:2], truths[:2], device=0, want_ops=True)  # load the library, warm the allocators
    # ---- the call alone, inputs on the device, device events
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    P = PAIRS
    work_bytes = int(L.nd_align_seqs_work_bytes(P, cells))
    off_d = torch.from_numpy(np.concatenate([call_off, truth_off])).to(dev)
    call_d, truth_d = torch.from_numpy(call.copy()).to(dev), torch.from_numpy(truth.copy()).to(dev)
    out_d = torch.empty(P * 6, dtype=torch.int32, device=dev)
    ops_d = torch.empty(call.size, dtype=torch.uint8, device=dev)
    work_d = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def enqueue():
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.nd_align_seqs(p(call_d), p(off_d), p(truth_d), p(off_d[P + 1:]), P, cells, p(out_d), p(ops_d),
                                   p(out_d[5 * P:]), p(work_d), work_bytes, stream), "nd_align_seqs")
    enqueue()  # warm-up
    torch.cuda.synchronize()
    kern_ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enqueue()
        e1.record()
        e1.synchronize()
        kern_ms.append(e0.elapsed_time(e1))
    # ---- the whole device path and the host rule
    dev_s, host_s = [], []
    for rep in range(max(reps, args.host_reps)):
        if rep < reps:
            torch.cuda.synchronize()
            t = time.perf_counter()
            stats = {}
            got = accuracy.align_reads(calls, truths, device=0, want_ops=True, stats=stats)
            dev_s.append(time.perf_counter() - t)
        if rep < args.host_reps:
            t = time.perf_counter()
            exp = accuracy.align_reads(calls, truths, want_ops=True)
            host_s.append(time.perf_counter() - t)
            print(f"host pass {rep}: {host_s[-1]:.1f} s", flush=True)
    assert stats["fallback"] == 0, "a pair fell back to the host: the device figure would include it"
    assert (got[0] == exp[0]).all() and all(a.tobytes() == b.tobytes() for a, b in zip(got[1], exp[1])), \
        "device and host results differ"
    k_ms, d_s, h_s = float(np.median(kern_ms)), float(np.median(dev_s)), float(np.median(host_s))
    ident = accuracy.identity(exp[0].sum(axis=0))
    res = dict(device=torch.cuda.get_device_name(0), pairs=PAIRS, truth_bases=TRUTH_BASES, error_rate=ERROR_RATE,
               seed=SEED, call_bases=int(call.size), cells=int(cells), work_bytes=work_bytes, reps=reps,
               host_reps=args.host_reps, pooled_identity=ident,
               timing="kernels: device events around nd_align_seqs alone, inputs on the device, one warm-up, median; "
                      "device and host: host clock around whole accuracy.align_reads calls (the device call "
                      "includes packing, H2D, the kernels and D2H and ends in a device synchronise), medians",
               kernels_ms=k_ms, kernels_ms_all=kern_ms, kernels_cells_per_s=cells / (k_ms * 1e-3),
               device_s=d_s, device_s_all=dev_s, device_cells_per_s=cells / d_s,
               host_s=h_s, host_s_all=host_s, host_cells_per_s=cells / h_s,
               device_beats_host=bool(d_s < h_s), speedup_whole_call=h_s / d_s, results_equal=True,
               kernels=kernel_meta_rows())
    print(f"{PAIRS} pairs, {cells} cells: kernels {k_ms:.2f} ms ({res['kernels_cells_per_s']:.3g} cells/s), whole "
          f"device call {d_s * 1e3:.1f} ms, host rule {h_s:.1f} s; results equal")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
