"""Time the mapping of called reads to a shared reference (-truth_ref): the index build, nd_locate_segs alone,
nd_align_fit alone, nd_align_seqs on pairs of the same n x m, and accuracy.map_reads end to end against the host
rule on a subset (needs an MI355X).

Input, from a fixed seed: a random reference of 4,000,000 bases in one record; 64 reads, each 12,000 bases of the
reference with 10 % errors (equal parts substitution, insertion and deletion), every second one reverse
complemented.  Measured in one process:
  index   : accuracy.build_index by the host clock, numpy's sort and torch.sort on the device
  locate  : nd_locate_segs alone, inputs on the device, between two device events; one warm-up, median of --reps
  fit     : nd_align_fit alone on the located windows, the same way
  global  : nd_align_seqs on the same (oriented segment, window) pairs, the same way: the fit form adds one compare
            per cell of a single row, so its cells/s should be within 10 % of this
  many    : fit and global again on the same pairs four times over (768 workgroups, three per compute unit): what
            the two forms do when workgroups share a compute unit
  device  : accuracy.map_reads(reads, ref, device=0, want_ops=True) by the host clock, median of --reps
  host    : accuracy.map_reads on the first --host-reads reads; the device results of those reads must be equal

  python tools/bench_mapping.py [--reps 7] [--host-reads 4] [--out profiles/mapping.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nanodecoder_amd import accuracy  # noqa: E402

REF_BASES, READS, READ_BASES, ERROR_RATE, SEED = 4_000_000, 64, 12_000, 0.10, 20261021
MANY = 4  # the segments this many times over: more workgroups than the device has compute units


def make_input():
    rng = np.random.default_rng(SEED)
    ref = rng.integers(0, 4, REF_BASES).astype(np.uint8)
    letters = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for k in range(READS):
        lo = int(rng.integers(0, REF_BASES - READ_BASES))
        t = ref[lo: lo + READ_BASES]
        u = rng.random(READ_BASES)
        other = (t + rng.integers(1, 4, READ_BASES)) % 4
        extra = rng.integers(0, 4, READ_BASES)
        out = []
        for b, x, o, e in zip(t.tolist(), u.tolist(), other.tolist(), extra.tolist()):
            if x < ERROR_RATE / 3:
                out.append(o)
            elif x < 2 * ERROR_RATE / 3:
                out += [b, e]
            elif x >= ERROR_RATE:
                out.append(b)
        call = letters[np.asarray(out, np.int64)]
        reads.append(accuracy.reverse_complement(call) if k % 2 else call)
    return accuracy.Reference(["ref"], [letters[ref]]), reads


def kernel_meta_rows():
    import kernel_meta
    rows = [r for r in kernel_meta.collect() if r["object"] in ("align.o", "locate.o")]
    if not rows:
        return None
    return [dict(kernel=r["name"].split("(")[0], lds_bytes=r.get("lds", 0), vgpr=r.get("vgpr", 0),
                 agpr=r.get("agpr", 0), vgpr_spill=r.get("vgpr_spill", 0), scratch_bytes=r.get("private", 0))
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reads", type=int, default=4)
    ap.add_argument("--meta-only", action="store_true", help="only add the kernels' LDS / VGPR use to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapping.json"))
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
        sys.exit("bench_mapping.py needs a GPU: the device path has no host stand-in")
    from nanodecoder_amd import _lib
    reps = max(5, args.reps)
    ref, reads = make_input()
    dev = torch.device("cuda", 0)
    # ---- the index
    t = time.perf_counter()
    idx_host = accuracy.build_index(ref.seq, ref.rec_off)
    index_host_s = time.perf_counter() - t
    accuracy.build_index(ref.seq[:100000], np.asarray([0, 100000]), device=0)  # warm torch
    t = time.perf_counter()
    idx_dev = accuracy.build_index(ref.seq, ref.rec_off, device=0)
    index_device_s = time.perf_counter() - t
    assert all((a == b).all() for a, b in zip(idx_host, idx_dev)), "the two index builds differ"
    ref._index = idx_host
    # ---- the kernels alone
    L = _lib.lib()
    segs = [accuracy.segments(r.size) for r in reads]
    seg_off = np.zeros(sum(len(s) for s in segs) + 1, np.int32)
    k = base = 0
    for r, sg in zip(reads, segs):
        for _, s1 in sg:
            k += 1
            seg_off[k] = base + s1
        base += int(r.size)
    P = len(seg_off) - 1
    n = np.diff(seg_off).astype(np.int64)
    cells_bound = int((n * (n + 3072)).sum())
    work_bytes = int(L.nd_align_fit_work_bytes(P, cells_bound))
    seq_d, rec_d, code_d, pos_d = ref.on_device(dev)
    call_d = torch.from_numpy(np.concatenate(reads)).to(dev)
    off_d = torch.from_numpy(seg_off).to(dev)
    or_d = torch.zeros(base, dtype=torch.uint8, device=dev)
    hit_d = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    status_d = torch.zeros(P, dtype=torch.int32, device=dev)
    counts_d = torch.zeros((P, 5), dtype=torch.int32, device=dev)
    span_d = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    ops_d = torch.zeros(base, dtype=torch.uint8, device=dev)
    work_d = torch.zeros(work_bytes, dtype=torch.uint8, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    def locate():
        _lib.check(L.nd_locate_segs(p(call_d), p(off_d), P, p(code_d), p(pos_d), int(code_d.numel()), p(rec_d), 1,
                                    p(hit_d), p(status_d), p(or_d), stream()), "nd_locate_segs")

    def fit():
        _lib.check(L.nd_align_fit(p(or_d), p(off_d), p(seq_d), ref.total, p(hit_d), P, cells_bound, p(counts_d),
                                  p(span_d), p(ops_d), p(status_d), p(work_d), work_bytes, stream()), "nd_align_fit")

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), ms
    locate_ms, locate_all = timed(locate)
    fit_ms, fit_all = timed(fit)
    hit, status = hit_d.cpu().numpy(), status_d.cpu().numpy()
    assert not status.any(), "an unmapped or refused segment: the figures would not cover it"
    m = (hit[:, 2] - hit[:, 1]).astype(np.int64)
    cells = int((n * m).sum())
    # nd_align_seqs on the same pairs: the windows copied out one after another
    truth_off = np.zeros(P + 1, np.int32)
    truth_off[1:] = np.cumsum(m)
    truth_d = torch.cat([seq_d[int(a): int(b)] for a, b in hit[:, 1:3]])
    toff_d = torch.from_numpy(truth_off).to(dev)
    gcounts_d = torch.zeros((P, 5), dtype=torch.int32, device=dev)
    gstatus_d = torch.zeros(P, dtype=torch.int32, device=dev)
    gwork = int(L.nd_align_seqs_work_bytes(P, cells))

    def glob():
        _lib.check(L.nd_align_seqs(p(or_d), p(off_d), p(truth_d), p(toff_d), P, cells, p(gcounts_d), p(ops_d),
                                   p(gstatus_d), p(work_d), gwork, stream()), "nd_align_seqs")
    global_ms, global_all = timed(glob)
    assert not gstatus_d.cpu().numpy().any()
    # ---- more workgroups than compute units: the same segments MANY times over, fit against global again
    Pm = MANY * P
    offm = np.concatenate([seg_off[:-1] + k * base for k in range(MANY)] + [[MANY * base]]).astype(np.int32)
    toffm = np.concatenate([truth_off[:-1].astype(np.int64) + k * int(truth_off[-1]) for k in range(MANY)]
                           + [[MANY * int(truth_off[-1])]]).astype(np.int32)
    orm_d, offm_d = or_d.repeat(MANY), torch.from_numpy(offm).to(dev)
    truthm_d, toffm_d = truth_d.repeat(MANY), torch.from_numpy(toffm).to(dev)
    hitm_d = hit_d.repeat(MANY, 1)
    statusm_d = torch.zeros(Pm, dtype=torch.int32, device=dev)
    countsm_d = torch.zeros((Pm, 5), dtype=torch.int32, device=dev)
    gcountsm_d = torch.zeros((Pm, 5), dtype=torch.int32, device=dev)
    spanm_d = torch.zeros((Pm, 2), dtype=torch.int32, device=dev)
    opsm_d = torch.zeros(MANY * base, dtype=torch.uint8, device=dev)
    workm = int(L.nd_align_fit_work_bytes(Pm, MANY * cells))
    workm_d = torch.zeros(workm, dtype=torch.uint8, device=dev)

    def fit_many():
        _lib.check(L.nd_align_fit(p(orm_d), p(offm_d), p(seq_d), ref.total, p(hitm_d), Pm, MANY * cells, p(countsm_d),
                                  p(spanm_d), p(opsm_d), p(statusm_d), p(workm_d), workm, stream()), "nd_align_fit")

    def glob_many():
        _lib.check(L.nd_align_seqs(p(orm_d), p(offm_d), p(truthm_d), p(toffm_d), Pm, MANY * cells, p(gcountsm_d),
                                   p(opsm_d), p(statusm_d), p(workm_d), workm, stream()), "nd_align_seqs")
    fit_many_ms, fit_many_all = timed(fit_many)
    assert not statusm_d.cpu().numpy().any() and \
        (countsm_d.cpu().numpy() == np.tile(counts_d.cpu().numpy(), (MANY, 1))).all(), \
        "the repeated segments' fits differ from the first pass"
    global_many_ms, global_many_all = timed(glob_many)
    assert not statusm_d.cpu().numpy().any()
    del workm_d, opsm_d, truthm_d, orm_d
    # ---- the whole device path and the host rule on a subset
    dev_s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        stats = {}
        got = accuracy.map_reads(reads, ref, device=0, want_ops=True, stats=stats)
        dev_s.append(time.perf_counter() - t)
    H = max(1, min(args.host_reads, READS))
    t = time.perf_counter()
    exp = accuracy.map_reads(reads[:H], ref, want_ops=True)
    host_s = time.perf_counter() - t
    assert (got[0][:H] == exp[0]).all() and all(a.tobytes() == b.tobytes() for a, b in zip(got[2][:H], exp[2])) and \
        all([r[:7] for r in a] == [r[:7] for r in b] for a, b in zip(got[1][:H], exp[1])), "device and host differ"
    kmers = int(2 * (n - 14).sum())
    probes = kmers * (int(math.ceil(math.log2(max(2, idx_host[0].size)))) + 1)
    fit_rate, global_rate = cells / (fit_ms * 1e-3), cells / (global_ms * 1e-3)
    res = dict(device=torch.cuda.get_device_name(0), ref_bases=REF_BASES, reads=READS, read_bases=READ_BASES,
               error_rate=ERROR_RATE, seed=SEED, segments=P, call_bases=base, reps=reps,
               index_entries=int(idx_host[0].size), index_bytes=int(8 * idx_host[0].size),
               index_host_s=index_host_s, index_device_sort_s=index_device_s,
               locate_ms=locate_ms, locate_ms_all=locate_all, locate_query_kmers=kmers,
               locate_probe_bytes=int(4 * probes),
               locate_bytes_note="every query k-mer binary-searches the sorted codes: ceil(log2(entries)) + 1 loads "
                                 "of 4 bytes each, requested; the index arrays themselves are index_bytes",
               cells=cells, cells_bound=cells_bound, work_bytes=work_bytes,
               fit_ms=fit_ms, fit_ms_all=fit_all, fit_cells_per_s=fit_rate,
               global_ms=global_ms, global_ms_all=global_all, global_cells_per_s=global_rate,
               fit_over_global=fit_rate / global_rate, fit_within_10_percent=bool(fit_rate >= 0.9 * global_rate),
               many_pairs=Pm, many_cells=MANY * cells, fit_many_ms=fit_many_ms, fit_many_ms_all=fit_many_all,
               global_many_ms=global_many_ms, global_many_ms_all=global_many_all,
               fit_many_cells_per_s=MANY * cells / (fit_many_ms * 1e-3),
               global_many_cells_per_s=MANY * cells / (global_many_ms * 1e-3),
               fit_over_global_many=global_many_ms / fit_many_ms,
               fit_many_within_10_percent=bool(global_many_ms / fit_many_ms >= 0.9),
               device_s=float(np.median(dev_s)), device_s_all=dev_s, host_reads=H, host_s=host_s,
               host_s_per_read=host_s / H, speedup_per_read=(host_s / H) / (float(np.median(dev_s)) / READS),
               results_equal=True, pooled_identity=accuracy.identity(got[0].sum(axis=0)), stats=stats,
               timing="kernels: device events around the call alone, inputs on the device, one warm-up, median; "
                      "device and host: host clock around whole accuracy.map_reads calls",
               kernels=kernel_meta_rows())
    print(f"index {index_host_s:.2f} s host / {index_device_s:.2f} s with the device sort; locate {locate_ms:.2f} ms; "
          f"fit {fit_ms:.2f} ms ({fit_rate:.3g} cells/s) against nd_align_seqs {global_ms:.2f} ms ({global_rate:.3g}): "
          f"ratio {fit_rate / global_rate:.3f}; {Pm} pairs: fit {fit_many_ms:.2f} ms, nd_align_seqs {global_many_ms:.2f} ms, ratio "
          f"{global_many_ms / fit_many_ms:.3f}; map_reads {np.median(dev_s) * 1e3:.0f} ms for {READS} reads, host "
          f"{host_s:.1f} s for {H}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
