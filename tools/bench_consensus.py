"""Time the consensus path of -truth_ref -consensus: nd_align_fit_pos against nd_align_fit on the same located
windows, nd_pileup_add alone, nd_pileup_call alone, and accuracy.Pileup end to end against the host rule on a
subset (needs an MI355X).

Input: bench_mapping.py's, from its fixed seed: a random reference of 4,000,000 bases in one record; 64 reads, each
12,000 bases of the reference with 10 % errors, every second one reverse complemented.  Measured in one process:
  fit / fit_pos : nd_align_fit and nd_align_fit_pos alone on the located windows, inputs on the device, between two
                  device events; one warm-up each, then --reps runs of each, interleaved (fit, fit_pos, fit, ...);
                  medians, and the spread of each: what the rpos stores cost the serial traceback
  add           : nd_pileup_add alone on those pairs, the same way, and the same pairs four times over in one call;
                  atomic bytes per second = 4 bytes per add (the table's sum after one call) over the time
  call          : nd_pileup_call alone at ref_len = 4,000,000, min_cov 5, on the table of one add
  device / host : accuracy.Pileup(ref, device=0).add(reads) + call(1) by the host clock, median of --reps, against
                  accuracy.Pileup(ref).add + call on the first --host-reads reads; the tables, the calls and the
                  record sums of those reads must be equal

  python tools/bench_consensus.py [--reps 7] [--host-reads 2] [--out profiles/consensus.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_mapping import READS, READ_BASES, REF_BASES, ERROR_RATE, SEED, make_input  # noqa: E402
from nanodecoder_amd import accuracy  # noqa: E402

MANY = 4
MIN_COV = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reads", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_consensus.py needs a GPU: the device path has no host stand-in")
    from nanodecoder_amd import _lib
    reps = max(5, args.reps)
    ref, reads = make_input()
    dev = torch.device("cuda", 0)
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
    work_bytes = int(L.nd_align_fit_pos_work_bytes(P, cells_bound))
    seq_d, rec_d, code_d, pos_d = ref.on_device(dev)
    call_d = torch.from_numpy(np.concatenate(reads)).to(dev)
    off_d = torch.from_numpy(seg_off).to(dev)
    or_d = torch.zeros(base + 1, dtype=torch.uint8, device=dev)
    hit_d = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    status_d = torch.zeros(P, dtype=torch.int32, device=dev)
    counts_d = torch.zeros((2, P, 5), dtype=torch.int32, device=dev)
    span_d = torch.zeros((2, P, 2), dtype=torch.int32, device=dev)
    ops_d = torch.zeros((2, base + 1), dtype=torch.uint8, device=dev)
    rpos_d = torch.zeros(base + 1, dtype=torch.int32, device=dev)
    work_d = torch.zeros(work_bytes, dtype=torch.uint8, device=dev)
    pile_d = torch.zeros(9 * ref.total + 1, dtype=torch.int32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    _lib.check(L.nd_locate_segs(p(call_d), p(off_d), P, p(code_d), p(pos_d), int(code_d.numel()), p(rec_d), 1,
                                p(hit_d), p(status_d), p(or_d), stream()), "nd_locate_segs")

    def fit():
        _lib.check(L.nd_align_fit(p(or_d), p(off_d), p(seq_d), ref.total, p(hit_d), P, cells_bound, p(counts_d[0]),
                                  p(span_d[0]), p(ops_d[0]), p(status_d), p(work_d), work_bytes, stream()),
                   "nd_align_fit")

    def fit_pos():
        _lib.check(L.nd_align_fit_pos(p(or_d), p(off_d), p(seq_d), ref.total, p(hit_d), P, cells_bound,
                                      p(counts_d[1]), p(span_d[1]), p(ops_d[1]), p(rpos_d), p(status_d), p(work_d),
                                      work_bytes, stream()), "nd_align_fit_pos")

    def add():
        _lib.check(L.nd_pileup_add(p(or_d), p(off_d), p(ops_d[1]), p(rpos_d), p(status_d), P, p(pile_d), ref.total,
                                   stream()), "nd_pileup_add")

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(*fns):
        """One warm-up of each, then reps rounds with the functions in turn: (median, all) per function."""
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                ms[k].append(once(fn))
        return [(float(np.median(m)), m) for m in ms]
    (fit_ms, fit_all), (pos_ms, pos_all) = timed(fit, fit_pos)
    assert not status_d.cpu().numpy().any(), "an unmapped or refused segment: the figures would not cover it"
    same = all(bool((t[0] == t[1]).all()) for t in (counts_d, span_d, ops_d))
    assert same, "nd_align_fit_pos and nd_align_fit differ"
    hit = hit_d.cpu().numpy()
    cells = int((n * (hit[:, 2] - hit[:, 1]).astype(np.int64)).sum())
    # ---- the pile
    pile_d.zero_()
    add()
    adds = int(pile_d.sum(dtype=torch.int64).item())
    (add_ms, add_all), = timed(add)
    offm = np.concatenate([seg_off[:-1].astype(np.int64) + k * base for k in range(MANY)]
                          + [[MANY * base]]).astype(np.int32)
    orm_d, opsm_d, rposm_d = or_d[:base].repeat(MANY), ops_d[1, :base].repeat(MANY), rpos_d[:base].repeat(MANY)
    offm_d, statusm_d = torch.from_numpy(offm).to(dev), status_d.repeat(MANY)

    def add_many():
        _lib.check(L.nd_pileup_add(p(orm_d), p(offm_d), p(opsm_d), p(rposm_d), p(statusm_d), MANY * P, p(pile_d),
                                   ref.total, stream()), "nd_pileup_add")
    pile_d.zero_()
    add_many()
    assert int(pile_d.sum(dtype=torch.int64).item()) == MANY * adds
    (add_many_ms, add_many_all), = timed(add_many)
    # ---- the call, on the table of one add
    pile_d.zero_()
    add()
    cons_d = torch.zeros(2 * ref.total + 1, dtype=torch.uint8, device=dev)
    cov_d = torch.zeros(ref.total + 1, dtype=torch.int32, device=dev)
    recs_d = torch.zeros(7, dtype=torch.int64, device=dev)

    def call():
        _lib.check(L.nd_pileup_call(p(pile_d), p(seq_d), ref.total, p(rec_d), 1, MIN_COV, p(cons_d),
                                    p(cons_d[ref.total:]), p(cov_d), p(recs_d), stream()), "nd_pileup_call")
    (call_ms, call_all), = timed(call)
    call_bytes = ref.total * (9 * 4 + 1 + 1 + 1 + 4)  # the nine planes and the reference read; cons, ins, cov written
    del orm_d, opsm_d, rposm_d, pile_d, work_d
    # ---- the whole device path and the host rule on a subset
    H = max(1, min(args.host_reads, READS))
    dev_s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pile, stats = accuracy.Pileup(ref, device=0), {}
        got = pile.add(reads, stats=stats)
        res_dev = pile.call(1)
        dev_s.append(time.perf_counter() - t)
    sub = accuracy.Pileup(ref, device=0)
    sub.add(reads[:H])
    t = time.perf_counter()
    host = accuracy.Pileup(ref)
    host.add(reads[:H])
    res_host = host.call(1)
    host_s = time.perf_counter() - t
    equal = sub.counts().tobytes() == host.counts().tobytes() and \
        all(a.tobytes() == b.tobytes() for a, b in zip(sub.call(1), res_host))
    assert equal, "device and host differ"
    rec = res_dev[3]
    res = dict(device=torch.cuda.get_device_name(0), ref_bases=REF_BASES, reads=READS, read_bases=READ_BASES,
               error_rate=ERROR_RATE, seed=SEED, segments=P, call_bases=base, cells=cells, reps=reps,
               fit_ms=fit_ms, fit_ms_all=fit_all, fit_pos_ms=pos_ms, fit_pos_ms_all=pos_all,
               fit_pos_over_fit=pos_ms / fit_ms, fit_outputs_equal=same,
               fit_spread_ms=[min(fit_all), max(fit_all)], fit_pos_spread_ms=[min(pos_all), max(pos_all)],
               add_ms=add_ms, add_ms_all=add_all, add_atomics=adds, add_atomic_bytes=4 * adds,
               add_atomic_bytes_per_s=4 * adds / (add_ms * 1e-3),
               add_many_pairs=MANY * P, add_many_ms=add_many_ms, add_many_ms_all=add_many_all,
               add_many_atomic_bytes_per_s=4 * MANY * adds / (add_many_ms * 1e-3),
               add_note="one thread per call base, one u32 atomic add of 4 bytes per piled base, deleted position "
                        "and insertion event; a wave's adds go to consecutive addresses of at most four planes; "
                        "the input read is 6 bytes per call base (call, op, rpos) plus the offsets' binary search",
               call_ms=call_ms, call_ms_all=call_all, call_min_cov=MIN_COV, call_bytes=call_bytes,
               call_bytes_per_s=call_bytes / (call_ms * 1e-3),
               device_s=float(np.median(dev_s)), device_s_all=dev_s, host_reads=H, host_s=host_s,
               host_s_per_read=host_s / H, speedup_per_read=(host_s / H) / (float(np.median(dev_s)) / READS),
               results_equal=equal, stats=stats, pooled_read_identity=accuracy.identity(got[0].sum(axis=0)),
               consensus_rec_min_cov_1=[int(v) for v in rec[0]],
               timing="kernels: device events around the call alone, inputs on the device, one warm-up, median; fit "
                      "and fit_pos interleaved in one process; device and host: host clock around whole "
                      "accuracy.Pileup add + call")
    print(f"fit {fit_ms:.3f} ms, fit_pos {pos_ms:.3f} ms (ratio {pos_ms / fit_ms:.4f}); add {add_ms * 1e3:.1f} us "
          f"({4 * adds / (add_ms * 1e-3):.3g} atomic B/s), x{MANY} {add_many_ms * 1e3:.1f} us "
          f"({4 * MANY * adds / (add_many_ms * 1e-3):.3g} B/s); call {call_ms * 1e3:.1f} us "
          f"({call_bytes / (call_ms * 1e-3):.3g} B/s); Pileup {np.median(dev_s) * 1e3:.0f} ms for {READS} reads, host "
          f"{host_s:.1f} s for {H}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
