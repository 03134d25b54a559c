"""translate.py driver (reference translate.py:59-187) on the MI355X engine.

Same inputs, outputs and resume rule: every ``*.signal`` / ``*.fast5`` in
``-src_dir`` whose ``result/<read>.fasta`` does not exist yet is normalised
and windowed in a worker pool (translate.py:131-163), translated, and written
as result/<read>.fasta, segment/<read>.txt and a line of speed.txt
(translate.py:81-98).  One bad read prints ``!!!error!!!`` and the run goes
on (translate.py:97-98).  ``-pack_reads N`` translates N reads per engine pass.
``-fastq`` also writes result/<read>.fastq with per-base qualities;
``-mod_probs`` (CpG models) result/<read>.mod.fastq with MM / ML tags.
``-truth FILE`` aligns every read that has a known sequence in FILE to it and
writes save_data/accuracy.tsv (with ``-fastq`` quality_calibration.tsv too).
``-truth_ref FILE`` maps every read to a shared reference instead (segments of
at most 4096 bases, either strand) and also writes save_data/mapping.paf;
with ``-consensus`` the mapped segments are piled up on the reference and the
run ends with save_data/consensus.fasta, variants.tsv and coverage.tsv.
"""
from __future__ import annotations

import logging
import multiprocessing
import codecs
import os
import sys
import time

from . import accuracy, frontend
from .opts import parse_translate_opts


def init_logger(log_file=None):
    """onmt/utils/logging.py:9-24."""
    fmt = logging.Formatter("[%(asctime)s %(levelname)s] %(message)s")
    logger = logging.getLogger()
    logger.setLevel(logging.INFO)
    h = logging.StreamHandler()
    h.setFormatter(fmt)
    logger.handlers = [h]
    if log_file:
        fh = logging.FileHandler(log_file)
        fh.setFormatter(fmt)
        logger.addHandler(fh)
    return logger


def list_reads(opt):
    """translate.py:134-163: pending reads (resume = skip existing fasta)."""
    todo, done = [], 0
    for name in sorted(os.listdir(opt.src_dir)):
        if name.endswith("fast5"):
            prefix, suffix = name.split(".fast5")[0] + ".txt", "fast5"
        elif name.endswith("signal"):
            prefix, suffix = name.split(".signal")[0] + ".txt", "signal"
        else:
            continue
        if os.path.exists(os.path.join(opt.save_data, "result", prefix.split(".txt")[0] + ".fasta")):
            done += 1
        else:
            todo.append((os.path.join(opt.src_dir, name), prefix, suffix))
    return todo, done


def _read_only(args):
    """-frontend gpu: the worker only reads the raw samples.  An empty read
    yields [prefix] alone and is skipped like the reference's
    (translate.py:102-103)."""
    path, prefix, suffix, norm, length, stride = args
    try:
        raw = frontend.read_raw(path, suffix)
        return [prefix, raw] if len(raw) else [prefix]
    except Exception:
        return ["!" + prefix]


def _gpu_chunks(opt, group):
    """[prefix, raw] reads -> [prefix, chunk, ...] with the device front end,
    on the translator's GPU (-gpu)."""
    sig, lens, rd = frontend.normalize_window_gpu([g[1] for g in group], opt.normalization_raw,
                                                  opt.src_seq_length, opt.src_seq_stride, device=max(0, opt.gpu))
    host = sig.cpu().numpy()
    out = [[g[0]] for g in group]
    for c in range(len(rd)):
        out[rd[c]].append(host[c, : lens[c]].copy())
    return out


def _n_chunks(opt, src, gpu_fe):
    """Chunks a pending read will contribute (for -pack_reads 0)."""
    if not gpu_fe:
        return len(src) - 1
    return len(frontend.windows(len(src[1]), opt.src_seq_length, opt.src_seq_stride))


def _run_group(opt, translator, pending, gpu_fe, evaluation, assembly_stats):
    """Front end (device) + translate for one packed group, with the
    per-group error isolation of translate.py:97-98.  -frontend gpu: the raw
    reads go to the translator, which normalises and windows every engine
    batch on the device right before its call (stream_raw_reads); with
    -attn_debug (its file needs each chunk's samples on the host) the chunks
    come back to the host first."""
    if gpu_fe and not opt.attn_debug:
        return _translate_group(opt, translator, pending, evaluation, assembly_stats, raw=True)
    if gpu_fe:
        try:
            pending = _gpu_chunks(opt, pending)
        except Exception as e:
            for g in pending:
                print("!!!error!!!data src: " + g[0].split(".txt")[0] + " (%r)" % (e,))
            return 0
    return _translate_group(opt, translator, pending, evaluation, assembly_stats)


def _extract(args):
    path, prefix, suffix, norm, length, stride = args
    try:
        return frontend.extract_raw(path, prefix, norm, length, stride, suffix)
    except Exception as e:  # surfaced per read, like the Pool error path
        return ["!" + prefix, repr(e)]


def write_output(opt, file_src, all_predictions, time_translate, sequence=None, weights=None, mods=None,
                 moves=None, accuracy_line=None, paf_lines=None):
    """translate.py:81-98.  ``sequence``: the read already assembled
    (-assembly gpu); None assembles it here.  ``weights`` (-fastq): the
    chunks' per-base weights; ``sequence`` is then (sequence, quality string),
    and result/<read>.fastq is written before the .fasta resume keys on.
    ``mods`` (-mod_probs, beside ``weights``): the chunks' per-base
    modification weights; ``sequence`` is then (sequence, quality string, ml),
    result/<read>.mod.fastq is written before the .fasta too, and the .fastq
    only with -fastq.  ``moves`` (-moves): the chunks' per-base chunk-relative
    signal positions; ``sequence`` then carries the read positions as its
    last entry ((sequence, positions) without ``weights``), and
    result/<read>.moves is written before the .fasta too.  ``accuracy_line``
    (-truth, -truth_ref): the read's line of save_data/accuracy.tsv, appended
    before the .fasta too, and ``paf_lines`` (-truth_ref) its mapped segments'
    lines of save_data/mapping.paf.  Returns True when everything was written."""
    try:
        name = file_src.split(".txt")[0]
        if sequence is None:
            c_bpread, quality, ml, rpos = frontend.assemble_read_annotated(
                all_predictions, opt.src_seq_length, opt.src_seq_stride, weights, mods, moves)
        else:  # as frontend.assemble_reads gives a read: the string, or a tuple with what was asked for, in order
            rest = list(sequence[1:]) if weights is not None or moves is not None else []
            c_bpread = sequence if not rest else sequence[0]
            quality, ml, rpos = (rest.pop(0) if given is not None else None for given in (weights, mods, moves))
        if mods is not None:
            with open(os.path.join(opt.save_data, "result", name + ".mod.fastq"), "w") as f:
                f.write(frontend.mod_fastq_record(name, c_bpread, quality, ml))
        if weights is not None and (mods is None or getattr(opt, "fastq", False)):
            with open(os.path.join(opt.save_data, "result", name + ".fastq"), "w") as f:
                f.write("@%s\n%s\n+\n%s\n" % (name, c_bpread, quality))
        if moves is not None:
            with open(os.path.join(opt.save_data, "result", name + ".moves"), "w") as f:
                f.write(frontend.moves_record(name, c_bpread, rpos))
        if accuracy_line is not None:
            with open(os.path.join(opt.save_data, "accuracy.tsv"), "a") as f:
                f.write(accuracy_line)
        if paf_lines:
            with open(os.path.join(opt.save_data, "mapping.paf"), "a") as f:
                f.writelines(paf_lines)
        with open(os.path.join(opt.save_data, "result", name + ".fasta"), "w") as f:
            f.writelines(">%s\n%s" % (name, c_bpread))
        with open(os.path.join(opt.save_data, "segment", file_src), "w+") as f:
            for n_best_preds in all_predictions:
                f.write("\n".join(n_best_preds) + "\n")
        with open(os.path.join(opt.save_data, "speed.txt"), "a+") as f:
            f.writelines("%s\t%0.2f\t%d\t%0.2f\n" % (name, float(time_translate), len(c_bpread),
                                                     len(c_bpread) / max(float(time_translate), 1e-9)))
        return True
    except Exception:
        print("!!!error!!!data src: " + file_src.split(".txt")[0])
        return False


def _assemble_missing(opt, outs, seqs, weights, mods, positions):
    """The reads of ``seqs`` still None, assembled by the host functions write_output would use."""
    for k, o in enumerate(outs):
        if seqs[k] is None:
            try:
                seqs[k] = frontend.assemble_reads([o[1]], opt.src_seq_length, opt.src_seq_stride,
                                                  **(dict(weights=[weights[k]]) if weights[k] is not None else {}),
                                                  **(dict(mod_weights=[mods[k]]) if mods[k] is not None else {}),
                                                  **(dict(positions=[positions[k]]) if positions[k] is not None
                                                     else {}))[0]
            except Exception:
                seqs[k] = None


def main(opt=None):
    opt = opt or parse_translate_opts()
    for flag in ("fastq", "mod_probs", "moves", "truth", "truth_ref"):
        if getattr(opt, flag) and opt.attn_debug:
            raise ValueError("-%s is not available together with -attn_debug" % flag)
    if opt.truth_ref and opt.truth:
        raise ValueError("-truth_ref and -truth exclude each other")
    if opt.consensus and not opt.truth_ref:
        raise ValueError("-consensus needs -truth_ref")
    if opt.consensus and opt.consensus_min_cov < 1:
        raise ValueError("-consensus_min_cov must be at least 1")
    logger = init_logger(opt.log_file)
    evaluation = accuracy.Evaluation(opt) if opt.truth or opt.truth_ref else None
    assembly_stats = {"reads": 0, "fallback": 0}  # -assembly gpu: reads assembled / of them on the host
    for sub in ("", "result", "segment") + (("attention",) if opt.attn_debug else ()):  # translate.py:64-71
        os.makedirs(os.path.join(opt.save_data, sub), exist_ok=True)
    from .translator import build_translator
    translator = build_translator(opt, report_score=False, logger=logger)
    if opt.mod_probs:
        translator._check_supported(mods=True)  # ValueError for a vocabulary without C or M, before any read
    todo, done = list_reads(opt)
    logger.info("%d reads have already translated, remains %d read\n" % (done, len(todo)))
    jobs = [(p, pre, suf, opt.normalization_raw, opt.src_seq_length, opt.src_seq_stride) for p, pre, suf in todo]
    ctx = multiprocessing.get_context("spawn")
    t_start = time.time()
    n_done = 0
    gpu_fe = opt.frontend == "gpu"
    # -pack_reads 0: flush once the pending reads fill the engine batch
    cap = int(getattr(translator, "max_batch", 0) or 256)
    with ctx.Pool(max(1, opt.thread)) as pool:
        pending, n_chunks = [], 0
        for src in pool.imap(_read_only if gpu_fe else _extract, jobs):
            if src and src[0].startswith("!"):
                print("!!!error!!!data src: " + src[0][1:].split(".txt")[0])
                continue
            if not src or len(src) == 1:   # translate.py:102-103
                continue
            pending.append(src)
            n_chunks += _n_chunks(opt, src, gpu_fe)
            full = len(pending) >= opt.pack_reads if opt.pack_reads > 0 else n_chunks >= cap
            if full:
                n_done += _run_group(opt, translator, pending, gpu_fe, evaluation, assembly_stats)
                pending, n_chunks = [], 0
        if pending:
            n_done += _run_group(opt, translator, pending, gpu_fe, evaluation, assembly_stats)
    logger.info("translated %d reads in %.1f s" % (n_done, time.time() - t_start))
    if opt.assembly == "gpu":
        logger.info("-assembly gpu: %d of %d reads were assembled on the host (fallback: a chunk of 200 or more "
                    "bases, or text outside ACGTM)" % (assembly_stats["fallback"], assembly_stats["reads"]))
    if evaluation is not None:
        evaluation.finish(opt.save_data, opt.fastq, logger)
    return n_done


def _translate_attn(opt, translator, group):
    """-attn_debug (translate.py:110-120): read by read, each into its own
    save_data/attention/<read> file (appended)."""
    outs = []
    for g in group:
        with codecs.open(os.path.join(opt.save_data, "attention", g[0]), "a+", "utf-8") as f:
            translator.setAttnFile(f)
            outs.append(translator.translate(src=list(g[1:]), batch_size=opt.batch_size, attn_debug=True))
    return outs


def _translate_group(opt, translator, group, evaluation, assembly_stats, raw=False):
    """One packed group translated and written.  ``evaluation`` (accuracy.Evaluation, or None without -truth and
    -truth_ref) evaluates the group's reads before they are written and takes a read's entry into its sums once
    the read is written; ``assembly_stats`` is the run's -assembly gpu count."""
    t0 = time.time()
    mod_probs = bool(getattr(opt, "mod_probs", False))
    fastq = bool(getattr(opt, "fastq", False)) or mod_probs  # the methylation values travel beside the qualities
    want = dict(qualities=True) if fastq else {}
    if mod_probs:
        want["mods"] = True
    moves = bool(getattr(opt, "moves", False))
    if moves:
        want["moves"] = True
    try:
        if opt.attn_debug:
            outs = _translate_attn(opt, translator, group)
        elif raw:  # [prefix, raw samples]: the front end runs on the device
            outs = translator.translate_raw_reads([g[1] for g in group], batch_size=opt.batch_size,
                                                  normalization=opt.normalization_raw,
                                                  src_seq_length=opt.src_seq_length,
                                                  src_seq_stride=opt.src_seq_stride, **want)
        else:
            outs = translator.translate_reads([g[1:] for g in group], batch_size=opt.batch_size, **want)
    except Exception as e:
        for g in group:
            print("!!!error!!!data src: " + g[0].split(".txt")[0] + " (%r)" % (e,))
        return 0
    dt = time.time() - t0
    total = max(1, sum(len(o[1]) for o in outs))
    seqs = [None] * len(outs)
    # per read: with -fastq per chunk its bases' weights, with -mod_probs their modification weights, with -moves
    # their chunk-relative signal positions; None for what was not asked
    parts = [translator.split_result(o, **want) for o in outs]
    weights, mods, positions = ([p[k] for p in parts] for k in (2, 3, 4))
    if getattr(opt, "assembly", "cpu") == "gpu":
        # the whole group in one device call; a read left None (its host fallback raised) is assembled
        # again by write_output, which reports that read's error as -assembly cpu does
        try:
            seqs = list(frontend.assemble_reads([o[1] for o in outs], opt.src_seq_length, opt.src_seq_stride,
                                                device=max(0, opt.gpu), stats=assembly_stats, defer_errors=True,
                                                **(dict(weights=weights) if fastq else {}),
                                                **(dict(mod_weights=mods) if mod_probs else {}),
                                                **(dict(positions=positions) if moves else {})))
        except Exception as e:
            for g in group:
                print("!!!error!!!data src: " + g[0].split(".txt")[0] + " (%r)" % (e,))
            return 0
    acc = [None] * len(group)
    if evaluation is not None:
        # the reads still None (-assembly cpu) are assembled here; one whose assembly raises stays None:
        # write_output assembles it again and reports it
        _assemble_missing(opt, outs, seqs, weights, mods, positions)
        acc = evaluation.evaluate([g[0].split(".txt")[0] for g in group], seqs, fastq)
    for g, o, seq, w, mw, ps, a in zip(group, outs, seqs, weights, mods, positions, acc):
        lines = dict(accuracy_line=a.line, paf_lines=a.paf_lines) if a is not None else {}
        if write_output(opt, g[0], o[1], dt * len(o[1]) / total, sequence=seq, weights=w,
                        **(dict(mods=mw) if mod_probs else {}), **(dict(moves=ps) if moves else {}), **lines) and lines:
            evaluation.account(a)
    return len(group)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
