"""Read assembly for a group (-assembly gpu), host side (no GPU): the flag, the packing of a group's chunk
strings for nd_assemble_reads, assemble_reads' host branches, and the entry point's argument errors."""
import ctypes

import numpy as np
import pytest

from nanodecoder_amd import frontend, opts

BASE = ["-model", "m.pt", "-save_data", "out"]


def test_assembly_flag_parses_and_defaults_to_cpu():
    assert opts.parse_translate_opts(BASE).assembly == "cpu"
    assert opts.parse_translate_opts(BASE + ["-assembly", "gpu"]).assembly == "gpu"
    assert opts.parse_translate_opts(BASE + ["--assembly", "cpu"]).assembly == "cpu"
    with pytest.raises(SystemExit):
        opts.parse_translate_opts(BASE + ["-assembly", "tpu"])


def test_pack_assembly_input_offsets():
    reads = [
        [],                                                       # a zero-chunk read
        [[""], [""]],                                             # only empty chunks
        [[""], ["A C"], [""], ["G G T"], [""]],                   # empty first, middle and last
        [["A C G T", "T T T T T T"], ["C", "G G"]],               # n-best lists: x[0] only
        [["acgm"]],
    ]
    bases, chunk_off, read_off, host = frontend.pack_assembly_input(reads)[:4]
    assert host == []
    assert bases.dtype == np.uint8 and chunk_off.dtype == np.int32 and read_off.dtype == np.int32
    assert bases.tobytes() == b"ACGGTACGTCacgm"
    assert list(read_off) == [0, 0, 2, 7, 9, 10]
    assert list(chunk_off) == [0, 0, 0, 0, 2, 2, 5, 5, 9, 10, 14]
    # every chunk reads back as the host path's string for it
    flat = [x[0].replace(" ", "") for p in reads for x in p]
    assert [bases[chunk_off[c]: chunk_off[c + 1]].tobytes().decode() for c in range(len(flat))] == flat


def test_pack_assembly_input_keeps_unpackable_reads_on_the_host():
    reads = [[["A C"], ["C G"]], [["A ç"], ["C"]], [["A"], [" "], ["C"]], [["G"]]]
    bases, chunk_off, read_off, host = frontend.pack_assembly_input(reads)[:4]
    # non-ASCII text, and a hypothesis of spaces alone (the host path keeps it as an empty string in its
    # chunk list, where it moves the next chunk): packed with no chunks, listed for assemble_read
    assert host == [1, 2]
    assert list(read_off) == [0, 2, 2, 2, 3]
    assert bases.tobytes() == b"ACCGG" and list(chunk_off) == [0, 2, 4, 5]
    empty = frontend.pack_assembly_input([])
    assert empty.bases.size == 0 and list(empty.chunk_off) == [0] and list(empty.read_off) == [0] and empty.host == []
    assert empty.qw is None and empty.mw is None and empty.bp is None


@pytest.fixture(scope="module")
def golden_reads():
    from tests import golden_util as gu
    z, meta = gu.load_frontend()
    n = len(meta["assembly"])
    assert n == 6
    return [[[str(p)] for p in z[f"asm_preds{j}"]] for j in range(n)], [str(z[f"asm_seq{j}"]) for j in range(n)], \
        [str(z[f"asm_concat{j}"]) for j in range(n)]


def test_assemble_reads_without_device_is_assemble_read(golden_reads):
    reads, seqs, _ = golden_reads
    stats = {}
    got = frontend.assemble_reads(reads, 300, 60, device=None, stats=stats)
    assert got == [frontend.assemble_read(p, 300, 60) for p in reads] == seqs
    assert stats == {}  # nothing went to a device, nothing fell back


def test_concatenation_branch_stays_on_the_host(golden_reads, monkeypatch):
    """src_seq_stride >= src_seq_length: no alignment, no device call even when given a device."""
    reads, _, concat = golden_reads

    def no_device(*a, **k):
        raise AssertionError("the concatenation branch made a device call")
    monkeypatch.setattr(frontend, "_assemble_device", no_device)
    assert frontend.assemble_reads(reads, 512, 512, device=0) == concat
    assert frontend.assemble_reads(reads, 300, 300, device=0) == \
        [frontend.assemble_read(p, 300, 300) for p in reads]
    with pytest.raises(AssertionError):
        frontend.assemble_reads(reads, 300, 60, device=0)


def test_assemble_reads_entry_point_argument_errors_without_gpu():
    """nd_assemble_reads refuses null buffers, negative sizes, total_bases >= 2^31 and a work size below
    nd_assemble_reads_work_bytes before any HIP call (no device is touched: this runs without one)."""
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert "nd_assemble_reads" in _lib.SIGNATURES and "nd_assemble_reads_work_bytes" in _lib.SIGNATURES
    need = L.nd_assemble_reads_work_bytes(3, 100)
    assert need >= 5 * 4 * 100 + 2 * 4 * 3        # five int32 count rows and two per-chunk words
    assert L.nd_assemble_reads_work_bytes(0, 0) == 0 and L.nd_assemble_reads_work_bytes(-1, 5) < 0
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.nd_assemble_reads(None, None, None, 2, 3, 100, None, None, None, None, need, None)
    assert rc == _lib.ND_ERR_ARG and b"null buffer" in L.nd_last_error()
    rc = L.nd_assemble_reads(p, p, p, 2, 3, 100, p, p, p, None, need, None)
    assert rc == _lib.ND_ERR_ARG and b"null buffer" in L.nd_last_error()
    rc = L.nd_assemble_reads(p, p, p, 2, 3, 100, p, p, p, p, need - 1, None)
    assert rc == _lib.ND_ERR_ARG and b"work_bytes" in L.nd_last_error()
    rc = L.nd_assemble_reads(p, p, p, -1, 3, 100, p, p, p, p, need, None)
    assert rc == _lib.ND_ERR_ARG and b">= 0" in L.nd_last_error()
    rc = L.nd_assemble_reads(p, p, p, 2, 3, 2 ** 31, p, p, p, p, 2 ** 40, None)
    assert rc == _lib.ND_ERR_ARG and b"2^31" in L.nd_last_error()
    # nothing to do: ND_OK at once
    assert L.nd_assemble_reads(None, p, p, 0, 0, 0, None, None, None, None, 0, None) == 0
