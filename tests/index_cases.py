"""Inputs the index tests share (CPU and GPU): the synthetic multi-level file, and the call of ``pc_bam_index_finish``."""
import ctypes
import functools
import os

import numpy as np

from tests import bam_writer, index_model

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hts_fixture.npz")

SYNTH_REFS = ["cA", "cEmpty", "cB", "cC"]
SYNTH_LENS = [300_000_000, 1000, 5_000_000, 100_000]
PILE_AT = 67_050_000


def synth_records():
    """14 306 records on 4 references: on a 300 Mbp reference 300 sparse reads, then 12 000 piled into one 16 kb window
    (every 53rd spliced over 20 kb, every 211th placed but unmapped without a CIGAR, every 997th spliced across 2^26); a
    reference without records; 2 000 sparse reads on 5 Mbp; one read that ends in a deletion; five unplaced reads."""
    rng = np.random.default_rng(7)
    recs = [(0, p, [(0, 30)], 0) for p in sorted(rng.integers(0, 60_000_000, 300).tolist())]
    for k, p in enumerate(sorted(rng.integers(PILE_AT, PILE_AT + 8000, 12000).tolist())):
        if k % 53 == 0:
            recs.append((0, p, [(0, 10), (3, 20000), (0, 10)], 16))
        elif k % 211 == 0:
            recs.append((0, p, [], 4))
        elif k % 997 == 0:
            recs.append((0, p, [(0, 10), (3, 60000), (0, 10)], 0))
        else:
            recs.append((0, p, [(0, int(rng.integers(20, 40)))], 16 if k & 1 else 0))
    recs += [(2, p, [(0, 30)], 0) for p in sorted(rng.integers(0, 4_990_000, 2000).tolist())]
    recs.append((3, 99_000, [(0, 25), (2, 3)], 0))
    recs += [(-1, -1, [], 4)] * 5
    return recs


def write_synth(path, index=False):
    bam_writer.write_bam(path, SYNTH_REFS, SYNTH_LENS, synth_records(), block_bytes=777, index=index)


@functools.lru_cache(maxsize=None)
def synth_model(path):
    """``(walk, pre-finish arrays, finished index)`` of the synthetic file at `path` (computed once per path)."""
    w = index_model.walk(open(path, "rb").read())
    pre = index_model.prefinish(w)
    return w, pre, index_model.finish(pre)


def assert_synth_shape(model):
    """The synthetic file still exercises what it was made for (asserted on the MODEL's index)."""
    refs, nn = model
    lvl = index_model.level
    bins_a, _ = refs[0]
    real = {b: c for b, c in bins_a.items() if b != index_model.META_BIN}
    assert {0, 4, 5} <= {lvl(b) for b in real}
    pile = 4681 + (PILE_AT >> 14)
    assert pile == 8773 and len(real[pile]) > 1 and (real[pile][-1][1] >> 16) - (real[pile][0][0] >> 16) >= 0x10000
    bins_b, lin_b = refs[2]
    covered = len({x for x in lin_b})     # distinct offsets <= covered windows
    assert 0 < sum(1 for b in bins_b if b != index_model.META_BIN and lvl(b) == 5) < covered
    assert refs[1] == ({}, [])
    assert nn == 5


def finish_with_library(pre):
    """``pc_bam_index_finish`` on the model's pre-finish arrays -> ``(bytes of the index, stats[8])``."""
    from plastid_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    keep = [np.ascontiguousarray(pre[k]) for k in ("run_tid", "run_bin", "run_beg", "run_end", "lin_start", "linear", "ref_beg", "ref_end",
                                                    "ref_mapped", "ref_unmapped")]
    _lib.check(L.pc_bam_index_finish(int(pre["n_ref"]), len(pre["run_tid"]), *[a.ctypes.data_as(ctypes.c_void_p) for a in keep],
                                     int(pre["n_no_coor"]), ctypes.byref(h)))
    try:
        n = ctypes.c_int64(0)
        _lib.check(L.pc_bam_index_bytes(h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(int(n.value), 1))
        _lib.check(L.pc_bam_index_bytes(h, buf, int(n.value), ctypes.byref(n)))
        st = np.zeros(8, np.int64)
        _lib.check(L.pc_bam_index_stats(h, st.ctypes.data_as(ctypes.c_void_p)))
    finally:
        L.pc_bam_index_close(h)
    return buf.raw[:int(n.value)], st
