"""smashgpu -- Python host side of the MI355X SMASH read -> bin-count path.

Mirrors the reference's driver layer (index_setup.sh / smash_mapping.sh /
binning.sh glue around mummer, mappability_tag, smashMEM.py and varbin.py)
over the C ABI of libsmashgpu.so (include/smash_gpu.h).  PyTorch is used only
for device memory, streams and torch.distributed; every computation runs in
the HIP kernels of smash-paper_amd/csrc.  There is no CPU fallback: if the
library is missing this module raises on import of the library.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsmashgpu.so")
# A/B measurement of library builds (tools/ab.sh): SMASH_LIB names another build
LIB_PATH = os.environ.get("SMASH_LIB", LIB_PATH)

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)
i64p = C.POINTER(C.c_int64)
i32p = C.POINTER(C.c_int32)
vp = C.c_void_p

SMASH_MODE_MAM = 1
SMASH_LEN_VAR = 0x80000000   # readers: *len = SMASH_LEN_VAR | M, mates of 1..M bases
SMASH_MODE_MAM_PLAIN = 2
SMASH_MODE_MUM = 3
SMASH_MODE_MEM = 4
MODES = {"MAM": SMASH_MODE_MAM, "MUM": SMASH_MODE_MUM, "MEM": SMASH_MODE_MEM}
SAM_PACKED = 0x80000000   # smash_sam_format: records packed read after read (| cap)

ERRORS = {1: "left mappability too big (mappability_tag.cpp:110)",
          2: "right mappability too big (mappability_tag.cpp:113)",
          -4: "out of device memory / key set full",
          -5: "unsupported (more matches per read than on-chip slots)"}

EXPORTS = [
    "smash_last_error", "smash_text_from_fasta", "smash_text_free",
    "smash_index_create", "smash_index_load", "smash_index_save",
    "smash_index_free", "smash_index_query", "smash_map_batch", "smash_match_batch",
    "smash_pipeline_create", "smash_pipeline_free", "smash_count_batch",
    "smash_phase_map", "smash_phase_export", "smash_dedup_owner",
    "smash_phase_import", "smash_phase_positions", "smash_phase_bin",
    "smash_pipeline_stats", "smash_pipeline_reset", "smash_pipeline_reset_ex", "smash_pipeline_reads_resident", "smash_pipeline_peek",
    "smash_pipeline_var_len", "smash_pipeline_peek_lens", "smash_pipeline_peek_matches",
    "smash_pipeline_samples", "smash_pipeline_sample_stats",
    "smash_pipeline_samples_sharded", "smash_phase_hdr_words",
    "smash_pipeline_profile", "smash_pipeline_profile_read",
    "smash_pipeline_positions", "smash_bin_positions", "smash_mappability_scan",
    "smash_sam_records", "smash_sam_format", "smash_sam_free",
    "smash_fastq_open", "smash_fastq_read", "smash_fastq_close", "smash_strnum_order",
    "smash_count_fastq", "smash_count_batches", "smash_count_batches_ready",
    "smash_pipeline_profile_active",
    "smash_pipeline_profile_intervals", "smash_fastq_read_parallel",
    "smash_fastq_index_open", "smash_fastq_index_pack", "smash_fastq_index_close",
    "smash_phase_map_ahead", "smash_sam_records_packed",
    "smash_text_from_fasta_layout", "smash_index_create_layout", "smash_index_load_layout",
    "smash_phase_search_ahead",
    "smash_fastq_shard_scan", "smash_fastq_shard_free_blob", "smash_fastq_shard_open",
    "smash_fastq_shard_pack", "smash_fastq_shard_stats", "smash_fastq_shard_close",
    "smash_read_stride", "smash_pipeline_max_batch",
    "smash_mappability_prepare", "smash_mappability_window", "smash_index_pack",
    "smash_pipeline_reserve_keys", "smash_pipeline_key_capacity", "smash_pipeline_error",
    "smash_mappability_release", "smash_pipeline_map_hints",
    "smash_index_verify", "smash_index_load_verified",
    "smash_bins_apportion", "smash_bins_design_raw", "smash_bins_design", "smash_bins_tile",
]

# smash_index_verify / Index.load(verify=...): the checks to run
VERIFY_LAYOUT = 1   # contig table vs text, rc halves
VERIFY_SA = 2       # SA is the suffix array of the text, ISA its inverse
VERIFY_LCP = 4      # every LCP value exact, overflow table well-formed
VERIFY_MAP = 8      # map.bin equals the map recomputed from the index
VERIFY_ALL = 15


class IndexInfo(C.Structure):
    _fields_ = [("N", C.c_uint64), ("logN", C.c_uint64), ("idx_bytes", C.c_uint32),
                ("n_seq", C.c_uint32), ("n_lcp_overflow", C.c_uint64),
                ("map_bytes", C.c_uint64), ("d_text", vp), ("d_sa", vp),
                ("d_isa", vp), ("d_lcp8", vp), ("d_lcp_ovf", vp), ("d_map", vp),
                ("device_bytes", C.c_uint64), ("build_seconds", C.c_double),
                ("kmer_k", C.c_uint32), ("d_uniq", vp), ("d_kmer", vp),
                ("bitmap_b", C.c_uint32), ("d_bitmap", vp), ("in_text", C.c_uint64 * 4),
                ("rcref", C.c_uint32), ("pos_bits", C.c_uint32)]


class PipelineCfg(C.Structure):
    _fields_ = [("min_len", C.c_uint32), ("read_len", C.c_uint32),
                ("max_pairs", C.c_uint64), ("n_contig", C.c_uint32),
                ("h_tag_offsets", u32p), ("h_small_chr", u8p),
                ("h_chrom_off", i64p), ("nbins", C.c_uint32),
                ("h_bin_starts", i64p), ("min_excess", C.c_int32),
                ("hit_window", C.c_int64), ("dedup_capacity", C.c_uint64),
                ("read_stride", C.c_uint32)]


class FeedStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("batches", C.c_uint64), ("wall_s", C.c_double),
                ("ingest_s", C.c_double), ("wait_s", C.c_double), ("read_len", C.c_uint32),
                ("parallel", C.c_uint32), ("index_s", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShardStats(C.Structure):
    _fields_ = [("input_bytes", C.c_uint64), ("scan_segments", C.c_uint64),
                ("scan_bytes", C.c_uint64), ("scan_bytes_in", C.c_uint64), ("scan_s", C.c_double),
                ("pack_pairs", C.c_uint64), ("pack_bytes", C.c_uint64),
                ("pack_bytes_in", C.c_uint64), ("pack_s", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("key_pairs", C.c_uint64),
                ("dupe_pairs", C.c_uint64), ("positions", C.c_uint64),
                ("dups", C.c_uint64), ("kept", C.c_uint64),
                ("matches", C.c_uint64), ("error", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SampleStats(C.Structure):
    """smash_sample_stats: one sample's counters of a run with a sample table"""
    _fields_ = [("pairs", C.c_uint64), ("key_pairs", C.c_uint64),
                ("dupe_pairs", C.c_uint64), ("positions", C.c_uint64),
                ("dups", C.c_uint64), ("kept", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VerifyReport(C.Structure):
    """smash_verify_report: per check the number of findings and the smallest
    bad rank / text position / table entry / map.bin byte (~0: none)."""
    _fields_ = [("layout_bad", C.c_uint64), ("layout_first", C.c_uint64),
                ("perm_bad", C.c_uint64), ("perm_first", C.c_uint64),
                ("order_bad", C.c_uint64), ("order_first", C.c_uint64),
                ("lcp_bad", C.c_uint64), ("lcp_first", C.c_uint64),
                ("ovf_bad", C.c_uint64), ("ovf_first", C.c_uint64),
                ("map_bad", C.c_uint64), ("map_first", C.c_uint64),
                ("n_lcp255", C.c_uint64), ("lcp_irreducible", C.c_uint64),
                ("lcp_bytes_compared", C.c_uint64), ("lcp_longest", C.c_uint64),
                ("checked", C.c_uint32), ("ok", C.c_uint32), ("seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SmashError(RuntimeError):
    """report: the VerifyReport of a load the verifier rejected (else None)"""
    report = None


_LIB = None


def lib():
    """Load libsmashgpu.so (raises if it was not built: no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SmashError("libsmashgpu.so not built (run `make -C smash-paper_amd` "
                         "or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.smash_last_error.restype = C.c_char_p
    L.smash_text_from_fasta.argtypes = [C.c_char_p, C.POINTER(u8p), u64p, u32p,
                                        C.POINTER(u64p), C.POINTER(u64p),
                                        C.POINTER(C.POINTER(C.c_char_p))]
    L.smash_text_from_fasta_layout.argtypes = [C.c_char_p, C.c_int, C.POINTER(u8p), u64p, u32p,
                                               C.POINTER(u64p), C.POINTER(u64p),
                                               C.POINTER(C.POINTER(C.c_char_p))]
    L.smash_text_free.argtypes = [u8p, C.c_uint32, u64p, u64p, C.POINTER(C.c_char_p)]
    L.smash_text_free.restype = None
    L.smash_index_create.argtypes = [u8p, C.c_uint64, C.c_uint32, u64p, u64p,
                                     C.POINTER(C.c_char_p), C.c_int, C.POINTER(vp)]
    L.smash_index_create_layout.argtypes = [u8p, C.c_uint64, C.c_uint32, u64p, u64p,
                                            C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                            C.POINTER(vp)]
    L.smash_index_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.smash_index_load_layout.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.smash_index_verify.argtypes = [vp, C.c_uint32, C.POINTER(VerifyReport), vp]
    L.smash_index_load_verified.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32,
                                            C.POINTER(VerifyReport), C.POINTER(vp)]
    L.smash_index_save.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.smash_index_free.argtypes = [vp]
    L.smash_index_free.restype = None
    L.smash_index_query.argtypes = [vp, C.POINTER(IndexInfo)]
    L.smash_map_batch.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                  C.c_uint32, C.c_uint64, vp, C.c_uint32, vp, vp]
    L.smash_match_batch.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                    C.c_uint32, C.c_uint64, vp, C.c_uint32, vp, vp]
    L.smash_pipeline_create.argtypes = [vp, C.POINTER(PipelineCfg), C.POINTER(vp)]
    L.smash_pipeline_free.argtypes = [vp]
    L.smash_pipeline_free.restype = None
    L.smash_count_batch.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.smash_count_batches.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp]
    L.smash_count_batches_ready.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.smash_phase_map_ahead.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp]
    L.smash_phase_search_ahead.argtypes = [vp, vp, C.c_uint64, vp]
    L.smash_pipeline_profile_active.argtypes = [vp, C.POINTER(C.c_double)]
    L.smash_pipeline_profile_intervals.argtypes = [vp, C.POINTER(C.c_double), C.c_uint64, u64p]
    L.smash_phase_map.argtypes = [vp, vp, C.c_uint64, vp]
    L.smash_phase_export.argtypes = [vp, C.c_int, C.c_uint64, i64p, i64p, C.POINTER(vp),
                                     C.POINTER(vp), vp]
    L.smash_dedup_owner.argtypes = [vp, vp, C.c_uint64, vp, i64p, i64p, C.c_int, vp, vp]
    L.smash_phase_import.argtypes = [vp, vp, vp]
    L.smash_phase_positions.argtypes = [vp, vp, vp]
    L.smash_phase_bin.argtypes = [vp, vp, vp, vp]
    L.smash_pipeline_stats.argtypes = [vp, C.POINTER(Stats)]
    L.smash_pipeline_samples.argtypes = [vp, u64p, C.c_uint32]
    L.smash_pipeline_samples_sharded.argtypes = [vp, u64p, C.c_uint32]
    L.smash_phase_hdr_words.argtypes = [vp]
    L.smash_phase_hdr_words.restype = C.c_uint32
    L.smash_pipeline_sample_stats.argtypes = [vp, C.POINTER(SampleStats), C.c_uint32]
    L.smash_pipeline_reset.argtypes = [vp, vp]
    L.smash_pipeline_reset_ex.argtypes = [vp, C.c_uint32, vp]
    L.smash_pipeline_reads_resident.argtypes = [vp, C.c_int]
    L.smash_pipeline_peek.argtypes = [vp, i32p, u8p, u64p, u64p]
    L.smash_pipeline_var_len.argtypes = [vp, C.c_int]
    L.smash_pipeline_peek_lens.argtypes = [vp, C.POINTER(C.c_uint16)]
    L.smash_pipeline_profile.argtypes = [vp, C.c_int]
    L.smash_pipeline_profile_read.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p]
    L.smash_pipeline_positions.argtypes = [vp, i64p, i64p, C.c_uint64, u64p]
    L.smash_bin_positions.argtypes = [vp, vp, C.c_uint64, C.c_int64, vp, C.c_uint32, vp, u64p,
                                      vp]
    L.smash_mappability_scan.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, i64p, vp,
                                         C.c_uint32, vp, vp, vp]
    L.smash_sam_records.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp,
                                    C.c_uint32, vp, vp, vp, vp]
    L.smash_sam_records_packed.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp,
                                           C.c_uint32, vp, vp, vp, vp, vp]
    L.smash_sam_format.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, vp, u32p, C.c_uint32, C.c_uint64,
                                   C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                   C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                   u8p, C.POINTER(C.c_void_p), u64p, i32p]
    L.smash_sam_free.argtypes = [C.c_void_p]
    L.smash_sam_free.restype = None
    L.smash_fastq_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p),
                                   C.c_uint32, C.POINTER(vp)]
    L.smash_fastq_read.argtypes = [vp, C.c_uint64, u32p, vp, vp, C.c_uint32, u64p]
    L.smash_fastq_close.argtypes = [vp]
    L.smash_fastq_close.restype = None
    L.smash_strnum_order.argtypes = [vp, C.c_uint32, C.c_uint64, u64p]
    L.smash_fastq_index_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32,
                                         C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, u32p,
                                         C.c_int, C.POINTER(vp), u64p]
    L.smash_fastq_index_pack.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint32]
    L.smash_fastq_index_close.argtypes = [vp]
    L.smash_fastq_index_close.restype = None
    L.smash_fastq_read_parallel.argtypes = [C.POINTER(C.c_char_p), C.c_uint32,
                                            C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32,
                                            u32p, C.c_uint64, vp, vp, C.c_uint32, u64p]
    L.smash_fastq_shard_scan.argtypes = [C.POINTER(C.c_char_p), C.c_uint32,
                                         C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.POINTER(vp), u64p]
    L.smash_fastq_shard_free_blob.argtypes = [vp]
    L.smash_fastq_shard_free_blob.restype = None
    L.smash_fastq_shard_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32,
                                         C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.POINTER(vp), u64p, C.c_uint32, u32p,
                                         C.c_int, C.POINTER(vp), u64p]
    L.smash_fastq_shard_pack.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.smash_fastq_shard_stats.argtypes = [vp, C.POINTER(ShardStats)]
    L.smash_fastq_shard_close.argtypes = [vp]
    L.smash_fastq_shard_close.restype = None
    L.smash_read_stride.argtypes = [C.c_uint32]
    L.smash_read_stride.restype = C.c_uint32
    L.smash_mappability_prepare.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.smash_index_pack.argtypes = [vp, C.c_int, vp]
    L.smash_mappability_release.argtypes = [vp]
    L.smash_pipeline_reserve_keys.argtypes = [vp, C.c_uint64, vp]
    L.smash_pipeline_key_capacity.argtypes = [vp]
    L.smash_pipeline_key_capacity.restype = C.c_uint64
    L.smash_pipeline_map_hints.argtypes = [vp]
    L.smash_pipeline_map_hints.restype = C.c_int
    L.smash_pipeline_error.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    L.smash_mappability_window.argtypes = [vp, C.c_uint64, C.c_uint64, u64p, u64p]
    L.smash_pipeline_max_batch.argtypes = [C.c_uint32, C.c_uint32]
    L.smash_pipeline_max_batch.restype = C.c_uint64
    L.smash_count_fastq.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32,
                                    C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_uint32, vp,
                                    C.POINTER(FeedStats), vp]
    L.smash_bins_apportion.argtypes = [u64p, i64p, C.c_uint32, C.c_uint32, u32p]
    L.smash_bins_design_raw.argtypes = [C.c_int, vp, vp, C.c_uint32, u64p, u64p, i64p, C.c_uint32,
                                        C.c_uint32, vp, u64p, vp]
    L.smash_bins_design.argtypes = [vp, i64p, C.c_uint32, C.c_uint32, vp, u64p, vp]
    L.smash_bins_tile.argtypes = []
    L.smash_bins_tile.restype = C.c_uint32
    _LIB = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().smash_last_error().decode(errors="replace")
        e = SmashError("%s failed (%d): %s" % (what, rc, msg))
        e.code = rc
        raise e


def _p(a, t):
    return a.ctypes.data_as(t)


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return int(stream)


# ---------------------------------------------------------------------------
# reference text
# ---------------------------------------------------------------------------
_LOWER = np.arange(256, dtype=np.uint8)
_LOWER[ord("A"):ord("Z") + 1] += 32
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"acgtrymkbdhvACGTRYMKBDHV", b"tgcayrkmvhdbTGCAYRKMVHDB"):
    _COMP[_a] = _b


def text_from_fasta(path, rcref=True):
    """Sequence::Sequence (fasta.cpp:133-285), in the library: with -rcref
    (default) or the forward-only layout of `mummer` without it."""
    L = lib()
    t = u8p()
    N = C.c_uint64()
    ns = C.c_uint32()
    sp = u64p()
    sz = u64p()
    nm = C.POINTER(C.c_char_p)()
    check(L.smash_text_from_fasta_layout(path.encode(), 1 if rcref else 0, C.byref(t),
                                         C.byref(N), C.byref(ns), C.byref(sp), C.byref(sz),
                                         C.byref(nm)),
          "smash_text_from_fasta")
    T = np.ctypeslib.as_array(t, shape=(N.value,)).copy()
    startpos = np.ctypeslib.as_array(sp, shape=(ns.value,)).copy()
    sizes = np.ctypeslib.as_array(sz, shape=(ns.value,)).copy()
    names = [nm[i].decode() for i in range(ns.value)]
    L.smash_text_free(t, ns, sp, sz, nm)
    return T, startpos, sizes, names


def text_from_contigs(contigs):
    """The same text layout from in-memory contigs [(name, ASCII uint8)]."""
    parts, sp, sz, names = [], [], [], []
    pos = 0
    for k, (name, s) in enumerate(contigs):
        f = _LOWER[s]
        sp.append(pos); sz.append(len(f)); names.append(name)
        parts.append(f)
        parts.append(np.array([ord("`")], np.uint8))
        pos += len(f) + 1
        sp.append(pos); sz.append(len(f)); names.append(name)
        parts.append(_COMP[f[::-1]])
        pos += len(f)
        if k + 1 < len(contigs):
            parts.append(np.array([ord("`")], np.uint8))
            pos += 1
    parts.append(np.array([ord("$")], np.uint8))
    return (np.concatenate(parts), np.array(sp, np.uint64), np.array(sz, np.uint64),
            names)


def prepare_reads(seqs, max_len=None) -> np.ndarray:
    """fastqs_to_sam replaceN (N->Z, fastqs_to_sam.cpp:289) + NewQuery::extend
    lowercasing (query.cpp:125-144).  seqs: uint8 [n, L] ASCII, or -- with
    max_len -- a list of byte strings of mixed lengths (each at most max_len):
    rows of max_len bytes, zero padded past each mate, as a variable-length
    Pipeline (var_len=True) reads them."""
    if max_len is not None:
        if not 1 <= max_len <= 255:
            raise SmashError("prepare_reads: max_len must be 1..255")
        a = np.zeros((len(seqs), max_len), np.uint8)
        for i, q in enumerate(seqs):
            q = bytes(q)
            if len(q) > max_len:
                raise SmashError("prepare_reads: read %d has %d bases, max_len is %d"
                                 % (i, len(q), max_len))
            if 0 in q:
                raise SmashError("prepare_reads: read %d holds a zero byte" % i)
            a[i, :len(q)] = np.frombuffer(q, np.uint8)
        a[a == ord("N")] = ord("Z")
        return _LOWER[a]   # (0 stays 0)
    a = np.asarray(seqs, np.uint8).copy()
    a[a == ord("N")] = ord("Z")
    return _LOWER[a]


# ---------------------------------------------------------------------------
# index
# ---------------------------------------------------------------------------
class Index:
    """HBM-resident SA/ISA/LCP/text/map.bin (replaces longSA, longSA.cpp:94)."""

    def __init__(self, handle, names, sizes):
        self.h = vp(handle)
        self.info = IndexInfo()
        check(lib().smash_index_query(self.h, C.byref(self.info)), "smash_index_query")
        self.rcref = bool(self.info.rcref)
        self.names = list(names)
        self.sizes = [int(x) for x in sizes]
        step = 2 if self.rcref else 1
        self.contigs = [self.names[i] for i in range(0, len(self.names), step)]
        self.contig_sizes = self.sizes[0::step]

    @classmethod
    def create(cls, T, startpos, sizes, names, device=0, rcref=True):
        T = np.ascontiguousarray(T, np.uint8)
        sp = np.ascontiguousarray(startpos, np.uint64)
        sz = np.ascontiguousarray(sizes, np.uint64)
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        h = vp()
        check(lib().smash_index_create_layout(_p(T, u8p), len(T), len(sp), _p(sp, u64p),
                                              _p(sz, u64p), arr, 1 if rcref else 0, device,
                                              C.byref(h)),
              "smash_index_create")
        return cls(h.value, names, sz)

    @classmethod
    def from_fasta(cls, path, device=0, rcref=True):
        return cls.create(*text_from_fasta(path, rcref), device=device, rcref=rcref)

    @classmethod
    def from_contigs(cls, contigs, device=0):
        return cls.create(*text_from_contigs(contigs), device=device)

    @classmethod
    def load(cls, fasta_path, device=0, rcref=True, verify=0):
        """Load the reference's <fasta>.bin/ cache (longSA.cpp:100-136).
        verify: VERIFY_* flags (LAYOUT | SA | LCP at least) to prove the files
        on the device before anything is built from them
        (smash_index_load_verified); a rejected cache raises SmashError with
        .code SMASH_ERR_IO (-3) and the findings in .report; the report of an
        accepted one is the index's verify_report."""
        h = vp()
        rep = None
        if verify:
            rep = VerifyReport()
            rc = lib().smash_index_load_verified(fasta_path.encode(), 1 if rcref else 0, device,
                                                 verify, C.byref(rep), C.byref(h))
            if rc != 0:
                msg = lib().smash_last_error().decode(errors="replace")
                e = SmashError("smash_index_load_verified failed (%d): %s" % (rc, msg))
                e.code = rc
                e.report = rep if rep.checked else None
                raise e
        else:
            check(lib().smash_index_load_layout(fasta_path.encode(), 1 if rcref else 0, device,
                                                C.byref(h)),
                  "smash_index_load")
        ix = cls._loaded(h, fasta_path, rcref)
        ix.verify_report = rep
        return ix

    @classmethod
    def _loaded(cls, h, fasta_path, rcref):
        names, sizes = [], []
        with open(fasta_path + ".bin/rc%d.ref.bin" % (1 if rcref else 0), "rb") as f:
            b = f.read()
        n = int.from_bytes(b[16:24], "little")
        off = 24
        for _ in range(n):
            sizes.append(int.from_bytes(b[off + 8:off + 16], "little"))
            L = int.from_bytes(b[off + 16:off + 24], "little")
            names.append(b[off + 24:off + 24 + L].decode())
            off += 24 + L
        return cls(h.value, names, sizes)

    verify_report = None   # Index.load(verify=...): the accepted cache's report

    def verify(self, flags=VERIFY_ALL, stream=None):
        """smash_index_verify: prove the resident arrays against the resident
        text (read-only, synchronous).  Returns the VerifyReport; its ok is
        the verdict, its checked the flags that ran (MAP is skipped for an
        index without a map, and unless LAYOUT, SA and LCP ran clean)."""
        rep = VerifyReport()
        check(lib().smash_index_verify(self.h, flags, C.byref(rep), vp(_stream(stream))),
              "smash_index_verify")
        return rep

    def save(self, fasta_path, fasta_size=None):
        if fasta_size is None:
            fasta_size = os.path.getsize(fasta_path)
        check(lib().smash_index_save(self.h, fasta_path.encode(), fasta_size),
              "smash_index_save")

    @property
    def N(self):
        return self.info.N

    @property
    def pos_mask(self):
        """the element bits of an SA / ISA word (packed index words keep the
        search's hints above them, smash_index_info.pos_bits)"""
        b = self.info.pos_bits
        return (1 << b) - 1 if b else (1 << (8 * self.info.idx_bytes)) - 1

    def pack(self, on=True):
        """smash_index_pack: put the search's hints into the SA / ISA words
        (on) or strip them (results are the same either way)"""
        check(lib().smash_index_pack(self.h, 1 if on else 0, None), "smash_index_pack")
        check(lib().smash_index_query(self.h, C.byref(self.info)), "smash_index_query")

    def download_sa_isa(self, plain=True):
        """host copies of SA and ISA (u32 / u64 as in HBM); plain: the
        elements alone (the packed hints masked off)"""
        i = self.info
        dt = np.uint32 if i.idx_bytes == 4 else np.uint64
        SA = download(i.d_sa, i.N * i.idx_bytes, dt)
        ISA = download(i.d_isa, i.N * i.idx_bytes, dt)
        if plain and i.pos_bits:
            m = dt(self.pos_mask)
            np.bitwise_and(SA, m, out=SA)
            np.bitwise_and(ISA, m, out=ISA)
        return SA, ISA

    def design_bins(self, chrom_sizes_or_off, k=36, nbins=50000, stream=None, unique=False):
        """smash_bins_design: the variable-width bin table of this genome for
        k-mers of k bases and nbins bins -- every bin of a contig holds the
        same number of unique bases, up to one -- as a BIN record array in
        contig order.  chrom_sizes_or_off: the chrom_sizes dict (binned
        contigs by contig_tables' rule) or an int64 offset per contig (< 0:
        not binned).  unique=True: also the unique bases per contig."""
        if isinstance(chrom_sizes_or_off, dict):
            off = contig_tables(self.contigs, self.contig_sizes, chrom_sizes_or_off)[2]
        else:
            off = np.ascontiguousarray(chrom_sizes_or_off, np.int64)
        if len(off) != len(self.contigs):
            raise SmashError("design_bins: %d offsets for %d contigs" % (len(off), len(self.contigs)))
        out = np.zeros(int(nbins), BIN)
        M = np.zeros(len(off), np.uint64)
        check(lib().smash_bins_design(self.h, _p(off, i64p), k, int(nbins), _p(out, vp),
                                      _p(M, u64p), vp(_stream(stream))), "smash_bins_design")
        return (out, M) if unique else out

    def __del__(self):
        try:
            if self.h:
                lib().smash_index_free(self.h)
                self.h = None
        except Exception:
            pass


# ---------------------------------------------------------------------------
# read -> bin-count pipeline
# ---------------------------------------------------------------------------
MAJOR = re.compile(r"^chr(\d+|[XY])$")


def contig_tables(contigs, sizes, chrom_sizes):
    """Host-side per-contig tables of the reference glue:
    tag offsets = cumulative sam_header.txt lengths (chromosomes.h:169-196,
    index_setup.sh:31); small = '_gl000'/'chrM' (mappability_tag.cpp:82);
    chrom_off = chrom_sizes.txt offset when the perl filter
    ^chr(\\d+|[XY]) \\d+$ (smash_mapping.sh:29) and varbin's filters
    (varbin.py:38-49) keep the contig, else -1."""
    tag = np.cumsum([0] + [int(s) for s in sizes[:-1]]).astype(np.uint32)
    small = np.array([1 if ("_gl000" in c or "chrM" in c) else 0 for c in contigs], np.uint8)
    off = np.array([chrom_sizes[c] if (MAJOR.match(c) and "_" not in c and c != "chrM"
                                       and c in chrom_sizes) else -1 for c in contigs],
                   np.int64)
    return tag, small, off


def read_chrom_sizes(path):
    out = {}
    for line in open(path):
        c = line.rstrip("\n").split("\t")
        if c[0] in out:
            continue    # fileToDictionary keeps the first (varbin.py:131-146)
        out[c[0]] = int(c[2])
    return out


def read_bins(path):
    rows = [line.rstrip("\n").split("\t") for line in open(path)]
    return rows, np.array([int(r[2]) for r in rows], np.int64)


def read_stride(read_len):
    """bytes of the device's native row for a mate of read_len bases
    (smash_read_stride): batches laid out in such rows (16-byte aligned, zero
    padded) are searched without a record build"""
    return int(lib().smash_read_stride(read_len))


def pipeline_max_batch(read_len, min_len=20):
    """The largest batch (pairs) a Pipeline of read_len-base mates accepts:
    max_pairs * 2 * (read_len - min_len + 1) < 2^32 (include/smash_gpu.h)."""
    return int(lib().smash_pipeline_max_batch(read_len, min_len))


def to_rows(d_reads, read_len=None):
    """a [2n, L] uint8 device tensor of mates as the native rows [2n, stride]
    (zero padded; zero-padded mates of mixed lengths stay what they are)"""
    import torch
    L = read_len or d_reads.shape[1]
    rows = torch.zeros((d_reads.shape[0], read_stride(L)), dtype=torch.uint8, device=d_reads.device)
    rows[:, :L] = d_reads[:, :L]
    return rows


class Pipeline:
    """prepare_matches + mappability_tag + smashMEM + varbin on the device.
    read_stride: the bytes from one mate to the next in the batches (0:
    read_len, dense; read_stride(read_len): native rows, see to_rows)."""

    # u64 words per key in phase_export's headers (SMASH_EXPORT_HDR_WORDS) and
    # int64 words of phase_positions' tail / phase_bin's prev + 1; both grow
    # by the sample with a sharded sample table (set_samples_sharded)
    hdr_words = 1
    tail_words = 2

    def __init__(self, index: Index, chrom_sizes: dict, bin_starts, read_len,
                 max_pairs, min_len=20, min_excess=4, hit_window=10000,
                 dedup_capacity=None, read_stride=0, var_len=False):
        self.index = index
        sizes = index.contig_sizes
        self.tag, self.small, self.off = contig_tables(index.contigs, sizes, chrom_sizes)
        self.bins = np.ascontiguousarray(bin_starts, np.int64)
        self.cfg = PipelineCfg(min_len, read_len, max_pairs, len(index.contigs),
                               _p(self.tag, u32p), _p(self.small, u8p),
                               _p(self.off, i64p), len(self.bins), _p(self.bins, i64p),
                               min_excess, hit_window,
                               dedup_capacity or max_pairs, read_stride)
        h = vp()
        check(lib().smash_pipeline_create(index.h, C.byref(self.cfg), C.byref(h)),
              "smash_pipeline_create")
        self.h = h
        self.read_len = read_len
        self.stride = read_stride or read_len
        self.max_pairs = max_pairs
        self.slots = read_len - min_len + 1
        self.var_len = False
        self.n_samples = 0
        if var_len:
            self.set_var_len(True)

    def set_var_len(self, on=True):
        """variable-length mode (smash_pipeline_var_len): a mate's length is
        the offset of the first zero byte of its row, read_len the longest a
        mate can be (prepare_reads(list, max_len) builds such rows); between
        runs only"""
        check(lib().smash_pipeline_var_len(self.h, 1 if on else 0), "smash_pipeline_var_len")
        self.var_len = bool(on)

    def set_samples(self, first):
        """the sample table of the runs to come (smash_pipeline_samples):
        sample s is the run's pairs [first[s], first[s + 1]), first[0] = 0,
        ascending; None or an empty table: the plain run again.  Right after a
        reset (or before the first batch) only.  count_batch / count_batches
        then take a [len(first) - 1, nbins] counts tensor, one row per sample."""
        f = np.ascontiguousarray([] if first is None else first, np.uint64)
        if f.ndim != 1 or len(f) == 1:
            raise SmashError("set_samples: first holds the samples' starts and the run's end")
        n = max(len(f) - 1, 0)
        check(lib().smash_pipeline_samples(self.h, _p(f, u64p) if n else None, n),
              "smash_pipeline_samples")
        self.n_samples = n
        self._phase_mode()

    def set_samples_sharded(self, first):
        """the sample table of a multi-GPU run (smash_pipeline_samples_sharded):
        as set_samples, but over the global pair indexes of the whole run --
        (step, rank, pair), phase_export's global_base -- and the same on every
        rank.  The phase calls then work per sample: phase_export's headers
        have hdr_words = 2 words per key, phase_positions writes tail_words =
        3 words {count, last pos0, its sample}, phase_bin reads {pos0, sample}
        and adds into a [len(first) - 1, nbins] counts tensor; count_batch*
        are refused.  sample_stats() is this rank's share."""
        f = np.ascontiguousarray([] if first is None else first, np.uint64)
        if f.ndim != 1 or len(f) == 1:
            raise SmashError("set_samples_sharded: first holds the samples' starts and the "
                             "run's end")
        n = max(len(f) - 1, 0)
        check(lib().smash_pipeline_samples_sharded(self.h, _p(f, u64p) if n else None, n),
              "smash_pipeline_samples_sharded")
        self.n_samples = n
        self._phase_mode()

    def _phase_mode(self):
        """the phase buffers' widths for the table now set"""
        self.hdr_words = int(lib().smash_phase_hdr_words(self.h))
        self.tail_words = 3 if self.hdr_words > 1 else 2

    def sample_stats(self):
        """the per-sample counters so far, a list of SampleStats
        (smash_pipeline_sample_stats); synchronises"""
        out = (SampleStats * max(self.n_samples, 1))()
        check(lib().smash_pipeline_sample_stats(self.h, out, self.n_samples),
              "smash_pipeline_sample_stats")
        return list(out[:self.n_samples])

    def _counts(self, d_counts):
        """the counts' pointer; with a sample table set a tensor must hold a
        row of bins per sample (the kernels add into every sample's row)"""
        rows = self.n_samples
        if rows and d_counts is not None and not isinstance(d_counts, int):
            if d_counts.numel() < rows * len(self.bins) or d_counts.element_size() != 8 or \
                    not d_counts.is_contiguous():
                raise SmashError("counts tensor: %d x %d contiguous 64-bit counters needed"
                                 % (rows, len(self.bins)))
        return _ptr(d_counts)

    def count_batch(self, d_reads, n_pairs, d_counts, stream=None):
        """d_reads: device uint8 [2*n_pairs, read_len] (torch tensor or ptr);
        d_counts: int64 [nbins], or [samples, nbins] with a sample table set."""
        check(lib().smash_count_batch(self.h, _reads(d_reads, n_pairs, self.stride), n_pairs,
                                      self._counts(d_counts),
                                      vp(_stream(stream))), "smash_count_batch")

    def count_fastq(self, r1_paths, r2_paths, d_counts, sort_names=True, threads=0,
                    stream=None):
        """File-fed counting (smash_count_fastq): the two mate lists parsed,
        batched in pinned memory, copied and counted with overlap.
        sort_names=False: the input is in samtools sort -n order already.
        Returns the feed statistics (pairs, batches, wall_s, ingest_s, wait_s)."""
        arr1 = _cstrs([os.fsencode(x) for x in r1_paths])
        arr2 = _cstrs([os.fsencode(x) for x in r2_paths])
        st = FeedStats()
        T = threads or min(16, os.cpu_count() or 1)
        check(lib().smash_count_fastq(self.h, arr1, len(r1_paths), arr2, len(r2_paths),
                                      int(bool(sort_names)), T, _ptr(d_counts), C.byref(st),
                                      vp(_stream(stream))), "smash_count_fastq")
        return st.as_dict()

    def count_batches(self, d_reads, n_pairs, batch_pairs, d_counts, stream=None,
                      resident=False):
        """n_pairs resident pairs in batches (smash_count_batches): one batch's
        search overlaps the previous one's tail.  resident=True: the reads are
        complete already (smash_count_batches_ready, no input event), so the
        searches need not wait for the work queued on the stream before this
        call -- consecutive runs over the same reads overlap."""
        if resident:
            check(lib().smash_count_batches_ready(self.h, _reads(d_reads, n_pairs, self.stride),
                                                  n_pairs, batch_pairs,
                                                  self._counts(d_counts), vp(_stream(stream)),
                                                  None),
                  "smash_count_batches_ready")
            return
        check(lib().smash_count_batches(self.h, _reads(d_reads, n_pairs, self.stride), n_pairs,
                                        batch_pairs,
                                        self._counts(d_counts), vp(_stream(stream))),
              "smash_count_batches")

    def phase_map(self, d_reads, n_pairs, stream=None):
        check(lib().smash_phase_map(self.h, _reads(d_reads, n_pairs, self.stride), n_pairs,
                                    vp(_stream(stream))),
              "smash_phase_map")

    def phase_map_ahead(self, d_reads, n_pairs, d_next, n_next, stream=None):
        """phase_map, and the next batch's search issued at once on the
        pipeline's other search stream (smash_phase_map_ahead)."""
        check(lib().smash_phase_map_ahead(self.h, _reads(d_reads, n_pairs, self.stride), n_pairs,
                                          _reads(d_next, n_next, self.stride) if n_next else None,
                                          n_next,
                                          vp(_stream(stream))), "smash_phase_map_ahead")

    def phase_search_ahead(self, d_reads, n_pairs, stream=None):
        """after phase_export of batch b: batch b + 2's search into the set
        b used (smash_phase_search_ahead)."""
        check(lib().smash_phase_search_ahead(self.h, _reads(d_reads, n_pairs, self.stride), n_pairs,
                                             vp(_stream(stream))), "smash_phase_search_ahead")

    def phase_export(self, world, global_base, stream=None):
        """(headers [n, hdr_words] int64, words [w] int64, per-owner key counts,
        per-owner word counts) -- the tensors alias pipeline-owned device
        memory, valid until the next export."""
        import torch
        counts = np.zeros(world, np.int64)
        wcounts = np.zeros(world, np.int64)
        ds, dw = vp(), vp()
        check(lib().smash_phase_export(self.h, world, global_base, _p(counts, i64p),
                                       _p(wcounts, i64p), C.byref(ds), C.byref(dw),
                                       vp(_stream(stream))), "smash_phase_export")
        n, w = int(counts.sum()), int(wcounts.sum())
        H = self.hdr_words
        hdr = device_view(ds.value, 8 * H * n, torch.int64).view(n, H) if n else \
            torch.zeros((0, H), dtype=torch.int64, device="cuda")
        words = device_view(dw.value, 8 * w, torch.int64) if w else \
            torch.zeros(0, dtype=torch.int64, device="cuda")
        return hdr, words, counts, wcounts

    def dedup_owner(self, d_recv, n_recv, d_recv_words, recv_counts, recv_words, d_flags,
                    stream=None):
        rc = np.ascontiguousarray(recv_counts, np.int64)
        rw = np.ascontiguousarray(recv_words, np.int64)
        check(lib().smash_dedup_owner(self.h, _ptr(d_recv), n_recv, _ptr(d_recv_words),
                                      _p(rc, i64p), _p(rw, i64p), len(rc), _ptr(d_flags),
                                      vp(_stream(stream))), "smash_dedup_owner")

    def phase_import(self, d_flags_back, stream=None):
        check(lib().smash_phase_import(self.h, _ptr(d_flags_back), vp(_stream(stream))),
              "smash_phase_import")

    def phase_positions(self, d_tail, stream=None):
        """d_tail: int64 [tail_words]"""
        check(lib().smash_phase_positions(self.h, _ptr(d_tail), vp(_stream(stream))),
              "smash_phase_positions")

    def phase_bin(self, d_prev, d_counts, stream=None):
        """d_prev: int64 [tail_words - 1]; d_counts as count_batch's"""
        check(lib().smash_phase_bin(self.h, _ptr(d_prev), self._counts(d_counts),
                                    vp(_stream(stream))), "smash_phase_bin")

    def reset(self, stream=None, keep_search=False):
        """a new run (smash_pipeline_reset); keep_search: look-ahead searches
        already issued stay valid for it (smash_pipeline_reset_ex,
        SMASH_RESET_KEEP_SEARCH)"""
        if keep_search:
            check(lib().smash_pipeline_reset_ex(self.h, 1, vp(_stream(stream))),
                  "smash_pipeline_reset_ex")
        else:
            check(lib().smash_pipeline_reset(self.h, vp(_stream(stream))), "smash_pipeline_reset")

    def reads_resident(self, on=True):
        """the reads later given to the phase calls are resident and complete:
        their searches wait on no input event (smash_pipeline_reads_resident)"""
        check(lib().smash_pipeline_reads_resident(self.h, 1 if on else 0),
              "smash_pipeline_reads_resident")

    @property
    def map_hints(self):
        """the searches hand the matches' right map.bin bytes to the post
        stage (smash_pipeline_map_hints)"""
        return bool(lib().smash_pipeline_map_hints(self.h))

    @property
    def key_capacity(self):
        """keys the persistent pair-key set takes for sure"""
        return int(lib().smash_pipeline_key_capacity(self.h))

    def reserve_keys(self, keys, stream=None):
        """grow the key set to `keys` keys; held keys move into the larger set
        (smash_pipeline_reserve_keys)"""
        check(lib().smash_pipeline_reserve_keys(self.h, int(keys), vp(_stream(stream))),
              "smash_pipeline_reserve_keys")

    def data_error(self, stream=None):
        """the data error recorded by the work queued on `stream` (0: none);
        waits for that stream only (smash_pipeline_error)"""
        e = C.c_int32()
        check(lib().smash_pipeline_error(self.h, vp(_stream(stream)), C.byref(e)),
              "smash_pipeline_error")
        return int(e.value)

    def stats(self, raise_on_error=True):
        """Counters of the run so far.  A data error the device recorded (the
        mappability_tag throw, a full key set) raises SmashError unless
        raise_on_error=False, so no caller can read counts of a failed run."""
        s = Stats()
        check(lib().smash_pipeline_stats(self.h, C.byref(s)), "smash_pipeline_stats")
        if s.error and raise_on_error:
            raise SmashError("pipeline data error %d: %s" % (s.error, ERRORS.get(s.error, "?")))
        return s

    def profile(self, enable=True):
        check(lib().smash_pipeline_profile(self.h, int(enable)), "smash_pipeline_profile")

    def profile_read(self):
        """(summed k_mam milliseconds, launches, reads searched)"""
        ms = C.c_double()
        n = C.c_uint64()
        r = C.c_uint64()
        check(lib().smash_pipeline_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(r)),
              "smash_pipeline_profile_read")
        return ms.value, n.value, r.value

    def profile_active(self):
        """milliseconds during which at least one profiled search launch ran"""
        ms = C.c_double()
        check(lib().smash_pipeline_profile_active(self.h, C.byref(ms)),
              "smash_pipeline_profile_active")
        return ms.value

    def profile_intervals(self):
        """[(start, end)] ms of every profiled search launch, from the first start"""
        n = C.c_uint64()
        check(lib().smash_pipeline_profile_intervals(self.h, None, 0, C.byref(n)),
              "smash_pipeline_profile_intervals")
        out = (C.c_double * (2 * max(n.value, 1)))()
        check(lib().smash_pipeline_profile_intervals(self.h, out, n.value, C.byref(n)),
              "smash_pipeline_profile_intervals")
        return [(out[2 * i], out[2 * i + 1]) for i in range(n.value)]

    def positions(self):
        """(pos0, abspos) int64 arrays of the positions the last batch emitted
        (smash_pipeline_positions), in emission order."""
        n = C.c_uint64()
        check(lib().smash_pipeline_positions(self.h, None, None, 0, C.byref(n)),
              "smash_pipeline_positions")
        pos0 = np.zeros(n.value, np.int64)
        absp = np.zeros(n.value, np.int64)
        check(lib().smash_pipeline_positions(self.h, _p(pos0, i64p), _p(absp, i64p), n.value,
                                             C.byref(n)), "smash_pipeline_positions")
        return pos0, absp

    def peek(self, n_pairs):
        nk = np.zeros(n_pairs, np.int32)
        keep = np.zeros(n_pairs, np.uint8)
        hits = np.zeros(n_pairs * 2 * self.slots, np.uint64)
        check(lib().smash_pipeline_peek(self.h, _p(nk, i32p), _p(keep, u8p),
                                        _p(hits, u64p), None), "smash_pipeline_peek")
        return nk, keep, hits.reshape(n_pairs, 2 * self.slots)

    def peek_lens(self, n_pairs):
        """the last batch's 2 * n_pairs mate lengths as the device took them"""
        lens = np.zeros(2 * n_pairs, np.uint16)
        check(lib().smash_pipeline_peek_lens(self.h, _p(lens, C.POINTER(C.c_uint16))),
              "smash_pipeline_peek_lens")
        return lens

    def peek_matches(self, n_pairs):
        """the last batch's raw match words, [2 * n_pairs, slots], and the
        mates' match counts (smash_pipeline_peek_matches)"""
        words = np.zeros((2 * n_pairs, self.slots), np.uint64)
        n = np.zeros(2 * n_pairs, np.uint32)
        # (declared here: tools/ab.sh also loads builds from before this call)
        f = lib().smash_pipeline_peek_matches
        f.argtypes = [vp, u64p, C.POINTER(C.c_uint32)]
        check(f(self.h, _p(words, u64p), _p(n, C.POINTER(C.c_uint32))),
              "smash_pipeline_peek_matches")
        return words, n

    def close(self):
        """free the pipeline's device buffers now (its streams are
        synchronised first); the object is unusable afterwards"""
        if self.h:
            lib().smash_pipeline_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _reads(x, n_pairs, read_len):
    """the pointer of a batch of n_pairs pairs: a torch tensor must hold
    2 * n_pairs * read_len bytes (the kernels read that many; a short tensor
    would be an out-of-bounds device read), a raw pointer is the caller's
    responsibility"""
    if x is not None and not isinstance(x, int) and n_pairs:
        have = x.numel() * x.element_size()
        if have < 2 * n_pairs * read_len:
            raise SmashError("reads tensor holds %d bytes, %d pairs x %d bp need %d"
                             % (have, n_pairs, read_len, 2 * n_pairs * read_len))
    return _ptr(x)


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return vp(x)
    return vp(x.data_ptr())


def map_batch(index: Index, d_reads, n_reads, read_len, d_out, cap, d_n, min_len=20,
              stream=None, mode=SMASH_MODE_MAM, d_lens=None):
    """longSA::MAM over a batch (smash_map_batch).  d_lens: a device uint16
    length per read (rows of read_len bytes, each read at its row's start)."""
    check(lib().smash_map_batch(index.h, mode, min_len, _ptr(d_reads),
                                read_len, _ptr(d_lens), read_len, n_reads, _ptr(d_out), cap,
                                _ptr(d_n), vp(_stream(stream))), "smash_map_batch")


def match_batch(index: Index, d_reads, n_reads, read_len, d_out, cap, d_n, mode="MAM",
                min_len=20, stream=None):
    """longSA::MAM / MUM / MEM over a batch (smash_match_batch, memsam's default /
    -mum / -maxmatch).  d_out: int64 tensor of 2*cap*n_reads words (smash_match
    {u64 ref; u32 query; u32 len})."""
    check(lib().smash_match_batch(index.h, MODES.get(mode, mode), min_len, _ptr(d_reads),
                                  read_len, None, read_len, n_reads, _ptr(d_out), cap,
                                  _ptr(d_n), vp(_stream(stream))), "smash_match_batch")


def bin_positions(d_pos0, d_abspos, n, prev_pos0, d_bin_starts, nbins, d_counts, stream=None):
    """varbin.py's counting loop on the device (smash_bin_positions); returns
    [TotalReads, DupsRemoved, ReadsKept] of this call."""
    st = np.zeros(3, np.uint64)
    check(lib().smash_bin_positions(_ptr(d_pos0), _ptr(d_abspos), n, prev_pos0,
                                    _ptr(d_bin_starts), nbins, _ptr(d_counts), _p(st, u64p),
                                    vp(_stream(stream))), "smash_bin_positions")
    return [int(x) for x in st]


def mappability_scan(index: Index, begin, end, k=36, d_map_out=None, chrom_off=None,
                     d_bin_starts=None, nbins=0, d_bin_counts=None, d_contig_counts=None,
                     stream=None):
    """map.bin bytes of forward bases [begin, end) and unique-k-mer counts
    (smash_mappability_scan).  chrom_off: host int64 per contig or None."""
    off = None if chrom_off is None else np.ascontiguousarray(chrom_off, np.int64)
    check(lib().smash_mappability_scan(index.h, begin, end, k, _ptr(d_map_out),
                                       None if off is None else _p(off, i64p),
                                       _ptr(d_bin_starts), nbins, _ptr(d_bin_counts),
                                       _ptr(d_contig_counts), vp(_stream(stream))),
          "smash_mappability_scan")


# smash_bin (include/smash_gpu.h): one row of a designed bin table
BIN = np.dtype([("contig", "<u4"), ("reserved", "<u4"), ("start", "<u8"), ("stop", "<u8"),
                ("abspos", "<i8"), ("n_unique", "<u8"), ("n_gc", "<u8"), ("n_acgt", "<u8")])


def bins_tile():
    """bases per tile of the bin design's counting pass (smash_bins_tile)"""
    return int(lib().smash_bins_tile())


def bins_apportion(unique, chrom_off, nbins):
    """smash_bins_apportion (host code): the bins of each contig out of nbins
    from its unique bases -- one per binned contig (offset >= 0), the rest by
    largest remainder, ties to the earlier contig"""
    M = np.ascontiguousarray(unique, np.uint64)
    off = np.ascontiguousarray(chrom_off, np.int64)
    if len(M) != len(off):
        raise SmashError("bins_apportion: %d counts for %d offsets" % (len(M), len(off)))
    out = np.zeros(len(M), np.uint32)
    check(lib().smash_bins_apportion(_p(M, u64p), _p(off, i64p), len(M), int(nbins),
                                     _p(out, u32p)), "smash_bins_apportion")
    return out


def bins_design_raw(d_map2, d_text, sizes, text_start, chrom_off, k, nbins, device=0,
                    stream=None, unique=False):
    """smash_bins_design_raw: the bin table from a device image of [left,
    right] byte pairs per base of the concatenated forward contigs (a torch
    uint8 tensor or a pointer) and, optionally, the lowercase text (contig c
    at d_text + text_start[c]; None: n_gc = n_acgt = 0).  Returns a BIN record
    array of nbins rows (with unique=True also the unique bases per contig)."""
    sz = np.ascontiguousarray(sizes, np.uint64)
    off = np.ascontiguousarray(chrom_off, np.int64)
    ts = np.ascontiguousarray(text_start if text_start is not None else np.zeros(len(sz)),
                              np.uint64)
    if not (len(sz) == len(off) == len(ts)):
        raise SmashError("bins_design_raw: sizes, text_start and chrom_off differ in length")
    if d_map2 is not None and not isinstance(d_map2, int) and \
            d_map2.numel() * d_map2.element_size() < 2 * int(sz.sum()):
        raise SmashError("bins_design_raw: the map holds %d bytes, %d bases need %d"
                         % (d_map2.numel() * d_map2.element_size(), int(sz.sum()),
                            2 * int(sz.sum())))
    if d_text is not None and not isinstance(d_text, int) and len(sz) and \
            d_text.numel() * d_text.element_size() < int((ts + sz).max()):
        raise SmashError("bins_design_raw: the text ends before a contig does")
    out = np.zeros(int(nbins), BIN)
    M = np.zeros(len(sz), np.uint64)
    check(lib().smash_bins_design_raw(device, _ptr(d_map2), _ptr(d_text), len(sz), _p(sz, u64p),
                                      _p(ts, u64p), _p(off, i64p), k, int(nbins), _p(out, vp),
                                      _p(M, u64p), vp(_stream(stream))), "smash_bins_design_raw")
    return (out, M) if unique else out


def mappability_prepare(index: Index, begin, end, stream=None):
    """C5's preparation from the index arrays (smash_mappability_prepare):
    U and its directory for the scan of forward bases [begin, end), rebuilt
    from SA + the LCP bytes, in place."""
    check(lib().smash_mappability_prepare(index.h, begin, end, vp(_stream(stream))),
          "smash_mappability_prepare")


def mappability_release(index: Index):
    """free mappability_prepare's scratch HBM (smash_mappability_release)"""
    check(lib().smash_mappability_release(index.h), "smash_mappability_release")


def mappability_window(index: Index, begin, end):
    """the text window [lo, hi) mappability_prepare(begin, end) rebuilds"""
    lo, hi = C.c_uint64(), C.c_uint64()
    check(lib().smash_mappability_window(index.h, begin, end, C.byref(lo), C.byref(hi)),
          "smash_mappability_window")
    return int(lo.value), int(hi.value)


def unpack_records(words, n, cap):
    """smash_match records (2 u64 words each) -> [(ref, query, len)] (first min(n, cap))"""
    w = np.asarray(words, np.uint64).reshape(-1, 2)[:min(int(n), cap)]
    return [(int(a), int(b & 0xFFFFFFFF), int(b >> 32)) for a, b in w]


def unpack_matches(words, n):
    """packed u64 (ref 48 | qoff 8 | len 8) -> [(ref, qoff, len)]"""
    w = np.asarray(words[:n], np.uint64)
    return [(int(x & 0xFFFFFFFFFFFF), int((x >> 48) & 0xFF), int(x >> 56)) for x in w]


_HIP = None


class _DeviceArray:
    """__cuda_array_interface__ view of raw device memory (torch.as_tensor)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 3,
                                         "strides": None}


def device_view(dptr, nbytes, torch_dtype):
    """A torch tensor aliasing nbytes of device memory at dptr (no copy)."""
    import torch
    size = torch.tensor([], dtype=torch_dtype).element_size()
    ts = {1: "|u1", 4: "<i4", 8: "<i8"}[size]
    return torch.as_tensor(_DeviceArray(dptr, nbytes // size, ts), device="cuda")


def download(dptr, nbytes, dtype=np.uint8):
    """Device -> host copy of raw device memory (tests / index export)."""
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        _HIP.hipDeviceSynchronize.argtypes = []
    out = np.empty(nbytes, np.uint8)
    _HIP.hipDeviceSynchronize()
    rc = _HIP.hipMemcpy(out.ctypes.data_as(vp), vp(dptr), nbytes, 2)
    if rc != 0:
        raise SmashError("hipMemcpy D2H failed (%d)" % rc)
    return out.view(dtype)


SAM_REC = np.dtype([("pos", "<i8"), ("tid", "<u4"), ("xe", "<u4"), ("prefix", "<u2"),
                    ("len", "<u2"), ("suffix", "<u2"), ("qpos", "<u2"), ("rc", "u1"),
                    ("pad", "u1"), ("spare", "<u2"), ("left", "<i4"), ("right", "<i4"),
                    ("reserved", "<u4")])


def _cstrs(xs):
    if xs is None:
        return None
    return (C.c_char_p * len(xs))(*[None if x is None else bytes(x) for x in xs])


def sam_format(contigs, h_rec, h_n, cap, names, seqs, quals=None, optionals=None, nomap=True,
               tag=False, small_chr=None):
    """Host half of the mapout writer (smash_sam_format, query.cpp:231-415):
    SAM lines from the per-match records (read r's at r * cap, or packed read
    after read when cap is 0, as sam_records returns them); returns
    (bytes, tag_error)."""
    h_rec = np.ascontiguousarray(h_rec)
    h_n = np.ascontiguousarray(h_n, np.uint32)
    packed = cap == 0 or bool(cap & SAM_PACKED)
    need = int(h_n.astype(np.int64).sum()) if packed else len(names) * cap
    assert h_rec.nbytes >= need * SAM_REC.itemsize and len(h_n) == len(names)
    sm = None if small_chr is None else np.ascontiguousarray(small_chr, np.uint8)
    out = C.c_void_p()
    olen = C.c_uint64()
    terr = C.c_int32()
    check(lib().smash_sam_format(_cstrs([c.encode() for c in contigs]), len(contigs),
                                 _p(h_rec, vp), _p(h_n, u32p), cap, len(names), _cstrs(names),
                                 _cstrs(seqs), _cstrs(quals), _cstrs(optionals), int(nomap),
                                 int(tag), None if sm is None else _p(sm, u8p), C.byref(out),
                                 C.byref(olen), C.byref(terr)), "smash_sam_format")
    try:
        text = C.string_at(out.value, olen.value)
    finally:
        lib().smash_sam_free(out)
    return text, terr.value


def sam_records(index: Index, d_reads, n, read_len, cap, tag_offsets=None, min_len=20,
                stream=None, d_lens=None):
    """MAM search + per-match records on the device (smash_map_batch ->
    smash_sam_records_packed); returns host copies (SAM_REC[sum(counts)] packed
    read after read, counts[n]).  The record table is sized by the matches
    found (an exclusive scan of the counts), not by n * cap.  d_lens: a device
    uint16 length per read, in rows of read_len >= 255 bytes."""
    import torch
    dev = d_reads.device
    d_m = torch.empty(n * cap, dtype=torch.int64, device=dev)
    d_n = torch.empty(n, dtype=torch.int32, device=dev)
    map_batch(index, d_reads, n, read_len, d_m, cap, d_n, min_len=min_len, stream=stream,
              d_lens=d_lens)
    cnt = d_n.to(torch.int64).clamp_(max=cap)
    d_off = torch.cumsum(cnt, 0) - cnt
    total = int(cnt.sum().item()) if n else 0
    d_rec = torch.empty(max(total, 1) * SAM_REC.itemsize, dtype=torch.uint8, device=dev)
    d_tag = None
    if tag_offsets is not None:
        d_tag = torch.from_numpy(np.ascontiguousarray(tag_offsets, np.uint32).view(np.int32)).to(dev)
    check(lib().smash_sam_records_packed(index.h, _ptr(d_reads), read_len, _ptr(d_lens), read_len, n, _ptr(d_m),
                                         cap, _ptr(d_n), _ptr(d_off), _ptr(d_tag), _ptr(d_rec),
                                         vp(_stream(stream))),
          "smash_sam_records_packed")
    torch.cuda.synchronize(dev)
    h_n = d_n.cpu().numpy().view(np.uint32).copy()
    if (h_n > cap).any():
        raise SmashError("sam_records: a read has more matches than cap")
    return d_rec[:total * SAM_REC.itemsize].cpu().numpy().view(SAM_REC), h_n


def sam_lines(index: Index, d_reads, read_len, names, seqs, quals=None, optionals=None,
              nomap=True, tag_offsets=None, small_chr=None, cap=None, min_len=20, stream=None,
              lens=None):
    """memsam `-rcref -samin -samout [-nomap]` lines for 2n mates (read 1, read 2 of
    each pair, names with the ':0'/':1' suffix of query.cpp:641-642): the MAM search
    (smash_map_batch), the per-match records on the device (smash_sam_records) and
    the host formatting of print_matches (query.cpp:331-415).  With tag_offsets
    (u32 sam_header offsets per forward contig) the mappability_tag L/R columns
    are appended (mappability_tag.cpp:93-124).  Returns (bytes, tag_error).
    lens: the reads' own lengths (mixed): d_reads is then [2n, read_len >= 255]
    with each read at its row's start."""
    n = len(names)
    d_lens = None
    if lens is not None:
        import torch
        lens = np.ascontiguousarray(lens, np.uint16)
        if len(lens) != n or read_len < 255 or (n and int(lens.max()) > 255):
            raise SmashError("sam_lines: one length (<= 255) per read, rows of >= 255 bytes")
        d_lens = torch.from_numpy(lens.view(np.int16)).to(d_reads.device)
    if cap is None and lens is not None:
        cap = max(1, (int(lens.max()) if n else 0) - min_len + 1)
    if cap is None:
        cap = read_len - min_len + 1
    h_rec, h_n = sam_records(index, d_reads, n, read_len, cap, tag_offsets, min_len, stream,
                             d_lens=d_lens)
    return sam_format(index.contigs, h_rec, h_n, SAM_PACKED | cap, names, seqs, quals, optionals,
                      nomap, tag_offsets is not None, small_chr)


def read_fastq_pairs(r1_paths, r2_paths, batch_pairs=1 << 20, name_stride=64, read_len=0):
    """All pairs of the two FASTQ lists through the native reader
    (smash_fastq_*): (names[n] as a fixed-width bytes array, reads[2n, L] u8
    after replaceN + lowercasing), in file order.  read_len: 0 (the first
    pair's length, which every mate must have), a required length, or
    SMASH_LEN_VAR | M: mates of 1..M bases in zero-padded rows of M bytes."""
    arr1 = _cstrs([p.encode() for p in r1_paths])
    arr2 = _cstrs([p.encode() for p in r2_paths])
    h = vp()
    check(lib().smash_fastq_open(arr1, len(r1_paths), arr2, len(r2_paths), C.byref(h)),
          "smash_fastq_open")
    try:
        L = C.c_uint32(read_len)
        reads, names = [], []
        while True:
            cap_len = (L.value & ~SMASH_LEN_VAR) or 255
            L = C.c_uint32(L.value | (read_len & SMASH_LEN_VAR))   # (cleared on return)
            rb = np.empty(2 * batch_pairs * cap_len, np.uint8)
            nb = np.zeros(batch_pairs, "S%d" % name_stride)
            n = C.c_uint64()
            check(lib().smash_fastq_read(h, batch_pairs, C.byref(L), _p(rb, vp), _p(nb, vp),
                                         name_stride, C.byref(n)), "smash_fastq_read")
            k = n.value
            if k:
                reads.append(rb[:2 * k * L.value].reshape(2 * k, L.value).copy())
                names.append(nb[:k].copy())
            if k < batch_pairs:
                break
    finally:
        lib().smash_fastq_close(h)
    if not reads:
        return np.zeros(0, "S%d" % name_stride), np.zeros((0, 0), np.uint8)
    return np.concatenate(names), np.concatenate(reads)


def read_fastq_pairs_parallel(r1_paths, r2_paths, threads=0, name_stride=64, read_len=0):
    """read_fastq_pairs through the parallel reader (smash_fastq_read_parallel):
    strict 4-line FASTQ only (SmashError SMASH_ERR_UNSUPPORTED otherwise).
    read_len as read_fastq_pairs', and SMASH_LEN_VAR alone: rows as wide as
    the input's longest mate."""
    arr1 = _cstrs([os.fsencode(p) for p in r1_paths])
    arr2 = _cstrs([os.fsencode(p) for p in r2_paths])
    T = threads or min(16, os.cpu_count() or 1)
    L = C.c_uint32(read_len)
    n = C.c_uint64()
    check(lib().smash_fastq_read_parallel(arr1, len(r1_paths), arr2, len(r2_paths), T, C.byref(L),
                                          0, None, None, name_stride, C.byref(n)),
          "smash_fastq_read_parallel")
    k = n.value
    rb = np.empty((2 * max(k, 1), max(L.value, 1)), np.uint8)
    nb = np.zeros(max(k, 1), "S%d" % name_stride)
    W = L.value                                            # (the first call returned the width)
    L = C.c_uint32(W | (read_len & SMASH_LEN_VAR))
    check(lib().smash_fastq_read_parallel(arr1, len(r1_paths), arr2, len(r2_paths), T, C.byref(L),
                                          k, _p(rb, vp), _p(nb, vp), name_stride, C.byref(n)),
          "smash_fastq_read_parallel")
    if not k:
        return np.zeros(0, "S%d" % name_stride), np.zeros((0, 0), np.uint8)
    return nb[:k], rb[:2 * k, :L.value]


class FastqIndex:
    """Both FASTQ lists indexed once by the parallel reader
    (smash_fastq_index_*): .n pairs of .L bases in samtools sort -n order;
    pack(k0, k1, out) fills a [2 (k1 - k0), L] uint8 array (or a pinned CPU
    tensor) with planned pairs [k0, k1).  Strict 4-line FASTQ only.
    read_len = SMASH_LEN_VAR | M (M = 0: the longest mate): mixed lengths,
    .L = the row width, every row zero padded past its mate."""

    def __init__(self, r1_paths, r2_paths, threads=0, read_len=0, sort_names=False):
        a1 = _cstrs([os.fsencode(p) for p in r1_paths])
        a2 = _cstrs([os.fsencode(p) for p in r2_paths])
        T = threads or min(16, os.cpu_count() or 1)
        L = C.c_uint32(read_len)
        n = C.c_uint64()
        h = vp()
        check(lib().smash_fastq_index_open(a1, len(r1_paths), a2, len(r2_paths), T, C.byref(L),
                                           int(bool(sort_names)), C.byref(h), C.byref(n)),
              "smash_fastq_index_open")
        self.h, self.n, self.L = h, n.value, L.value

    def pack(self, k0, k1, out):
        ptr = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
        check(lib().smash_fastq_index_pack(self.h, k0, k1, vp(ptr), None, 0),
              "smash_fastq_index_pack")
        return out

    def close(self):
        if self.h:
            lib().smash_fastq_index_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SMASH_ERR_ARG = -1
SMASH_ERR_NOMEM = -4
SMASH_ERR_UNSUPPORTED = -5


class FastqShards:
    """The rank-local reader of the multi-GPU driver (smash_fastq_shard_*):
    this rank scans only its share of the segments of both FASTQ lists,
    `allgather(bytes) -> [bytes of rank 0, ..., rank world-1]` exchanges the
    scans, and every rank gets the same plan.  Same interface as FastqIndex
    (.n planned pairs of .L bases, pack(k0, k1, out)), but a pack reads only
    the bytes of the pairs asked for.  Raises SmashError with .code
    SMASH_ERR_UNSUPPORTED where FastqIndex must take over (input not strict
    4-line FASTQ, or not in samtools sort -n order when sort_names)."""

    def __init__(self, r1_paths, r2_paths, rank, world, allgather, threads=0, read_len=0,
                 sort_names=False):
        a1 = _cstrs([os.fsencode(p) for p in r1_paths])
        a2 = _cstrs([os.fsencode(p) for p in r2_paths])
        T = threads or min(16, os.cpu_count() or 1)
        blob, nb = vp(), C.c_uint64()
        L = lib()
        rc = L.smash_fastq_shard_scan(a1, len(r1_paths), a2, len(r2_paths), world, rank, T,
                                      C.byref(blob), C.byref(nb))
        mine = b""
        err = None
        if rc == 0:
            mine = C.string_at(blob.value, nb.value)
            L.smash_fastq_shard_free_blob(blob)
        else:
            err = (rc, L.smash_last_error().decode(errors="replace"))
        blobs = allgather(mine)     # every rank joins, even after a local failure
        if err is not None:
            e = SmashError("smash_fastq_shard_scan failed (%d): %s" % err)
            e.code = err[0]
            raise e
        if any(len(b) == 0 for b in blobs):
            e = SmashError("smash_fastq_shard_scan failed on another rank")
            e.code = -1
            raise e
        bufs = [C.create_string_buffer(b, len(b)) for b in blobs]
        ptrs = (vp * world)(*[C.cast(b, vp) for b in bufs])
        sizes = np.array([len(b) for b in blobs], np.uint64)
        Lr = C.c_uint32(read_len)
        n = C.c_uint64()
        h = vp()
        rc = L.smash_fastq_shard_open(a1, len(r1_paths), a2, len(r2_paths), world, rank, ptrs,
                                      _p(sizes, u64p), T, C.byref(Lr), int(bool(sort_names)),
                                      C.byref(h), C.byref(n))
        if rc != 0:
            e = SmashError("smash_fastq_shard_open failed (%d): %s"
                           % (rc, L.smash_last_error().decode(errors="replace")))
            e.code = rc
            raise e
        self.h, self.n, self.L = h, n.value, Lr.value

    def pack(self, k0, k1, out):
        ptr = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
        check(lib().smash_fastq_shard_pack(self.h, k0, k1, vp(ptr)), "smash_fastq_shard_pack")
        return out

    def stats(self):
        st = ShardStats()
        check(lib().smash_fastq_shard_stats(self.h, C.byref(st)), "smash_fastq_shard_stats")
        return st.as_dict()

    def close(self):
        if self.h:
            lib().smash_fastq_shard_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def first_read_length(paths):
    """bases in the first record of the first file (FASTQ / FASTA, gzip or
    plain): the read length a file-fed pipeline is built for."""
    import gzip
    with open(paths[0], "rb") as f:
        magic = f.read(2)
    op = gzip.open if magic == b"\x1f\x8b" else open
    with op(paths[0], "rb") as f:
        for line in f:
            t = line.strip()
            if not t:
                continue
            if t[:1] not in (b"@", b">"):
                raise SmashError("%s: not FASTQ / FASTA" % paths[0])
            return len(next(f).rstrip(b"\r\n"))
    raise SmashError("%s: no records" % paths[0])


def strnum_order(names):
    """Stable `samtools sort -n` order of a fixed-width bytes array
    (smash_strnum_order)."""
    names = np.ascontiguousarray(names)
    perm = np.empty(len(names), np.uint64)
    check(lib().smash_strnum_order(_p(names, vp), names.dtype.itemsize, len(names),
                                   _p(perm, u64p)), "smash_strnum_order")
    return perm.astype(np.int64)
