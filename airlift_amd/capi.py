"""ctypes mirror of include/airlift.h (names and argument meaning follow the C-ABI, which in turn
follows the reference's minimap.h for this path)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class AirliftError(RuntimeError):
    pass


# mapping option flags (include/airlift.h; the values of the fork's MM_F_*)
AL_F_CIGAR = 0x004
AL_F_OUT_SAM = 0x008
AL_F_OUT_CG = 0x020
AL_F_OUT_CS = 0x40
AL_F_OUT_CS_LONG = 0x800
AL_F_SR = 0x1000
AL_F_FRAG_MODE = 0x2000
AL_F_NO_PRINT_2ND = 0x4000
AL_F_SOFTCLIP = 0x80000
AL_F_HEAP_SORT = 0x400000
AL_F_OUT_MD = 0x1000000
AL_F_EQX = 0x4000000
AL_F_PAF_NO_HIT = 0x8000000
AL_F_SAM_HIT_ONLY = 0x40000000
AL_F_OUT_PAF = 0x100000000   # ours (above the fork's 32 bits): PAF output; only with it is AL_F_CIGAR looked at (clear = map-only)
AL_F_IN_GPU_INFLATE = 0x200000000   # ours: BGZF FASTQ input of the file-mapping calls inflated on the GPU by the stream driver (--gpu-inflate)


def lib_path():
    # AIRLIFT_LIB: another build of the same library (A/B timing of kernel variants on one GPU box)
    return os.environ.get("AIRLIFT_LIB") or os.path.join(HERE, "lib", "libairlift.so")


def build(verbose=False):
    """Compile every HIP source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-s", "-j4", "-C", os.path.join(HERE, "csrc")], capture_output=not verbose)
    if r.returncode != 0:
        raise AirliftError("build failed:\n" + (r.stderr.decode() if r.stderr else ""))
    return lib_path()


class IdxOpt(C.Structure):
    _fields_ = [("k", C.c_short), ("w", C.c_short), ("flag", C.c_short), ("bucket_bits", C.c_short),
                ("mini_batch_size", C.c_int), ("batch_size", C.c_uint64)]


class MapOpt(C.Structure):
    _fields_ = [("flag", C.c_int64), ("seed", C.c_int), ("bw", C.c_int), ("max_gap", C.c_int), ("max_gap_ref", C.c_int),
                ("max_frag_len", C.c_int), ("max_chain_skip", C.c_int), ("max_chain_iter", C.c_int), ("min_cnt", C.c_int),
                ("min_chain_score", C.c_int), ("mask_level", C.c_float), ("pri_ratio", C.c_float), ("best_n", C.c_int),
                ("a", C.c_int), ("b", C.c_int), ("q", C.c_int), ("e", C.c_int), ("q2", C.c_int), ("e2", C.c_int),
                ("sc_ambi", C.c_int), ("zdrop", C.c_int), ("zdrop_inv", C.c_int), ("end_bonus", C.c_int), ("min_dp_max", C.c_int),
                ("max_clip_ratio", C.c_float), ("pe_ori", C.c_int), ("pe_bonus", C.c_int), ("mid_occ", C.c_int32),
                ("max_occ", C.c_int32), ("mini_batch_size", C.c_int)]


class Reg(C.Structure):
    _fields_ = [("id", C.c_int32), ("cnt", C.c_int32), ("rid", C.c_int32), ("score", C.c_int32),
                ("qs", C.c_int32), ("qe", C.c_int32), ("rs", C.c_int32), ("re", C.c_int32),
                ("parent", C.c_int32), ("subsc", C.c_int32), ("mlen", C.c_int32), ("blen", C.c_int32),
                ("n_sub", C.c_int32), ("score0", C.c_int32),
                ("mapq", C.c_uint32, 8), ("split", C.c_uint32, 2), ("rev", C.c_uint32, 1), ("inv", C.c_uint32, 1),
                ("sam_pri", C.c_uint32, 1), ("proper_frag", C.c_uint32, 1), ("pe_thru", C.c_uint32, 1), ("seg_split", C.c_uint32, 1),
                ("seg_id", C.c_uint32, 8), ("split_inv", C.c_uint32, 1), ("dummy", C.c_uint32, 7),
                ("hash", C.c_uint32), ("dp_score", C.c_int32), ("dp_max", C.c_int32), ("dp_max2", C.c_int32),
                ("n_ambi", C.c_uint32), ("n_cigar", C.c_uint32), ("cigar", C.POINTER(C.c_uint32))]


class BatchStat(C.Structure):
    _fields_ = [("n_frag", C.c_uint64), ("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_mini", C.c_uint64),
                ("n_anchor", C.c_uint64), ("n_chain", C.c_uint64), ("n_regs_aln", C.c_uint64), ("n_refbases", C.c_uint64),
                ("n_cigar", C.c_uint64), ("n_rechain", C.c_uint64), ("n_heap_fallback", C.c_uint64), ("n_sort_tie_flag", C.c_uint64),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("algorithmic_bytes", C.c_double),
                ("ms_total", C.c_float), ("ms_kernel", C.c_float * 40), ("n_stage", C.c_int), ("ms_side_stream", C.c_float), ("n_chain_fallback", C.c_uint64),
                ("dp_jobs", C.c_uint64 * 10), ("dp_target_bases", C.c_uint64 * 10)]


class LiftStat(C.Structure):
    """AlLiftStat of al_lift_bam."""
    _fields_ = [("kept", C.c_uint64), ("unlifted", C.c_uint64), ("unmapped_kept", C.c_uint64), ("pieces", C.c_uint64), ("bytes_in", C.c_uint64), ("held", C.c_uint64),
                ("read_s", C.c_double), ("up_s", C.c_double), ("inflate_s", C.c_double), ("walk_s", C.c_double), ("lift_s", C.c_double), ("down_s", C.c_double),
                ("deflate_s", C.c_double), ("wall_s", C.c_double), ("on_device", C.c_int)]


LIFT_HOST = 1                 # AL_LIFT_HOST of include/airlift.h
LIFT_GPU_DEFLATE = 2          # AL_LIFT_GPU_DEFLATE
LIFT_SORTED = 4               # AL_LIFT_SORTED: the lifted BAM in coordinate order


class MergeStat(C.Structure):
    """AlMergeStat of al_merge_bams."""
    _fields_ = [("n_in", C.c_uint64), ("records", C.c_uint64), ("rounds", C.c_uint64), ("refills", C.c_uint64), ("bytes_in", C.c_uint64), ("held", C.c_uint64),
                ("records_in", C.c_uint64 * 8),
                ("read_s", C.c_double), ("up_s", C.c_double), ("inflate_s", C.c_double), ("walk_s", C.c_double), ("key_s", C.c_double), ("merge_s", C.c_double), ("gather_s", C.c_double),
                ("down_s", C.c_double), ("deflate_s", C.c_double), ("wall_s", C.c_double), ("on_device", C.c_int)]


MERGE_HOST = 1                # AL_MERGE_HOST of include/airlift.h
MERGE_GPU_DEFLATE = 2         # AL_MERGE_GPU_DEFLATE
MERGE_WRITE_INDEX = 4         # AL_MERGE_WRITE_INDEX: bam_out + ".bai" as index_bam writes it
LIFT_WRITE_INDEX = 8          # AL_LIFT_WRITE_INDEX: the same for al_lift_bam, with LIFT_SORTED only


class BaiStat(C.Structure):
    """AlBaiStat of al_index_bam."""
    _fields_ = [("records", C.c_uint64), ("unplaced", C.c_uint64), ("pieces", C.c_uint64), ("bytes_in", C.c_uint64), ("chunks", C.c_uint64), ("bai_bytes", C.c_uint64), ("held", C.c_uint64),
                ("read_s", C.c_double), ("up_s", C.c_double), ("inflate_s", C.c_double), ("walk_s", C.c_double), ("key_s", C.c_double), ("assemble_s", C.c_double), ("wall_s", C.c_double),
                ("on_device", C.c_int)]


BAI_HOST = 1                  # AL_BAI_HOST of include/airlift.h


def index_bam(bam, bai=None, flags=0, device=-1, n_threads=3, piece_bytes=0):
    """al_index_bam: the BAI of the coordinate-sorted BAM `bam` written to `bai` (None: bam + ".bai").  Returns the BaiStat."""
    st = BaiStat()
    rc = load().al_index_bam(os.fsencode(bam), None if bai is None else os.fsencode(bai), flags, device, n_threads, piece_bytes, C.byref(st))
    if rc != 0:
        raise AirliftError("al_index_bam failed: %d" % rc)
    return st


def merge_bams(bams_in, bam_out, flags=0, device=-1, n_threads=3, level=5, piece_bytes=0):
    """al_merge_bams: the coordinate-sorted BAMs `bams_in` merged into `bam_out`.  Returns the MergeStat."""
    st = MergeStat()
    arr = (C.c_char_p * len(bams_in))(*[os.fsencode(b) for b in bams_in])
    rc = load().al_merge_bams(arr, len(bams_in), os.fsencode(bam_out), flags, device, n_threads, level, piece_bytes, C.byref(st))
    if rc != 0:
        raise AirliftError("al_merge_bams failed: %d" % rc)
    return st


def lift_bam(bam_in, chain, bam_out, bed_out, flags=0, device=-1, n_threads=3, level=5, piece_bytes=0):
    """al_lift_bam: the constant-region reads of `bam_in` moved across `chain` into `bam_out`, the reads that do not lift as rows of `bed_out`.  Returns the LiftStat."""
    st = LiftStat()
    rc = load().al_lift_bam(os.fsencode(bam_in), os.fsencode(chain), os.fsencode(bam_out), os.fsencode(bed_out), flags, device, n_threads, level, piece_bytes, C.byref(st))
    if rc != 0:
        raise AirliftError("al_lift_bam failed: %d" % rc)
    return st


_lib = None


def load():
    """dlopen libairlift.so; fails loudly if it is missing (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise AirliftError("libairlift.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)")
    L = C.CDLL(p)
    vp, ci, cs = C.c_void_p, C.c_int, C.c_char_p
    L.al_set_opt.argtypes = [cs, C.POINTER(IdxOpt), C.POINTER(MapOpt)]; L.al_set_opt.restype = ci
    L.al_check_opt.argtypes = [C.POINTER(IdxOpt), C.POINTER(MapOpt)]; L.al_check_opt.restype = ci
    L.al_idx_build.argtypes = [cs, C.POINTER(IdxOpt), ci]; L.al_idx_build.restype = vp
    L.al_idx_build_device.argtypes = [cs, C.POINTER(IdxOpt), ci]; L.al_idx_build_device.restype = vp
    L.al_idx_export_pos.argtypes = [vp, vp, C.c_int64]; L.al_idx_export_pos.restype = C.c_int64
    L.al_ctx_set_threads.argtypes = [vp, ci]; L.al_ctx_set_threads.restype = None
    L.al_batch_count_candidates.argtypes = [vp, C.POINTER(C.c_int64)]; L.al_batch_count_candidates.restype = ci
    L.al_count_candidates_file.argtypes = [vp, cs, C.POINTER(MapOpt), ci, ci, C.POINTER(C.c_int64)]; L.al_count_candidates_file.restype = ci
    L.al_idx_str.argtypes = [ci, ci, ci, C.POINTER(cs), C.POINTER(cs)]; L.al_idx_str.restype = vp
    L.al_idx_destroy.argtypes = [vp]; L.al_idx_destroy.restype = None
    L.al_idx_n_seq.argtypes = [vp]; L.al_idx_n_seq.restype = C.c_uint32
    L.al_idx_seq_name.argtypes = [vp, C.c_uint32]; L.al_idx_seq_name.restype = cs
    L.al_idx_seq_len.argtypes = [vp, C.c_uint32]; L.al_idx_seq_len.restype = C.c_uint32
    L.al_idx_stat.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]; L.al_idx_stat.restype = None
    L.al_ctx_init.argtypes = [vp, C.POINTER(MapOpt), ci]; L.al_ctx_init.restype = vp
    L.al_ctx_destroy.argtypes = [vp]; L.al_ctx_destroy.restype = None
    L.al_batch_upload.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(cs), C.POINTER(cs)]; L.al_batch_upload.restype = ci
    L.al_batch_run.argtypes = [vp]; L.al_batch_run.restype = ci
    L.al_batch_fetch.argtypes = [vp, C.POINTER(ci), C.POINTER(C.POINTER(Reg)), C.POINTER(ci)]; L.al_batch_fetch.restype = ci
    L.al_map_batch.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(cs), C.POINTER(cs), C.POINTER(ci), C.POINTER(C.POINTER(Reg)), C.POINTER(ci)]
    L.al_map_batch.restype = ci
    L.al_map_frag.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(cs), C.POINTER(ci), C.POINTER(C.POINTER(Reg)), vp, C.POINTER(MapOpt), cs]; L.al_map_frag.restype = None
    L.al_map_file_frag.argtypes = [vp, ci, C.POINTER(cs), C.POINTER(MapOpt), ci, vp, cs, ci]; L.al_map_file_frag.restype = ci
    L.al_map_file_frag_bam.argtypes = [vp, ci, C.POINTER(cs), C.POINTER(MapOpt), ci, vp, cs, ci, ci, ci]; L.al_map_file_frag_bam.restype = ci
    L.al_map_tokens_file.argtypes = [vp, cs, ci, ci, C.POINTER(MapOpt), ci, vp, cs, ci]; L.al_map_tokens_file.restype = ci
    L.al_device_reserve.argtypes = [ci, C.c_uint64]; L.al_device_reserve.restype = ci
    L.al_device_reserve_peak.argtypes = []; L.al_device_reserve_peak.restype = C.c_uint64
    L.al_device_reserve_report.argtypes = [vp]; L.al_device_reserve_report.restype = None   # (a FILE *)
    L.al_winsrc_create.argtypes = [vp, cs, C.c_uint64]; L.al_winsrc_create.restype = vp
    L.al_winsrc_destroy.argtypes = [vp]; L.al_winsrc_destroy.restype = None
    L.al_batch_upload_windows.argtypes = [vp, vp, ci, C.POINTER(C.c_uint64), ci, C.POINTER(cs)]; L.al_batch_upload_windows.restype = ci
    L.al_batch_stat.argtypes = [vp, C.POINTER(BatchStat)]; L.al_batch_stat.restype = None
    L.al_stage_name.argtypes = [ci]; L.al_stage_name.restype = cs
    L.al_stage_kernel.argtypes = [ci]; L.al_stage_kernel.restype = cs
    L.al_dbg_copy.argtypes = [vp, cs, vp, C.c_int64]; L.al_dbg_copy.restype = C.c_int64
    L.al_dbg_alser_count.argtypes = [vp, C.POINTER(C.c_int64)]; L.al_dbg_alser_count.restype = ci
    L.al_write_sam.argtypes = [C.c_char_p, C.c_size_t, vp, cs, ci, cs, cs, ci, ci, ci, C.POINTER(ci), C.POINTER(C.POINTER(Reg)), cs, ci]; L.al_write_sam.restype = ci
    L.al_write_paf.argtypes = [C.c_char_p, C.c_size_t, vp, cs, ci, C.POINTER(Reg), C.c_int64, ci, cs]; L.al_write_paf.restype = ci
    L.al_dbg_paf_selftest.argtypes = [C.c_uint64, ci]; L.al_dbg_paf_selftest.restype = ci
    L.al_dbg_bam_selftest.argtypes = [C.c_uint64, ci]; L.al_dbg_bam_selftest.restype = ci
    if hasattr(L, "al_dbg_bgzf_deflate"):   # (test taps of the BGZF compressor; a test that needs them fails by name on an older library)
        szp = C.POINTER(C.c_size_t)
        L.al_dbg_bgzf_deflate.argtypes = [ci, vp, C.c_size_t, ci, vp, C.c_size_t, szp, szp]; L.al_dbg_bgzf_deflate.restype = ci
        L.al_dbg_bgzf_deflate_host.argtypes = [vp, C.c_size_t, ci, vp, C.c_size_t, szp, szp]; L.al_dbg_bgzf_deflate_host.restype = ci
        L.al_dbg_bgzf_stream.argtypes = [ci, vp, C.c_size_t, C.c_size_t, ci, vp, C.c_size_t, szp]; L.al_dbg_bgzf_stream.restype = ci
        L.al_dbg_bgzf_stream_dev.argtypes = [ci, vp, C.c_size_t, C.c_size_t, ci, C.c_size_t, ci, vp, C.c_size_t, szp]; L.al_dbg_bgzf_stream_dev.restype = ci
        L.al_dbg_deflate_hist.argtypes = [vp, C.c_size_t, ci, C.POINTER(C.c_uint32)]; L.al_dbg_deflate_hist.restype = ci
        L.al_dbg_deflate_selftest.argtypes = [C.c_uint64]; L.al_dbg_deflate_selftest.restype = ci
    if hasattr(L, "al_dbg_bgzf_inflate"):   # (--gpu-inflate: the extraction with a choice of reader, and the test taps of the BGZF inflater)
        szp = C.POINTER(C.c_size_t); u32p = C.POINTER(C.c_uint32)
        L.al_extract_reads_ex.argtypes = [cs, cs, ci, ci, vp, C.c_uint, ci, ci]; L.al_extract_reads_ex.restype = C.c_int64
        L.al_dbg_bgzf_inflate_host.argtypes = [vp, C.c_size_t, vp, C.c_size_t, szp, u32p, C.c_size_t, szp]; L.al_dbg_bgzf_inflate_host.restype = ci
        L.al_dbg_bgzf_inflate.argtypes = [ci, vp, C.c_size_t, vp, C.c_size_t, szp, u32p, C.c_size_t, szp]; L.al_dbg_bgzf_inflate.restype = ci
        L.al_dbg_bgzf_inflate_guard.argtypes = [ci, vp, C.c_size_t, vp, C.c_size_t, szp, u32p, C.c_size_t, szp]; L.al_dbg_bgzf_inflate_guard.restype = ci
    if hasattr(L, "al_dbg_fq_select"):   # (--gpu-select: the sequence extraction with a choice of selector, and the selector's test taps)
        szp = C.POINTER(C.c_size_t); u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64); i64p = C.POINTER(C.c_int64)
        L.al_extract_sequence_ex.argtypes = [cs, cs, cs, cs, i64p, i64p, C.c_uint, ci, ci, C.c_size_t]; L.al_extract_sequence_ex.restype = ci
        L.al_dbg_fq_select_host.argtypes = [vp, C.c_size_t, vp, C.c_size_t, u32p, C.c_size_t, u64p, u64p, vp, C.c_size_t, szp, u32p, C.c_size_t, szp]; L.al_dbg_fq_select_host.restype = ci
        L.al_dbg_fq_select.argtypes = [ci, vp, C.c_size_t, vp, C.c_size_t, u32p, C.c_size_t, u64p, u64p, vp, C.c_size_t, szp, u32p, C.c_size_t, szp]; L.al_dbg_fq_select.restype = ci
    if hasattr(L, "al_map_tokens_regions"):   # (tokens --regions-bed / --merged-bed: the merged gap regions instead of SAM, and the merge's test taps)
        u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64)
        L.al_map_tokens_regions.argtypes = [vp, cs, ci, ci, C.POINTER(MapOpt), ci, vp, vp, ci]; L.al_map_tokens_regions.restype = ci
        for f in (L.al_dbg_regions_merge, L.al_dbg_regions_merge_host):
            f.argtypes = [C.c_uint64, u32p, u32p, u32p, u32p, C.c_uint64, ci, u32p, u32p, u32p, u32p, u64p]; f.restype = ci
    if hasattr(L, "al_map_tokens_bed_file"):   # (tokens --gaps-bed: the tokens cut from the indexed reference by the rows of a gaps BED, and the set-up kernel's test taps)
        u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64)
        L.al_map_tokens_bed_file.argtypes = [vp, cs, ci, ci, C.POINTER(MapOpt), ci, vp, cs, ci]; L.al_map_tokens_bed_file.restype = ci
        L.al_map_tokens_bed_regions.argtypes = [vp, cs, ci, ci, C.POINTER(MapOpt), ci, vp, vp, ci]; L.al_map_tokens_bed_regions.restype = ci
        for f in (L.al_dbg_tokens_table, L.al_dbg_tokens_table_host):
            f.argtypes = [C.c_uint32, C.c_char_p, C.c_size_t, u64p, u32p, ci, ci, ci, C.c_uint64, C.c_uint64, u64p, u32p, u64p, u32p]; f.restype = ci
    if hasattr(L, "al_chain_beds"):   # (chain-beds / tokens --chain: the chain file's region logic, and its test taps)
        u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64); u32 = C.c_uint32
        L.al_chain_beds.argtypes = [cs, ci, ci, cs, vp, vp, vp, C.c_uint, ci]; L.al_chain_beds.restype = ci
        L.al_map_tokens_chain_file.argtypes = [vp, cs, ci, ci, ci, C.POINTER(MapOpt), ci, vp, cs, ci, vp]; L.al_map_tokens_chain_file.restype = ci
        L.al_map_tokens_chain_regions.argtypes = [vp, cs, ci, ci, ci, C.POINTER(MapOpt), ci, vp, vp, ci, vp, vp, vp]; L.al_map_tokens_chain_regions.restype = ci
        for f in (L.al_dbg_chainreg, L.al_dbg_chainreg_host):
            f.argtypes = [C.c_uint64, u32p, u32p, u32p, u32p, u32, u32p, u32p, u32, u32p, C.c_uint64, u32p, u32p, u32p, u32, u32p, u32p, ci, ci, u32p, u64p, u32p, u64p, u32p, u64p]; f.restype = ci
    if hasattr(L, "al_chain_exact"):   # (chain-exact verify|build: the exact chain file, and its test taps)
        u8p = C.POINTER(C.c_uint8); u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64); u32 = C.c_uint32; u64 = C.c_uint64
        L.al_chain_exact.argtypes = [cs, cs, cs, ci, ci, vp, C.c_uint, ci]; L.al_chain_exact.restype = ci
        for f in (L.al_dbg_chainexact, L.al_dbg_chainexact_host):
            f.argtypes = [u8p, u64, u8p, u64, u64, u32p, u32p, u32p, u32p, u32p, u32, u64p, u64p, u32p, ci, ci, u32p, u32p, u64, u64p, u32p, u64, u64p, u32p, u64, u64p, u32p]; f.restype = ci
        L.al_dbg_chainexact_tile.argtypes = []; L.al_dbg_chainexact_tile.restype = u32
    if hasattr(L, "al_lift_bam"):   # (lift: the constant-region reads of a BAM across the chain file, and its test taps)
        szp = C.POINTER(C.c_size_t); u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64)
        L.al_lift_bam.argtypes = [cs, cs, cs, cs, C.c_uint, ci, ci, ci, C.c_size_t, C.POINTER(LiftStat)]; L.al_lift_bam.restype = ci
        L.al_dbg_lift_host.argtypes = [vp, C.c_size_t, cs, u32p, u32p, C.c_size_t, u64p, vp, C.c_size_t, szp, vp, C.c_size_t, szp]; L.al_dbg_lift_host.restype = ci
        L.al_dbg_lift.argtypes = [ci, vp, C.c_size_t, cs, u32p, u32p, C.c_size_t, u64p, vp, C.c_size_t, szp, vp, C.c_size_t, szp, szp]; L.al_dbg_lift.restype = ci
        L.al_dbg_lift_window.argtypes = []; L.al_dbg_lift_window.restype = C.c_uint32
    if hasattr(L, "al_dbg_lift_sorted"):   # (lift --sorted: the taps of the sorted form)
        szp = C.POINTER(C.c_size_t); u32p = C.POINTER(C.c_uint32); u64p = C.POINTER(C.c_uint64)
        L.al_dbg_lift_sorted_host.argtypes = [vp, C.c_size_t, cs, u32p, u32p, C.c_size_t, u64p, vp, C.c_size_t, szp, vp, C.c_size_t, szp, u32p, u64p]; L.al_dbg_lift_sorted_host.restype = ci
        L.al_dbg_lift_sorted.argtypes = [ci, vp, C.c_size_t, cs, u32p, u32p, C.c_size_t, u64p, vp, C.c_size_t, szp, vp, C.c_size_t, szp, u32p, u64p, C.c_uint, szp]; L.al_dbg_lift_sorted.restype = ci
    L.al_dbg_bam_de_bits.argtypes = [C.c_uint64]; L.al_dbg_bam_de_bits.restype = C.c_uint32
    L.al_dbg_ksw.argtypes = [vp, ci, vp, C.c_size_t, vp, vp, vp, ci]; L.al_dbg_ksw.restype = ci
    if hasattr(L, "al_merge_bams"):   # (merge: coordinate-sorted BAMs merged into one, and its test taps)
        cs, ci, vp, u32p, u64p, szp = C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.al_merge_bams.argtypes = [C.POINTER(C.c_char_p), ci, cs, C.c_uint, ci, ci, ci, C.c_size_t, C.POINTER(MergeStat)]; L.al_merge_bams.restype = ci
        L.al_dbg_merge_host.argtypes = [C.POINTER(C.c_char_p), szp, ci, C.c_size_t, u32p, u64p, C.c_size_t, szp, vp, C.c_size_t, szp, u64p]; L.al_dbg_merge_host.restype = ci
        L.al_dbg_merge.argtypes = [ci, C.POINTER(C.c_char_p), szp, ci, C.c_size_t, u32p, u64p, C.c_size_t, szp, vp, C.c_size_t, szp, u64p, szp]; L.al_dbg_merge.restype = ci
        L.al_dbg_merge_tile.argtypes = []; L.al_dbg_merge_tile.restype = C.c_uint32
    if hasattr(L, "al_index_bam"):   # (bam-index: the BAI of a coordinate-sorted BAM, and its test taps)
        cs, ci, vp, u32p, u64p, szp = C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.al_index_bam.argtypes = [cs, cs, C.c_uint, ci, ci, C.c_size_t, C.POINTER(BaiStat)]; L.al_index_bam.restype = ci
        L.al_dbg_bai_host.argtypes = [vp, C.c_size_t, u64p, u64p, u32p, C.c_size_t, C.c_uint64, C.c_size_t, vp, C.c_size_t, szp]; L.al_dbg_bai_host.restype = ci
        L.al_dbg_bai.argtypes = [ci, vp, C.c_size_t, u64p, u64p, u32p, C.c_size_t, C.c_uint64, C.c_size_t, vp, C.c_size_t, szp, szp]; L.al_dbg_bai.restype = ci
    if hasattr(L, "al_dbg_ext_dp"):   # (a test tap: an older library named by AIRLIFT_LIB for A/B timing has none, and the test that calls it then fails by name)
        L.al_dbg_ext_dp.argtypes = [vp, ci, vp, vp, vp, ci, vp]; L.al_dbg_ext_dp.restype = ci
    if hasattr(L, "al_dbg_chain"):
        L.al_dbg_chain.argtypes = [vp] * 9; L.al_dbg_chain.restype = ci
    if hasattr(L, "al_dbg_regs"):
        L.al_dbg_regs.argtypes = [vp] * 13; L.al_dbg_regs.restype = ci
        L.al_dbg_regs_fetch.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64]; L.al_dbg_regs_fetch.restype = ci
    if hasattr(L, "al_dbg_align"):
        L.al_dbg_align.argtypes = [vp] * 8; L.al_dbg_align.restype = ci
    if hasattr(L, "al_dbg_seed"):
        L.al_dbg_seed.argtypes = [vp, vp, ci, vp]; L.al_dbg_seed.restype = ci
    L.al_version.restype = cs
    L.al_gen_cs.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(ci), vp, C.POINTER(Reg), cs, ci]; L.al_gen_cs.restype = ci
    L.al_gen_MD.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(ci), vp, C.POINTER(Reg), cs]; L.al_gen_MD.restype = ci
    _lib = L
    return L


def gen_tag(idx, reg, seq, kind="MD", no_iden=True):
    """al_gen_MD / al_gen_cs (mm_gen_MD / mm_gen_cs): the MD:Z or cs:Z value of one record `reg` (a Reg) of the read `seq` (bytes,
    sequencing orientation) against index handle `idx`.  The slow per-record path for API callers."""
    L = load()
    buf = C.c_char_p(None); ml = C.c_int(0)
    libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
    if kind == "MD":
        n = L.al_gen_MD(None, C.byref(buf), C.byref(ml), idx, C.byref(reg), seq)
    else:
        n = L.al_gen_cs(None, C.byref(buf), C.byref(ml), idx, C.byref(reg), seq, 1 if no_iden else 0)
    out = C.string_at(buf, n) if n >= 0 else None
    if buf:
        libc.free(C.cast(buf, C.c_void_p))
    if n < 0:
        raise AirliftError("al_gen_%s failed" % kind)
    return out


def write_paf(idx, qname, l_seq, reg, opt_flag=0, rep_len=-1, tag=None):
    """al_write_paf (mm_write_paf3): the PAF line (with its newline) of hit `reg` (a Reg as al_map_frag returned it; None: the line of a
    read without hits) of read `qname` (bytes) with `l_seq` bases.  opt_flag: AL_F_OUT_CG prints cg:Z:, AL_F_OUT_MD / AL_F_OUT_CS name
    the value `tag` (bytes from gen_tag) holds."""
    L = load()
    buf = C.create_string_buffer(65536 + (len(tag) if tag else 0) + (16 * reg.n_cigar if reg is not None else 0))
    n = L.al_write_paf(buf, len(buf), idx, qname, l_seq, C.byref(reg) if reg is not None else None, opt_flag, rep_len, tag)
    if n < 0:
        raise AirliftError("al_write_paf failed")
    return buf.raw[:n]


def read_fastx(path):
    """Minimal FASTA/FASTQ(.gz) reader for tests: returns (names, seqs, quals) as lists of bytes."""
    op = gzip.open if path.endswith(".gz") else open
    names, seqs, quals = [], [], []
    with op(path, "rb") as f:
        data = f.read().split(b"\n")
    i = 0
    while i < len(data):
        l = data[i]
        if not l:
            i += 1; continue
        if l[:1] == b"@":
            names.append(l[1:].split()[0]); seqs.append(data[i + 1].strip()); quals.append(data[i + 3].strip()); i += 4
        elif l[:1] == b">":
            nm = l[1:].split()[0]; i += 1; s = []
            while i < len(data) and data[i][:1] != b">":
                s.append(data[i].strip()); i += 1
            names.append(nm); seqs.append(b"".join(s)); quals.append(None)
        else:
            i += 1
    return names, seqs, quals


class Index:
    """al_idx_t (replaces mm_idx_t)."""

    def __init__(self, fasta=None, seqs=None, names=None, preset="sr", n_threads=4, on_device=None, k=None, w=None):
        L = load()
        self.io, self.mo = IdxOpt(), MapOpt()
        L.al_set_opt(None, C.byref(self.io), C.byref(self.mo))
        if L.al_set_opt(preset.encode(), C.byref(self.io), C.byref(self.mo)) != 0:
            raise AirliftError("unknown preset " + preset)
        if k is not None:
            self.io.k = k
        if w is not None:
            self.io.w = w
        self.mo.flag |= 0x004 | 0x008
        if fasta is not None and on_device is not None:     # sketch + sort + table built by kernels on that GPU
            self.h = L.al_idx_build_device(fasta.encode(), C.byref(self.io), on_device)
        elif fasta is not None:
            self.h = L.al_idx_build(fasta.encode(), C.byref(self.io), n_threads)
        else:
            n = len(seqs)
            sa = (C.c_char_p * n)(*seqs); na = (C.c_char_p * n)(*names)
            self.h = L.al_idx_str(self.io.w, self.io.k, n, sa, na)
        if not self.h:
            raise AirliftError("index build failed")

    @property
    def names(self):
        L = load()
        return [L.al_idx_seq_name(self.h, i).decode() for i in range(L.al_idx_n_seq(self.h))]

    def stat(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        load().al_idx_stat(self.h, C.byref(a), C.byref(b), C.byref(c))
        return {"n_keys": a.value, "n_pos": b.value, "n_bases": c.value}

    def cal_max_occ(self, f):
        """mm_idx_cal_max_occ (index.c:164-185)."""
        fn = load().al_idx_cal_max_occ
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_float]
        v = fn(self.h, f)
        if v < 0:
            raise AirliftError("al_idx_cal_max_occ failed")
        return v

    def positions(self):
        """The occurrence array (grouped by minimizer hash ascending, positions ascending inside a group)."""
        n = load().al_idx_export_pos(self.h, None, 0)
        out = np.zeros(max(n, 0), dtype=np.uint64)
        if n > 0 and load().al_idx_export_pos(self.h, out.ctypes.data_as(C.c_void_p), n) != n:
            raise AirliftError("al_idx_export_pos failed")
        return out

    def close(self):
        if self.h:
            load().al_idx_destroy(self.h); self.h = None


class Context:
    """al_ctx_t (replaces mm_tbuf_t): one per host thread / GPU."""

    def __init__(self, index, device=-1):
        self.idx = index
        self.h = load().al_ctx_init(index.h, C.byref(index.mo), device)
        if not self.h:
            raise AirliftError("al_ctx_init failed: no usable HIP device (there is no CPU fallback)")
        self._keep = None

    def upload(self, n_segs, seqs, names):
        L = load()
        nf, nr = len(n_segs), len(seqs)
        a_ns = (C.c_int * nf)(*n_segs); a_ql = (C.c_int * nr)(*[len(s) for s in seqs])
        a_sq = (C.c_char_p * nr)(*seqs); a_nm = (C.c_char_p * nr)(*names)
        self._keep = (a_ns, a_ql, a_sq, a_nm); self.n_frag, self.n_reads = nf, nr
        rc = L.al_batch_upload(self.h, nf, a_ns, a_ql, a_sq, a_nm)
        if rc != 0:
            raise AirliftError("al_batch_upload failed: %d" % rc)

    def run(self):
        rc = load().al_batch_run(self.h)
        if rc != 0:
            raise AirliftError("al_batch_run failed: %d" % rc)

    def stat(self):
        st = BatchStat(); load().al_batch_stat(self.h, C.byref(st)); return st

    def fetch(self):
        """Returns (n_regs[list], regs[list of list of dict], rep_len[list])."""
        L = load()
        n_regs = (C.c_int * self.n_reads)(); regs = (C.POINTER(Reg) * self.n_reads)(); rep = (C.c_int * self.n_frag)()
        rc = L.al_batch_fetch(self.h, n_regs, regs, rep)
        if rc != 0:
            raise AirliftError("al_batch_fetch failed: %d" % rc)
        return n_regs, regs, rep

    def tap(self, name, dtype, count):
        arr = np.zeros(count, dtype=dtype)
        n = load().al_dbg_copy(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes)
        if n < 0:
            raise AirliftError("tap %s failed" % name)
        return arr[: n // arr.itemsize]

    CHAIN_COUNTS = ("lane_lo", "lane_mid", "wave_mid", "tile_items", "tile_frags", "handed_back", "deferred", "deferred_coop", "compacted", "legacy_frags", "wave_segs", "order_frags",
                    "whole_wave", "tie_round", "seg_big", "fallback_frags", "n_chain_fallback", "lds_ok", "tiles_ok", "tile_from", "lb1", "lb65", "lb129", "lmin")

    def chain(self, anchors, a_off, tie_flag):
        """al_dbg_chain: the chain stage on caller-supplied anchors ((n, 2) uint64; a_off uint64[n_frag + 1]; tie_flag uint32[n_frag]) for the
        uploaded batch (not run).  Returns (frag_nu, u, uo, chained, counts by name); fragment f's chain list starts at a_off[f] + f."""
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2); a_off = np.ascontiguousarray(a_off, dtype=np.uint64); tie_flag = np.ascontiguousarray(tie_flag, dtype=np.uint32)
        nf, tot = self.n_frag, int(a_off[-1])
        if len(a_off) != nf + 1 or len(tie_flag) != nf or len(anchors) != tot:
            raise AirliftError("al_dbg_chain: arrays do not fit the uploaded batch")
        nu = np.zeros(nf, dtype=np.uint32); u = np.zeros(tot + nf + 1, dtype=np.uint64); uo = np.zeros(tot + nf + 1, dtype=np.uint32)
        ch = np.zeros((max(tot, 1), 2), dtype=np.uint64); cnt = np.zeros(24, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = load().al_dbg_chain(self.h, p(anchors), p(a_off), p(tie_flag), p(nu), p(u), p(uo), p(ch), p(cnt))
        if rc != 0:
            raise AirliftError("al_dbg_chain failed: %d" % rc)
        return nu, u, uo, ch[:tot], dict(zip(self.CHAIN_COUNTS, (int(x) for x in cnt)))

    REGS_COUNTS = ("lb5", "lb65", "lb1025", "lb8193", "lb2049", "lb4097", "lb257", "heavy12", "heavy24", "heavy48", "heavy72", "heavy200", "log_miss", "sort_ties", "select_ran",
                   "map_only_wave", "log_n")

    def regs(self, nu, u, uo, chained, a_off, frag_rep):
        """al_dbg_regs + al_dbg_regs_fetch: the stage between chaining and extension on caller-supplied chains (what chain() returns, and the
        fragments' rep_len) for the uploaded batch (not run).  Returns a dict: reg_cnt, seg_na (per read), regs_n0, frag_hash (per fragment), regs (the
        per-mate hits, (n, 28) uint32 device records, read after read), seg_a ((n, 2) uint64), dense (the map-only output, or None), counts by name."""
        nf, nr = self.n_frag, self.n_reads
        a_off = np.ascontiguousarray(a_off, dtype=np.uint64); tot = int(a_off[-1])
        nu = np.ascontiguousarray(nu, dtype=np.uint32); u = np.ascontiguousarray(u, dtype=np.uint64); uo = np.ascontiguousarray(uo, dtype=np.uint32)
        chained = np.ascontiguousarray(chained, dtype=np.uint64).reshape(-1, 2); frag_rep = np.ascontiguousarray(frag_rep, dtype=np.int32)
        if len(a_off) != nf + 1 or len(nu) != nf or len(frag_rep) != nf or len(u) != tot + nf + 1 or len(uo) != tot + nf + 1 or len(chained) != tot:
            raise AirliftError("al_dbg_regs: arrays do not fit the uploaded batch")
        rc_, sna = np.zeros(nr, dtype=np.uint32), np.zeros(nr, dtype=np.uint32); n0, fh = np.zeros(nf, dtype=np.uint32), np.zeros(nf, dtype=np.uint32)
        cnt = np.zeros(17, dtype=np.uint64); sizes = np.zeros(2, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = load().al_dbg_regs(self.h, p(nu), p(u), p(uo), p(chained), p(a_off), p(frag_rep), p(rc_), p(sna), p(n0), p(fh), p(cnt), p(sizes))
        if rc != 0:
            raise AirliftError("al_dbg_regs failed: %d" % rc)
        regs = np.zeros((int(sizes[0]) + 1, 28), dtype=np.uint32); seg_a = np.zeros((tot + 1, 2), dtype=np.uint64); dense = np.zeros((int(sizes[1]) + 1, 28), dtype=np.uint32)
        rc = load().al_dbg_regs_fetch(self.h, p(regs), int(sizes[0]), p(seg_a), p(dense), int(sizes[1]))
        if rc != 0:
            raise AirliftError("al_dbg_regs_fetch failed: %d" % rc)
        return {"reg_cnt": rc_, "seg_na": sna, "regs_n0": n0, "frag_hash": fh, "regs": regs[:-1], "seg_a": seg_a[:tot], "dense": dense[:-1] if self.idx.mo.flag & AL_F_OUT_PAF and not self.idx.mo.flag & AL_F_CIGAR else None,
                "counts": dict(zip(self.REGS_COUNTS, (int(x) for x in cnt)))}

    ALIGN_COUNTS = ("n_early", "n_slow", "solo_early", "solo_slow", "mono_all", "long_mode", "tmax", "prep_heavy", "fin_heavy", "wave_prep", "wave_finish", "closed_form", "n_jobs",
                    "limit", "log_miss", "arena_overflow", "reruns", "records", "arena_words", "dp_lane16", "dp_lane32", "dp_lane64", "dp_g1", "dp_g2", "dp_g4", "dp_g8", "dp_g22", "dp_g32", "dp_lds")

    def align(self, nu, u, uo, chained, a_off, frag_rep):
        """al_dbg_align: the extension stage on caller-supplied chains (what chain() returns, and the fragments' rep_len) for the uploaded batch (not
        run), to its end and through the arena-overflow re-runs; fetch() then returns the records as after run().  Returns the counts by name."""
        nf = self.n_frag
        a_off = np.ascontiguousarray(a_off, dtype=np.uint64); tot = int(a_off[-1])
        nu = np.ascontiguousarray(nu, dtype=np.uint32); u = np.ascontiguousarray(u, dtype=np.uint64); uo = np.ascontiguousarray(uo, dtype=np.uint32)
        chained = np.ascontiguousarray(chained, dtype=np.uint64).reshape(-1, 2); frag_rep = np.ascontiguousarray(frag_rep, dtype=np.int32)
        if len(a_off) != nf + 1 or len(nu) != nf or len(frag_rep) != nf or len(u) != tot + nf + 1 or len(uo) != tot + nf + 1 or len(chained) != tot:
            raise AirliftError("al_dbg_align: arrays do not fit the uploaded batch")
        cnt = np.zeros(len(self.ALIGN_COUNTS), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = load().al_dbg_align(self.h, p(nu), p(u), p(uo), p(chained), p(a_off), p(frag_rep), p(cnt))
        if rc != 0:
            raise AirliftError("al_dbg_align failed: %d" % rc)
        return dict(zip(self.ALIGN_COUNTS, (int(x) for x in cnt)))

    SEED_COUNTS = ("small", "reg_2_1_128", "reg_4_1_256", "reg_8_1_512", "reg_16_1_512", "reg_8_4_1024", "reg_16_4_1024", "reg_16_8_1024", "sort1024", "merge_frags", "merge_tiles", "merge_passes",
                   "radix_frags", "radix_chunks", "flag_all", "compact", "rid_bits", "pos_bits", "rank_bits", "nl", "lb65", "lb129", "lb257", "lb513", "lb1025", "lb2049", "lb4097", "lb_big",
                   "heap_merges", "spec_made", "spec_taken", "flagged", "heap_lanes2", "heap_lanes1", "heap_serial0", "heap_wave", "heap_serial48", "heap_serial96", "sketch_form", "sketch_pb")

    def seed(self, second=None):
        """al_dbg_seed: the seed stage of the uploaded batch without the chaining: the first pass, and with `second` (ascending fragment ids) the
        re-chain pass of those fragments with max_occ.  Returns one dict per pass: frag_na, frag_nm, frag_rep, a_off, flags (the pass's tie_list
        word per fragment), anchors ((n, 2) uint64, all of the batch so far; fragment f's lie at a_off[f]), counts by name (heap_merges: of this pass)."""
        L = load(); nf = self.n_frag; out = []
        for lst in ([None] if second is None else [None, np.ascontiguousarray(second, dtype=np.uint32)]):
            cnt = np.zeros(40, dtype=np.uint64)
            rc = L.al_dbg_seed(self.h, None if lst is None else lst.ctypes.data_as(C.c_void_p), 0 if lst is None else len(lst), cnt.ctypes.data_as(C.c_void_p))
            if rc != 0:
                raise AirliftError("al_dbg_seed failed: %d" % rc)
            d = dict(zip(self.SEED_COUNTS, (int(x) for x in cnt)))
            d["rank_bits"] -= 64; d["sketch_pb"] -= 64
            a_off = self.tap("a_off", np.uint64, nf + 1).copy(); na = self.tap("frag_na", np.uint32, nf).copy()
            tot = int((a_off[:nf].astype(np.int64) + na).max()) if nf else 0
            out.append({"frag_na": na, "frag_nm": self.tap("frag_nm", np.uint32, nf).copy(), "frag_rep": self.tap("frag_rep", np.int32, nf).copy(), "a_off": a_off,
                        "flags": self.tap("tie_list", np.uint32, nf).copy(), "anchors": self.tap("anchors", np.uint64, tot * 2).reshape(-1, 2).copy(), "counts": d})
        return out

    def alser_count(self):
        v = C.c_int64()
        if load().al_dbg_alser_count(self.h, C.byref(v)) != 0:
            raise AirliftError("alser count failed")
        return v.value

    def close(self):
        if self.h:
            load().al_ctx_destroy(self.h); self.h = None
