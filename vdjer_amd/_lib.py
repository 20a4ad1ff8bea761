"""ctypes loader of vdjer_amd/libvdjx.so (the HIP hot path).  There is no CPU fallback: if the library is
missing or cannot be loaded this raises, loudly."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# VDJX_LIB_PATH: another build of the same library (profiles/: the -DVDJX_ABLATE build, `make -C vdjer_amd/csrc ablate`)
LIB_PATH = os.environ.get("VDJX_LIB_PATH") or os.path.join(_HERE, "libvdjx.so")
_lib = None

# every symbol include/vdjx.h declares
SYMBOLS = [
    "vdjx_last_error", "vdjx_version", "vdjx_init", "vdjx_shutdown", "vdjx_sync", "vdjx_trim", "vdjx_read_index_drop", "vdjx_device_copy",
    "vdjx_pool_load", "vdjx_pool_load_forward", "vdjx_pool_load_forward_begin", "vdjx_pool_wait", "vdjx_packed_read_bytes", "vdjx_pack_reads", "vdjx_pool_load_packed", "vdjx_pool_load_packed_begin", "vdjx_pool_load_device", "vdjx_pool_records", "vdjx_pool_free",
    "vdjx_anchor_sets_load", "vdjx_anchor_probe", "vdjx_index_generate", "vdjx_anchor_sets_from_anchors",
    "vdjx_kmer_build", "vdjx_graph_nodes", "vdjx_graph_pre_nodes", "vdjx_graph_export", "vdjx_graph_export_begin", "vdjx_graph_export_end", "vdjx_graph_block_layout", "vdjx_graph_export_block", "vdjx_graph_export_block_begin", "vdjx_graph_free",
    "vdjx_vregion_load", "vdjx_root_score", "vdjx_graph_roots", "vdjx_root_part", "vdjx_root_score_graph", "vdjx_root_score_graph_begin", "vdjx_root_score_graph_end",
    "vdjx_read_index_build", "vdjx_read_index_build_device", "vdjx_read_index_build_begin", "vdjx_read_index_build_device_begin", "vdjx_read_index_build_end", "vdjx_window_score", "vdjx_window_pairs", "vdjx_window_pairs_fetch", "vdjx_window_cover", "vdjx_map_emit", "vdjx_map_emit_begin", "vdjx_map_emit_end", "vdjx_sam_names_load", "vdjx_sam_text", "vdjx_sam_blocks", "vdjx_sam_merge", "vdjx_rows_scatter", "vdjx_quant", "vdjx_quant_pairs", "vdjx_quant_boot", "vdjx_quant_pairs_boot", "vdjx_quant_boot_summary", "vdjx_germline_load", "vdjx_annotate", "vdjx_constant_load", "vdjx_isotype", "vdjx_dsegment_load", "vdjx_dcall", "vdjx_lineage", "vdjx_lineage_distance_table", "vdjx_lineage_model", "vdjx_lineage_link", "vdjx_threshold_kernel", "vdjx_lineage_threshold", "vdjx_tree", "vdjx_tree_support", "vdjx_tree_nj_nodes", "vdjx_tree_nj", "vdjx_tree_mp", "vdjx_tree_spr", "vdjx_tree_sankoff", "vdjx_sankoff_costs", "vdjx_tree_sankoff_spr", "vdjx_tree_split_support", "vdjx_tree_split_compare", "vdjx_mutations_layout", "vdjx_mutations", "vdjx_selection", "vdjx_selection_convolve", "vdjx_selection_compare", "vdjx_targeting_counts", "vdjx_targeting_model", "vdjx_consensus_layout", "vdjx_consensus", "vdjx_consensus_hits", "vdjx_diversity", "vdjx_scan_u32", "vdjx_part_u64",
    "vdjx_host_alloc", "vdjx_host_free", "vdjx_host_take_rows",
    "vdjx_stat", "vdjx_profile_enable", "vdjx_profile_only", "vdjx_profile_reset", "vdjx_profile_count", "vdjx_profile_get",
    "vdjx_shard_begin", "vdjx_shard_begin_share", "vdjx_shard_free", "vdjx_shard_record_bytes", "vdjx_shard_count", "vdjx_shard_geometry", "vdjx_shard_symmetric", "vdjx_shard_geometry2", "vdjx_shard_local", "vdjx_shard_local_fill",
    "vdjx_shard_merge", "vdjx_shard_queries", "vdjx_shard_reply", "vdjx_shard_resolve",
    "vdjx_shard_survivors", "vdjx_shard_edges", "vdjx_shard_finish",
]


class VdjxError(RuntimeError):
    pass


class CovParams(C.Structure):
    _fields_ = [("eval_start", C.c_int), ("eval_stop", C.c_int), ("read_span", C.c_int), ("mate_span", C.c_int),
                ("insert_low", C.c_int), ("insert_high", C.c_int), ("floor", C.c_int)]


class Pair(C.Structure):
    _fields_ = [("pair_id", C.c_uint32), ("rec1", C.c_uint32), ("rec2", C.c_uint32),
                ("pos1", C.c_int16), ("pos2", C.c_int16), ("insert", C.c_int16),
                ("rc1", C.c_uint8), ("rc2", C.c_uint8)]


class QuantParams(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double)]


class QuantInfo(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("alignments", C.c_uint64), ("unique_pairs", C.c_uint64), ("iterations", C.c_uint32),
                ("converged", C.c_uint32), ("eff_len", C.c_double)]


class QuantBootParams(C.Structure):
    _fields_ = [("replicates", C.c_int), ("seed", C.c_uint64)]


class QuantBootInfo(C.Structure):
    _fields_ = [("replicates", C.c_uint32), ("converged", C.c_uint32), ("batches", C.c_uint32), ("max_iterations", C.c_uint32),
                ("iterations", C.c_uint64)]


class AnnotParams(C.Structure):
    _fields_ = [("match", C.c_int), ("mismatch", C.c_int), ("gap_open", C.c_int), ("gap_extend", C.c_int), ("min_v_score", C.c_int),
                ("min_j_score", C.c_int)]


class IsotypeParams(C.Structure):
    _fields_ = [("match", C.c_int), ("mismatch", C.c_int), ("gap_open", C.c_int), ("gap_extend", C.c_int), ("min_score", C.c_int),
                ("tail", C.c_int)]


class DcallParams(C.Structure):
    _fields_ = [("match", C.c_int), ("mismatch", C.c_int), ("gap_open", C.c_int), ("gap_extend", C.c_int), ("min_score", C.c_int)]


class LineageParams(C.Structure):
    _fields_ = [("num", C.c_int), ("den", C.c_int)]


class LineageInfo(C.Structure):
    _fields_ = [("items", C.c_uint32), ("buckets", C.c_uint32), ("largest_bucket", C.c_uint32), ("clones", C.c_uint32),
                ("pairs", C.c_uint64), ("links", C.c_uint64)]


class LineageModelParams(C.Structure):
    _fields_ = [("num", C.c_int), ("den", C.c_int), ("symmetry", C.c_int)]


class LineageLinkParams(C.Structure):
    _fields_ = [("num", C.c_int), ("den", C.c_int), ("symmetry", C.c_int), ("linkage", C.c_int)]


class LineageLinkInfo(C.Structure):
    _fields_ = [("components", C.c_uint32), ("largest_component", C.c_uint32), ("merges", C.c_uint32), ("clones_single", C.c_uint32),
                ("batches", C.c_uint32), ("reserved", C.c_uint32), ("cells", C.c_uint64)]


class LineageTableInfo(C.Structure):
    _fields_ = [("mean", C.c_double), ("min_cost", C.c_uint32), ("max_cost", C.c_uint32)]


class ThresholdParams(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("max_k", "peak_shift", "valley_num", "valley_den", "min_values")]


class ThresholdInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("values", "distinct", "status", "k", "peaks_all", "peaks", "p1_first", "p1_last", "p2_first", "p2_last",
                                          "t_first", "t_last", "threshold", "reserved")] + [(f, C.c_uint64) for f in ("y1", "y2", "m", "ymax")]


assert C.sizeof(ThresholdParams) == 20 and C.sizeof(ThresholdInfo) == 88                          # include/vdjx.h

THRESHOLD_GRID, THRESHOLD_MAX_K, THRESHOLD_TILE = 10000, 200, 256                                 # VDJX_THRESHOLD_GRID, _MAX_K, _TILE
THRESHOLD_STATUS = ("found", "too few values", "no scale", "one mode", "shallow valley")          # VDJX_THRESHOLD_FOUND .. _SHALLOW


class TreeInfo(C.Structure):
    _fields_ = [("members", C.c_uint32), ("clones", C.c_uint32), ("largest_clone", C.c_uint32), ("rounds", C.c_uint32),
                ("edges", C.c_uint64), ("weight", C.c_uint64)]


class TreeSupportParams(C.Structure):
    _fields_ = [("replicates", C.c_uint32), ("seed", C.c_uint64)]


class TreeSupportInfo(C.Structure):
    _fields_ = [("members", C.c_uint32), ("clones", C.c_uint32), ("largest_clone", C.c_uint32), ("replicates", C.c_uint32),
                ("batches", C.c_uint32), ("rounds", C.c_uint32), ("edges", C.c_uint64), ("matched", C.c_uint64), ("full", C.c_uint64)]


class TreeNjInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("members", "clones", "largest_clone", "internal", "batches", "negative")] + [
        (f, C.c_uint64) for f in ("edges", "joins", "cells", "parsimony")] + [("length", C.c_int64)]


assert C.sizeof(TreeNjInfo) == 64                                                                 # include/vdjx.h

class TreeMpParams(C.Structure):
    _fields_ = [("max_rounds", C.c_uint32), ("reserved", C.c_uint32)]


class TreeMpInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds")] + [
        (f, C.c_uint64) for f in ("edges", "moves", "candidates", "parsimony_start", "parsimony")]


assert C.sizeof(TreeMpInfo) == 72                                                                 # include/vdjx.h


class TreeSprParams(C.Structure):
    _fields_ = TreeMpParams._fields_


class TreeSprInfo(C.Structure):
    _fields_ = TreeMpInfo._fields_                                                                # the same fields; candidates counts SPR's


assert C.sizeof(TreeSprInfo) == 72                                                                # include/vdjx.h


class TreeSankoffParams(C.Structure):
    _fields_ = [("max_rounds", C.c_uint32), ("search", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TreeSankoffInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds")] + [
        (f, C.c_uint64) for f in ("edges", "moves", "candidates", "cost_start", "cost", "mutations")]


class SankoffCostsInfo(C.Structure):
    _fields_ = [("mean", C.c_double), ("min_cost", C.c_uint32), ("max_cost", C.c_uint32)]


assert C.sizeof(TreeSankoffParams) == 16 and C.sizeof(TreeSankoffInfo) == 80 and C.sizeof(SankoffCostsInfo) == 16      # include/vdjx.h


class TreeSankoffSprParams(C.Structure):
    _fields_ = [("max_rounds", C.c_uint32), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(TreeSankoffSprParams) == 16                                                        # include/vdjx.h

class TreeSplitParams(C.Structure):
    _fields_ = [("replicates", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class TreeSplitInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("members", "clones", "largest_clone", "replicates", "batches", "units")] + [
        (f, C.c_uint64) for f in ("scored", "matched", "full", "joins", "cells")]


assert C.sizeof(TreeSplitParams) == 16 and C.sizeof(TreeSplitInfo) == 64                          # include/vdjx.h

NJ_LDS_MEMBERS, NJ_MAX_MEMBERS = 64, 4096                                                         # VDJX_NJ_LDS_MEMBERS, VDJX_NJ_MAX_MEMBERS


class MutRow(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("cols", "v_r", "v_s", "v_stop", "v_na", "v_codons", "j_mis", "flags")]


class MutInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("contigs", "aligned", "cols", "v_r", "v_s", "v_stop", "v_na", "v_codons")] + [
        ("truncated", C.c_uint32), ("clipped", C.c_uint32)]


class SelInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("contigs", "used", "no_regions", "truncated")] + [
        (f, C.c_uint32) for f in ("groups", "regions", "chunks", "large_rows")]


class SelConvInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("members", "leaves", "combines")] + [
        (f, C.c_uint32) for f in ("groups", "regions", "rows", "levels", "batches", "pad")]


class SelTest(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("p_greater", "pvalue", "fdr")]


class TgtInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("contigs", "used", "truncated", "units", "positions", "obs_s", "obs_r", "opp_s", "opp_r")] + [
        ("batches", C.c_uint32), ("pad", C.c_uint32)]


class ConsParams(C.Structure):
    _fields_ = [("num", C.c_int), ("den", C.c_int)]


class ConsUnit(C.Structure):
    _fields_ = [("group", C.c_int32), ("gene", C.c_int32), ("members", C.c_uint32), ("off_record", C.c_uint32), ("lo", C.c_int32),
                ("hi", C.c_int32), ("off", C.c_uint64)]


class ConsInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("contigs", "used", "truncated", "off_record", "units", "columns", "votes", "inserted",
                                          "undecided")] + [("batches", C.c_uint32), ("large_units", C.c_uint32)]


assert C.sizeof(ConsParams) == 8 and C.sizeof(ConsUnit) == 32 and C.sizeof(ConsInfo) == 80      # include/vdjx.h


class DiversityParams(C.Structure):
    _fields_ = [("replicates", C.c_uint32), ("depth", C.c_uint32), ("seed", C.c_uint64)]


class DiversityInfo(C.Structure):
    _fields_ = [("clones", C.c_uint32), ("weighted", C.c_uint32), ("weight", C.c_uint64), ("depth", C.c_uint32), ("replicates", C.c_uint32),
                ("batches", C.c_uint32), ("path", C.c_uint32)]


class AnnotHit(C.Structure):
    _fields_ = [("gene", C.c_int32), ("score", C.c_int32), ("n_tied", C.c_int32), ("tied", C.c_int32 * 8),
                ("seq_start", C.c_int32), ("seq_end", C.c_int32), ("germ_start", C.c_int32), ("germ_end", C.c_int32),
                ("matches", C.c_int32), ("mismatches", C.c_int32), ("ins", C.c_int32), ("del_", C.c_int32), ("opens", C.c_int32),
                ("n_runs", C.c_int32), ("runs", C.c_uint32 * 64)]


def build() -> str:
    """Compile libvdjx.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64; whichever HIP runtime is loaded first serves the whole process.  When torch
    # is used in the same process (bench.py, shard.py) it must come first so that device pointers are shared.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for the single-GPU C ABI
        pass
    if not os.path.exists(LIB_PATH):
        raise VdjxError(f"{LIB_PATH} is missing: build it with `make -C vdjer_amd/csrc` "
                        "(there is no CPU fallback for the hot path)")
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.vdjx_last_error.restype = C.c_char_p
    L.vdjx_version.restype = C.c_char_p
    L.vdjx_init.argtypes = [i32, C.POINTER(vp)]
    L.vdjx_shutdown.argtypes = [vp]
    L.vdjx_shutdown.restype = None
    L.vdjx_sync.argtypes = [vp]
    L.vdjx_pool_load.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_pool_load_device.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_pool_load_forward.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_pool_load_forward_begin.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_pool_load_packed.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_pool_load_packed_begin.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(vp)]
    L.vdjx_packed_read_bytes.argtypes = [i32]
    L.vdjx_packed_read_bytes.restype = C.c_size_t
    L.vdjx_pack_reads.argtypes = [vp, sz, i32, vp]
    L.vdjx_pool_wait.argtypes = [vp]
    L.vdjx_pool_records.argtypes = [vp]
    L.vdjx_pool_records.restype = sz
    L.vdjx_pool_free.argtypes = [vp]
    L.vdjx_pool_free.restype = None
    L.vdjx_anchor_sets_load.argtypes = [vp, vp, sz, vp, sz]
    L.vdjx_anchor_probe.argtypes = [vp, C.c_char_p, i32, vp, vp]
    L.vdjx_kmer_build.argtypes = [vp, vp, i32, i32, i32, C.POINTER(vp)]
    L.vdjx_graph_nodes.argtypes = [vp]
    L.vdjx_graph_nodes.restype = sz
    L.vdjx_graph_pre_nodes.argtypes = [vp]
    L.vdjx_graph_pre_nodes.restype = sz
    L.vdjx_graph_export.argtypes = [vp] + [vp] * 10
    L.vdjx_graph_export_begin.argtypes = [vp] + [vp] * 10
    L.vdjx_graph_export_end.argtypes = [vp]
    L.vdjx_graph_block_layout.argtypes = [vp, vp, vp]
    L.vdjx_graph_export_block.argtypes = [vp, vp]
    L.vdjx_graph_export_block_begin.argtypes = [vp, vp]
    L.vdjx_graph_free.argtypes = [vp]
    L.vdjx_graph_free.restype = None
    L.vdjx_vregion_load.argtypes = [vp, C.POINTER(C.c_char_p), sz, i32]
    L.vdjx_root_score.argtypes = [vp, C.c_char_p, sz, i32, i32, vp]
    L.vdjx_read_index_build.argtypes = [vp, vp, vp, vp, vp, vp, u32]
    L.vdjx_read_index_build_device.argtypes = [vp, vp, vp, vp, vp, vp, u32]
    L.vdjx_read_index_build_begin.argtypes = [vp, vp, vp, vp, vp, vp, u32]
    L.vdjx_read_index_build_device_begin.argtypes = [vp, vp, vp, vp, vp, vp, u32]
    L.vdjx_read_index_build_end.argtypes = [vp]
    L.vdjx_window_score.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(CovParams), vp, vp]
    L.vdjx_map_emit.argtypes = [vp, C.c_char_p, sz, i32, vp, vp]
    L.vdjx_window_pairs.argtypes = [vp, C.c_char_p, sz, i32, vp, vp]
    L.vdjx_window_pairs_fetch.argtypes = [vp, vp, sz, vp]
    L.vdjx_window_cover.argtypes = [vp, sz, i32, i32, C.POINTER(CovParams), vp, sz, vp, vp]
    L.vdjx_map_emit_begin.argtypes = [vp, C.c_char_p, sz, i32, vp, vp]
    L.vdjx_map_emit_end.argtypes = [vp]
    L.vdjx_sam_names_load.argtypes = [vp, C.c_char_p, vp, u32]
    L.vdjx_sam_text.argtypes = [vp, C.c_char_p, sz, i32, C.c_char_p, vp, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
    L.vdjx_sam_blocks.argtypes = [vp, C.c_char_p, sz, i32, C.c_char_p, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.vdjx_sam_merge.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
    L.vdjx_quant.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(QuantParams), vp, C.POINTER(QuantInfo)]
    L.vdjx_quant_pairs.argtypes = [vp, vp, vp, sz, i32, C.c_uint32, C.POINTER(QuantParams), vp, C.POINTER(QuantInfo)]
    L.vdjx_quant_boot.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(QuantParams), C.POINTER(QuantBootParams), vp, C.POINTER(QuantInfo), vp, vp,
                                  C.POINTER(QuantBootInfo)]
    L.vdjx_quant_pairs_boot.argtypes = [vp, vp, vp, sz, i32, C.c_uint32, C.POINTER(QuantParams), C.POINTER(QuantBootParams), vp, vp, vp,
                                        C.POINTER(QuantInfo), vp, vp, C.POINTER(QuantBootInfo)]
    L.vdjx_quant_boot_summary.argtypes = [vp, C.c_uint32, sz, vp, vp, vp, vp]
    L.vdjx_quant_boot_summary.restype = None
    L.vdjx_germline_load.argtypes = [vp, C.c_char_p, vp, C.c_char_p, sz]
    L.vdjx_annotate.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(AnnotParams), vp, vp]
    L.vdjx_constant_load.argtypes = [vp, C.c_char_p, vp, sz]
    L.vdjx_isotype.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(IsotypeParams), vp, vp]
    L.vdjx_dsegment_load.argtypes = [vp, C.c_char_p, vp, sz]
    L.vdjx_dcall.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, C.POINTER(DcallParams), vp, vp]
    L.vdjx_lineage.argtypes = [vp, C.c_char_p, vp, vp, sz, C.POINTER(LineageParams), vp, vp, C.POINTER(LineageInfo)]
    L.vdjx_lineage_distance_table.argtypes = [vp, vp, C.POINTER(LineageTableInfo)]
    L.vdjx_lineage_model.argtypes = [vp, C.c_char_p, vp, vp, sz, C.POINTER(LineageModelParams), vp, vp, vp, C.POINTER(LineageInfo)]
    L.vdjx_lineage_link.argtypes = [vp, C.c_char_p, vp, vp, sz, C.POINTER(LineageLinkParams), vp, vp, vp, C.POINTER(LineageInfo),
                                    C.POINTER(LineageLinkInfo)]
    L.vdjx_threshold_kernel.argtypes = [i32, vp, C.POINTER(u32)]
    L.vdjx_lineage_threshold.argtypes = [vp, vp, vp, sz, u32, C.POINTER(ThresholdParams), vp, vp, vp, C.POINTER(ThresholdInfo)]
    L.vdjx_tree.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, vp, vp, C.POINTER(TreeInfo)]
    L.vdjx_tree_support.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, C.POINTER(TreeSupportParams), vp, C.POINTER(TreeSupportInfo)]
    L.vdjx_tree_nj_nodes.argtypes = [vp, sz, C.POINTER(C.c_uint64)]
    L.vdjx_tree_nj.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(TreeNjInfo)]
    L.vdjx_tree_mp.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, C.POINTER(TreeMpParams), vp, vp, vp, vp, vp, C.POINTER(TreeMpInfo)]
    L.vdjx_tree_spr.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, C.POINTER(TreeSprParams), vp, vp, vp, vp, vp, C.POINTER(TreeSprInfo)]
    L.vdjx_tree_sankoff.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, vp, C.POINTER(TreeSankoffParams), vp, vp, vp, vp, vp, vp,
                                    C.POINTER(TreeSankoffInfo)]
    L.vdjx_sankoff_costs.argtypes = [vp, vp, C.POINTER(SankoffCostsInfo)]
    L.vdjx_tree_sankoff_spr.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, vp, C.POINTER(TreeSankoffSprParams), vp, vp, vp, vp, vp, vp,
                                        C.POINTER(TreeSankoffInfo)]
    L.vdjx_tree_split_support.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, C.POINTER(TreeSplitParams), vp, vp, C.POINTER(TreeSplitInfo)]
    L.vdjx_tree_split_compare.argtypes = [vp, sz, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vdjx_mutations_layout.argtypes = [vp, vp, vp, sz, vp]
    L.vdjx_mutations.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(MutInfo)]
    L.vdjx_selection.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, sz, vp, vp, u32, vp, vp, vp, C.POINTER(SelInfo)]
    L.vdjx_selection_convolve.argtypes = [vp, vp, sz, u32, vp, u32, vp, vp, C.POINTER(SelConvInfo)]
    L.vdjx_selection_convolve.restype = C.c_int
    L.vdjx_selection_compare.argtypes = [vp, sz, vp, sz, vp, vp]
    L.vdjx_selection_compare.restype = C.c_int
    L.vdjx_targeting_counts.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, vp, C.POINTER(TgtInfo)]
    L.vdjx_targeting_model.argtypes = [vp, i32, C.c_uint64, C.c_uint64, vp, vp]
    L.vdjx_consensus_layout.argtypes = [vp, vp, vp, sz, i32, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vdjx_consensus.argtypes = [vp, C.c_char_p, sz, i32, vp, vp, vp, C.POINTER(ConsParams), vp, vp, vp, vp, vp, vp, C.POINTER(ConsInfo)]
    L.vdjx_consensus_hits.argtypes = [vp, sz, vp, vp, i32, vp, vp, C.POINTER(i32)]
    L.vdjx_diversity.argtypes = [vp, vp, sz, vp, sz, C.POINTER(DiversityParams), vp, vp, vp, vp, vp, C.POINTER(DiversityInfo)]
    L.vdjx_scan_u32.argtypes =[vp, vp, sz, i32, i32, vp]
    L.vdjx_part_u64.argtypes = [vp, vp, sz, i32, u32, i32, u32, u32, u32, vp, vp]
    L.vdjx_trim.argtypes = [vp]
    L.vdjx_read_index_drop.argtypes = [vp]
    L.vdjx_device_copy.argtypes = [vp, vp, vp, C.c_size_t]
    L.vdjx_graph_roots.argtypes = [vp]
    L.vdjx_graph_roots.restype = C.c_size_t
    L.vdjx_root_part.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.vdjx_root_part.restype = C.c_size_t
    L.vdjx_root_score_graph.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp]
    L.vdjx_root_score_graph_begin.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp]
    L.vdjx_root_score_graph_end.argtypes = [vp]
    L.vdjx_index_generate.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), vp, vp]
    L.vdjx_anchor_sets_from_anchors.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int]
    L.vdjx_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.vdjx_host_free.argtypes = [vp, vp]
    L.vdjx_host_free.restype = None
    L.vdjx_host_take_rows.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    L.vdjx_stat.argtypes = [vp, C.c_char_p]
    L.vdjx_stat.restype = C.c_uint64
    L.vdjx_profile_enable.argtypes = [vp, i32]
    L.vdjx_profile_only.argtypes = [vp, C.c_char_p]
    L.vdjx_profile_reset.argtypes = [vp]
    L.vdjx_profile_count.argtypes = [vp]
    L.vdjx_profile_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise VdjxError(f"{what or 'vdjx'} failed ({rc}): {lib().vdjx_last_error().decode(errors='replace')}")
