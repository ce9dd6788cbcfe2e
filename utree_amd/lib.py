"""ctypes binding of the C-ABI in include/utree_amd.h.

The shared library is built in-tree (utree_amd/libutree_amd.so) by `make -C utree_amd/csrc` or
`__graft_entry__.build()`.  If it is missing, load() raises: there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("UTREE_AMD_SO") or os.path.join(_HERE, "libutree_amd.so")   # override: kernel experiments only
CLI_PATH = os.path.join(_HERE, "xtree-searchGG")
COMPRESS_CLI_PATH = os.path.join(_HERE, "xtree-compress")
RANK_CLI_PATH = os.path.join(_HERE, "xtree-search")
BUILD_GG_CLI_PATH = os.path.join(_HERE, "utree-buildGG")
BUILD_CLI_PATH = os.path.join(_HERE, "utree-build")
MERGE_GG_CLI_PATH = os.path.join(_HERE, "utree-mergeGG")
MERGE_CLI_PATH = os.path.join(_HERE, "utree-merge")
COMPARE_CLI_PATH = os.path.join(_HERE, "utree-compare")
INSPECT_CLI_PATH = os.path.join(_HERE, "utree-inspect")
TILES_CLI_PATH = os.path.join(_HERE, "utree-tiles")
_LIB = None

OK, E_IO, E_FORMAT, E_UNSUPPORTED, E_NOMEM, E_HIP, E_ARG, E_NOLABELS, E_FASTA, E_RCCL, E_BUILD, E_DEVICE, E_PROFILE, E_COVERAGE, E_PAIRS, E_HITMAP = range(16)
HIT_MISS, HIT_INVALID = 0xFFFFFFFF, 0xFFFFFFFE
TILE_MAX_BP, TILES_MAX_BATCH = 16777214, 1 << 21
REDIST_KEY_NONE = 0xFFFFFFFF
BUILD_E_MAP_EMPTY, BUILD_E_MAP, BUILD_E_FASTA, BUILD_E_NO_KMERS, BUILD_E_NAME = range(1, 6)
FINE_AUTO = -1
FANOUT_NONE, FANOUT_BROADCAST, FANOUT_UPLOAD = range(3)
REPLICATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p))
UPLOAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p))
INPUT_REFERENCE, INPUT_FASTQ, INPUT_FASTA_MULTILINE, INPUT_AUTO = range(4)


class CtrInfo(C.Structure):
    _fields_ = [("W", C.c_uint32), ("I", C.c_uint32), ("k", C.c_uint32), ("SZ", C.c_uint32), ("n_nodes", C.c_uint64),
                ("n_labels", C.c_uint32), ("binix_width", C.c_uint32), ("bin_total", C.c_uint64),
                ("file_bytes", C.c_uint64)]


class DevInfo(C.Structure):
    _fields_ = [("fine_bits", C.c_uint32), ("record_bytes", C.c_uint32), ("image_bytes", C.c_uint64),
                ("irregular_bins", C.c_uint64), ("generic_mode", C.c_uint32), ("device", C.c_int32),
                ("vote_table", C.c_uint32), ("lane_pass", C.c_uint32), ("bucket_bytes", C.c_uint32), ("strand_views", C.c_uint32),
                ("overflow_chains", C.c_uint32), ("pad0", C.c_uint32), ("overflow_bytes", C.c_uint64)]


class FastaError(C.Structure):
    _fields_ = [("code", C.c_int), ("read_index", C.c_uint64)]


class SearchStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("good_finds", C.c_uint64), ("seconds_total", C.c_double),
                ("seconds_kernels", C.c_double), ("fasta_error", FastaError), ("pipeline", C.c_int), ("n_lanes", C.c_int),
                ("seconds_read", C.c_double), ("seconds_frame", C.c_double), ("seconds_classify_format", C.c_double),
                ("seconds_order_wait", C.c_double), ("seconds_d2h", C.c_double), ("seconds_write", C.c_double),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64)]


class CompressStats(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_labels", C.c_uint64), ("label_count_total", C.c_uint64), ("W", C.c_uint32),
                ("I", C.c_uint32), ("seconds", C.c_double)]


class BuildStats(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("n_kmers", C.c_uint64), ("n_nodes", C.c_uint64), ("n_labels", C.c_uint64),
                ("error_line", C.c_uint64), ("error_kind", C.c_int), ("W", C.c_uint32), ("I", C.c_uint32),
                ("seconds", C.c_double), ("n_distinct", C.c_uint64), ("map_bytes", C.c_uint64), ("map_lines", C.c_uint64),
                ("map_error", C.c_int)]


class MergeStats(C.Structure):
    """utree_merge_stats: nodes read and written, the shared words and what became of them, labels written, passes."""
    _fields_ = [("n_in_nodes", C.c_uint64), ("n_nodes", C.c_uint64), ("n_shared", C.c_uint64), ("n_relabelled", C.c_uint64),
                ("n_dropped", C.c_uint64), ("n_labels", C.c_uint64), ("W", C.c_uint32), ("I", C.c_uint32), ("n_inputs", C.c_uint32),
                ("n_passes", C.c_uint32), ("seconds", C.c_double)]


class MergeInput(C.Structure):
    """utree_merge_input: how utree_merge_files reads one input file."""
    _fields_ = [("W", C.c_uint32), ("I", C.c_uint32), ("is_ctr", C.c_uint32), ("pad", C.c_uint32), ("n_nodes", C.c_uint64),
                ("n_labels", C.c_uint64)]


class MergeEdit(C.Structure):
    """utree_merge_edit: the edit of utree_merge_files_edit; the paths are bytes or None, `size` is filled in."""
    _fields_ = [("size", C.c_uint32), ("ranks", C.c_uint32), ("drop_path", C.c_char_p), ("keep_path", C.c_char_p),
                ("rename_path", C.c_char_p), ("minus_paths", C.POINTER(C.c_char_p)), ("n_minus", C.c_int)]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(MergeEdit), **kw)


class MergeEditStats(C.Structure):
    """utree_merge_edit_stats: what the label edit did to the label lines, and the nodes it and the MINUS inputs kept from being fed."""
    _fields_ = [("n_label_lines", C.c_uint64), ("n_labels_dropped", C.c_uint64), ("n_labels_renamed", C.c_uint64),
                ("n_labels_cut", C.c_uint64), ("n_rules_unmatched", C.c_uint64), ("n_nodes_dropped", C.c_uint64),
                ("n_minus_nodes", C.c_uint64), ("n_nodes_subtracted", C.c_uint64)]


class CompareStats(C.Structure):
    """utree_compare_stats: the seven figures summed over all label texts (a, b: the nodes of A and of B; left == arrived == changed), the
    distinct words and those in both, the label texts each side's nodes carry, the distinct moves, W, passes, identical, seconds."""
    _fields_ = [("a", C.c_uint64), ("b", C.c_uint64), ("same", C.c_uint64), ("only_a", C.c_uint64), ("only_b", C.c_uint64),
                ("left", C.c_uint64), ("arrived", C.c_uint64), ("words", C.c_uint64), ("both", C.c_uint64), ("a_labels", C.c_uint64),
                ("b_labels", C.c_uint64), ("n_moves", C.c_uint64), ("W", C.c_uint32), ("n_passes", C.c_uint32), ("identical", C.c_uint32),
                ("pad", C.c_uint32), ("seconds", C.c_double)]


class CompareInput(C.Structure):
    """utree_compare_input: how a report's `# a` / `# b` line describes an input."""
    _fields_ = [("path", C.c_char_p), ("is_ctr", C.c_uint32), ("W", C.c_uint32), ("I", C.c_uint32), ("pad", C.c_uint32)]


class CompareEntry(C.Structure):
    """utree_compare_entry: a label text and its five counted figures."""
    _fields_ = [("text", C.c_char_p), ("len", C.c_uint32), ("pad", C.c_uint32), ("same", C.c_uint64), ("only_a", C.c_uint64),
                ("only_b", C.c_uint64), ("left", C.c_uint64), ("arrived", C.c_uint64)]


class CompareMove(C.Structure):
    """utree_compare_move: `kmers` changed words whose label is entry `from_` in A and entry `to` in B."""
    _fields_ = [("from_", C.c_uint32), ("to", C.c_uint32), ("kmers", C.c_uint64)]


class InspectStats(C.Structure):
    """utree_inspect_stats: the nodes and their four classes summed over all label texts, the pair events and the distinct pairs, the label
    texts nodes carry, how the input reads, passes, clean (no conflict node), seconds in all and in the neighbour pass."""
    _fields_ = [("kmers", C.c_uint64), ("isolated", C.c_uint64), ("same", C.c_uint64), ("lineage", C.c_uint64), ("conflict", C.c_uint64),
                ("pair_events", C.c_uint64), ("distinct_pairs", C.c_uint64), ("labels", C.c_uint64), ("W", C.c_uint32), ("I", C.c_uint32),
                ("is_ctr", C.c_uint32), ("n_passes", C.c_uint32), ("clean", C.c_uint32), ("pad", C.c_uint32), ("seconds", C.c_double),
                ("seconds_neighbours", C.c_double)]


class InspectEntry(C.Structure):
    """utree_inspect_entry: a label text and its four class counts."""
    _fields_ = [("text", C.c_char_p), ("len", C.c_uint32), ("pad", C.c_uint32), ("isolated", C.c_uint64), ("same", C.c_uint64),
                ("lineage", C.c_uint64), ("conflict", C.c_uint64)]


class InspectPair(C.Structure):
    """utree_inspect_pair: `pairs` pair events from nodes of entry `from_` to neighbours of entry `to`."""
    _fields_ = [("from_", C.c_uint32), ("to", C.c_uint32), ("pairs", C.c_uint64)]


class RankParams(C.Structure):
    """SLACK, SPARSITY, TOLERANCE_THRESHOLD of the rank-specific search (itree.c:952-960)."""
    _fields_ = [("slack", C.c_uint32), ("sparsity", C.c_uint32), ("tolerance", C.c_uint32)]


class SearchRequest(C.Structure):
    """utree_search_request: one whole-file search as utree_search_run takes it; the paths are bytes or None, `size` is filled in."""
    _fields_ = [("size", C.c_uint32), ("do_rc", C.c_int), ("host_threads", C.c_int), ("input_format", C.c_int),
                ("reads_path", C.c_char_p), ("mates_path", C.c_char_p), ("interleaved", C.c_int), ("out_path", C.c_char_p),
                ("rank", C.POINTER(RankParams)), ("profile_path", C.c_char_p), ("coverage_path", C.c_char_p),
                ("redistribute_path", C.c_char_p), ("max_passes", C.c_uint32), ("hitmap_path", C.c_char_p), ("samples_path", C.c_char_p),
                ("sample_redistribute_path", C.c_char_p), ("sample_delim", C.c_int), ("redistribute_reads_path", C.c_char_p)]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(SearchRequest), **kw)


class ProfileEntry(C.Structure):
    """utree_profile_entry: reads whose line prints (label, cut) -- cut -2 whole label, -1 empty taxon, >= 0 the first cut bytes."""
    _fields_ = [("label", C.c_uint32), ("cut", C.c_int32), ("reads", C.c_uint64)]


class CoverageEntry(C.Structure):
    """utree_coverage_entry: per label, the records the dump holds, the distinct ones hit, the hits."""
    _fields_ = [("label", C.c_uint32), ("pad", C.c_uint32), ("db_kmers", C.c_uint64), ("covered", C.c_uint64), ("hits", C.c_uint64)]


class RedistSet(C.Structure):
    """utree_redist_set: a distinct candidate set -- `reads` reads, labels [first, first + n) of the flat label array."""
    _fields_ = [("reads", C.c_uint64), ("first", C.c_uint64), ("n", C.c_uint32), ("pad", C.c_uint32)]


class RedistEntry(C.Structure):
    """utree_redist_entry: per label, the reads assigned to it after the passes and the reads whose only candidate it is."""
    _fields_ = [("label", C.c_uint32), ("pad", C.c_uint32), ("assigned", C.c_uint64), ("unique", C.c_uint64)]


class PairsMeta(C.Structure):
    """utree_pairs_meta: what the device join of a batch of pairs reports (error 0, 1 joined buffer too small, 2 a pair too long)."""
    _fields_ = [("total_bases", C.c_uint64), ("max_len", C.c_uint32), ("error", C.c_uint32)]


class HitRun(C.Structure):
    """utree_hit_run: a maximal stretch of windows with one code (a label index, HIT_MISS or HIT_INVALID)."""
    _fields_ = [("code", C.c_uint32), ("count", C.c_uint32)]


class HitmapMeta(C.Structure):
    """utree_hitmap_meta: error 0, 1 run_capacity too small, 2 total_bases too small, 3 a query of 2^32 windows or more."""
    _fields_ = [("total_runs", C.c_uint64), ("total_windows", C.c_uint64), ("error", C.c_uint32), ("pad", C.c_uint32)]


class TilesMeta(C.Structure):
    """utree_tiles_meta: the batch's tiles; the bases and the longest tile of a range of them; error 1: the range ends behind the tiles."""
    _fields_ = [("total_tiles", C.c_uint64), ("total_bases", C.c_uint64), ("max_len", C.c_uint32), ("error", C.c_uint32)]


class TilesRun(C.Structure):
    """utree_tiles_run: the run of tiles that utree_tiles_segments_format holds open between two calls."""
    _fields_ = [("open", C.c_uint32), ("query", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64), ("n_tiles", C.c_uint64),
                ("found", C.c_uint64), ("classified", C.c_uint32), ("label", C.c_uint32), ("taxon_len", C.c_uint64)]


class TilesParams(C.Structure):
    """utree_tiles_params: tile length and step in bases, RC, UTREE_INPUT_*, the formatting team; `size` is filled in."""
    _fields_ = [("size", C.c_uint32), ("tile_bp", C.c_uint32), ("step_bp", C.c_uint32), ("do_rc", C.c_int32), ("input_format", C.c_int32),
                ("host_threads", C.c_int32)]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(TilesParams), **kw)


class TilesStats(C.Structure):
    """utree_tiles_stats: what utree_tiles_file counted and how long it took; `size` is filled in."""
    _fields_ = [("size", C.c_uint32), ("pad", C.c_uint32), ("n_queries", C.c_uint64), ("n_tiles", C.c_uint64), ("classified", C.c_uint64),
                ("segments", C.c_uint64), ("bytes_in", C.c_uint64), ("n_batches", C.c_uint64), ("fasta_error", FastaError),
                ("seconds_total", C.c_double), ("seconds_device", C.c_double)]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(TilesStats), **kw)


class SamplesCell(C.Structure):
    """utree_samples_cell: reads of sample `sample` whose line prints (label, cut), keyed as ProfileEntry."""
    _fields_ = [("sample", C.c_uint32), ("label", C.c_uint32), ("cut", C.c_int32), ("pad", C.c_uint32), ("reads", C.c_uint64)]


class SamplesTable(C.Structure):
    """utree_samples_table: one handle's read-back as utree_samples_write takes it."""
    _fields_ = [("ids", C.c_void_p), ("id_off", C.c_void_p), ("reads", C.c_void_p), ("unclassified", C.c_void_p), ("n_samples", C.c_size_t),
                ("cells", C.c_void_p), ("n_cells", C.c_size_t), ("n_reads", C.c_uint64)]


class SredistCell(C.Structure):
    """utree_sredist_cell: `reads` reads of sample `sample` whose candidates are labels [first, first + n) of the flat label array."""
    _fields_ = [("sample", C.c_uint32), ("n", C.c_uint32), ("first", C.c_uint64), ("reads", C.c_uint64)]


class SredistEntry(C.Structure):
    """utree_sredist_entry: per (sample, label), the reads assigned after the sample's passes and the reads whose only candidate it is."""
    _fields_ = [("sample", C.c_uint32), ("label", C.c_uint32), ("assigned", C.c_uint64), ("unique", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [("label", C.c_uint32), ("cut", C.c_int32), ("found", C.c_uint32), ("uix", C.c_uint32),
                ("sl", C.c_uint32), ("ol", C.c_uint32)]


# every symbol include/utree_amd.h declares
SYMBOLS = {
    "utree_strerror": (C.c_char_p, [C.c_int]),
    "utree_abi_version": (C.c_int, []),
    "utree_last_hip_error": (C.c_char_p, []),
    "utree_ctr_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "utree_ctr_from_memory": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "utree_ctr_close": (None, [C.c_void_p]),
    "utree_ctr_get_info": (C.c_int, [C.c_void_p, C.POINTER(CtrInfo)]),
    "utree_ctr_label": (C.c_void_p, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "utree_dev_image_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "utree_dev_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "utree_dev_upload_seconds": (C.c_int, [C.POINTER(C.c_double)]),
    "utree_dev_build": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.POINTER(C.c_void_p)]),
    "utree_dev_image": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "utree_dev_attach": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "utree_dev_free": (None, [C.c_void_p]),
    "utree_dev_get_info": (C.c_int, [C.c_void_p, C.POINTER(DevInfo)]),
    "utree_dev_replicate": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "utree_dev_replicate_seconds": (C.c_double, []),
    "utree_dev_fanout": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "utree_dev_fanout_with": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                        C.c_void_p, C.c_void_p]),
    "utree_rccl_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "utree_dev_replicate_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_void_p)]),
    "utree_classify_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int]),
    "utree_classify_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                       C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "utree_classify_poll": (C.c_int, [C.c_void_p]),
    "utree_lookup_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "utree_classify_kernel_name": (C.c_char_p, [C.c_void_p]),
    "utree_model_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "utree_classify_kernel_time": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "utree_fasta_frame": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(FastaError)]),
    "utree_format_records": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "utree_compress_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(CompressStats)]),
    "utree_rank_params_default": (None, [C.POINTER(RankParams)]),
    "utree_rank_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int,
                                                C.POINTER(RankParams)]),
    "utree_rank_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32,
                                   C.c_int, C.POINTER(RankParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "utree_rank_reset": (C.c_int, [C.c_void_p]),
    "utree_format_rank_records": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "utree_rank_search_file": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RankParams),
                                         C.c_int, C.POINTER(SearchStats)]),
    "utree_reads_frame": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(FastaError)]),
    "utree_search_file_opts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(SearchStats)]),
    "utree_rank_search_file_opts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RankParams),
                                              C.c_int, C.c_int, C.POINTER(SearchStats)]),
    "utree_build_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(BuildStats)]),
    "utree_merge_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(MergeStats)]),
    "utree_merge_probe": (C.c_int, [C.c_char_p, C.POINTER(MergeInput)]),
    "utree_merge_files_edit": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(MergeEdit),
                                         C.POINTER(MergeStats), C.POINTER(MergeEditStats)]),
    "utree_merge_edit_preview": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.POINTER(MergeEdit), C.c_char_p, C.POINTER(MergeEditStats)]),
    "utree_compare_files": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(CompareStats)]),
    "utree_compare_write": (C.c_int, [C.POINTER(CompareInput), C.POINTER(CompareInput), C.POINTER(CompareEntry), C.c_size_t,
                                      C.POINTER(CompareMove), C.c_size_t, C.c_char_p, C.c_char_p, C.POINTER(CompareStats)]),
    "utree_inspect_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(InspectStats)]),
    "utree_inspect_write": (C.c_int, [C.POINTER(CompareInput), C.POINTER(InspectEntry), C.c_size_t, C.POINTER(InspectPair), C.c_size_t,
                                      C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.POINTER(InspectStats)]),
    "utree_search_prepare":(C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "utree_search_file": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                    C.POINTER(SearchStats)]),
    "utree_search_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(SearchRequest), C.POINTER(SearchStats)]),
    "utree_profile_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "utree_profile_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "utree_profile_reset": (C.c_int, [C.c_void_p]),
    "utree_profile_max_entries": (C.c_size_t, [C.c_void_p]),
    "utree_profile_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]),
    "utree_profile_free": (None, [C.c_void_p]),
    "utree_profile_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_char_p]),
    "utree_search_file_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                            C.c_int, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_coverage_bytes": (C.c_size_t, [C.c_void_p]),
    "utree_coverage_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "utree_coverage_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "utree_coverage_reset": (C.c_int, [C.c_void_p]),
    "utree_coverage_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "utree_coverage_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]),
    "utree_coverage_free": (None, [C.c_void_p]),
    "utree_coverage_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_char_p]),
    "utree_search_file_coverage": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                             C.c_int, C.c_char_p, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_redist_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "utree_redist_reset": (C.c_int, [C.c_void_p]),
    "utree_redist_free": (None, [C.c_void_p]),
    "utree_redist_classify_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                              C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "utree_redist_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "utree_redist_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "utree_redist_solve": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint64)]),
    "utree_redist_classify_batch_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                                   C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "utree_redist_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "utree_redist_reads_format": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_size_t]),
    "utree_redist_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p]),
    "utree_search_file_redistribute": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                                 C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(SearchStats)]),
    "utree_pairs_join": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                   C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "utree_search_pairs_file": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                          C.c_int, C.c_char_p, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_hitmap_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int]),
    "utree_hitmap_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "utree_hitmap_format": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "utree_search_file_hitmap": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                           C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_rank_search_file_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RankParams),
                                                 C.c_int, C.c_int, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_samples_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "utree_samples_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "utree_samples_reset": (C.c_int, [C.c_void_p]),
    "utree_samples_free": (None, [C.c_void_p]),
    "utree_samples_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "utree_samples_write": (C.c_int, [C.c_void_p, C.POINTER(SamplesTable), C.c_size_t, C.c_char_p]),
    "utree_search_file_samples": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                            C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int,
                                            C.POINTER(SearchStats)]),
    "utree_rank_search_file_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RankParams),
                                                 C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(SearchStats)]),
    "utree_sredist_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "utree_sredist_reset": (C.c_int, [C.c_void_p]),
    "utree_sredist_free": (None, [C.c_void_p]),
    "utree_sredist_classify_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32,
                                               C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
    "utree_sredist_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "utree_sredist_insert": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.c_uint64]),
    "utree_sredist_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "utree_sredist_solve": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "utree_sredist_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_size_t, C.c_uint64, C.c_char_p]),
    "utree_search_file_sample_redistribute": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p,
                                                        C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p,
                                                        C.c_char_p, C.c_int, C.c_char_p, C.POINTER(SearchStats)]),
    "utree_tiles_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32]),
    "utree_tiles_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "utree_tiles_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "utree_tiles_format": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "utree_tiles_segments_format": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(TilesRun), C.c_void_p, C.c_size_t,
                                                 C.POINTER(C.c_uint64)]),
    "utree_tiles_file": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(TilesParams), C.POINTER(TilesStats)]),
}


def kernel_source_sha256() -> str:
    """Content hash of the sources the search kernels are compiled from: a kept profile (profiles/traffic.json) is only valid
    for the library built from exactly these files (bench.py checks it)."""
    import hashlib
    h = hashlib.sha256()
    for f in ("kernels.hip", "lanes_kernel.hip", "lanes_core.hpp", "lanes_part.hip", "wave_common.hpp", "device_common.hpp", "utree_internal.h", "Makefile"):
        with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read() + b"\0")
    return h.hexdigest()


class UtreeError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = load().utree_strerror(code).decode() if _LIB is not None else str(code)
        if _LIB is not None and code in (4, 5, 11, 12, 13, 14, 15):    # UTREE_E_HITMAP: why; UTREE_E_NOMEM, UTREE_E_HIP, UTREE_E_DEVICE: which call, and what the runtime said; UTREE_E_PROFILE / UTREE_E_COVERAGE: why; UTREE_E_PAIRS: which file ended first
            hip = (_LIB.utree_last_hip_error() or b"").decode(errors="replace")
            if hip:
                msg += " [" + hip + "]"
        super().__init__("%s: %s (code %d)" % (what, msg, code))


def load():
    """Load libutree_amd.so. Raises (loudly) when it has not been built: no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise ImportError("utree_amd: %s is missing -- build it with `make -C utree_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback" % SO_PATH)
        # torch ships its own libamdhip64.so.7 / librccl.so.1.  Loading it FIRST makes the dynamic loader
        # resolve this library's HIP/RCCL dependencies to those same copies (matching sonames), so the
        # process holds ONE HIP runtime and torch's device pointers / streams are valid in our calls.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)          # AttributeError if the .so does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def check(code, what=""):
    if code != OK:
        raise UtreeError(code, what)
