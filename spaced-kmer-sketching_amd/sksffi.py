"""ctypes binding of libsks.so (include/sks.h) for the tests and bench.py.

This is plumbing only: every computation happens in libsks.so (HIP kernels for
gfx950 + host ingress).  There is deliberately no CPU fallback — if the library
or a GPU is missing, the calls below raise.  Device buffers are torch tensors
on `cuda:N` whose data_ptr() is handed to the C ABI.
"""
import ctypes as C
import math
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SKS_LIB") or os.path.join(PKG_DIR, "lib", "libsks.so")

SKS_FRAC_MOD = 0
SKS_BOTTOM_S = 1
SKS_FILTER_SUBTRACT, SKS_FILTER_INTERSECT = 0, 1  # sks_filter_kind
FILTER_NONE = 0xFFFFFFFF  # a filter_of entry: the sketch is copied unchanged
ABUND_NO_LIMIT = 0xFFFFFFFF  # max_abund of sks_sketch_build_counted / sks_sketch_set_abund_trim: no upper limit
TALLY_NO_LIMIT = 0xFFFFFFFF  # a max_count entry of Context.tally: no upper limit
INTERSECT_AUTO, INTERSECT_MERGE, INTERSECT_JOIN, INTERSECT_GLOBAL = 0, 1, 2, 3
FRAC_POST_AUTO, FRAC_POST_GENERAL, FRAC_POST_FUSED = 0, 1, 2
BUILD_PATH_GENERAL, BUILD_PATH_FUSED, BUILD_PATH_FUSED_THEN_GENERAL_POST = 0, 1, 2
FLAVOUR_BOOST_MIX = 0
FLAVOUR_BOOST_LEGACY = 1


# sks_status (include/sks.h)
SKS_OK, SKS_E_ARG, SKS_E_HIP, SKS_E_IO, SKS_E_NOMEM, SKS_E_UNSUPPORTED, SKS_E_LENGTH = range(7)


class SksError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sks error {code}: {msg}")
        self.code = code


class Policy(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flavour", C.c_int32), ("param", C.c_uint64),
                ("nonce", C.c_int64)]


class SketchInfo(C.Structure):
    _fields_ = [("window", C.c_int32), ("elem_words", C.c_int32), ("mask", C.c_uint64 * 2),
                ("policy", Policy), ("n", C.c_uint32), ("has_names", C.c_int32)]


class Timings(C.Structure):
    _fields_ = [("scan_ms", C.c_float), ("post_ms", C.c_float), ("total_ms", C.c_float),
                ("windows", C.c_uint64), ("scan_launches", C.c_uint64),
                ("survivors", C.c_uint64)]


EXPORTED = [
    "sks_abi_version", "sks_last_error", "sks_build_info", "sks_mask_generate", "sks_mask_contiguous",
    "sks_frac_min_hash", "sks_containment", "sks_binomial_estimator", "sks_ani_from_counts",
    "sks_fasta_open", "sks_fasta_close", "sks_fasta_num_records", "sks_fasta_record",
    "sks_fasta_stream", "sks_fasta_stream_bytes", "sks_fasta_runs", "sks_ctx_create",
    "sks_ctx_destroy", "sks_ctx_set_stream", "sks_ctx_synchronize", "sks_ctx_last_timings",
    "sks_sketch_build", "sks_sketch_set_free", "sks_sketch_set_free_on_stream", "sks_sketch_set_num", "sks_sketch_set_elem_words",
    "sks_ctx_set_layout_blocks_hint", "sks_ctx_ani_table",
    "sks_sketch_set_sizes", "sks_sketch_set_windows", "sks_sketch_set_device_data",
    "sks_sketch_set_device_starts", "sks_sketch_set_device_sizes", "sks_sketch_set_starts",
    "sks_sketch_set_copy", "sks_sketch_set_export", "sks_intersect_pairs", "sks_intersect_all",
    "sks_synth_bases", "sks_intersect_sym", "sks_intersect_sym_tiles",
    "sks_ctx_last_intersect_ms", "sks_ctx_set_scan_grid", "sks_ctx_set_intersect_kernel", "sks_join_layout_log_b", "sks_sketch_union", "sks_sketch_union_wide",
    "sks_join_layout_capacity", "sks_join_layout_build", "sks_intersect_sym_layout", "sks_fasta_parse_device",
    "sks_ctx_last_ingress_ms", "sks_kmer_list_build", "sks_kmer_list_free", "sks_kmer_list_total",
    "sks_kmer_list_counts", "sks_kmer_list_device_positions", "sks_kmer_list_device_bits",
    "sks_kmer_list_copy", "sks_ctx_device", "sks_sketch_set_info", "sks_sketch_set_set_names",
    "sks_sketch_set_name", "sks_sketch_set_save", "sks_sketch_set_load", "sks_sketch_set_concat",
    "sks_intersect_layout_tiles",
    "sks_join_layout_bounds", "sks_join_layout_groups", "sks_join_layout_boff_words",
    "sks_ctx_set_join_check", "sks_ctx_join_check_violations", "sks_intersect_layout_pair_tiles",
    "sks_sketch_set_export_csr", "sks_ani_matrix", "sks_ani_rows", "sks_ani_tiles",
    "sks_intersect_layout_ani", "sks_host_alloc", "sks_host_free", "sks_join_layout_stat_copy",
    "sks_sketches_export", "sks_all_pairs_ani", "sks_windows_dense", "sks_windows_dense_row_words",
    "sks_join_layout_bounds_for_mask", "sks_layout_tiles_ani",
    "sks_ctx_set_frac_post", "sks_ctx_last_build_path",
    "sks_search", "sks_search_sets", "sks_ctx_set_search_batch", "sks_sketch_set_downsample",
    "sks_sketch_set_merge", "sks_cluster", "sks_cluster_set",
    "sks_gather", "sks_gather_sets", "sks_ctx_set_gather_rounds",
    "sks_search_topk", "sks_search_topk_sets", "sks_sketch_set_filter", "sks_sketch_set_tally",
    "sks_join_layout_region_log", "sks_join_launch_plan",
    "sks_sketch_build_counted", "sks_sketch_set_has_abund", "sks_sketch_set_device_abund",
    "sks_sketch_set_abund_copy", "sks_sketch_set_abund_totals", "sks_sketch_set_abund_trim", "sks_abund_pairs",
]

# sks_hit (include/sks.h): one record of Context.search's result
HIT_DTYPE = np.dtype([("query", "<u4"), ("ref", "<u4"), ("shared", "<i4"), ("query_size", "<i4"),
                      ("containment", "<f8"), ("ani", "<f8")])
assert HIT_DTYPE.itemsize == 32

# sks_rank_kind, SKS_TOPK_MAX and sks_top_hit (include/sks.h): one slot of Context.search_topk's result
SKS_RANK_QUERY, SKS_RANK_REF, SKS_RANK_MAX = 0, 1, 2
SKS_TOPK_MAX = 64
TOP_HIT_DTYPE = np.dtype([("query", "<u4"), ("ref", "<u4"), ("shared", "<i4"), ("query_size", "<i4"),
                          ("ref_size", "<i4"), ("rank", "<u4"), ("score", "<f8"), ("ani", "<f8")])
assert TOP_HIT_DTYPE.itemsize == 40


# sks_gather_hit (include/sks.h): the C structure, and one record of Context.gather's result
class GatherHit(C.Structure):
    _fields_ = [("ref", C.c_uint32), ("shared", C.c_int32), ("shared_new", C.c_int32), ("ref_size", C.c_int32),
                ("f_query_new", C.c_double), ("ani", C.c_double)]


GATHER_HIT_DTYPE = np.dtype([("ref", "<u4"), ("shared", "<i4"), ("shared_new", "<i4"), ("ref_size", "<i4"),
                             ("f_query_new", "<f8"), ("ani", "<f8")])
assert GATHER_HIT_DTYPE.itemsize == 32 == C.sizeof(GatherHit)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libsks.so not built ({LIB_PATH}); run __graft_entry__.build()")
    # PyTorch-ROCm ships its own libamdhip64 with the same SONAME as /opt/rocm's
    # (libamdhip64.so.7): whichever loads first serves both.  Load torch first
    # when it is installed, so a process that also uses torch device memory and
    # streams runs ONE HIP runtime — the order every GPU test and bench.py use.
    # (libsks loaded first, then torch, left sks_ctx_create without devices.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    u64p = C.POINTER(C.c_uint64)
    vp = C.c_void_p
    L.sks_last_error.restype = C.c_char_p
    L.sks_build_info.restype = C.c_char_p
    L.sks_mask_generate.argtypes = [C.c_int, C.c_int, C.c_uint64, u64p]
    L.sks_mask_contiguous.argtypes = [C.c_int, u64p]
    L.sks_frac_min_hash.argtypes = [u64p, u64p, C.c_int, C.c_int64, C.c_int]
    L.sks_frac_min_hash.restype = C.c_uint64
    L.sks_containment.argtypes = [C.c_int, C.c_int]
    L.sks_containment.restype = C.c_double
    L.sks_binomial_estimator.argtypes = [C.c_double, C.c_int]
    L.sks_binomial_estimator.restype = C.c_double
    L.sks_ani_from_counts.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp]
    L.sks_fasta_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.sks_fasta_close.argtypes = [vp]
    L.sks_fasta_close.restype = None
    L.sks_fasta_num_records.argtypes = [vp]
    L.sks_fasta_num_records.restype = C.c_uint64
    L.sks_fasta_record.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p]
    L.sks_fasta_stream.argtypes = [vp]
    L.sks_fasta_stream.restype = vp
    L.sks_fasta_stream_bytes.argtypes = [vp]
    L.sks_fasta_stream_bytes.restype = C.c_uint64
    L.sks_fasta_runs.argtypes = [vp, vp, vp, u64p, u64p]
    L.sks_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.sks_ctx_destroy.argtypes = [vp]
    L.sks_ctx_set_stream.argtypes = [vp, vp]
    L.sks_ctx_synchronize.argtypes = [vp]
    L.sks_ctx_last_timings.argtypes = [vp, C.POINTER(Timings)]
    L.sks_ctx_set_scan_grid.argtypes = [vp, C.c_int]
    L.sks_ctx_set_intersect_kernel.argtypes = [vp, C.c_int]
    L.sks_ctx_set_frac_post.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
    L.sks_ctx_last_build_path.argtypes = [vp]
    L.sks_sketch_union.argtypes = [vp, vp, C.c_uint64, vp, u64p]
    L.sks_sketch_union_wide.argtypes = [vp, vp, C.c_uint64, vp, u64p]
    L.sks_join_layout_log_b.argtypes = [C.c_uint32]
    L.sks_join_layout_log_b.restype = C.c_uint32
    L.sks_join_layout_capacity.argtypes = []
    L.sks_join_layout_capacity.restype = C.c_uint32
    L.sks_join_layout_region_log.argtypes = [C.c_uint32, C.c_uint32]
    L.sks_join_layout_region_log.restype = C.c_uint32
    L.sks_join_launch_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sks_join_launch_plan.restype = C.c_int
    L.sks_join_layout_build.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, vp,
                                        vp, vp, vp, vp, C.POINTER(C.c_uint32)]
    L.sks_join_layout_bounds.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp]
    L.sks_join_layout_groups.argtypes = [C.c_uint32]
    L.sks_join_layout_groups.restype = C.c_uint32
    L.sks_join_layout_boff_words.argtypes = [C.c_uint32]
    L.sks_join_layout_boff_words.restype = C.c_uint32
    L.sks_intersect_sym_layout.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, C.c_uint64,
                                           C.c_uint64, vp]
    L.sks_intersect_layout_tiles.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, C.c_uint32,
                                             vp, C.c_uint64, C.c_uint64, C.c_int, vp]
    L.sks_intersect_layout_pair_tiles.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp,
                                                  C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64,
                                                  C.c_uint64, C.c_int, vp]
    L.sks_intersect_layout_ani.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, C.c_uint32,
                                           vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, C.c_int, vp,
                                           vp, C.c_int, vp]
    L.sks_host_alloc.argtypes = [C.c_uint64, C.c_int, C.POINTER(vp)]
    L.sks_host_free.argtypes = [vp]
    L.sks_join_layout_stat_copy.argtypes = [vp, vp]
    L.sks_sketches_export.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, vp, C.c_uint64, vp]
    L.sks_all_pairs_ani.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, vp, vp,
                                    vp]
    L.sks_layout_tiles_ani.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, vp,
                                       C.c_uint32, C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, C.c_int, vp, vp, vp]
    L.sks_sketch_set_export_csr.argtypes = [vp, vp, vp]
    L.sks_ani_matrix.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp]
    L.sks_ani_rows.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp]
    L.sks_ani_tiles.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_int, vp]
    L.sks_ctx_set_join_check.argtypes = [vp, C.c_int]
    L.sks_ctx_ani_table.argtypes = [vp, C.c_uint32, C.c_int]
    L.sks_ctx_join_check_violations.argtypes = [vp, u64p]
    L.sks_ctx_last_intersect_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.sks_ctx_last_ingress_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.sks_ctx_device.argtypes = [vp]
    L.sks_sketch_set_info.argtypes = [vp, C.POINTER(SketchInfo)]
    L.sks_sketch_set_set_names.argtypes = [vp, vp]
    L.sks_sketch_set_name.argtypes = [vp, C.c_uint32]
    L.sks_sketch_set_name.restype = C.c_char_p
    L.sks_sketch_set_save.argtypes = [vp, C.c_char_p]
    L.sks_sketch_set_load.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.sks_sketch_set_concat.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
    L.sks_sketch_set_downsample.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp)]
    L.sks_sketch_set_merge.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.sks_sketch_set_filter.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
    L.sks_sketch_set_tally.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.POINTER(vp), vp,
                                       C.c_uint64]
    L.sks_sketch_build_counted.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, u64p, C.POINTER(Policy),
                                           C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sks_sketch_set_has_abund.argtypes = [vp]
    L.sks_sketch_set_device_abund.argtypes = [vp]
    L.sks_sketch_set_device_abund.restype = vp
    L.sks_sketch_set_abund_copy.argtypes = [vp, C.c_uint32, vp]
    L.sks_sketch_set_abund_totals.argtypes = [vp, vp]
    L.sks_sketch_set_abund_trim.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sks_abund_pairs.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, vp, vp]
    L.sks_kmer_list_build.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, u64p,
                                      C.POINTER(Policy), C.POINTER(vp)]
    L.sks_windows_dense.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, u64p, vp, vp]
    L.sks_windows_dense_row_words.argtypes = [C.c_int]
    L.sks_join_layout_bounds_for_mask.argtypes = [u64p, C.c_uint32, C.c_int, vp]
    L.sks_kmer_list_free.argtypes = [vp]
    L.sks_kmer_list_total.argtypes = [vp]
    L.sks_kmer_list_total.restype = C.c_uint64
    L.sks_kmer_list_counts.argtypes = [vp, vp]
    L.sks_kmer_list_copy.argtypes = [vp, vp, vp]
    for f in ("sks_kmer_list_device_positions", "sks_kmer_list_device_bits"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.sks_fasta_parse_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64,
                                         u64p, u64p]
    L.sks_sketch_build.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, u64p,
                                   C.POINTER(Policy), C.POINTER(vp)]
    L.sks_sketch_set_free.argtypes = [vp]
    L.sks_sketch_set_free_on_stream.argtypes = [vp, vp]
    L.sks_sketch_set_num.argtypes = [vp]
    L.sks_sketch_set_num.restype = C.c_uint32
    L.sks_sketch_set_elem_words.argtypes = [vp]
    L.sks_sketch_set_sizes.argtypes = [vp, vp]
    L.sks_sketch_set_windows.argtypes = [vp, vp]
    L.sks_sketch_set_starts.argtypes = [vp, vp]
    for f in ("sks_sketch_set_device_data", "sks_sketch_set_device_starts",
              "sks_sketch_set_device_sizes"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.sks_sketch_set_copy.argtypes = [vp, C.c_uint32, vp]
    L.sks_sketch_set_export.argtypes = [vp, vp, C.c_uint64, vp]
    L.sks_intersect_pairs.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_uint64, vp]
    L.sks_intersect_all.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                    vp]
    L.sks_intersect_sym.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64,
                                    vp]
    L.sks_intersect_sym_tiles.argtypes = [C.c_uint32]
    L.sks_intersect_sym_tiles.restype = C.c_uint64
    L.sks_synth_bases.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double,
                                  C.c_uint64]
    L.sks_search.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_uint32,
                             C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_int32, vp, C.c_uint64,
                             u64p]
    L.sks_search_sets.argtypes = [vp, vp, vp, C.c_double, C.c_int32, vp, C.c_uint64, u64p]
    L.sks_ctx_set_search_batch.argtypes = [vp, C.c_uint32]
    L.sks_cluster.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_double,
                              C.c_int32, vp, vp, C.POINTER(C.c_uint32)]
    L.sks_cluster_set.argtypes = [vp, vp, C.c_double, C.c_int32, vp, vp, C.POINTER(C.c_uint32)]
    L.sks_gather.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                             C.c_int32, C.c_uint32, vp, C.c_uint64, u64p, C.POINTER(C.c_uint32)]
    L.sks_gather_sets.argtypes = [vp, vp, C.c_uint32, vp, C.c_int32, C.c_uint32, vp, C.c_uint64, u64p,
                                  C.POINTER(C.c_uint32)]
    L.sks_ctx_set_gather_rounds.argtypes = [vp, C.c_uint32]
    L.sks_search_topk.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_uint32,
                                  C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_double,
                                  C.c_int32, C.c_int, vp, vp]
    L.sks_search_topk_sets.argtypes = [vp, vp, vp, C.c_int, C.c_uint32, C.c_double, C.c_int32, C.c_int, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise SksError(rc, lib().sks_last_error().decode(errors="replace"))


def _mask_arr(mask):
    return (C.c_uint64 * 2)(mask & (2**64 - 1), mask >> 64)


# ---- host helpers -------------------------------------------------------------------
def mask_generate(window, k, seed=0):
    out = (C.c_uint64 * 2)()
    check(lib().sks_mask_generate(window, k, seed, out))
    return int(out[0]) | (int(out[1]) << 64)


def mask_contiguous(length):
    out = (C.c_uint64 * 2)()
    check(lib().sks_mask_contiguous(length, out))
    return int(out[0]) | (int(out[1]) << 64)


def frac_min_hash(kmer, mask, window, nonce=1, flavour=0):
    return int(lib().sks_frac_min_hash(_mask_arr(kmer), _mask_arr(mask), window, nonce, flavour))


def join_layout_log_b(max_sketch_size):
    return int(lib().sks_join_layout_log_b(max_sketch_size))


def join_layout_capacity():
    return int(lib().sks_join_layout_capacity())


def join_layout_region_log(n_blocks, log_b):
    """sks_join_layout_region_log: log2 of the value groups per region a layout
    build of n_blocks blocks takes in this process (SKS_LAYOUT_RG applied)."""
    return int(lib().sks_join_layout_region_log(n_blocks, log_b))


def join_launch_plan(tiles, log_b):
    """sks_join_launch_plan: (workgroups per tile, tiles per launch) of a join
    call of `tiles` tiles in this process (SKS_JOIN_WGS applied)."""
    g, t = C.c_uint32(0), C.c_uint64(0)
    check(lib().sks_join_launch_plan(int(tiles), log_b, C.byref(g), C.byref(t)))
    return int(g.value), int(t.value)


def join_layout_groups(log_b):
    return int(lib().sks_join_layout_groups(log_b))


def join_layout_bounds_for_mask(mask, log_b, elem_words=1):
    """sks_join_layout_bounds_for_mask: the mask-derived group bounds, a uint64 array
    of (join_layout_groups(log_b) + 1) * elem_words words (host)."""
    out = np.zeros((join_layout_groups(log_b) + 1) * elem_words, dtype=np.uint64)
    check(lib().sks_join_layout_bounds_for_mask(_mask_arr(mask), log_b, elem_words, out.ctypes.data))
    return out


def join_layout_boff_words(log_b):
    """u32 words of one block's boff row (2^log_b bucket starts + region ends)."""
    return int(lib().sks_join_layout_boff_words(log_b))


def intersect_sym_tiles(n):
    return int(lib().sks_intersect_sym_tiles(n))


def containment(inter, size):
    return float(lib().sks_containment(inter, size))


def binomial_estimator(c, k):
    return float(lib().sks_binomial_estimator(c, k))


def ani_from_counts(inter, size_first, k):
    inter = np.ascontiguousarray(inter, dtype=np.int32)
    size_first = np.ascontiguousarray(size_first, dtype=np.int32)
    cont = np.zeros(inter.shape, dtype=np.float64)
    ani = np.zeros(inter.shape, dtype=np.float64)
    check(lib().sks_ani_from_counts(inter.ctypes.data, size_first.ctypes.data, inter.size, k,
                                    cont.ctypes.data, ani.ctypes.data))
    return cont, ani


class Fasta:
    """sks_fasta_open: the reference's strings_from_fasta record rules."""

    def __init__(self, path):
        h = C.c_void_p()
        check(lib().sks_fasta_open(os.fsencode(path), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().sks_fasta_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_records(self):
        return int(lib().sks_fasta_num_records(self.h))

    def records(self):
        out = []
        for i in range(self.num_records()):
            p = C.c_void_p()
            n = C.c_uint64()
            check(lib().sks_fasta_record(self.h, i, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value) if n.value else b"")
        return out

    def stream(self):
        n = int(lib().sks_fasta_stream_bytes(self.h))
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        p = lib().sks_fasta_stream(self.h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).copy()

    def runs(self):
        nc, nr = C.c_uint64(0), C.c_uint64(0)
        check(lib().sks_fasta_runs(self.h, None, None, C.byref(nc), C.byref(nr)))
        codes = np.zeros(max(nc.value, 1), dtype=np.uint8)
        lens = np.zeros(max(nr.value, 1), dtype=np.uint64)
        check(lib().sks_fasta_runs(self.h, codes.ctypes.data, lens.ctypes.data, C.byref(nc),
                                   C.byref(nr)))
        codes, lens = codes[:nc.value], lens[:nr.value]
        out, o = [], 0
        for n in lens:
            out.append(codes[o:o + int(n)].tobytes())
            o += int(n)
        return out


class HostBuffer:
    """sks_host_alloc: pinned host memory mapped for the devices (the destination
    of sks_intersect_layout_ani), coherent (fine-grained) or not; .array is a
    numpy view of it."""

    def __init__(self, nbytes, dtype=np.float64, coherent=False):
        p = C.c_void_p()
        check(lib().sks_host_alloc(int(nbytes), 1 if coherent else 0, C.byref(p)))
        self.ptr = int(p.value or 0)
        self.nbytes = int(nbytes)
        n = self.nbytes // np.dtype(dtype).itemsize
        self.array = (np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.nbytes,))
                      .view(dtype)[:n] if self.ptr else np.zeros(0, dtype=dtype))

    def free(self):
        if self.ptr:
            self.array = None
            check(lib().sks_host_free(C.c_void_p(self.ptr)))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- device ---------------------------------------------------------------------------------
class Context:
    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib().sks_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        self.stream = stream or 0  # hipStream_t handle the context's work is queued on (0: null)

    def set_stream(self, stream):
        check(lib().sks_ctx_set_stream(self.h, C.c_void_p(stream) if stream else None))
        self.stream = stream or 0

    def set_scan_grid(self, grid):
        check(lib().sks_ctx_set_scan_grid(self.h, grid))

    def set_frac_post(self, mode=0, bucket_capacity=0, buckets=0):
        """sks_ctx_set_frac_post: FRAC_POST_AUTO / _GENERAL / _FUSED, and (tests)
        a lower bucket capacity and bucket count for the fused path."""
        check(lib().sks_ctx_set_frac_post(self.h, mode, bucket_capacity, buckets))

    def last_build_path(self):
        """BUILD_PATH_* of the context's last sketch_build."""
        return int(lib().sks_ctx_last_build_path(self.h))

    def sketch_union(self, d_in, n, d_out, elem_words=1):
        """sks_sketch_union (elem_words 1: u64 values) or sks_sketch_union_wide
        (elem_words 2: n (lo, hi) pairs): sorted distinct k-mers of d_in into d_out;
        returns the count."""
        k = C.c_uint64(0)
        fn = lib().sks_sketch_union if elem_words == 1 else lib().sks_sketch_union_wide
        check(fn(self.h, C.c_void_p(d_in), n, C.c_void_p(d_out), C.byref(k)))
        return int(k.value)

    def join_layout_build(self, data_ptr, starts_ptr, sizes_ptr, n, log_b, out_vals, out_masks,
                          out_boff, out_bstart, stat=True, total=None, bounds=None, elem_words=1):
        """sks_join_layout_build; returns the largest block-bucket population
        (entries; 2**32 - 1: layout invalid), or None with stat=False (no
        read-back).  total: the sizes' sum when known (with stat=False the call
        then does not wait for the stream at all); bounds: device pointer of the
        group bounds (None: the set's own)."""
        mx = C.c_uint32(0)
        check(lib().sks_join_layout_build(self.h, C.c_void_p(data_ptr), C.c_void_p(starts_ptr),
                                          C.c_void_p(sizes_ptr), elem_words, n,
                                          (1 << 64) - 1 if total is None else int(total), log_b,
                                          C.c_void_p(bounds) if bounds else None,
                                          C.c_void_p(out_vals), C.c_void_p(out_masks), C.c_void_p(out_boff),
                                          C.c_void_p(out_bstart), C.byref(mx) if stat else None))
        return mx.value if stat else None

    def set_layout_blocks_hint(self, blocks):
        """sks_ctx_set_layout_blocks_hint: blocks that hold sketches in the next layout builds (0: all)."""
        check(lib().sks_ctx_set_layout_blocks_hint(self.h, C.c_uint32(int(blocks))))

    def ani_table(self, size, kmer_num_ones):
        """sks_ctx_ani_table: ANI by shared-element count for sets of `size` elements (fused ANI reads it)."""
        check(lib().sks_ctx_ani_table(self.h, C.c_uint32(int(size)), int(kmer_num_ones)))

    def all_pairs_ani(self, data, starts, sizes, n, max_size, total, kmer_num_ones, ani, counts, status,
                      elem_words=1):
        """sks_all_pairs_ani (device pointers; ani: device or pinned host pointer, or 0
        for counts only; counts / status may be 0)."""
        check(lib().sks_all_pairs_ani(self.h, C.c_void_p(data), C.c_void_p(starts), C.c_void_p(sizes), elem_words,
                                      n, max_size, total, kmer_num_ones, C.c_void_p(ani) if ani else None,
                                      C.c_void_p(counts) if counts else None, C.c_void_p(status) if status else None))

    def layout_tiles_ani(self, data, starts, sizes, n, total, log_b, bounds, blocks_hint, blk0, tiles, n_tiles,
                         n_global, sizes_global, kmer_num_ones, ani, counts, status, elem_words=1):
        """sks_layout_tiles_ani (device pointers; ani: device or pinned host pointer,
        or 0 for counts only): layout + join of a global tile list in one call."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        check(lib().sks_layout_tiles_ani(self.h, v(data), v(starts), v(sizes), elem_words, n, total, log_b,
                                         v(bounds), blocks_hint, blk0, v(tiles), n_tiles, n_global,
                                         v(sizes_global), kmer_num_ones, v(ani), v(counts), v(status)))

    def sketches_export(self, data, starts, sizes, n, dst, stride, dst_sizes, elem_words=1):
        """sks_sketches_export (device pointers): sketches padded to a fixed stride."""
        check(lib().sks_sketches_export(self.h, C.c_void_p(data), C.c_void_p(starts), C.c_void_p(sizes), elem_words,
                                        n, C.c_void_p(dst), stride, C.c_void_p(dst_sizes)))

    def join_layout_stat_copy(self, d_dst):
        """sks_join_layout_stat_copy: the last build's (max block bucket, invalid)
        words into the device buffer d_dst (2 x u32), queued on the stream."""
        check(lib().sks_join_layout_stat_copy(self.h, C.c_void_p(d_dst)))

    def join_layout_bounds(self, data_ptr, starts_ptr, sizes_ptr, n, log_b, out_bounds, elem_words=1):
        """sks_join_layout_bounds: the set's group bounds (device pointer out_bounds,
        (join_layout_groups(log_b) + 1) * elem_words words)."""
        check(lib().sks_join_layout_bounds(self.h, C.c_void_p(data_ptr), C.c_void_p(starts_ptr),
                                           C.c_void_p(sizes_ptr), elem_words, n, log_b, C.c_void_p(out_bounds)))

    def intersect_sym_layout(self, n, log_b, vals, masks, boff, bstart, tile_begin, tile_end, out,
                             elem_words=1):
        check(lib().sks_intersect_sym_layout(self.h, n, log_b, elem_words, C.c_void_p(vals), C.c_void_p(masks),
                                             C.c_void_p(boff), C.c_void_p(bstart), tile_begin,
                                             tile_end, C.c_void_p(out)))

    def intersect_layout_tiles(self, n, log_b, vals, masks, boff, bstart, blk0, tiles, tile_begin, tile_end,
                               packed, out, elem_words=1):
        """sks_intersect_layout_tiles: join tiles over a layout whose block 0 is
        global block blk0; counts ADDED to `out` (n x n both halves, or packed
        [tile][64][64]); tiles: device pointer of (I, J) u32 pairs, or 0."""
        check(lib().sks_intersect_layout_tiles(self.h, n, log_b, elem_words, C.c_void_p(vals), C.c_void_p(masks),
                                               C.c_void_p(boff), C.c_void_p(bstart), blk0,
                                               C.c_void_p(tiles) if tiles else None, tile_begin, tile_end,
                                               1 if packed else 0, C.c_void_p(out)))

    def intersect_layout_pair_tiles(self, n, log_b, rows, r_blk0, cols, c_blk0, tiles, tile_begin, tile_end,
                                    packed, out, elem_words=1):
        """sks_intersect_layout_pair_tiles: rows / cols are (vals, masks, boff, bstart)
        device pointers of two layouts; tiles: device pointer of (I, J) u32 pairs."""
        check(lib().sks_intersect_layout_pair_tiles(self.h, n, log_b, elem_words,
                                                    *(C.c_void_p(p) for p in rows), r_blk0,
                                                    *(C.c_void_p(p) for p in cols), c_blk0, C.c_void_p(tiles),
                                                    tile_begin, tile_end, 1 if packed else 0, C.c_void_p(out)))

    def intersect_layout_ani(self, n, log_b, rows, r_blk0, cols, c_blk0, tiles, tile_begin, tile_end, packed,
                             out, sizes, kmer_num_ones, ani, elem_words=1):
        """sks_intersect_layout_ani: intersect_layout_pair_tiles (tiles = 0: the
        upper-triangle range of one layout) plus the ANI of every counted pair,
        written by the join itself into `ani` (n * n float64; a device pointer or
        pinned host memory from HostBuffer); sizes: device int32 |S_i|."""
        check(lib().sks_intersect_layout_ani(self.h, n, log_b, elem_words, *(C.c_void_p(p) for p in rows), r_blk0,
                                             *(C.c_void_p(p) for p in cols), c_blk0,
                                             C.c_void_p(tiles) if tiles else None, tile_begin, tile_end,
                                             1 if packed else 0, C.c_void_p(out), C.c_void_p(sizes),
                                             kmer_num_ones, C.c_void_p(ani)))

    def ani_matrix(self, counts, n, kmer_num_ones, ani, cont=None):
        """sks_ani_matrix (device pointers): ANI of every ordered pair of the n x n counts."""
        check(lib().sks_ani_matrix(self.h, C.c_void_p(counts), n, kmer_num_ones,
                                   C.c_void_p(cont) if cont else None, C.c_void_p(ani)))

    def ani_rows(self, counts, n, row_begin, row_end, kmer_num_ones, ani, cont=None):
        """sks_ani_rows (device pointers): rows [row_begin, row_end) of ani_matrix."""
        check(lib().sks_ani_rows(self.h, C.c_void_p(counts), n, row_begin, row_end, kmer_num_ones,
                                 C.c_void_p(cont) if cont else None, C.c_void_p(ani)))

    def ani_tiles(self, packed, tiles, n_tiles, n, sizes, kmer_num_ones, ani):
        """sks_ani_tiles (device pointers): both orientations of every pair of packed tiles."""
        check(lib().sks_ani_tiles(self.h, C.c_void_p(packed), C.c_void_p(tiles), n_tiles, n, C.c_void_p(sizes),
                                  kmer_num_ones, C.c_void_p(ani)))

    def set_join_check(self, on):
        """sks_ctx_set_join_check: instrumented layout / join kernels (diagnostics)."""
        check(lib().sks_ctx_set_join_check(self.h, 1 if on else 0))

    def join_check_violations(self):
        v = C.c_uint64(0)
        check(lib().sks_ctx_join_check_violations(self.h, C.byref(v)))
        return int(v.value)

    def set_intersect_kernel(self, kind):
        """INTERSECT_AUTO / _MERGE / _JOIN / _GLOBAL (sks.h); all give identical counts."""
        check(lib().sks_ctx_set_intersect_kernel(self.h, kind))
        self._intersect_kernel = kind

    def synchronize(self):
        check(lib().sks_ctx_synchronize(self.h))

    def timings(self):
        t = Timings()
        check(lib().sks_ctx_last_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_}

    def last_intersect_ms(self):
        ms = C.c_float()
        check(lib().sks_ctx_last_intersect_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def last_ingress_ms(self):
        ms = C.c_float()
        check(lib().sks_ctx_last_ingress_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def fasta_parse_device(self, d_raw_ptr, n_raw, d_stream_ptr=None, stream_cap=0,
                           d_rec_end_ptr=None, rec_cap=0):
        """Device strings_from_fasta; returns (stream_bytes, n_records)."""
        nb, nr = C.c_uint64(), C.c_uint64()
        check(lib().sks_fasta_parse_device(self.h, C.c_void_p(d_raw_ptr), n_raw,
                                           C.c_void_p(d_stream_ptr), stream_cap,
                                           C.c_void_p(d_rec_end_ptr), rec_cap, C.byref(nb),
                                           C.byref(nr)))
        return int(nb.value), int(nr.value)

    def close(self):
        if self.h:
            lib().sks_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sketch_build(self, d_seq_ptr, n_bytes, seg_off, window, mask, kind=SKS_FRAC_MOD,
                     param=200, nonce=1, flavour=0):
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
        pol = Policy(kind, flavour, param, nonce)
        h = C.c_void_p()
        check(lib().sks_sketch_build(self.h, C.c_void_p(d_seq_ptr), n_bytes, seg.ctypes.data,
                                     len(seg) - 1, window, _mask_arr(mask), C.byref(pol),
                                     C.byref(h)))
        return SketchSet(h)

    def sketch_build_counted(self, d_seq_ptr, n_bytes, seg_off, window, mask, kind=SKS_FRAC_MOD,
                             param=200, nonce=1, flavour=0, min_abund=1, max_abund=None):
        """sks_sketch_build_counted: sketch_build that also counts how often every
        kept k-mer was selected, keeping those with max(min_abund, 1) <= count <=
        max_abund (None: no limit).  The SketchSet has abundances (SketchSet.abund)."""
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
        pol = Policy(kind, flavour, param, nonce)
        h = C.c_void_p()
        check(lib().sks_sketch_build_counted(self.h, C.c_void_p(d_seq_ptr), n_bytes, seg.ctypes.data,
                                             len(seg) - 1, window, _mask_arr(mask), C.byref(pol),
                                             int(min_abund), ABUND_NO_LIMIT if max_abund is None else int(max_abund),
                                             C.byref(h)))
        return SketchSet(h)

    def abund_trim(self, sketch_set, min_abund=1, max_abund=None):
        """sks_sketch_set_abund_trim: the elements of a counted SketchSet with
        max(min_abund, 1) <= abundance <= max_abund (None: no limit), as a counted set."""
        h = C.c_void_p()
        check(lib().sks_sketch_set_abund_trim(self.h, sketch_set.h, int(min_abund),
                                              ABUND_NO_LIMIT if max_abund is None else int(max_abund), C.byref(h)))
        return SketchSet(h)

    def abund_pairs(self, samples, refs, a, b):
        """sks_abund_pairs: for every pair (a[p], b[p]) of a counted sample sketch and
        a reference sketch, (shared, weight) = (|A n B|, the sum of A's abundances
        over A n B) as int32 and uint64 numpy arrays; an index outside its set
        gives shared -1."""
        import torch
        dev = torch.device("cuda", self.device)
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.ascontiguousarray(b, dtype=np.int32)
        if len(a) != len(b):
            raise ValueError(f"{len(a)} sample indices for {len(b)} reference indices")
        n = len(a)
        d_a = torch.from_numpy(a).to(dev)
        d_b = torch.from_numpy(b).to(dev)
        shared = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        weight = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        check(lib().sks_abund_pairs(self.h, samples.h, refs.h, C.c_void_p(d_a.data_ptr()) if n else None,
                                    C.c_void_p(d_b.data_ptr()) if n else None, n,
                                    C.c_void_p(shared.data_ptr()) if n else None,
                                    C.c_void_p(weight.data_ptr()) if n else None))
        self.synchronize()
        return shared.cpu().numpy()[:n].copy(), weight.cpu().numpy()[:n].view(np.uint64).copy()

    def kmer_list(self, d_seq_ptr, n_bytes, seg_off, window, mask, c=200, nonce=1, flavour=0):
        """nucleotide_string_list_to_kmers on the device: returns (positions,
        bits[n, 4] = kmer_bits lo, hi, masked lo, hi, counts per segment)."""
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
        pol = Policy(SKS_FRAC_MOD, flavour, c, nonce)
        h = C.c_void_p()
        check(lib().sks_kmer_list_build(self.h, C.c_void_p(d_seq_ptr), n_bytes, seg.ctypes.data,
                                        len(seg) - 1, window, _mask_arr(mask), C.byref(pol),
                                        C.byref(h)))
        try:
            n = int(lib().sks_kmer_list_total(h))
            pos = np.zeros(max(n, 1), np.uint64)
            bits = np.zeros(max(4 * n, 1), np.uint64)
            counts = np.zeros(max(len(seg) - 1, 1), np.uint64)
            check(lib().sks_kmer_list_copy(h, pos.ctypes.data, bits.ctypes.data))
            check(lib().sks_kmer_list_counts(h, counts.ctypes.data))
        finally:
            lib().sks_kmer_list_free(h)
        return pos[:n], bits[:4 * n].reshape(n, 4), counts[:len(seg) - 1]

    def windows_dense(self, d_seq_ptr, n_bytes, first, n_windows, window, mask, d_rows, d_valid):
        """sks_windows_dense (device pointers; queued on the context stream): every
        window starting in [first, first + n_windows) of the piece, dense by start."""
        check(lib().sks_windows_dense(self.h, C.c_void_p(d_seq_ptr), C.c_uint64(n_bytes), C.c_uint64(first),
                                      C.c_uint64(n_windows), window, _mask_arr(mask), C.c_void_p(d_rows),
                                      C.c_void_p(d_valid)))

    def load_sketches(self, path):
        h = C.c_void_p()
        check(lib().sks_sketch_set_load(self.h, str(path).encode(), C.byref(h)))
        return SketchSet(h)

    def concat(self, sets):
        arr = (C.c_void_p * len(sets))(*[s.h for s in sets])
        h = C.c_void_p()
        check(lib().sks_sketch_set_concat(self.h, arr, len(sets), C.byref(h)))
        return SketchSet(h)

    def downsample(self, sketch_set, param):
        """sks_sketch_set_downsample: a coarser copy of a SketchSet, equal to a direct
        build at `param` (FracMinHash: a multiple of the set's c; bottom-s: s' <= s)."""
        h = C.c_void_p()
        check(lib().sks_sketch_set_downsample(self.h, sketch_set.h, int(param), C.byref(h)))
        return SketchSet(h)

    def merge(self, sets, groups):
        """sks_sketch_set_merge: one sketch per entry of `groups`, the union of the
        source sketches it lists (indices into the sketches of `sets` in concat
        order: set 0's, then set 1's, ...).  The result has no names."""
        arr = (C.c_void_p * len(sets))(*[s.h for s in sets])
        off = np.zeros(len(groups) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(g) for g in groups], dtype=np.int64)
        mem = np.array([i for g in groups for i in g] + [0], dtype=np.uint32)
        h = C.c_void_p()
        check(lib().sks_sketch_set_merge(self.h, arr, len(sets), off.ctypes.data, mem.ctypes.data, len(groups),
                                         C.byref(h)))
        return SketchSet(h)

    def tally(self, sets, groups, min_count=None, max_count=None, counts=False):
        """sks_sketch_set_tally: one sketch per entry of `groups` (as merge takes
        them), holding the values that min_count .. max_count of the group's listed
        members hold.  min_count / max_count: None (1 / no limit), one integer for
        every group, or one value per group; TALLY_NO_LIMIT as a max is no limit.
        counts=True: returns (set, counts), counts a host u32 array in the set's
        flat order (entry starts[g] + j: the members holding element j of sketch g)."""
        arr = (C.c_void_p * len(sets))(*[s.h for s in sets])
        off = np.zeros(len(groups) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(g) for g in groups], dtype=np.int64)
        mem = np.array([i for g in groups for i in g] + [0], dtype=np.uint32)

        def per_group(v, what):
            if v is None:
                return None
            a = np.full(len(groups), v, dtype=np.uint32) if np.isscalar(v) else np.array(list(v), dtype=np.uint32)
            if len(a) != len(groups):
                raise ValueError(f"{what} has {len(a)} entries for {len(groups)} groups")
            return np.append(a, np.uint32(0))  # never empty

        lo, hi = per_group(min_count, "min_count"), per_group(max_count, "max_count")
        buf, cap = None, 0
        if counts:
            import torch
            src = np.concatenate([s.sizes() for s in sets]) if sets else np.zeros(0, np.uint32)
            cap = int(sum(int(src[i]) for g in groups for i in g if i < len(src)))  # always suffices
            buf = torch.zeros(max(cap, 1), dtype=torch.int32, device=torch.device("cuda", self.device))
        h = C.c_void_p()
        check(lib().sks_sketch_set_tally(self.h, arr, len(sets), off.ctypes.data, mem.ctypes.data, len(groups),
                                         None if lo is None else lo.ctypes.data,
                                         None if hi is None else hi.ctypes.data, C.byref(h),
                                         None if buf is None else C.c_void_p(buf.data_ptr()), cap))
        out = SketchSet(h)
        if not counts:
            return out
        self.synchronize()
        total = int(out.sizes().sum()) if out.n else 0
        return out, buf.cpu().numpy().view(np.uint32)[:total].copy()

    def core(self, sets, groups, min_fraction):
        """The k-mers held by at least min_fraction of each group's listed members:
        tally with min_count = max(1, ceil(min_fraction * members)), the fraction
        taken as the decimal it prints as (0.9 of 10 is 9)."""
        from fractions import Fraction
        f = Fraction(str(min_fraction))
        if not 0 <= f <= 1:
            raise ValueError(f"min_fraction {min_fraction} is not within 0 .. 1")
        return self.tally(sets, groups, min_count=[max(1, math.ceil(f * len(g))) for g in groups])

    def filter(self, sketch_set, filters, kind, filter_of=None):
        """sks_sketch_set_filter: sketch i of the result holds the elements of sketch i
        of `sketch_set` absent from (SKS_FILTER_SUBTRACT) or present in
        (SKS_FILTER_INTERSECT) sketch filter_of[i] of `filters`; FILTER_NONE copies
        sketch i.  filter_of None: every sketch against the one sketch of `filters`."""
        fo = None if filter_of is None else np.ascontiguousarray(list(filter_of) + [0], dtype=np.uint32)
        if fo is not None and len(fo) - 1 != sketch_set.n:
            raise ValueError(f"filter_of has {len(fo) - 1} entries for {sketch_set.n} sketches")
        h = C.c_void_p()
        check(lib().sks_sketch_set_filter(self.h, sketch_set.h, filters.h, None if fo is None else fo.ctypes.data,
                                          int(kind), C.byref(h)))
        return SketchSet(h)

    def subtract(self, sketch_set, filters, filter_of=None):
        return self.filter(sketch_set, filters, SKS_FILTER_SUBTRACT, filter_of)

    def intersect(self, sketch_set, filters, filter_of=None):
        return self.filter(sketch_set, filters, SKS_FILTER_INTERSECT, filter_of)

    def intersect_pairs(self, data_ptr, starts_ptr, sizes_ptr, elem_words, a_ptr, b_ptr,
                        n_pairs, out_ptr):
        check(lib().sks_intersect_pairs(self.h, data_ptr, starts_ptr, sizes_ptr, elem_words,
                                        a_ptr, b_ptr, n_pairs, out_ptr))

    def intersect_all(self, data_ptr, starts_ptr, sizes_ptr, elem_words, n, row_begin, row_end,
                      out_ptr):
        check(lib().sks_intersect_all(self.h, data_ptr, starts_ptr, sizes_ptr, elem_words, n,
                                      row_begin, row_end, out_ptr))

    def intersect_sym(self, data_ptr, starts_ptr, sizes_ptr, elem_words, n, tile_begin, tile_end,
                      out_ptr):
        check(lib().sks_intersect_sym(self.h, data_ptr, starts_ptr, sizes_ptr, elem_words, n,
                                      tile_begin, tile_end, out_ptr))

    def set_search_batch(self, ref_blocks):
        """sks_ctx_set_search_batch: 64-sketch reference blocks per batch of search (0: the engine's choice)."""
        check(lib().sks_ctx_set_search_batch(self.h, C.c_uint32(int(ref_blocks))))

    def search_sets_raw(self, queries, refs, min_containment, min_shared, d_hits, hit_cap):
        """sks_search_sets with a caller buffer (device pointer or 0 for a size
        query); returns (status code, exact hit count) without raising on
        SKS_E_LENGTH, so a caller can see the count a short buffer still reports."""
        n = C.c_uint64(0)
        rc = lib().sks_search_sets(self.h, queries.h, refs.h, float(min_containment), int(min_shared),
                                   C.c_void_p(d_hits) if d_hits else None, int(hit_cap), C.byref(n))
        if rc not in (SKS_OK, SKS_E_LENGTH):
            check(rc)
        return rc, int(n.value)

    def search_arrays(self, q, r, elem_words, kmer_num_ones, min_containment=0.0, min_shared=1):
        """sks_search, the device-array form: q and r are (data, starts, sizes, n,
        max_size, total) with device pointers (0 allowed when n is 0).  A size
        query, then a fill; returns a HIT_DTYPE array in (query, ref) order."""
        import torch
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731

        def call(d_hits, cap, n):
            check(lib().sks_search(self.h, v(q[0]), v(q[1]), v(q[2]), int(q[3]), int(q[4]), int(q[5]),
                                   v(r[0]), v(r[1]), v(r[2]), int(r[3]), int(r[4]), int(r[5]), elem_words,
                                   kmer_num_ones, float(min_containment), int(min_shared), v(d_hits), cap,
                                   C.byref(n)))
        n = C.c_uint64(0)
        call(0, 0, n)
        if n.value == 0:
            return np.zeros(0, dtype=HIT_DTYPE)
        cap = int(n.value)
        buf = torch.empty(cap * HIT_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        call(buf.data_ptr(), cap, n)
        self.synchronize()
        return buf.cpu().numpy().view(HIT_DTYPE)[:int(n.value)].copy()

    def search(self, queries, refs, min_containment=0.0, min_shared=1):
        """sks_search_sets: the (query, ref) pairs of two SketchSets sharing at least
        max(min_shared, 1) k-mers with containment(shared, |query|) >=
        min_containment, as a HIT_DTYPE array in (query, ref) order.  A size
        query, then a fill of a device buffer of exactly that many records."""
        import torch
        n = C.c_uint64(0)
        check(lib().sks_search_sets(self.h, queries.h, refs.h, float(min_containment), int(min_shared), None, 0,
                                    C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=HIT_DTYPE)
        cap = int(n.value)
        buf = torch.empty(cap * HIT_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        check(lib().sks_search_sets(self.h, queries.h, refs.h, float(min_containment), int(min_shared),
                                    C.c_void_p(buf.data_ptr()), cap, C.byref(n)))
        self.synchronize()
        return buf.cpu().numpy().view(HIT_DTYPE)[:int(n.value)].copy()

    def search_topk_sets_raw(self, queries, refs, rank, k, min_score, min_shared, skip_same_index, d_hits, d_counts):
        """sks_search_topk_sets with caller buffers (device pointers, 0 for NULL;
        either set may be None); returns the status code without raising."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        return lib().sks_search_topk_sets(self.h, queries.h if queries is not None else None,
                                          refs.h if refs is not None else None, int(rank), int(k), float(min_score),
                                          int(min_shared), int(bool(skip_same_index)), v(d_hits), v(d_counts))

    def search_topk_arrays_raw(self, q, r, elem_words, kmer_num_ones, rank, k, min_score, min_shared,
                               skip_same_index, d_hits, d_counts):
        """sks_search_topk with caller buffers: q and r as search_arrays takes its
        sides.  Returns the status code without raising."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        return lib().sks_search_topk(self.h, v(q[0]), v(q[1]), v(q[2]), int(q[3]), int(q[4]), int(q[5]),
                                     v(r[0]), v(r[1]), v(r[2]), int(r[3]), int(r[4]), int(r[5]), int(elem_words),
                                     int(kmer_num_ones), int(rank), int(k), float(min_score), int(min_shared),
                                     int(bool(skip_same_index)), v(d_hits), v(d_counts))

    def _search_topk(self, q_n, k, call):
        import torch
        dev = torch.device("cuda", self.device)
        slots = int(q_n) * max(int(k), 0)
        buf = torch.empty(max(slots, 1) * TOP_HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        cnt = torch.empty(max(int(q_n), 1), dtype=torch.int32, device=dev)
        check(call(buf.data_ptr(), cnt.data_ptr()))
        self.synchronize()
        hits = buf.cpu().numpy().view(TOP_HIT_DTYPE)[:slots].copy().reshape(int(q_n), int(k))
        return hits, cnt.cpu().numpy().view(np.uint32)[:int(q_n)].copy()

    def search_topk(self, queries, refs, k, rank=SKS_RANK_QUERY, min_score=0.0, min_shared=1, skip_same_index=False):
        """sks_search_topk_sets: for every sketch of `queries` its k best sketches
        of `refs`, best first, by containment of the shared k-mers in the query
        (SKS_RANK_QUERY), in the reference (SKS_RANK_REF) or in the smaller of the
        two (SKS_RANK_MAX); ties go to the larger shared, then the smaller ref.
        Listed are references sharing at least max(min_shared, 1) k-mers with
        score >= min_score, and with skip_same_index not the query's own index.
        Returns (hits TOP_HIT_DTYPE[q_n, k], counts u32[q_n]): row q holds
        counts[q] records, then empty slots (ref 0xffffffff)."""
        return self._search_topk(queries.n, k, lambda d, n: self.search_topk_sets_raw(
            queries, refs, rank, k, min_score, min_shared, skip_same_index, d, n))

    def search_topk_arrays(self, q, r, elem_words, kmer_num_ones, k, rank=SKS_RANK_QUERY, min_score=0.0,
                           min_shared=1, skip_same_index=False):
        """sks_search_topk, the device-array form: q and r are (data, starts, sizes,
        n, max_size, total) with device pointers, as search_arrays takes them."""
        return self._search_topk(int(q[3]), k, lambda d, n: self.search_topk_arrays_raw(
            q, r, elem_words, kmer_num_ones, rank, k, min_score, min_shared, skip_same_index, d, n))

    def cluster_set_raw(self, sketch_set, min_containment, min_shared, d_cluster, d_rep):
        """sks_cluster_set with caller buffers (device pointers, 0 for NULL; the set
        may be None); returns (status code, number of clusters) without raising."""
        n = C.c_uint32(0xffffffff)
        rc = lib().sks_cluster_set(self.h, sketch_set.h if sketch_set is not None else None, float(min_containment),
                                   int(min_shared), C.c_void_p(d_cluster) if d_cluster else None,
                                   C.c_void_p(d_rep) if d_rep else None, C.byref(n))
        return rc, int(n.value)

    def cluster_arrays_raw(self, side, elem_words, kmer_num_ones, min_containment, min_shared, d_cluster, d_rep):
        """sks_cluster with caller buffers; `side` as search_arrays takes it.
        Returns (status code, number of clusters) without raising."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        n = C.c_uint32(0xffffffff)
        rc = lib().sks_cluster(self.h, v(side[0]), v(side[1]), v(side[2]), int(side[3]), int(side[4]), int(side[5]),
                               int(elem_words), int(kmer_num_ones), float(min_containment), int(min_shared),
                               v(d_cluster), v(d_rep), C.byref(n))
        return rc, int(n.value)

    def _cluster(self, n, call):
        import torch
        dev = torch.device("cuda", self.device)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        reps = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        rc, c = call(labels.data_ptr(), reps.data_ptr())
        check(rc)
        self.synchronize()
        return (labels.cpu().numpy().view(np.uint32)[:n].copy(), reps.cpu().numpy().view(np.uint32)[:c].copy())

    def cluster(self, sketch_set, min_containment=0.0, min_shared=1):
        """sks_cluster_set: single-linkage clusters of a SketchSet.  Two sketches are
        linked iff they share at least max(min_shared, 1) k-mers and the larger of
        their two containments is >= min_containment.  Returns (labels u32[n],
        reps u32[C]): clusters numbered by ascending smallest member, each
        cluster's representative its largest sketch (ties: the smallest index)."""
        return self._cluster(sketch_set.n, lambda lab, rep: self.cluster_set_raw(sketch_set, min_containment,
                                                                                 min_shared, lab, rep))

    def cluster_arrays(self, side, elem_words, kmer_num_ones, min_containment=0.0, min_shared=1):
        """sks_cluster, the device-array form: side is (data, starts, sizes, n,
        max_size, total) with device pointers, as search_arrays takes a side."""
        return self._cluster(int(side[3]), lambda lab, rep: self.cluster_arrays_raw(
            side, elem_words, kmer_num_ones, min_containment, min_shared, lab, rep))

    def set_gather_rounds(self, rounds_per_wait):
        """sks_ctx_set_gather_rounds: rounds of gather queued per host wait (0: the engine's choice)."""
        check(lib().sks_ctx_set_gather_rounds(self.h, C.c_uint32(int(rounds_per_wait))))

    def gather_sets_raw(self, queries, q, refs, min_shared, max_rounds, d_hits, hit_cap, want_unexplained=True):
        """sks_gather_sets with a caller buffer (device pointer, 0 for a size query;
        either set may be None); returns (status code, exact number of hits,
        n_unexplained or None when want_unexplained is False) without raising."""
        n = C.c_uint64(0xffffffff)
        un = C.c_uint32(0)
        rc = lib().sks_gather_sets(self.h, queries.h if queries is not None else None, int(q),
                                   refs.h if refs is not None else None, int(min_shared), int(max_rounds),
                                   C.c_void_p(d_hits) if d_hits else None, int(hit_cap), C.byref(n),
                                   C.byref(un) if want_unexplained else None)
        return rc, int(n.value), (int(un.value) if want_unexplained else None)

    def gather_arrays_raw(self, query, refs, elem_words, kmer_num_ones, min_shared, max_rounds, d_hits, hit_cap,
                          want_unexplained=True):
        """sks_gather with caller buffers: query is (device pointer, q_size), refs
        (data, starts, sizes, n, max_size, total) as search_arrays takes a side.
        Returns (status code, number of hits, n_unexplained or None) without raising."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        n = C.c_uint64(0xffffffff)
        un = C.c_uint32(0)
        rc = lib().sks_gather(self.h, v(query[0]), int(query[1]), v(refs[0]), v(refs[1]), v(refs[2]), int(refs[3]),
                              int(refs[4]), int(refs[5]), int(elem_words), int(kmer_num_ones), int(min_shared),
                              int(max_rounds), v(d_hits), int(hit_cap), C.byref(n),
                              C.byref(un) if want_unexplained else None)
        return rc, int(n.value), (int(un.value) if want_unexplained else None)

    def _gather(self, cap, call):
        import torch
        cap = max(int(cap), 1)  # min(r_n, q_size) records always suffice
        buf = torch.empty(cap * GATHER_HIT_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        rc, n, un = call(buf.data_ptr(), cap)
        check(rc)
        self.synchronize()
        return buf.cpu().numpy().view(GATHER_HIT_DTYPE)[:n].copy(), un

    def gather(self, queries, q, refs, min_shared=1, max_rounds=0):
        """sks_gather_sets: the greedy min-set cover of sketch q of `queries` by the
        sketches of `refs`.  Each round reports the reference sharing the most
        still unexplained query elements (ties: the smallest index), at least
        max(min_shared, 1) of them, and removes its elements from the query;
        max_rounds 0 is no limit.  Returns (GATHER_HIT_DTYPE array in round
        order, n_unexplained)."""
        q_size = int(queries.sizes()[q]) if 0 <= q < queries.n else 0
        return self._gather(min(refs.n, q_size), lambda d, cap: self.gather_sets_raw(
            queries, q, refs, min_shared, max_rounds, d, cap))

    def gather_arrays(self, query, refs, elem_words, kmer_num_ones, min_shared=1, max_rounds=0):
        """sks_gather, the device-array form: query is (device pointer, q_size), refs
        (data, starts, sizes, n, max_size, total) with device pointers."""
        return self._gather(min(int(refs[3]), int(query[1])), lambda d, cap: self.gather_arrays_raw(
            query, refs, elem_words, kmer_num_ones, min_shared, max_rounds, d, cap))

    def synth_bases(self, d_out_ptr, n, seed, mut_seed=0, mut_rate=0.0, pos_offset=0):
        check(lib().sks_synth_bases(self.h, C.c_void_p(d_out_ptr), n, seed, mut_seed, mut_rate,
                                    pos_offset))


class _DeviceArray:
    """A device buffer described by __cuda_array_interface__ (torch.as_tensor
    wraps it without a copy)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 3, "strides": None}


class SketchSet:
    def __init__(self, h):
        self.h = h
        self.n = int(lib().sks_sketch_set_num(h))
        self.elem_words = int(lib().sks_sketch_set_elem_words(h))

    def free(self, stream=None):
        """sks_sketch_set_free, or with `stream` (a hipStream_t handle, e.g.
        torch.cuda.Stream().cuda_stream) sks_sketch_set_free_on_stream: no
        device-wide wait; every use of the set must be ordered on that stream."""
        if self.h:
            if stream is None:
                lib().sks_sketch_set_free(self.h)
            else:
                lib().sks_sketch_set_free_on_stream(self.h, C.c_void_p(stream))
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def info(self):
        i = SketchInfo()
        check(lib().sks_sketch_set_info(self.h, C.byref(i)))
        return {"window": i.window, "elem_words": i.elem_words,
                "mask": int(i.mask[0]) | int(i.mask[1]) << 64, "kind": i.policy.kind,
                "flavour": i.policy.flavour, "param": i.policy.param, "nonce": i.policy.nonce,
                "n": i.n, "has_names": bool(i.has_names)}

    def set_names(self, names):
        if names is None:
            check(lib().sks_sketch_set_set_names(self.h, None))
            return
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        check(lib().sks_sketch_set_set_names(self.h, arr))

    def names(self):
        out = []
        for i in range(self.n):
            v = lib().sks_sketch_set_name(self.h, i)
            if v is None:
                return None
            out.append(v.decode())
        return out

    def save(self, path):
        check(lib().sks_sketch_set_save(self.h, str(path).encode()))

    def sizes(self):
        out = np.zeros(max(self.n, 1), dtype=np.uint32)
        check(lib().sks_sketch_set_sizes(self.h, out.ctypes.data))
        return out[:self.n]

    def windows(self):
        out = np.zeros(max(self.n, 1), dtype=np.uint64)
        check(lib().sks_sketch_set_windows(self.h, out.ctypes.data))
        return out[:self.n]

    def starts(self):
        out = np.zeros(max(self.n, 1), dtype=np.uint64)
        check(lib().sks_sketch_set_starts(self.h, out.ctypes.data))
        return out[:self.n]

    def sketch(self, i):
        """Sketch i as a uint64 array of shape (size, 2) = (lo, hi)."""
        n = int(self.sizes()[i])
        buf = np.zeros(max(n * self.elem_words, 1), dtype=np.uint64)
        check(lib().sks_sketch_set_copy(self.h, i, buf.ctypes.data))
        buf = buf[:n * self.elem_words]
        if self.elem_words == 1:
            return np.stack([buf, np.zeros_like(buf)], axis=1)
        return buf.reshape(-1, 2)

    def has_abund(self):
        """Whether the set carries an abundance per element (a counted set)."""
        return int(lib().sks_sketch_set_has_abund(self.h))

    def abund(self, i):
        """The abundances of sketch i's elements, a uint32 array in the elements' order."""
        n = int(self.sizes()[i])
        buf = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().sks_sketch_set_abund_copy(self.h, i, buf.ctypes.data))
        return buf[:n]

    def abund_totals(self):
        """The sum of every sketch's abundances, a uint64 array of n entries."""
        out = np.zeros(max(self.n, 1), dtype=np.uint64)
        check(lib().sks_sketch_set_abund_totals(self.h, out.ctypes.data))
        return out[:self.n]

    def copy_into(self, i, host_ptr):
        """Sketch i (size * elem_words u64) into caller memory (e.g. pinned); returns size."""
        check(lib().sks_sketch_set_copy(self.h, i, C.c_void_p(host_ptr)))
        return int(self.sizes()[i])

    def device_ptrs(self):
        L = lib()
        return (L.sks_sketch_set_device_data(self.h), L.sks_sketch_set_device_starts(self.h),
                L.sks_sketch_set_device_sizes(self.h))

    def device_tensors(self, device=0):
        """Zero-copy torch views of the set's device arrays: (data int64
        [total * elem_words], starts int64 [n], sizes int32 [n]).  The views do
        not keep the set alive: use them while the set is."""
        import torch
        d, st, sz = self.device_ptrs()
        total = int(self.sizes().astype(np.int64).sum()) * self.elem_words
        dev = torch.device("cuda", device)

        def view(ptr, n, typestr, dtype):
            if n == 0 or not ptr:
                return torch.zeros(0, dtype=dtype, device=dev)
            return torch.as_tensor(_DeviceArray(ptr, n, typestr), device=dev)
        return view(d, total, "<i8", torch.int64), view(st, self.n, "<i8", torch.int64), \
            view(sz, self.n, "<i4", torch.int32)

    def export(self, d_dst_ptr, stride, d_sizes_ptr):
        check(lib().sks_sketch_set_export(self.h, C.c_void_p(d_dst_ptr), stride,
                                          C.c_void_p(d_sizes_ptr)))


def build_info():
    """'src:<hash>' of the sources libsks.so was linked from (srchash.py)."""
    return lib().sks_build_info().decode()
