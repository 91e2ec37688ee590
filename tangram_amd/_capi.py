"""ctypes binding of libtangram_hip.so (C ABI declared in include/tangram_hip.h).

The product path loads the in-tree HIP library built by `__graft_entry__.build()` /
`tangram_amd._build.build()` and fails loudly when it is missing: there is no CPU fallback.
(The CPU test-suite installs an *emulated* build of the same sources through
`_install_library_for_tests`; nothing else calls that hook.)
"""
from __future__ import annotations

import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libtangram_hip.so")      # the in-tree build, nothing else (experiments: scripts/with_lib.py)

TG_ABI_VERSION = 6
TG_MODE_MAPPER, TG_MODE_CONSTRAINED = 0, 1
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2}
H_NTERMS = 16
TOPK_MAX = 64          # TG_TOPK_MAX / TG_TOPK_CHUNK of csrc/tg_topk.h (checked against tg_debug_topk_limits by the tests)
TOPK_CHUNK = 8192
SPOT_TOPK_MAX = 32     # TG_SPOT_TOPK_MAX of csrc/tg_spot_topk.h: the largest k of result_spot_topk (these three are checked against
SPOT_TOPK_STRIP = 256  # TG_SPOT_STRIP: spots per workgroup                                          tg_debug_spot_topk_limits by the tests)
SPOT_TOPK_MIN_SLAB_ROWS = 8   # TG_SPOT_UNROLL: rows loaded ahead = the smallest slab_rows a caller may force
CONSIST_MAX_RUNS = 8  # TG_CONSIST_MAX_RUNS of csrc/tg_consist.h
H_TOTAL, H_MAIN, H_VG, H_KL, H_ENTROPY, H_L1, H_L2, H_NB, H_CT, H_COUNT, H_FREG, H_GETIS, H_MORAN, H_GEARY = range(14)


class TgConfig(ct.Structure):
    _fields_ = [(n, ct.c_int32) for n in
                ("abi_version", "mode", "precision", "n_cells", "n_genes", "n_spots", "n_spots_total",
                 "has_density", "has_d_source", "fwd_splits", "tile_size", "pipeline_bands")] + \
               [(n, ct.c_float) for n in
                ("lambda_g1", "lambda_d", "lambda_g2", "lambda_r", "lambda_l1", "lambda_l2",
                 "lambda_count", "lambda_f_reg", "target_count", "lambda_neighborhood_g1", "lambda_ct_islands")] + \
               [(n, ct.c_int32) for n in ("n_cell_types", "nnz_w", "nnz_n")] + \
               [(n, ct.c_float) for n in ("lambda_getis_ord", "lambda_moran", "lambda_geary")] + [("nnz_s", ct.c_int32)] + \
               [(n, ct.c_float) for n in ("beta1", "beta2", "eps")] + \
               [(n, ct.c_int32) for n in ("n_ranks", "bwd_tile", "spot_offset", "s_exact_mode")]


ALL_REDUCE_FN = ct.CFUNCTYPE(ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p)                 # tg_all_reduce_sum_fn
ALL_GATHER_FN = ct.CFUNCTYPE(ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p)    # tg_all_gather_fn


class TgSizes(ct.Structure):
    _fields_ = [("state_bytes", ct.c_size_t), ("workspace_bytes", ct.c_size_t),
                ("m_pitch", ct.c_int32), ("history_terms", ct.c_int32), ("peer_step_floats", ct.c_size_t)]


class TgInputs(ct.Structure):
    _fields_ = [(n, ct.c_void_p) for n in ("S_dev", "G_dev", "d_dev", "d_source_dev", "M0_dev", "F0_dev", "ct_encode_dev",
                                           "w_indptr", "w_indices", "w_data", "wt_indptr", "wt_indices", "wt_data",
                                           "n_indptr", "n_indices", "n_data", "nt_indptr", "nt_indices", "nt_data",
                                           "s_indptr", "s_indices", "s_data", "st_indptr", "st_indices", "st_data")]


_lib = None
_is_sim = False


def _signatures():
    """Every entry point of include/tangram_hip.h that this package calls: name -> (restype, argtypes).  The one list of names."""
    vp, i32, i64, f32, sz, P = ct.c_void_p, ct.c_int32, ct.c_int64, ct.c_float, ct.c_size_t, ct.POINTER
    planes = [P(vp), i32, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    return {
        "tg_abi_version": (i32, []),
        "tg_last_error": (ct.c_char_p, []),
        "tg_query_sizes": (i32, [P(TgConfig), P(TgSizes)]),
        "tg_mapper_create": (i32, [P(TgConfig), P(TgInputs), vp, vp, vp, P(vp)]),
        "tg_mapper_destroy": (None, [vp]),
        "tg_mapper_step": (i32, [vp, i32, f32, vp, i32]),
        "tg_comm_create_callbacks": (i32, [i32, i32, ALL_REDUCE_FN, ALL_GATHER_FN, vp, P(vp)]),
        "tg_comm_rccl_unique_id": (i32, [ct.c_char_p, vp]),
        "tg_comm_create_rccl": (i32, [ct.c_char_p, vp, i32, i32, P(vp)]),
        "tg_comm_peer_create": (i32, [i32, i32, sz, i32, vp, P(vp)]),
        "tg_comm_peer_create_stepped": (i32, [i32, i32, sz, sz, i32, i32, vp, P(vp)]),
        "tg_comm_peer_connect": (i32, [vp, vp]),
        "tg_comm_peer_status": (i32, [vp, P(i32)]),
        "tg_comm_peer_set_timeout_ms": (i32, [vp, ct.c_double]),
        "tg_comm_all_reduce_sum": (i32, [vp, vp, sz, vp]),
        "tg_comm_all_gather": (i32, [vp, vp, vp, sz, vp]),
        "tg_comm_destroy": (None, [vp]),
        "tg_mapper_attach_comm": (i32, [vp, vp]),
        "tg_mapper_result": (i32, [vp, vp, vp]),
        "tg_mapper_result_topk": (i32, [vp, i32, vp, vp]),
        "tg_topk_merge": (i32, [vp, vp, i64, i32, i64, i32, vp, vp, vp]),
        "tg_mapper_spot_topk_query_bytes": (i32, [vp, i32, i32, P(sz)]),
        "tg_mapper_result_spot_topk": (i32, [vp, i32, f32, i32, vp, vp, vp, vp]),
        "tg_debug_spot_topk_limits": (i32, [i32, i32, P(i32)]),
        "tg_mapper_project": (i32, [vp, vp]),
        "tg_mapper_project_genes": (i32, [vp, vp, i64, i32, vp, i64, i32]),
        "tg_csr_columns_to_dense": (i32, [vp, vp, vp, i64, i32, i32, vp, i64, vp]),
        "tg_sparse_map_query_bytes": (i32, [i64, i64, i64, P(sz)]),
        "tg_sparse_map_build": (i32, [vp, vp, vp, i64, i64, i64, vp, vp]),
        "tg_sparse_map_project": (i32, [vp, i64, i64, i64, vp, i64, i32, vp, i64, vp]),
        "tg_debug_sparse_map_layout": (i32, [i64, i64, P(i64)]),
        "tg_consistency_query_bytes": (i32, [i32, i64, P(sz)]),
        "tg_mapper_consistency": (i32, [P(vp), i32, vp, vp, vp, vp, vp]),
        "tg_planes_consistency": (i32, planes),
        "tg_debug_planes_consistency": (i32, planes + [i32]),
        "tg_consistency_packet_bytes": (i32, [i32, i64, P(sz)]),
        "tg_mapper_consistency_shard": (i32, [P(vp), i32, vp, vp]),
        "tg_planes_consistency_shard": (i32, [P(vp), i32, i64, i64, i64, i64, i64, i32, vp, vp, vp]),
        "tg_consistency_merge": (i32, [vp, i32, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp]),
        "tg_gene_scores_query_bytes": (i32, [i64, i32, P(sz)]),
        "tg_gene_scores": (i32, [vp, i64, vp, i64, i64, i32, vp, vp, vp, vp]),
        "tg_gene_scores_merge": (i32, [vp, i32, i32, vp, vp, vp]),
        "tg_batch_query_bytes": (sz, [i32]),
        "tg_batch_create": (i32, [P(vp), i32, vp, P(vp)]),
        "tg_batch_step": (i32, [vp, i32, f32, P(vp), i32]),
        "tg_batch_destroy": (None, [vp]),
        "tg_csr_gather_columns": (i32, [vp, vp, vp, i64, vp, i32, vp, i64, vp]),
        "tg_row_sums": (i32, [vp, i64, i32, vp, vp, i64, vp, i32, vp]),
        "tg_cluster_aggregate": (i32, [vp, i64, i32, vp, vp, i32, i32, vp, i64, vp]),
        "tg_init_logits_normal": (i32, [vp, i64, i64, i64, ct.c_uint64, i64, i64, vp]),
        "tg_mapper_state": (i32, [vp, P(vp), P(vp), P(vp), P(i32), P(i64)]),
        "tg_mapper_set_step": (i32, [vp, i64]),
        "tg_mapper_effective_precision": (i32, [vp]),
        "tg_mapper_filter_state": (i32, [vp, P(vp), P(i32)]),
        "tg_mapper_validate": (i32, [vp, vp]),
        "tg_mapper_profile": (i32, [vp, i32]),
        "tg_mapper_profile_read": (i32, [vp, ct.c_char_p, sz, P(f32), P(i32), i32, P(i32)]),
    }


SIGNATURES = _signatures()
EXPORTS = [name for name in SIGNATURES if not name.startswith("tg_debug_")]     # what include/tangram_hip.h declares


def _declare(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def lib():
    """The loaded HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). tangram_amd has no CPU fallback.")
        _lib = _declare(ct.CDLL(LIB_PATH))
        if _lib.tg_abi_version() != TG_ABI_VERSION:
            raise RuntimeError("libtangram_hip.so ABI version mismatch (rebuild: python -c 'import __graft_entry__ as g; g.build()')")
    return _lib


def is_emulated():
    return _is_sim


def _install_library_for_tests(path):
    """TEST HOOK: use an emulated (TG_SIM) build of the same C ABI; `None` restores the HIP library."""
    global _lib, _is_sim
    if path is None:
        _lib, _is_sim = None, False
    else:
        _lib, _is_sim = _declare(ct.CDLL(path)), True


class TangramHipError(RuntimeError):
    pass


def check(rc):
    if rc == 0:
        return
    msg = lib().tg_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    raise TangramHipError(f"libtangram_hip error {rc}: {msg}")
