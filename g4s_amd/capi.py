"""ctypes binding of libg4s_hip.so (the C-ABI declared in include/g4s.h and include/g4s_synth.h).

The library is the product; this module only loads it and declares argument types. It fails loudly when the
shared object is missing — there is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G4S_LIB") or os.path.join(_HERE, "lib", "libg4s_hip.so")   # G4S_LIB: the host-sanitized build (tools/run_sanitized_cpu_tests.sh)

OK, ERR_INVALID, ERR_NOMEM, ERR_HIP, ERR_OVERFLOW, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
HOST_POINTERS, DEVICE_POINTERS, SORT_OUTPUT, SPMV_NO_NT, SPMV_BLOCKED, SPMV_STREAM, DIST_LOOPBACK, DIST_ALLGATHER, SPMV_UPDATABLE = 0, 1, 2, 4, 8, 16, 32, 64, 128
SPMM_COL_MAJOR = 256
SPMV_ACCUMULATE = 2048                                                   # semiring SpMV: y := y ⊕ (A ⊗ x) (g4s.h)
TRAVERSE_PUSH, TRAVERSE_PULL, TRAVERSE_SYMMETRIC, TRAVERSE_BATCH = 4096, 8192, 16384, 16   # g4s_sssp / g4s_bfs (g4s.h)
PAGERANK_SYMMETRIC, PAGERANK_WARM_START, PAGERANK_BATCH = 65536, 131072, 8                 # g4s_pagerank (g4s.h)
BC_ACCUMULATE, BC_BATCH = 262144, 16                                     # g4s_betweenness (g4s.h)
CC_SYMMETRIC = 32768                                                     # g4s_connected_components: the pattern is declared symmetric (g4s.h)
KCORE_BATCH, KCORE_FULL = 16, 2**31 - 1                                  # g4s_kcore: launches per state read at least; max_k of the full decomposition (g4s.h)
SCC_BATCH = 16                                                           # g4s_strongly_connected_components: launches per state read at least (g4s.h)
MSF_MAXIMUM, MSF_BATCH = 1048576, 16                                     # g4s_minimum_spanning_forest: the maximum forest; launches per state read at least (g4s.h)
KTRUSS_BATCH, KTRUSS_FULL = 16, 2**31 - 1                                # g4s_ktruss: launches per state read at least; max_k of the full decomposition (g4s.h)
COLOR_LARGEST_FIRST, COLOR_BATCH, COLOR_MASK_COLORS, COLOR_WINDOW = 524288, 16, 64, 256   # g4s_color: key := degree; launches per state read; mask width; scan window (g4s.h)
TRSV_UPPER, TRSV_UNIT_DIAGONAL, TRSV_NO_CHAINS = 2097152, 4194304, 8388608   # g4s_sptrsv_analyse: the triangle, the diagonal, one launch per level (g4s.h)
TRSV_WAVE_ROW, TRSV_CHAIN_WIDTH, TRSV_CHAIN_LEVELS, TRSV_HUB_ROW = 32, 256, 1024, 4096   # g4s_sptrsv: the row classes of the documented sum and the chaining rule (g4s.h)
TRSV_COL_MAJOR, TRSV_RHS_TILE, TRSV_MAX_RHS = 33554432, 8, 32768          # g4s_sptrsv_solve_multi / g4s_ilu0_apply_multi: the layout flag, the column tile, the cap on k (g4s.h)
ILU0_NO_CHAINS, ILU0_LANE_ROW, ILU0_WAVE_ROW = 16777216, 8, 512            # g4s_ilu0_analyse: one launch per level; the row classes of the factorisation (g4s.h)
EWISE_UNION, EWISE_INTERSECT, EWISE_DIFFERENCE = 0, 1, 2                 # g4s_csr_ewise_*: op (a plain int, not a flag bit; g4s.h)
COMBINE_PLUS, COMBINE_TIMES, COMBINE_MIN, COMBINE_MAX, COMBINE_FIRST, COMBINE_SECOND = 0, 1, 2, 3, 4, 5
DUP_KEEP = -1                                                            # g4s_csr_from_coo_*: dup is DUP_KEEP or a COMBINE_* value (g4s.h)
SELECT_TRIL, SELECT_TRIU, SELECT_OFFDIAG, SELECT_DIAG, SELECT_NONZERO, SELECT_GT, SELECT_GE, SELECT_LT, SELECT_LE = 0, 1, 2, 3, 4, 5, 6, 7, 8   # g4s_csr_select_*: pred
SEMIRING_PLUS_TIMES, SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS, SEMIRING_OR_AND, SEMIRING_MASK = 0, 512, 1024, 1536, 1536   # SpGEMM / SpMV value semiring (g4s.h)
PATTERN_ELEMENT_BLOCK_MATVEC, PATTERN_DENSE_ROW_TIMES_MATRIX, PATTERN_SYM_QUADRATIC_FORM = 1, 2, 3
DENSE_DGEMM, DENSE_DSYMM, DENSE_DTRMM, DENSE_DGEMV, DENSE_DSYMV, DENSE_DTRMV, DENSE_DSPMV = 1, 2, 3, 4, 5, 6, 7

i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)
vp = C.c_void_p

FUN_GATHER = C.CFUNCTYPE(None, C.c_int, C.c_int, C.POINTER(f64p), f64p, f64p)   # citcoms/lib/global_defs.h:48
FUN_APPLY = C.CFUNCTYPE(None, C.c_int, C.POINTER(f64p), f64p, f64p)             # citcoms/lib/global_defs.h:49


class CsrInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("nnz", C.c_int64),
                ("stream_blocks", C.c_int32), ("long_rows", C.c_int32), ("long_chunks", C.c_int32),
                ("tile_nnz", C.c_int32), ("tile_rows", C.c_int32), ("long_chunk_nnz", C.c_int32),
                ("algorithmic_bytes", C.c_int64), ("plan_bytes", C.c_int64), ("spmv_path", C.c_int32), ("reserved", C.c_int32)]


class TraverseInfo(C.Structure):
    """g4s_traverse_info: what a g4s_sssp / g4s_bfs call did."""
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("push_steps", C.c_int32), ("pull_steps", C.c_int32),
                ("host_waits", C.c_int32), ("reserved", C.c_int32), ("reached", C.c_int64), ("edges_relaxed", C.c_int64)]


class PagerankInfo(C.Structure):
    """g4s_pagerank_info: what a g4s_pagerank call did."""
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("host_waits", C.c_int32), ("products", C.c_int32),
                ("dangling", C.c_int64), ("residual", C.c_double)]


class BcInfo(C.Structure):
    """g4s_bc_info: what a g4s_betweenness call did."""
    _fields_ = [("sources", C.c_int32), ("max_depth", C.c_int32), ("host_waits", C.c_int32), ("sigma_exact", C.c_int32),
                ("levels", C.c_int64), ("reached", C.c_int64), ("edges_walked", C.c_int64), ("sigma_max", C.c_double)]


class MaskedInfo(C.Structure):
    """g4s_masked_info: what a g4s_spgemm_masked / g4s_triangle_count call did (which class the rows took)."""
    _fields_ = [("mask_nnz", C.c_int64), ("products", C.c_int64), ("rows_wave", C.c_int32), ("rows_lds", C.c_int32), ("rows_global", C.c_int32),
                ("rows_split", C.c_int32)]


class CCInfo(C.Structure):
    """g4s_cc_info: what a g4s_connected_components call found and did."""
    _fields_ = [("components", C.c_int64), ("largest", C.c_int64), ("edges_linked", C.c_int64), ("largest_label", C.c_int32),
                ("sample_rounds", C.c_int32), ("skipped", C.c_int32), ("host_waits", C.c_int32)]


class SCCInfo(C.Structure):
    """g4s_scc_info: what a g4s_strongly_connected_components call found and did."""
    _fields_ = [("components", C.c_int64), ("largest", C.c_int64), ("largest_label", C.c_int32), ("trimmed", C.c_int32), ("pivot", C.c_int32),
                ("pivot_size", C.c_int32), ("color_rounds", C.c_int32), ("reserved", C.c_int32), ("edges_walked", C.c_int64), ("launches", C.c_int32),
                ("resumes", C.c_int32), ("host_waits", C.c_int32), ("built_transpose", C.c_int32)]


class MSFInfo(C.Structure):
    """g4s_msf_info: what a g4s_minimum_spanning_forest call found and did."""
    _fields_ = [("components", C.c_int64), ("edges", C.c_int64), ("weight", C.c_double), ("entries_walked", C.c_int64), ("rounds", C.c_int32),
                ("launches", C.c_int32), ("resumes", C.c_int32), ("host_waits", C.c_int32)]


class KCoreInfo(C.Structure):
    """g4s_kcore_info: what a g4s_kcore call found and did."""
    _fields_ = [("edges_walked", C.c_int64), ("top_core_size", C.c_int64), ("degeneracy", C.c_int32), ("levels", C.c_int32), ("rounds", C.c_int32),
                ("scans", C.c_int32), ("launches", C.c_int32), ("resumes", C.c_int32), ("host_waits", C.c_int32), ("capped", C.c_int32)]


class KTrussInfo(C.Structure):
    """g4s_ktruss_info: what a g4s_ktruss call found and did."""
    _fields_ = [("triangles", C.c_int64), ("edges_walked", C.c_int64), ("support_walked", C.c_int64), ("top_truss_edges", C.c_int64),
                ("max_truss", C.c_int32), ("levels", C.c_int32), ("rounds", C.c_int32), ("scans", C.c_int32), ("launches", C.c_int32),
                ("resumes", C.c_int32), ("host_waits", C.c_int32), ("capped", C.c_int32)]


class ColorInfo(C.Structure):
    """g4s_color_info: what a g4s_color call found and did."""
    _fields_ = [("edges_walked", C.c_int64), ("class0", C.c_int64), ("colors", C.c_int32), ("rounds", C.c_int32), ("overflow", C.c_int32),
                ("launches", C.c_int32), ("resumes", C.c_int32), ("scan_resumes", C.c_int32), ("host_waits", C.c_int32), ("reserved", C.c_int32)]


class TRSVInfo(C.Structure):
    """g4s_trsv_info: what a g4s_sptrsv_analyse call found and did, and what a solve on its handle costs."""
    _fields_ = [("nnz_triangle", C.c_int64), ("n", C.c_int32), ("levels", C.c_int32), ("widest_level", C.c_int32), ("launches_per_solve", C.c_int32),
                ("chains", C.c_int32), ("bad_row", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32), ("resumes", C.c_int32),
                ("reserved", C.c_int32)]


class ILU0Info(C.Structure):
    """g4s_ilu0_info: what a g4s_ilu0_analyse call found and did, and what a factorisation and an apply on its handle cost."""
    _fields_ = [("nnz", C.c_int64), ("n", C.c_int32), ("levels", C.c_int32), ("widest_level", C.c_int32), ("launches_per_factor", C.c_int32),
                ("chains", C.c_int32), ("launches_per_apply", C.c_int32), ("bad_row", C.c_int32), ("bad_pivot", C.c_int32), ("launches", C.c_int32),
                ("host_waits", C.c_int32)]


class EwiseInfo(C.Structure):
    """g4s_ewise_info: what a g4s_csr_ewise_symbolic call found (entry counts, work units)."""
    _fields_ = [("nnz_a", C.c_int64), ("nnz_b", C.c_int64), ("nnz_c", C.c_int64), ("units", C.c_int64), ("unit_entries", C.c_int32),
                ("rows_split", C.c_int32), ("host_waits", C.c_int32), ("reserved", C.c_int32)]


class CooInfo(C.Structure):
    """g4s_coo_info: what a g4s_csr_from_coo_symbolic call found and did (counts, the longest run, the sort's shape)."""
    _fields_ = [("nnz_in", C.c_int64), ("nnz_out", C.c_int64), ("longest_run", C.c_int64), ("row_bits", C.c_int32), ("col_bits", C.c_int32),
                ("digit_bits", C.c_int32), ("sort_passes", C.c_int32), ("tile_entries", C.c_int32), ("presorted", C.c_int32), ("host_waits", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class ExtractInfo(C.Structure):
    """g4s_extract_info: what a g4s_csr_extract_symbolic / _numeric call found and did (counts, the kind of J, which class sorted how many rows)."""
    _fields_ = [("nnz_a", C.c_int64), ("nnz_rows", C.c_int64), ("nnz_c", C.c_int64), ("units", C.c_int64), ("unit_entries", C.c_int32),
                ("j_kind", C.c_int32), ("rows_in_order", C.c_int32), ("rows_sorted_wave", C.c_int32), ("rows_sorted_lds", C.c_int32),
                ("rows_sorted_radix", C.c_int32), ("lds_sort_max", C.c_int32), ("host_waits", C.c_int32), ("reserved", C.c_int32 * 4)]


class DistInfo(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("local_rows", C.c_int32), ("n_ref", C.c_int32), ("nnz_own", C.c_int64), ("nnz_rem", C.c_int64),
                ("send_bytes", C.c_int64), ("recv_bytes", C.c_int64), ("own_path", C.c_int32), ("rem_path", C.c_int32), ("connected", C.c_int32),
                ("reserved", C.c_int32)]


class DistSplit(C.Structure):
    """g4s_dist_split: one rank's rows cut into own-column and remote-column parts (host arrays from g4s_malloc)."""
    _fields_ = [("local_rows", C.c_int32), ("n_ref", C.c_int32), ("merged", C.c_int32), ("allgather", C.c_int32),
                ("nnz_own", C.c_int64), ("nnz_rem", C.c_int64), ("pad", C.c_int64),
                ("own_rowptr", C.POINTER(C.c_int32)), ("own_colids", C.POINTER(C.c_int32)), ("own_values", C.POINTER(C.c_double)),
                ("rem_rowptr", C.POINTER(C.c_int32)), ("rem_colids", C.POINTER(C.c_int32)), ("rem_values", C.POINTER(C.c_double)),
                ("want", C.POINTER(C.c_int32)), ("recv_cut", C.POINTER(C.c_int64))]


ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)      # g4s_transport.allreduce_sum_f64(ctx, buf_dev, count, stream)
EXCHANGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)                  # g4s_transport.exchange(ctx, h, stream)


class Transport(C.Structure):
    """g4s_transport: the two collectives of a partitioned Krylov solver as callbacks."""
    _fields_ = [("ctx", C.c_void_p), ("allreduce_sum_f64", ALLREDUCE_CB), ("exchange", EXCHANGE_CB)]


class Timings(C.Structure):
    """mm/inc/Timings.h:4-23 — seven stage times in milliseconds."""
    _fields_ = [(n, C.c_double) for n in ("create", "spmm", "convert", "order", "export_csr", "destroy", "total")]


class PatternDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("num_elems", C.c_int32), ("nodes_per_elem", C.c_int32), ("dof", C.c_int32),
                ("ien", vp), ("id", vp), ("nno", C.c_int32), ("neq", C.c_int32), ("edge_weight_base", C.c_int32),
                ("static_weights", C.c_int32), ("inner", C.c_int32), ("numbers", C.c_int32)]


class StokesParams(C.Structure):
    """g4s_stokes_params — the controls solve_Ahat_p_fhat_CG reads (citcoms/lib/Stokes_flow_Incomp.c:188-452)."""
    _fields_ = [("imp", C.c_double), ("inner_accuracy_scale", C.c_double), ("v_res", C.c_double), ("v_steps_low", C.c_int32),
                ("steps_max", C.c_int32), ("check_continuity_convergence", C.c_int32), ("check_pressure_convergence", C.c_int32)]


class StokesResult(C.Structure):
    _fields_ = [("outer_iterations", C.c_int32), ("last_solve_valid", C.c_int32), ("inner_iterations", C.c_int64),
                ("incompressibility", C.c_double), ("v_norm", C.c_double), ("p_norm", C.c_double), ("dvelocity", C.c_double),
                ("dpressure", C.c_double)]


# name -> (restype, argtypes); every symbol declared in include/*.h appears here (tests check the export list).
SIGNATURES = {
    "g4s_version": (C.c_char_p, []),
    "g4s_build_info": (C.c_char_p, []),
    "g4s_warm_up": (C.c_int, []),
    "g4s_last_error": (C.c_char_p, []),
    "g4s_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "g4s_set_device": (C.c_int, [C.c_int]),
    "g4s_device_synchronize": (C.c_int, []),
    "g4s_shutdown": (C.c_int, []),
    "g4s_trim": (C.c_int, []),
    "g4s_malloc": (vp, [C.c_size_t]),
    "g4s_free": (None, [vp]),
    "g4s_dev_alloc": (C.c_int, [C.POINTER(vp), C.c_size_t]),
    "g4s_dev_free": (C.c_int, [vp]),
    "g4s_memcpy_h2d": (C.c_int, [vp, vp, C.c_size_t]),
    "g4s_memcpy_d2h": (C.c_int, [vp, vp, C.c_size_t]),
    "g4s_csr_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, C.c_uint]),
    "g4s_csr_destroy": (C.c_int, [vp]),
    "g4s_csr_update_values": (C.c_int, [vp, vp, C.c_uint, vp]),
    "g4s_spmv_dist_update_values": (C.c_int, [vp, vp, C.c_uint, vp]),
    "g4s_csr_get_info": (C.c_int, [vp, C.POINTER(CsrInfo)]),
    "g4s_csr_device_arrays": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "g4s_spmv": (C.c_int, [vp, vp, vp, C.c_double, C.c_double, vp]),
    "g4s_spmv_csr_i32_f64": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_uint]),
    "g4s_spmv_semiring": (C.c_int, [vp, vp, vp, C.c_uint, vp]),
    "g4s_spmv_semiring_csr_i32_f64": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_uint]),
    "g4s_csr_transpose": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp]),
    "g4s_csr_transpose_reserve": (C.c_int, [vp]),
    "g4s_csr_transpose_info": (C.c_int, [vp, C.POINTER(CsrInfo)]),
    "g4s_spmv_transpose": (C.c_int, [vp, vp, vp, C.c_double, C.c_double, vp]),
    "g4s_spmv_semiring_transpose": (C.c_int, [vp, vp, vp, C.c_uint, vp]),
    "g4s_csr_traverse_reserve": (C.c_int, [vp, C.c_uint]),
    "g4s_sssp": (C.c_int, [vp, vp, C.c_int32, vp, C.c_int32, C.c_uint, C.POINTER(TraverseInfo), vp]),
    "g4s_bfs": (C.c_int, [vp, vp, C.c_int32, vp, C.c_int32, C.c_uint, C.POINTER(TraverseInfo), vp]),
    "g4s_csr_pagerank_reserve": (C.c_int, [vp, C.c_uint]),
    "g4s_pagerank": (C.c_int, [vp, C.c_double, C.c_double, C.c_int32, vp, vp, C.c_uint, C.POINTER(PagerankInfo), vp]),
    "g4s_csr_betweenness_reserve": (C.c_int, [vp, C.c_uint]),
    "g4s_betweenness": (C.c_int, [vp, vp, C.c_int32, C.c_double, vp, C.c_uint, C.POINTER(BcInfo), vp]),
    "g4s_spmm": (C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.c_double, C.c_double, C.c_uint, vp]),
    "g4s_csr_spmm_reserve": (C.c_int, [vp, C.c_int32]),
    "g4s_spmm_csr_i32_f64": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int64, vp, C.c_int64, C.c_double, C.c_double, C.c_uint]),
    "g4s_prim_exclusive_scan_i32": (C.c_int, [vp, vp, C.c_int64, vp]),
    "g4s_prim_exclusive_scan_i64": (C.c_int, [vp, vp, C.c_int64, vp]),
    "g4s_prim_sort_pairs_desc_i32": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "g4s_row_partition": (C.c_int, [C.c_int32, vp, vp, C.c_int64, C.c_int32, i64p, C.c_uint]),
    "g4s_dist_split_rows": (C.c_int, [C.c_int32, C.c_int32, i64p, C.c_int64, vp, vp, vp, C.c_uint, C.POINTER(DistSplit)]),
    "g4s_dist_split_free": (None, [C.POINTER(DistSplit)]),
    "g4s_spmv_dist_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, i64p, C.c_int64, vp, vp, vp, C.c_uint]),
    "g4s_spmv_dist_create_rect": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, i64p, i64p, vp, vp, vp, C.c_uint]),
    "g4s_spmv_dist_create_columns": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, i64p, C.c_int32, vp, vp, vp, C.c_uint]),
    "g4s_spmv_dist_destroy": (C.c_int, [vp]),
    "g4s_spmv_dist_get_info": (C.c_int, [vp, C.POINTER(DistInfo)]),
    "g4s_spmv_dist_connect_rccl": (C.c_int, [vp, vp]),
    "g4s_spmv_dist_want": (C.c_int, [vp, C.c_int32, i64p, C.POINTER(vp)]),
    "g4s_spmv_dist_set_give": (C.c_int, [vp, C.c_int32, C.c_int64, vp, C.c_uint]),
    "g4s_spmv_dist_apply": (C.c_int, [vp, vp, vp, vp]),
    "g4s_spmv_dist_begin": (C.c_int, [vp, vp, vp, vp]),
    "g4s_spmv_dist_buffers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i64p), C.POINTER(vp), C.POINTER(i64p)]),
    "g4s_spmv_dist_finish": (C.c_int, [vp, vp, vp]),
    "g4s_transport_rccl": (C.c_int, [vp, C.POINTER(Transport)]),
    "g4s_conj_grad_dist_tr": (C.c_int, [vp, C.POINTER(Transport), C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_double, C.c_int32, C.POINTER(C.c_int32), f64p, vp]),
    "g4s_stokes_uzawa_cg_dist": (C.c_int, [vp, vp, vp, C.POINTER(Transport), C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_double, vp, C.c_int32, vp, vp, vp,
                                           C.POINTER(StokesParams), C.POINTER(StokesResult), vp, C.c_int32, vp]),
    "g4s_comm_unique_id": (C.c_int, [vp]),
    "g4s_comm_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, vp]),
    "g4s_comm_destroy": (C.c_int, [vp]),
    "g4s_comm_allreduce_sum_f64": (C.c_int, [vp, vp, C.c_int64, vp]),
    "g4s_conj_grad_dist": (C.c_int, [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), vp]),
    "g4s_spgemm_flop": (C.c_int, [C.c_int32, vp, vp, vp, i64p, vp, C.c_uint]),
    "g4s_spgemm_csr_i32_f64": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                          C.c_int32, C.c_int32, C.c_int32, i64p, C.POINTER(Timings), C.c_uint]),
    "g4s_spgemm_symbolic": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, i64p, vp]),
    "g4s_spgemm_numeric": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp]),
    "g4s_spgemm_masked": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(MaskedInfo), vp]),
    "g4s_triangle_count": (C.c_int, [C.c_int32, vp, vp, i64p, C.c_uint, C.POINTER(MaskedInfo), vp]),
    "g4s_connected_components": (C.c_int, [C.c_int32, vp, vp, vp, C.c_uint, C.POINTER(CCInfo), vp]),
    "g4s_strongly_connected_components": (C.c_int, [C.c_int32, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(SCCInfo), vp]),
    "g4s_minimum_spanning_forest": (C.c_int, [C.c_int32, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(MSFInfo), vp]),
    "g4s_kcore": (C.c_int, [C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_uint, C.POINTER(KCoreInfo), vp]),
    "g4s_ktruss": (C.c_int, [C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_uint, C.POINTER(KTrussInfo), vp]),
    "g4s_color": (C.c_int, [C.c_int32, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint, C.POINTER(ColorInfo), vp]),
    "g4s_sptrsv_analyse": (C.c_int, [C.POINTER(vp), C.c_int32, vp, vp, vp, vp, C.c_uint, C.POINTER(TRSVInfo), vp]),
    "g4s_sptrsv_solve": (C.c_int, [vp, vp, vp, vp]),
    "g4s_sptrsv_solve_multi": (C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.c_uint, vp]),
    "g4s_sptrsv_update_values": (C.c_int, [vp, vp, C.c_uint, vp]),
    "g4s_sptrsv_get_info": (C.c_int, [vp, C.POINTER(TRSVInfo)]),
    "g4s_sptrsv_destroy": (C.c_int, [vp]),
    "g4s_ilu0_analyse": (C.c_int, [C.POINTER(vp), C.c_int32, vp, vp, vp, C.c_uint, C.POINTER(ILU0Info), vp]),
    "g4s_ilu0_factor": (C.c_int, [vp, vp, C.c_uint, vp, vp]),
    "g4s_ilu0_apply": (C.c_int, [vp, vp, vp, vp]),
    "g4s_ilu0_apply_multi": (C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.c_uint, vp]),
    "g4s_ilu0_get_factors": (C.c_int, [vp, vp, C.c_uint, vp]),
    "g4s_ilu0_get_info": (C.c_int, [vp, C.POINTER(ILU0Info)]),
    "g4s_ilu0_destroy": (C.c_int, [vp]),
    "g4s_csr_ewise_symbolic": (C.c_int, [C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, i64p, C.c_uint, C.POINTER(EwiseInfo), vp]),
    "g4s_csr_ewise_numeric": (C.c_int, [C.c_int, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp]),
    "g4s_csr_select_symbolic": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_int32, C.c_int32, vp, vp, vp, vp, i64p, C.c_uint, vp]),
    "g4s_csr_select_numeric": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_uint, vp]),
    "g4s_csr_from_coo_symbolic": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, i64p, C.c_uint, C.POINTER(CooInfo), vp]),
    "g4s_csr_from_coo_numeric": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp]),
    "g4s_csr_row_indices": (C.c_int, [C.c_int32, C.c_int64, vp, vp, C.c_uint, vp]),
    "g4s_csr_extract_symbolic": (C.c_int, [C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, i64p, C.c_uint, C.POINTER(ExtractInfo), vp]),
    "g4s_csr_extract_numeric": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(ExtractInfo), vp]),
    "g4s_register_pattern":(C.c_int, [FUN_GATHER, FUN_APPLY, C.POINTER(PatternDesc)]),
    "g4s_unregister_pattern": (C.c_int, [FUN_GATHER, FUN_APPLY]),
    "g4s_set_host_callback_policy": (C.c_int, [C.c_int32]),
    "g4s_set_host_callback_policy_thread": (C.c_int, [C.c_int32, C.POINTER(C.c_int32)]),
    "spmm_dense": (None, [C.c_uint32, C.c_uint32, vp, vp, vp, vp, FUN_GATHER, FUN_APPLY, f64p, C.c_int]),
    "g4s_spmm_dense": (C.c_int, [C.c_uint32, C.c_uint32, vp, vp, vp, vp, FUN_GATHER, FUN_APPLY, f64p, C.c_int]),
    "g4s_elem_op_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp]),
    "g4s_elem_op_destroy": (C.c_int, [vp]),
    "g4s_elem_op_apply": (C.c_int, [vp, vp, vp, vp]),
    "g4s_elem_op_inverse_diagonal": (C.c_int, [vp, vp, vp]),
    "g4s_conj_grad": (C.c_int, [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_double, C.POINTER(C.c_int32), f64p, vp]),
    "g4s_cg_ws_create": (C.c_int, [C.POINTER(vp), C.c_int32]),
    "g4s_cg_ws_destroy": (C.c_int, [vp]),
    "g4s_cg_begin": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, vp]),
    "g4s_cg_direction": (C.c_int, [vp, C.c_int32, C.c_double, vp]),
    "g4s_cg_state": (C.c_int, [vp, i32p, i32p, f64p, vp]),
    "g4s_cg_buffers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "g4s_cg_reduce_pAp": (C.c_int, [vp, vp]),
    "g4s_cg_update": (C.c_int, [vp, vp, vp, vp]),
    "g4s_cg_end": (C.c_int, [vp, vp, vp, C.c_int32, vp]),
    "g4s_node_op_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]),
    "g4s_node_op_destroy": (C.c_int, [vp]),
    "g4s_node_op_apply": (C.c_int, [vp, vp, vp, vp, C.c_int32, vp]),
    "g4s_conj_grad_node": (C.c_int, [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_double, C.POINTER(C.c_int32), f64p, vp]),
    "g4s_elem_op_div_u": (C.c_int, [vp, vp, vp, vp, vp]),
    "g4s_elem_op_grad_p": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, vp]),
    "g4s_elem_op_pressure_preconditioner": (C.c_int, [vp, vp, vp, vp, vp]),
    "g4s_stokes_uzawa_cg": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, C.c_int32, vp, vp, vp, C.POINTER(StokesParams),
                                      C.POINTER(StokesResult), vp, C.c_int32, vp]),
    "g4s_dense_rows_times_matrix": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]),
    "g4s_dense_rows_times_matrix_grad": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]),
    "g4s_sym_quadratic_form": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp]),
    "g4s_dense_mm": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, C.c_uint]),
    "g4s_dense_mv": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, C.c_uint]),
    # include/g4s_synth.h
    "g4s_synth_rmat_keys": (C.c_int, [C.c_uint64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, vp, vp]),
    "g4s_synth_csr_from_keys": (C.c_int, [C.c_uint64, C.c_int64, C.c_int32, vp, C.c_int64, vp, vp, vp, vp]),
    "g4s_synth_vector": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, vp, vp]),
    "g4s_synth_laplacian_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, vp, vp, vp, vp,
                                           C.c_int32, vp]),
    "g4s_synth_banded": (C.c_int, [C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp]),
}


class G4SError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"g4s status {status}: {message}")
        self.status = status


_lib = None


def load():
    """Load libg4s_hip.so once. torch is imported first so that the HIP runtime both sides use is the one
    already mapped (same SONAME, libamdhip64.so.7); two runtimes in one process would not share device pointers."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"or `make -C g4s_amd/csrc`. g4s_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (maps torch's libamdhip64.so.7 before ours resolves its NEEDED entry)
    except Exception:  # pragma: no cover - torch is plumbing; a plain C++ host does not need it
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here == a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != OK:
        raise G4SError(status, load().g4s_last_error().decode())
    return status

HOST_CALLBACKS_SERIAL, HOST_CALLBACKS_PARALLEL, HOST_CALLBACKS_REFUSE = 0, 1, 2   # g4s_set_host_callback_policy
