"""ctypes binding of libartn_hip.so (C ABI: include/artn.h).

PyTorch is plumbing here: it owns device memory (`Tensor.data_ptr()`), the current HIP
stream and, elsewhere, torch.distributed.  All arithmetic of the hot path happens in the
HIP kernels behind the C ABI.  There is NO CPU fallback: if the library is missing or a
tensor is not on a GPU the call raises.
"""
import ctypes
import os
import threading

import torch

ABI_VERSION = 9
ARTN_MAX_LABELS = 96
ARTN_PROGRAM_MAX_EXT = 256
ARTN_C64, ARTN_C128, ARTN_C64_BF16 = 0, 1, 2
KERNEL_GENERIC, KERNEL_BITS_MFMA, KERNEL_GEMM_MFMA, KERNEL_PGEMM, KERNEL_XGEMM = 0, 1, 2, 4, 5

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARTN_LIB") or os.path.join(_HERE, "libartn_hip.so")  # ARTN_LIB: diagnostic builds


class ArtnStepDesc(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("n_labels", ctypes.c_int32),
        ("extent", ctypes.c_int64 * ARTN_MAX_LABELS),
        ("stride_a", ctypes.c_int64 * ARTN_MAX_LABELS),
        ("stride_b", ctypes.c_int64 * ARTN_MAX_LABELS),
        ("stride_c", ctypes.c_int64 * ARTN_MAX_LABELS),
    ]


class ArtnStepInfo(ctypes.Structure):
    _fields_ = [
        ("kernel", ctypes.c_int32),
        ("k_bits", ctypes.c_int32),
        ("m_tile_bits", ctypes.c_int32),
        ("n_tile_bits", ctypes.c_int32),
        ("tile_in_bits", ctypes.c_int32),
        ("tile_out_bits", ctypes.c_int32),
        ("run_in_bits", ctypes.c_int32),
        ("run_out_bits", ctypes.c_int32),
        ("lds_bytes", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("n_tiles", ctypes.c_int64),
        ("a_rereads", ctypes.c_int64),
        ("flops", ctypes.c_double),
        ("bytes", ctypes.c_double),
        ("k2_bits", ctypes.c_int32),
        ("n2_tile_bits", ctypes.c_int32),
        ("tile_mid_bits", ctypes.c_int32),
        ("arith", ctypes.c_int32),
        ("mfma_flops", ctypes.c_double),
        ("workspace_bytes", ctypes.c_int64),
        ("k3_bits", ctypes.c_int32),
        ("stage1_reruns", ctypes.c_int32),
    ]


class ArtnBornPlan(ctypes.Structure):
    _fields_ = [
        ("block_bits", ctypes.c_int32),
        ("overlap_grid", ctypes.c_int32),
        ("n_blocks", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
    ]


MARGINAL_GENERIC, MARGINAL_STREAM = 0, 1


class ArtnMarginalDesc(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("n_dims", ctypes.c_int32),
        ("extent", ctypes.c_int64 * ARTN_MAX_LABELS),
        ("stride", ctypes.c_int64 * ARTN_MAX_LABELS),
        ("keep", ctypes.c_int32 * ARTN_MAX_LABELS),
    ]


class ArtnMarginalInfo(ctypes.Structure):
    _fields_ = [
        ("kernel", ctypes.c_int32),
        ("chunk_bits", ctypes.c_int32),
        ("bin_bits", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("workspace_bytes", ctypes.c_int64),
        ("out_elems", ctypes.c_int64),
    ]


RDM_GENERIC, RDM_STREAM = 0, 1


class ArtnRdmInfo(ctypes.Structure):
    _fields_ = [
        ("kernel", ctypes.c_int32),
        ("panel_bits", ctypes.c_int32),
        ("tiles", ctypes.c_int32),
        ("splits", ctypes.c_int32),
        ("dim", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("flops", ctypes.c_double),
    ]


class ArtnPauliInfo(ctypes.Structure):
    _fields_ = [
        ("n_groups", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("terms_per_launch", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("workspace_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
    ]


class ArtnPauliApplyInfo(ctypes.Structure):
    _fields_ = [
        ("n_groups", ctypes.c_int32),
        ("n_xmask_hi", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


class ArtnPauliEvolveInfo(ctypes.Structure):
    _fields_ = [
        ("n_runs", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("max_rank", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


PAULI_EVOLVE_MAX_RANK = 4


class ArtnPauliAdjointInfo(ctypes.Structure):
    _fields_ = [
        ("n_runs", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("max_rank", ctypes.c_int32),
        ("n_measured", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


PAULI_ADJOINT_MAX_RANK = 3


class ArtnGatesInfo(ctypes.Structure):
    _fields_ = [
        ("n_runs", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("max_rank", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


GATES_MAX_RANK = 4
GATE_DIAGONAL, GATE_LOCAL = 1, 2


class ArtnGatesAdjointInfo(ctypes.Structure):
    _fields_ = [
        ("n_runs", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("max_rank", ctypes.c_int32),
        ("n_measured", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


GATES_ADJOINT_MAX_RANK = 3
GATES_ADJOINT_GATE_BYTES = 592


class ArtnWgateInfo(ctypes.Structure):
    _fields_ = [
        ("k", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("diagonal", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("n_tiles", ctypes.c_int64),
        ("segment", ctypes.c_int64),
        ("lds_bytes", ctypes.c_int64),
        ("table_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


WGATE_MAX_K = 5
WGATE_TILE_BITS = {ARTN_C64: 12, ARTN_C128: 11}
WGATE_TABLE_HEADER_BYTES = 480
ArtnMgateInfo = ArtnWgateInfo                                  # (include/artn.h: the same fields)
MGATE_MIN_K, MGATE_MAX_K = 3, 7
MGATE_TABLE_HEADER_BYTES = 544


class ArtnCgateInfo(ctypes.Structure):
    _fields_ = [
        ("t", ctypes.c_int32),
        ("c", ctypes.c_int32),
        ("c_high", ctypes.c_int32),
        ("c_low", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("diagonal", ctypes.c_int32),
        ("n_selected", ctypes.c_int64),
        ("n_tiles", ctypes.c_int64),
        ("segment", ctypes.c_int64),
        ("lds_bytes", ctypes.c_int64),
        ("table_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


CGATE_LINE_BITS = {ARTN_C64: 4, ARTN_C128: 3}
CGATE_MAX_HOLES = 64
CGATE_TABLE_HEADER_BYTES = 1000

KRYLOV_BATCH = 8
KRYLOV_MAX_VECS = 64


class ArtnKrylovInfo(ctypes.Structure):
    _fields_ = [
        ("grid", ctypes.c_int32),
        ("batch", ctypes.c_int32),
        ("dots_launches", ctypes.c_int32),
        ("combine_launches", ctypes.c_int32),
        ("dots_workspace_bytes", ctypes.c_int64),
        ("combine_workspace_bytes", ctypes.c_int64),
        ("dots_bytes_read", ctypes.c_int64),
        ("combine_bytes_read", ctypes.c_int64),
        ("combine_bytes_written", ctypes.c_int64),
    ]


MEASURE_MAX_DIMS = 10
MEASURE_RECORD_BYTES = 32


class ArtnMeasureInfo(ctypes.Structure):
    _fields_ = [
        ("k", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("collapse_launches", ctypes.c_int32),
        ("reset_launches", ctypes.c_int32),
        ("dim", ctypes.c_int64),
        ("n", ctypes.c_int64),
        ("record_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
        ("mem_bit", ctypes.c_int32 * MEASURE_MAX_DIMS),
    ]


CHANNEL_MAX_OPS = 256
CHANNEL_FIXED, CHANNEL_DIAGONAL, CHANNEL_DENSE = 0, 1, 2
CHANNEL_FORMS = ("FIXED", "DIAGONAL", "DENSE")
CHANNEL_OP_DIAGONAL, CHANNEL_OP_IDENTITY = 1, 2
CHANNEL_TABLE_HEADER_BYTES = 512


class ArtnChannelInfo(ctypes.Structure):
    _fields_ = [
        ("t", ctypes.c_int32),
        ("m", ctypes.c_int32),
        ("form", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("launches", ctypes.c_int32 * 3),
        ("reduction", ctypes.c_int32 * 3),
        ("n_tiles", ctypes.c_int64),
        ("segment", ctypes.c_int64),
        ("lds_bytes", ctypes.c_int64),
        ("weight_doubles", ctypes.c_int64),
        ("table_bytes", ctypes.c_int64),
        ("record_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
    ]


BATCH_MAX_BITS, BATCH_MAX_FIELDS = 24, 24


class ArtnBatchInfo(ctypes.Structure):
    _fields_ = [
        ("n_fields", ctypes.c_int32),
        ("batch_bits", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("launches", ctypes.c_int32),
        ("reset_launches", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("n", ctypes.c_int64),
        ("n_tiles", ctypes.c_int64),
        ("segment", ctypes.c_int64),
        ("lds_bytes", ctypes.c_int64),
        ("table_bytes", ctypes.c_int64),
        ("record_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("bytes_written", ctypes.c_int64),
        ("field_shift", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_width", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_pos", ctypes.c_int32 * BATCH_MAX_FIELDS),
    ]


CGATE_BATCH_MAX_CASES = 16
CGATE_CASE_DIAGONAL, CGATE_CASE_IDENTITY = 1, 2
CGATE_BATCH_CASES_BYTES = 400


class ArtnCgateBatchInfo(ctypes.Structure):
    _fields_ = ArtnCgateInfo._fields_ + [
        ("m", ctypes.c_int32),
        ("batch_bits", ctypes.c_int32),
        ("n_fields", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("field_shift", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_width", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_pos", ctypes.c_int32 * BATCH_MAX_FIELDS),
    ]


class ArtnPauliBatchInfo(ctypes.Structure):
    _fields_ = [
        ("n_groups", ctypes.c_int32),
        ("n_launches", ctypes.c_int32),
        ("terms_per_launch", ctypes.c_int32),
        ("batch_bits", ctypes.c_int32),
        ("local_bits", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("n_fields", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("chunks", ctypes.c_int64),
        ("chunks_halved", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("n", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("out_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64),
        ("field_shift", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_width", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_pos", ctypes.c_int32 * BATCH_MAX_FIELDS),
    ]


SAMPLE_BATCH_SMALL, SAMPLE_BATCH_TILED = 0, 1


class ArtnSampleBatchInfo(ctypes.Structure):
    _fields_ = [
        ("form", ctypes.c_int32),
        ("launches", ctypes.c_int32),
        ("batch_bits", ctypes.c_int32),
        ("local_bits", ctypes.c_int32),
        ("block_bits", ctypes.c_int32),
        ("n_fields", ctypes.c_int32),
        ("grid", ctypes.c_int32 * 3),
        ("reserved", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("n", ctypes.c_int64),
        ("blocks_per_trajectory", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("bytes_read_min", ctypes.c_int64),
        ("field_shift", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_width", ctypes.c_int32 * BATCH_MAX_FIELDS),
        ("field_pos", ctypes.c_int32 * BATCH_MAX_FIELDS),
    ]


DIAG_MAX_GROUPS, DIAG_MAX_TERMS, DIAG_TILE_BITS = 64, 65536, 10
DIAG_PHASE, DIAG_MULTIPLY = 0, 1
DIAG_PAIR_EVOLVE, DIAG_PAIR_TRANSITION = 0, 1
DIAG_OPS = ("VALUES", "EXPECT", "PHASE", "MULTIPLY", "PAIR")
DIAG_TABLE_HEADER_BYTES = 64


class ArtnDiagInfo(ctypes.Structure):
    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("n_static", ctypes.c_int32),
        ("n_dynamic", ctypes.c_int32),
        ("n_groups", ctypes.c_int32),
        ("tile_bits", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("n_tiles", ctypes.c_int64),
        ("table_bytes", ctypes.c_int64),
        ("workspace_bytes", ctypes.c_int64),
        ("bytes_read", ctypes.c_int64 * 5),
        ("bytes_written", ctypes.c_int64 * 5),
    ]


BITPERM_MAX_BITS, BITPERM_MAX_PASSES = 40, 8
BITPERM_TABLE_HEADER_BYTES, BITPERM_PASS_BYTES = 64, 576


class ArtnBitpermInfo(ctypes.Structure):
    _fields_ = [
        ("n_bits", ctypes.c_int32),
        ("passes", ctypes.c_int32),
        ("line_bits", ctypes.c_int32),
        ("moved", ctypes.c_int32),
        ("moved_high", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("table_bytes", ctypes.c_int64),
        ("lds_bytes", ctypes.c_int64),
        ("bytes_moved", ctypes.c_int64),
        ("tile_bits", ctypes.c_int32 * 8),
        ("grid", ctypes.c_int32 * 8),
        ("load_degree", ctypes.c_int32 * 8),
        ("store_degree", ctypes.c_int32 * 8),
        ("n_tiles", ctypes.c_int64 * 8),
        ("moved_mask", ctypes.c_uint64 * 8),
    ]


_lib = None
_lock = threading.Lock()

_EXPORTS = {
    "artn_abi_version": (ctypes.c_int, []),
    "artn_last_error": (ctypes.c_char_p, []),
    "artn_device_count": (ctypes.c_int, []),
    "artn_contract_query": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.POINTER(ArtnStepInfo)]),
    "artn_last_plan_note": (ctypes.c_char_p, []),
    "artn_contract": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "artn_contract_ws": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "artn_contract_gather": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_contract2_query": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.POINTER(ArtnStepDesc),
                                            ctypes.POINTER(ArtnStepInfo)]),
    "artn_contract2": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_contract_acc": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "artn_contract2_acc": (ctypes.c_int, [ctypes.POINTER(ArtnStepDesc), ctypes.POINTER(ArtnStepDesc), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_program_record_bytes": (ctypes.c_int64, []),
    "artn_program_image_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "artn_program_build": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int64]),
    "artn_program_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "artn_gather_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_axpy_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "artn_sum_axis_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_void_p]),
    "artn_axpy_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "artn_sum_axis_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_void_p]),
    "artn_probe_mfma_rate": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "artn_absmax_normalize_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "artn_absmax_normalize_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "artn_born_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ArtnBornPlan)]),
    "artn_born_overlap": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_born_block_sums": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "artn_born_pick": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_marginal_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.POINTER(ArtnMarginalInfo)]),
    "artn_marginal": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p]),
    "artn_rdm_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.POINTER(ArtnRdmInfo)]),
    "artn_rdm_row_offsets": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p]),
    "artn_rdm": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 (a library built before them lacks both: has("artn_pauli_expect"))
    "artn_pauli_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.POINTER(ArtnPauliInfo), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "artn_pauli_expect": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: y = H a (has("artn_pauli_apply"))
    "artn_pauli_apply_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.POINTER(ArtnPauliApplyInfo), ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_pauli_apply_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_int64]),
    "artn_pauli_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: in-place circuits of Pauli steps (has("artn_pauli_evolve"))
    "artn_pauli_evolve_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_int32, ctypes.POINTER(ArtnPauliEvolveInfo), ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "artn_pauli_evolve_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "artn_pauli_evolve": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: the same circuits on two states with transition elements (has("artn_pauli_adjoint"))
    "artn_pauli_adjoint_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ArtnPauliAdjointInfo), ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "artn_pauli_adjoint_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "artn_pauli_adjoint": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    # additive to ABI 9 as well: in-place circuits of dense one- and two-qubit gates (has("artn_gates_apply"))
    "artn_gates_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ArtnGatesInfo), ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_gates_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "artn_gates_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p]),
    # additive to ABI 9 as well: the same circuits on two states with transition elements (has("artn_gates_adjoint"))
    "artn_gates_adjoint_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                ctypes.POINTER(ArtnGatesAdjointInfo), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_gates_adjoint_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                               ctypes.c_int64]),
    "artn_gates_adjoint": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    # additive to ABI 9 as well: one dense gate on one to five qubits, in place (has("artn_wgate_apply"))
    "artn_wgate_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(ArtnWgateInfo), ctypes.c_void_p, ctypes.c_void_p]),
    "artn_wgate_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64]),
    "artn_wgate_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: one dense gate on three to seven qubits on the f64 matrix cores (has("artn_mgate_apply"))
    "artn_mgate_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(ArtnMgateInfo), ctypes.c_void_p, ctypes.c_void_p]),
    "artn_mgate_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64]),
    "artn_mgate_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: one dense gate under any number of controls and a device-resident condition (has("artn_cgate_apply"))
    "artn_cgate_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ArtnCgateInfo),
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_cgate_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "artn_cgate_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: the vector algebra of Krylov drivers (has("artn_krylov_combine"))
    "artn_krylov_query": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ArtnKrylovInfo)]),
    "artn_krylov_dots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_krylov_combine": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    # additive to ABI 9 as well: measurement, post-selection and reset in place (has("artn_measure_collapse"))
    "artn_measure_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.POINTER(ArtnMeasureInfo)]),
    "artn_measure_choose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "artn_measure_collapse": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_void_p]),
    # additive to ABI 9 as well: noise channels drawn and applied on the device (has("artn_channel_apply"))
    "artn_channel_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ArtnChannelInfo), ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "artn_channel_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "artn_channel_choose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p]),
    "artn_channel_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p]),
    # additive to ABI 9 as well: batched trajectories -- measurement, reset and channels per state (has("artn_channel_batch_apply"))
    "artn_measure_batch_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.POINTER(ArtnBatchInfo)]),
    "artn_measure_batch_choose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_measure_batch_collapse": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "artn_channel_batch_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.POINTER(ArtnBatchInfo), ctypes.c_void_p, ctypes.c_void_p]),
    "artn_channel_batch_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int64]),
    "artn_channel_batch_choose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "artn_channel_batch_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    # additive to ABI 9 as well: conditional gates -- a controlled gate chosen per trajectory by a device-side selector
    # (has("artn_cgate_batch_apply"))
    "artn_cgate_batch_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.POINTER(ArtnCgateBatchInfo), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_cgate_batch_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "artn_cgate_batch_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: Pauli expectation values per trajectory of a batched tensor (has("artn_pauli_batch_expect"))
    "artn_pauli_batch_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.POINTER(ArtnPauliBatchInfo), ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_pauli_batch_expect": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_void_p]),
    # additive to ABI 9 as well: bitstring sampling per trajectory of a batched tensor (has("artn_sample_batch"))
    "artn_sample_batch_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.POINTER(ArtnSampleBatchInfo)]),
    "artn_sample_batch": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    # additive to ABI 9 as well: diagonal operators -- cost-function phases, moments and pairs in one pass (has("artn_diag_apply"))
    "artn_diag_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(ArtnDiagInfo), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "artn_diag_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.c_void_p, ctypes.c_int64]),
    "artn_diag_values": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_diag_expect": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "artn_diag_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]),
    "artn_diag_pair": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double,
                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    # additive to ABI 9 as well: in-place permutations of the index bits of a state (has("artn_bitperm_apply"))
    "artn_bitperm_query": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.POINTER(ArtnBitpermInfo), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "artn_bitperm_pack": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_int64]),
    "artn_bitperm_apply": (ctypes.c_int, [ctypes.POINTER(ArtnMarginalDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
}


# entry points of DEVELOPMENT builds only (make dev): bound when the loaded library has them
_DEV_EXPORTS = {
    "artn_contract3_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "artn_contract3": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}


def has(name):
    """True when the loaded library exports `name` (the development-only entry points)."""
    try:
        getattr(lib(), name)
        return True
    except AttributeError:
        return False


def exported_symbols():
    """Names include/artn.h declares (used by the CPU test that checks the library exports them)."""
    return sorted(_EXPORTS)


def lib():
    """Load libartn_hip.so (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); "
                "artensor_amd has no CPU fallback")
        # torch must be imported first so that its bundled libamdhip64.so (same SONAME)
        # is the HIP runtime this library binds to -- one runtime per process.
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in _EXPORTS.items():
            if os.environ.get("ARTN_LIB") and not hasattr(handle, name):
                continue  # diagnostic builds of older revisions (tools/libartn_prev.so) may lack newer entry points
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in _DEV_EXPORTS.items():
            if hasattr(handle, name):
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
        if handle.artn_abi_version() != ABI_VERSION:
            raise RuntimeError("libartn_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().artn_last_error()
        raise RuntimeError(f"artn error {rc}: {msg.decode() if msg else '?'}")


def current_stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(
            f"{what}: artensor_amd executes on MI355X only (got "
            f"{'a ' + str(t.device) + ' tensor' if isinstance(t, torch.Tensor) else type(t).__name__}); "
            "there is no CPU fallback -- move the tensors to a 'cuda' device")
