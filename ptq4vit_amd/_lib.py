"""ctypes binding of the C ABI in include/ptq4vit_hip.h (libptq4vit_hip.so, built in-tree).

The library is the product: if it cannot be loaded this module raises -- there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P4V_LIB") or os.path.join(_HERE, "csrc", "libptq4vit_hip.so")   # P4V_LIB: tuning builds only

METRICS = {
    "L1_norm": 0,
    "L2_norm": 1,
    "linear_weighted_L2_norm": 2,
    "square_weighted_L2_norm": 3,
    "hessian": 4,
    "cosine": 5,
}


class LinearDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "tokens", "in_features", "out_features", "n_V", "n_H", "n_a", "w_bit", "a_bit", "metric",
        "eq_n", "search_round", "twin_postgelu", "init_layerwise", "has_bias", "reserved")]


class MlpDesc(C.Structure):
    """p4v_mlp_desc: the two Linear layers of a fused MLP forward."""
    _fields_ = [("fc1", LinearDesc), ("fc2", LinearDesc)]


class MatMulDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("batch", "heads", "M", "K", "N")] + [("_pad0", C.c_int32)] +
                [("a_stride", C.c_int64 * 4), ("b_stride", C.c_int64 * 4)] +
                [(n, C.c_int32) for n in ("A_bit", "B_bit", "metric", "eq_n", "search_round", "sos",
                                          "init_layerwise", "reserved")])


class AttnDesc(C.Structure):
    """p4v_attn_desc: the two MatMuls of a fused attention forward and the factor between them."""
    _fields_ = [("qk", MatMulDesc), ("pv", MatMulDesc), ("scale", C.c_float), ("reserved", C.c_int32)]


class WattnDesc(C.Structure):
    """p4v_wattn_desc: the two MatMuls of a fused window attention forward, the windows per image, whether a shift mask comes."""
    _fields_ = [("qk", MatMulDesc), ("pv", MatMulDesc), ("n_windows", C.c_int32), ("has_mask", C.c_int32)]


class WattnTensors(C.Structure):
    """p4v_wattn_tensors: the device pointers of a p4v_wattn_quant_forward call, its workspace and the workspace's size."""
    POINTERS = ("q", "kT", "v", "bias", "mask", "qk_A_interval", "qk_B_interval", "pv_A_interval", "pv_B_interval", "split", "out", "probs", "ws")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + [("ws_bytes", C.c_size_t)]


class QkvAttnDesc(C.Structure):
    """p4v_qkv_attn_desc: the qkv Linear layer, the two MatMuls of the attention block behind it and the factor between those."""
    _fields_ = [("qkv", LinearDesc), ("qk", MatMulDesc), ("pv", MatMulDesc), ("scale", C.c_float), ("reserved", C.c_int32)]


class QkvAttnTensors(C.Structure):
    """p4v_qkv_attn_tensors: the device pointers of a p4v_qkv_attn_quant_forward call, its workspace and the workspace's size."""
    POINTERS = ("x", "w", "bias", "w_interval", "a_interval", "qk_A_interval", "qk_B_interval", "pv_A_interval", "pv_B_interval", "split",
                "out", "qkv_out", "probs", "ws")
    _fields_ = [(n, C.c_void_p) for n in POINTERS] + [("ws_bytes", C.c_size_t)]


class MatMulBlocksDesc(C.Structure):
    """p4v_matmul_blocks_desc: the MatMul descriptor plus the row / column block counts of both operands."""
    _fields_ = [("mm", MatMulDesc)] + [(n, C.c_int32) for n in ("n_V_A", "n_H_A", "n_V_B", "n_H_B")]


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "in_channels", "height", "width", "out_channels", "kernel_h", "kernel_w", "stride_h", "stride_w",
        "pad_h", "pad_w", "dil_h", "dil_w", "w_bit", "a_bit", "metric", "eq_n", "search_round", "channelwise",
        "init_layerwise", "has_bias", "reserved")]


class KernelStats(C.Structure):
    _fields_ = [("sweep_i8_ms", C.c_double), ("sweep_i8_launches", C.c_int64), ("sweep_i8_macs", C.c_double),
                ("sweep_f32_ms", C.c_double), ("sweep_f32_launches", C.c_int64), ("sweep_f32_macs", C.c_double),
                ("sweep_i8_alg_macs", C.c_double), ("sweep_f32_alg_macs", C.c_double),
                ("sweep6_ms", C.c_double), ("sweep6_launches", C.c_int64), ("sweep6_macs", C.c_double), ("sweep6_alg_macs", C.c_double),
                ("memo_hits", C.c_int64), ("memo_misses", C.c_int64),
                ("sweep7_ms", C.c_double), ("sweep7_launches", C.c_int64), ("sweep7_macs", C.c_double), ("sweep7_alg_macs", C.c_double),
                ("sweep7_twin_ms", C.c_double), ("sweep7_twin_launches", C.c_int64), ("event_overhead_ms", C.c_double)]


class LaunchRecord(C.Structure):
    _fields_ = [("kind", C.c_int32), ("stage", C.c_int32), ("grid_x", C.c_int32), ("grid_z", C.c_int32),
                ("ms", C.c_double), ("ops", C.c_double), ("alg_ops", C.c_double), ("alg_bytes", C.c_double)]


LAUNCH_KINDS = {0: "k_sweep<int8>", 1: "k_sweep<float>", 2: "k_sweep6", 3: "k_sweep7", 4: "k_sweep7 (twin)", 5: "k_sweep4/5", 6: "k_sweep9",
                7: "k_sweep8", 8: "k_sweep2g", 9: "k_sweep2", 11: "k_sos_split", 12: "k_bound", 13: "k_slice_b", 14: "k_slice_a", 15: "k_sweep_seg", 16: "k_mlp_fc1",
                17: "k_attn_qk", 18: "k_qkv_heads"}
LAUNCH_STAGES = {0: "full", 1: "A", 2: "B1", 3: "B2", 4: "A2"}


class PlaneDesc(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("cols_padded", C.c_int64), ("rows_per_scale", C.c_int64),
                ("mode", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("qmax", C.c_int32),
                ("const_scale", C.c_float), ("reserved", C.c_int32)]


class ExportDesc(C.Structure):
    _fields_ = [("dims", C.c_int32 * 4), ("src_stride", C.c_int64 * 4),
                ("scale1_stride", C.c_int64 * 4), ("scale1_div", C.c_int32 * 4),
                ("scale2_stride", C.c_int64 * 4), ("scale2_div", C.c_int32 * 4),
                ("scale2_const", C.c_float),
                ("mode", C.c_int32), ("lo1", C.c_int32), ("hi1", C.c_int32), ("lo2", C.c_int32), ("hi2", C.c_int32),
                ("qmax", C.c_int32), ("reserved", C.c_int32)]


class GroupJob(C.Structure):
    """p4v_group_job: one member of a p4v_calibrate_group call (= one p4v_*_calibrate call)."""
    _fields_ = [("kind", C.c_int32), ("status", C.c_int32), ("desc", C.c_void_p), ("inp", C.c_void_p * 5), ("mult", C.c_void_p),
                ("out", C.c_void_p * 3), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


JOB_LINEAR, JOB_MATMUL, JOB_CONV, JOB_MATMUL_BLOCKS = 0, 1, 2, 3
# bits of a descriptor's `reserved` word (include/ptq4vit_hip.h documents which descriptor reads which)
RESERVED_FP32_PLANES, RESERVED_NO_MEMO, RESERVED_FORWARD_ONLY, RESERVED_NO_PRUNE = 1, 2, 4, 8
RESERVED_BLOCK_SHIFT = 8     # bits 8..11 (p4v_linear_search_w / _a): 1 + b runs the step of block b alone


def reserved_block(block):
    """The block field of `reserved`: 0 (every block in turn) for None, else 1 + block."""
    return 0 if block is None else (int(block) + 1) << RESERVED_BLOCK_SHIFT


PLANE_SYM, PLANE_SOS_HI, PLANE_SOS_LO, PLANE_TWIN = 1, 2, 3, 4
EXPORT_SYM_I8, EXPORT_SYM_F32, EXPORT_GELU_U8, EXPORT_SOS_U8 = 0, 1, 2, 3


EXPORTS = [
    "p4v_version", "p4v_last_error",
    "p4v_linear_workspace_bytes", "p4v_linear_calibrate",
    "p4v_matmul_workspace_bytes", "p4v_matmul_calibrate",
    "p4v_matmul_blocks_workspace_bytes", "p4v_matmul_blocks_calibrate", "p4v_amax_init_matmul_blocks",
    "p4v_matmul_blocks_search", "p4v_matmul_blocks_quant_forward",
    "p4v_conv_workspace_bytes", "p4v_conv_calibrate",
    "p4v_calibrate_group", "p4v_launch_counters",
    "p4v_linear_quant_forward", "p4v_matmul_quant_forward", "p4v_mlp_workspace_bytes", "p4v_mlp_quant_forward",
    "p4v_attn_workspace_bytes", "p4v_attn_quant_forward", "p4v_wattn_workspace_bytes", "p4v_wattn_quant_forward",
    "p4v_qkv_attn_workspace_bytes", "p4v_qkv_attn_quant_forward",
    "p4v_amax_init_linear", "p4v_linear_search_w", "p4v_linear_search_a",
    "p4v_amax_init_matmul", "p4v_matmul_search_A", "p4v_sos_search_split", "p4v_matmul_search_B",
    "p4v_amax_init_conv", "p4v_conv_search_w_channelwise", "p4v_conv_search_w_layerwise", "p4v_conv_search_a",
    "p4v_score_argmax_gather",
    "p4v_quantize_i8", "p4v_pack_plane_i8", "p4v_fake_quant", "p4v_export_quantize", "p4v_multi_copy",
    "p4v_stats_enable", "p4v_stats_reset", "p4v_stats_get", "p4v_stats_launches", "p4v_prune_counters",
    "p4v_debug_set_variant", "p4v_debug_set_tuning", "p4v_debug_bound_totals", "p4v_debug_topk_rows", "p4v_debug_pack_dual", "p4v_debug_prep_epi6",
    "p4v_debug_pack_cands", "p4v_debug_gather_im2col", "p4v_debug_sos_sweep",
    "p4v_debug_set_arena_gap", "p4v_debug_arena_ranges", "p4v_debug_mlp_planes", "p4v_debug_attn_planes", "p4v_debug_qkv_planes",
    "p4v_debug_prune_tables", "p4v_debug_prune_decide",
]

_lib = None


def load():
    """Load libptq4vit_hip.so (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"ptq4vit_amd: HIP extension {LIB_PATH} is missing -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the calibration path.")
    # torch ships its own libamdhip64 (same soname as /opt/rocm's).  Import torch FIRST so that this library
    # binds to the HIP runtime torch already initialised: two runtimes in one process cannot both own the GPU.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, fp, ip = C.c_void_p, C.c_void_p, C.c_void_p
    lib.p4v_version.restype = C.c_int
    lib.p4v_last_error.restype = C.c_char_p
    lib.p4v_linear_workspace_bytes.restype = C.c_size_t
    lib.p4v_linear_workspace_bytes.argtypes = [C.POINTER(LinearDesc)]
    lib.p4v_linear_calibrate.restype = C.c_int
    lib.p4v_linear_calibrate.argtypes = [C.POINTER(LinearDesc), fp, fp, fp, fp, fp, fp, fp, fp, fp, ip, vp, C.c_size_t, vp]
    lib.p4v_matmul_workspace_bytes.restype = C.c_size_t
    lib.p4v_matmul_workspace_bytes.argtypes = [C.POINTER(MatMulDesc)]
    lib.p4v_matmul_calibrate.restype = C.c_int
    lib.p4v_matmul_calibrate.argtypes = [C.POINTER(MatMulDesc), fp, fp, fp, fp, fp, fp, fp, fp, fp, ip, vp, C.c_size_t, vp]
    MBD = C.POINTER(MatMulBlocksDesc)
    lib.p4v_matmul_blocks_workspace_bytes.restype = C.c_size_t
    lib.p4v_matmul_blocks_workspace_bytes.argtypes = [MBD]
    lib.p4v_matmul_blocks_calibrate.restype = C.c_int
    lib.p4v_matmul_blocks_calibrate.argtypes = [MBD, fp, fp, fp, fp, fp, fp, fp, fp, fp, ip, vp, C.c_size_t, vp]
    lib.p4v_amax_init_matmul_blocks.restype = C.c_int
    lib.p4v_amax_init_matmul_blocks.argtypes = [MBD, fp, fp, fp, fp, vp, C.c_size_t, vp]
    lib.p4v_matmul_blocks_search.restype = C.c_int
    lib.p4v_matmul_blocks_search.argtypes = [MBD, C.c_int32, C.c_int32, C.c_int32] + [fp] * 9 + [ip, vp, C.c_size_t, vp]
    lib.p4v_matmul_blocks_quant_forward.restype = C.c_int
    lib.p4v_matmul_blocks_quant_forward.argtypes = [MBD, fp, fp, fp, fp, fp, fp, vp, C.c_size_t, vp]
    lib.p4v_conv_workspace_bytes.restype = C.c_size_t
    lib.p4v_conv_workspace_bytes.argtypes = [C.POINTER(ConvDesc)]
    lib.p4v_conv_calibrate.restype = C.c_int
    lib.p4v_conv_calibrate.argtypes = [C.POINTER(ConvDesc), fp, fp, fp, fp, fp, fp, fp, fp, fp, ip, vp, C.c_size_t, vp]
    lib.p4v_linear_quant_forward.restype = C.c_int
    lib.p4v_linear_quant_forward.argtypes = [C.POINTER(LinearDesc), fp, fp, fp, fp, fp, fp, vp, C.c_size_t, vp]
    lib.p4v_mlp_workspace_bytes.restype = C.c_size_t
    lib.p4v_mlp_workspace_bytes.argtypes = [C.POINTER(MlpDesc)]
    lib.p4v_mlp_quant_forward.restype = C.c_int
    lib.p4v_mlp_quant_forward.argtypes = [C.POINTER(MlpDesc)] + [fp] * 11 + [vp, C.c_size_t, vp]
    lib.p4v_debug_mlp_planes.restype = C.c_int
    lib.p4v_debug_mlp_planes.argtypes = [C.POINTER(C.c_uint64)]
    lib.p4v_attn_workspace_bytes.restype = C.c_size_t
    lib.p4v_attn_workspace_bytes.argtypes = [C.POINTER(AttnDesc)]
    lib.p4v_attn_quant_forward.restype = C.c_int
    lib.p4v_attn_quant_forward.argtypes = [C.POINTER(AttnDesc)] + [fp] * 10 + [vp, C.c_size_t, vp]
    lib.p4v_wattn_workspace_bytes.restype = C.c_size_t
    lib.p4v_wattn_workspace_bytes.argtypes = [C.POINTER(WattnDesc)]
    lib.p4v_wattn_quant_forward.restype = C.c_int
    lib.p4v_wattn_quant_forward.argtypes = [C.POINTER(WattnDesc), C.POINTER(WattnTensors), vp]
    lib.p4v_debug_attn_planes.restype = C.c_int
    lib.p4v_debug_attn_planes.argtypes = [C.POINTER(C.c_uint64)]
    lib.p4v_qkv_attn_workspace_bytes.restype = C.c_size_t
    lib.p4v_qkv_attn_workspace_bytes.argtypes = [C.POINTER(QkvAttnDesc)]
    lib.p4v_qkv_attn_quant_forward.restype = C.c_int
    lib.p4v_qkv_attn_quant_forward.argtypes = [C.POINTER(QkvAttnDesc), C.POINTER(QkvAttnTensors), vp]
    lib.p4v_debug_qkv_planes.restype = C.c_int
    lib.p4v_debug_qkv_planes.argtypes = [C.POINTER(C.c_uint64)]
    lib.p4v_matmul_quant_forward.restype = C.c_int
    lib.p4v_matmul_quant_forward.argtypes = [C.POINTER(MatMulDesc), fp, fp, fp, fp, fp, fp, vp, C.c_size_t, vp]
    # granular entry points: (desc, tensors..., workspace, bytes, stream)
    LD, MD, CD = C.POINTER(LinearDesc), C.POINTER(MatMulDesc), C.POINTER(ConvDesc)
    tail = [vp, C.c_size_t, vp]
    for name, args in (
            ("p4v_amax_init_linear", [LD] + [fp] * 4),
            ("p4v_linear_search_w", [LD] + [fp] * 9 + [ip]),
            ("p4v_linear_search_a", [LD] + [fp] * 9 + [ip]),
            ("p4v_amax_init_matmul", [MD] + [fp] * 4),
            ("p4v_matmul_search_A", [MD] + [fp] * 8 + [ip]),
            ("p4v_sos_search_split", [MD] + [fp] * 7 + [ip]),
            ("p4v_matmul_search_B", [MD] + [fp] * 9 + [ip]),
            ("p4v_amax_init_conv", [CD] + [fp] * 4),
            ("p4v_conv_search_w_channelwise", [CD] + [fp] * 9 + [ip]),
            ("p4v_conv_search_w_layerwise", [CD] + [fp] * 9 + [ip]),
            ("p4v_conv_search_a", [CD] + [fp] * 9 + [ip])):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args + tail
    lib.p4v_score_argmax_gather.restype = C.c_int
    lib.p4v_score_argmax_gather.argtypes = [fp, C.c_int32, C.c_int32, fp, fp, ip, vp]
    lib.p4v_quantize_i8.restype = C.c_int
    lib.p4v_quantize_i8.argtypes = [fp, C.c_int64, C.c_int64, C.c_int64, fp, C.c_int64, C.c_int32, C.c_int32, vp, vp]
    lib.p4v_fake_quant.restype = C.c_int
    lib.p4v_fake_quant.argtypes = [fp, C.c_int64, C.c_int64, fp, C.c_int64, C.c_int32, C.c_int32, fp, vp]
    lib.p4v_pack_plane_i8.restype = C.c_int
    lib.p4v_pack_plane_i8.argtypes = [C.POINTER(PlaneDesc), fp, fp, vp, vp]
    lib.p4v_export_quantize.restype = C.c_int
    lib.p4v_export_quantize.argtypes = [C.POINTER(ExportDesc), fp, fp, fp, vp, vp]
    lib.p4v_multi_copy.restype = C.c_int
    lib.p4v_multi_copy.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, vp]
    lib.p4v_debug_topk_rows.restype = C.c_int
    lib.p4v_debug_topk_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.p4v_debug_pack_dual.restype = C.c_int
    lib.p4v_debug_pack_dual.argtypes = [fp, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_float, vp, vp, vp]
    lib.p4v_debug_pack_cands.restype = C.c_int
    lib.p4v_debug_pack_cands.argtypes = [fp, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, fp, C.c_int, vp, vp,
                                         C.c_int, C.c_int, vp, vp]
    lib.p4v_debug_gather_im2col.restype = C.c_int
    lib.p4v_debug_gather_im2col.argtypes = [C.c_int] * 12 + [fp, ip, C.c_int, fp, vp]
    lib.p4v_debug_sos_sweep.restype = C.c_int
    lib.p4v_debug_sos_sweep.argtypes = [C.POINTER(MatMulDesc), fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, vp, C.c_size_t, vp]
    lib.p4v_debug_prep_epi6.restype = C.c_int
    lib.p4v_debug_prep_epi6.argtypes = [fp, fp, fp, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, vp]
    lib.p4v_debug_set_variant.restype = C.c_int
    lib.p4v_debug_set_variant.argtypes = [C.c_int, C.c_int]
    lib.p4v_debug_set_tuning.restype = C.c_int
    lib.p4v_debug_set_tuning.argtypes = [C.c_int, C.c_int]
    lib.p4v_debug_set_arena_gap.restype = C.c_int
    lib.p4v_debug_set_arena_gap.argtypes = [C.c_size_t]
    lib.p4v_debug_arena_ranges.restype = C.c_int
    lib.p4v_debug_arena_ranges.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    lib.p4v_debug_bound_totals.restype = C.c_int
    lib.p4v_debug_bound_totals.argtypes = [fp, C.c_int64, C.POINTER(C.c_int64)]
    lib.p4v_debug_prune_tables.restype = C.c_int
    lib.p4v_debug_prune_tables.argtypes = [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
    lib.p4v_debug_prune_decide.restype = C.c_int
    lib.p4v_debug_prune_decide.argtypes = [fp, fp, fp, fp] + [C.c_int] * 5 + [ip, ip, ip, fp, ip, C.POINTER(C.c_int32), vp]
    lib.p4v_stats_enable.restype = C.c_int
    lib.p4v_stats_enable.argtypes = [C.c_int]
    lib.p4v_stats_reset.restype = C.c_int
    lib.p4v_stats_get.restype = C.c_int
    lib.p4v_stats_get.argtypes = [C.POINTER(KernelStats)]
    lib.p4v_stats_launches.restype = C.c_int
    lib.p4v_stats_launches.argtypes = [C.POINTER(LaunchRecord), C.c_int64, C.POINTER(C.c_int64)]
    lib.p4v_prune_counters.restype = C.c_int
    lib.p4v_prune_counters.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.p4v_launch_counters.restype = C.c_int
    lib.p4v_launch_counters.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.p4v_calibrate_group.restype = C.c_int
    lib.p4v_calibrate_group.argtypes = [C.POINTER(GroupJob), C.c_int32, vp, vp]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().p4v_last_error().decode("utf-8", "replace")
        if rc == -2:
            raise NotImplementedError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def source_hash():
    """Short hash of the engine's sources (kernels, host side of the C ABI, the header): profiles committed under profiles/ carry
    it, and bench.py only quotes a profile's PMC traffic when it was measured on THIS code."""
    import hashlib
    root = os.path.dirname(os.path.abspath(__file__))
    h = hashlib.sha256()
    for rel in ("csrc/p4v_kernels.h", "csrc/p4v_api.hip", "../include/ptq4vit_hip.h"):
        with open(os.path.join(root, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]
