"""mopro_msm_hip -- Python host-side mirror of the reference's MSM operator interface, over the
C ABI of libmsm_hip.so (include/msm_hip.h).

Reference surface mirrored (mopro-msm/src/msm/metal_msm/metal_msm.rs):
  metal_variable_base_msm(&bases, &scalars) -> Result<G1Projective, Box<dyn Error>>   :642-695
      * empty input            -> Err("Empty input")                                   :647-649
      * unequal lengths        -> silently truncated to the shorter one                :652-656
  test_utils::generate_random_bases_and_scalars(size)                                  :698-731
The Rust shim a maintainer would add is in rust/mopro-msm-hip; this module is the
same thin layer for Python callers, tests and bench.py.  It holds no arithmetic: every result comes
from the HIP library, and importing/using it without the built library or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSM_HIP_LIB overrides the in-tree library (A/B runs of two builds: tools/sweep_env.py MSM_HIP_LIB a.so b.so)
LIB_PATH = os.environ.get("MSM_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libmsm_hip.so")

FORM_STD, FORM_MONT = 0, 1
FLAG_UNSIGNED_DIGITS = 1
FLAG_NO_GLV = 2
FLAG_WINDOW_TABLE = 4  # resident sets carry their window table
FLAG_DETERMINISTIC = 8  # jacobian_mont is the canonical Z = 1 representative: the same 24 words for the same group element (ABI 6)
NTT_INVERSE, NTT_IN_MONT, NTT_OUT_MONT = 1, 2, 4  # MSM_NTT_*: inverse transform (1/n included) / input words are arkworks Fr.0 / output words likewise
R1CS_COEF_STD, R1CS_COEF_MONT, R1CS_COEF_MONT2 = 0, 1, 2  # MSM_R1CS_COEF_*: a coefficient's words are c / c * 2^256 (arkworks Fr.0) / c * 2^512 (a snarkjs zkey's section 4)
R1CS_C_FROM_AB = 8  # MSM_R1CS_C_FROM_AB: the eval writes c[i] = a[i] * b[i] instead of (matrix 2) * w
FB_OUT_STD = 8  # MSM_FB_OUT_STD: the fixed-base products come out in standard form (default: arkworks Montgomery words); NTT_IN_MONT is honoured too
PM_BASES_STD = 16  # MSM_PM_BASES_STD: the bases of the element-wise multiplication are standard-form integers (default: arkworks Montgomery words)
FR_SCAN_EXCLUSIVE = 32  # MSM_FR_SCAN_EXCLUSIVE: the running product starts at 1 and leaves the last element out (Z as PLONK stores it)
G2_CHECK_CURVE, G2_CHECK_SUBGROUP = 1, 2  # MSM_G2_CHECK_*: coordinates < p and on the twist / [r]P = O (implies the curve check)
OK, ERR_EMPTY, ERR_BAD_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_STATE, ERR_INVALID_DATA = 0, -1, -2, -3, -4, -5, -6, -7

# every symbol include/msm_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "msm_abi_version", "msm_ctx_create", "msm_ctx_destroy", "msm_last_error", "msm_bn254_g1",
    "msm_bn254_g1_arkworks", "msm_bn254_g1_upload_bases", "msm_bn254_g1_resident", "msm_bn254_g1_resident_batch", "msm_tune_batch", "msm_bn254_g1_resident_device", "msm_bn254_g1_device",
    "msm_bn254_g1_combine", "msm_bn254_g1_combine_flags", "msm_get_timings_sized", "msm_multi_get_timings_sized", "msm_multi_get_clock_stats", "msm_multi_set_kernel_timing",
    "msm_plan", "msm_get_timings", "msm_set_stage_timing", "msm_set_kernel_timing", "msm_get_accumulate_kernel_stats", "msm_reset_kernel_stats", "msm_get_clock_stats",
    "msm_bn254_g1_decompress", "msm_bn254_g1_upload_compressed", "msm_bn254_g1_compress",
    "msm_multi_create", "msm_multi_destroy", "msm_multi_last_error", "msm_multi_num_devices", "msm_multi_exchange",
    "msm_bn254_g1_multi", "msm_bn254_g1_multi_arkworks", "msm_bn254_g1_multi_device", "msm_multi_get_timings",
    "msm_multi_get_exchange_stats", "msm_multi_get_exchange_probe",
    "msm_bn254_g2", "msm_bn254_g2_device", "msm_bn254_g2_combine",
    "msm_bn254_g2_compress", "msm_bn254_g2_decompress", "msm_bn254_g2_decompress_device", "msm_bn254_g2_validate", "msm_bn254_g2_validate_device",
    "msm_bn254_g1_validate",
    "msm_bn254_fr_root_of_unity", "msm_bn254_fr_ntt_plan", "msm_bn254_fr_ntt_device", "msm_bn254_fr_ntt", "msm_bn254_fr_mul_sub_scale_device",
    "msm_bn254_fr_r1cs_plan", "msm_bn254_fr_r1cs_upload", "msm_bn254_fr_r1cs_info", "msm_bn254_fr_r1cs_eval_device", "msm_bn254_fr_r1cs_eval",
    "msm_bn254_g1_fixed_base_plan", "msm_bn254_g1_fixed_base_mul_device", "msm_bn254_g1_fixed_base_mul",
    "msm_bn254_g2_fixed_base_plan", "msm_bn254_g2_fixed_base_mul_device", "msm_bn254_g2_fixed_base_mul",
    "msm_bn254_fr_vector_plan", "msm_bn254_fr_powers_device", "msm_bn254_fr_batch_inverse_device", "msm_bn254_fr_batch_inverse",
    "msm_bn254_fr_lagrange_device", "msm_bn254_fr_lincomb_device",
    "msm_bn254_fr_scan_plan", "msm_bn254_fr_poly_eval_device", "msm_bn254_fr_poly_div_linear_device", "msm_bn254_fr_poly_div_linear",
    "msm_bn254_fr_running_product_device",
    "msm_bn254_g1_pointwise_mul_plan", "msm_bn254_g1_pointwise_mul_device", "msm_bn254_g1_scale_device", "msm_bn254_g1_pointwise_mul",
    "msm_bn254_g1_fft_plan", "msm_bn254_g1_fft_device", "msm_bn254_g1_fft",
    "msm_bn254_g2_pointwise_mul_plan", "msm_bn254_g2_pointwise_mul_device", "msm_bn254_g2_scale_device", "msm_bn254_g2_pointwise_mul",
    "msm_bn254_g2_fft_plan", "msm_bn254_g2_fft_device", "msm_bn254_g2_fft",
]
ABI_VERSION = 7  # == MSM_HIP_ABI_VERSION of include/msm_hip.h this binding was written against (checked when a library is loaded)
ERR_RCCL = -8
EXCHANGE_AUTO, EXCHANGE_RCCL, EXCHANGE_HOST = 0, 1, 2
# msm_config_t.batch_layout (include/msm_hip.h MSM_BATCH_LAYOUT_*)
BATCH_LAYOUT_AUTO, BATCH_LAYOUT_ONE_STREAM, BATCH_LAYOUT_ONE_STREAM_REDUCE, BATCH_LAYOUT_TWO_STREAMS = 0, 1, 2, 3


class MsmError(RuntimeError):
    """Counterpart of the reference's Box<dyn Error>; .code is the C-ABI status."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("window_bits", C.c_uint32), ("flags", C.c_uint32),
                ("stream_chunk_log2", C.c_uint32), ("max_points", C.c_uint64), ("batch_layout", C.c_uint32), ("host_threads", C.c_uint32)]


class Plan(C.Structure):
    _fields_ = [("window_bits", C.c_uint32), ("num_windows", C.c_uint32), ("num_buckets", C.c_uint32),
                ("signed_digits", C.c_uint32), ("workspace_bytes", C.c_uint64), ("virtual_points", C.c_uint64),
                ("glv", C.c_uint32), ("scalar_bits", C.c_uint32), ("table_factor", C.c_uint32), ("bucket_arrays", C.c_uint32),
                ("table_bytes", C.c_uint64), ("top_digit_bits", C.c_uint32), ("reserved", C.c_uint32)]


class Timings(C.Structure):
    _fields_ = [("h2d_ms", C.c_float), ("convert_ms", C.c_float), ("decompose_ms", C.c_float),
                ("sort_ms", C.c_float), ("accumulate_ms", C.c_float), ("reduce_ms", C.c_float),
                ("finish_ms", C.c_float), ("total_ms", C.c_float), ("num_points", C.c_uint64),
                ("num_adds", C.c_uint64), ("stream_chunks", C.c_uint32), ("batch_layout", C.c_uint32),
                ("plan_ms", C.c_float), ("combine_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class R1csInfo(C.Structure):
    """msm_r1cs_info_t: what an upload of constraint matrices builds"""
    _fields_ = [("entries", C.c_uint64 * 3), ("rows_with_entries", C.c_uint64 * 3), ("longest_row", C.c_uint64), ("plus_one", C.c_uint64),
                ("minus_one", C.c_uint64), ("distinct_values", C.c_uint64), ("work_items", C.c_uint64), ("max_item_len", C.c_uint64),
                ("fold_rows", C.c_uint64), ("partial_sums", C.c_uint64), ("device_bytes", C.c_uint64), ("build_ms", C.c_double),
                ("upload_ms", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("entries", "rows_with_entries") else getattr(self, k)) for k, _ in self._fields_}


class FixedBasePlan(C.Structure):
    """msm_fixed_base_plan_t: the window table and the inversion group of a fixed-base multiplication"""
    _fields_ = [("window_bits", C.c_uint32), ("num_windows", C.c_uint32), ("table_entries", C.c_uint64), ("table_bytes", C.c_uint64),
                ("inv_group", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class FixedBaseG2Plan(C.Structure):
    """msm_fixed_base_g2_plan_t: the window table, the inversion group and the scratch array of a G2 fixed-base multiplication"""
    _fields_ = [("window_bits", C.c_uint32), ("num_windows", C.c_uint32), ("table_entries", C.c_uint64), ("table_bytes", C.c_uint64),
                ("inv_group", C.c_uint32), ("chunk_points", C.c_uint32), ("scratch_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrVectorPlan(C.Structure):
    """msm_fr_vector_plan_t: the inversion group and the elements a workgroup covers in the scalar-vector calls"""
    _fields_ = [("inv_group", C.c_uint32), ("block_points", C.c_uint32), ("powers_block_points", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class FrScanPlan(C.Structure):
    """msm_fr_scan_plan_t: the chain of a lane, the elements of a workgroup, the launches and the scratch bytes of a scalar-field scan"""
    _fields_ = [("chain", C.c_uint32), ("block_points", C.c_uint32), ("eval_launches", C.c_uint32), ("div_launches", C.c_uint32),
                ("blocks", C.c_uint64), ("scratch_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PointwisePlan(C.Structure):
    """msm_pointwise_plan_t: the inversion group, the ladder's positions and the points a lane keeps of an element-wise multiplication"""
    _fields_ = [("inv_group", C.c_uint32), ("ladder_bits", C.c_uint32), ("table_points", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


G2PointwisePlan = PointwisePlan  # msm_pointwise_g2_plan_t: the same three figures for the G2 element-wise multiplication


class G1FftPlan(C.Structure):
    """msm_g1_fft_plan_t: the stages of a G1 group transform, those that run a ladder, the inversion group and the bytes of its twiddle table"""
    _fields_ = [("stages", C.c_uint16), ("ladder_stages", C.c_uint16), ("inv_group", C.c_uint32), ("table_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


G2FftPlan = G1FftPlan  # msm_g2_fft_plan_t: the same four fields for the G2 group transform (one twiddle table serves both groups)


# msm_r1cs_coef_t: matrix, row, col, 8 value words -- 44 bytes, the layout of one entry of a zkey's coefficient section
R1CS_COEF_DTYPE = np.dtype([("matrix", "<u4"), ("row", "<u4"), ("col", "<u4"), ("value", "<u4", (8,))])

_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_lib = None


def _preload_torch():
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64 and the
    # library links the same soname from /opt/rocm.  Whichever is loaded first serves both, and loading
    # ours first leaves torch with a mixed runtime ("No HIP GPUs are available").  Python callers use torch
    # for device memory and torch.distributed, so let torch bring in its runtime before we dlopen.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def bind_product_abi(L):
    """ctypes signatures of every include/msm_hip.h entry point on a loaded library (product or hooks build)"""
    vp = C.c_void_p
    L.msm_abi_version.restype = C.c_uint32
    L.msm_ctx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.msm_ctx_destroy.argtypes = [vp]
    L.msm_ctx_destroy.restype = None
    L.msm_last_error.argtypes = [vp]
    L.msm_last_error.restype = C.c_char_p
    L.msm_bn254_g1.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_arkworks.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_upload_bases.argtypes = [vp, _u32p, C.c_uint32, _u8p, C.c_size_t]
    L.msm_bn254_g1_resident.argtypes = [vp, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_resident_batch.argtypes = [vp, C.POINTER(_u32p), C.c_size_t, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_tune_batch.argtypes = [vp, C.POINTER(_u32p), C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.msm_bn254_g1_device.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_resident_device.argtypes = [vp, vp, C.c_size_t, vp, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_combine.argtypes = [_u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_combine_flags.argtypes = [_u32p, C.c_size_t, C.c_uint32, _u32p, _u32p, _u8p]
    L.msm_get_timings_sized.argtypes = [vp, vp, C.c_size_t]
    L.msm_multi_get_timings_sized.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    L.msm_multi_set_kernel_timing.argtypes = [vp, C.c_uint32]
    L.msm_multi_get_clock_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.msm_plan.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(Plan)]
    L.msm_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.msm_set_stage_timing.argtypes = [vp, C.c_int32]
    L.msm_set_kernel_timing.argtypes = [vp, C.c_uint32]
    L.msm_get_accumulate_kernel_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.msm_reset_kernel_stats.argtypes = [vp]
    L.msm_reset_kernel_stats.restype = None
    L.msm_get_clock_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.msm_bn254_g1_decompress.argtypes = [vp, _u8p, C.c_size_t, _u32p, _u8p, C.POINTER(C.c_int64)]
    L.msm_bn254_g1_upload_compressed.argtypes = [vp, _u8p, C.c_size_t, C.POINTER(C.c_int64)]
    L.msm_bn254_g1_compress.argtypes = [_u32p, C.c_uint32, _u8p, C.c_size_t, _u8p]
    L.msm_multi_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(Config), C.c_uint32, C.POINTER(vp)]
    L.msm_multi_destroy.argtypes = [vp]
    L.msm_multi_destroy.restype = None
    L.msm_multi_last_error.argtypes = [vp]
    L.msm_multi_last_error.restype = C.c_char_p
    L.msm_multi_num_devices.argtypes = [vp]
    L.msm_multi_exchange.argtypes = [vp]
    L.msm_multi_exchange.restype = C.c_uint32
    L.msm_bn254_g1_multi.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_multi_arkworks.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g1_multi_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), _u32p, _u32p, _u8p]
    L.msm_multi_get_timings.argtypes = [vp, C.c_int32, C.POINTER(Timings)]
    L.msm_multi_get_exchange_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32]
    L.msm_multi_get_exchange_probe.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.msm_bn254_g2.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, _u32p, _u32p, _u8p]
    L.msm_bn254_g2_device.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, _u32p, _u32p, _u8p]
    L.msm_bn254_g2_combine.argtypes = [_u32p, C.c_size_t, C.c_uint32, _u32p, _u32p, _u8p]
    i64p = C.POINTER(C.c_int64)
    L.msm_bn254_g2_compress.argtypes = [_u32p, C.c_uint32, _u8p, C.c_size_t, _u8p]
    L.msm_bn254_g2_decompress.argtypes = [vp, _u8p, C.c_size_t, C.c_uint32, _u32p, _u8p, i64p]
    L.msm_bn254_g2_decompress_device.argtypes = [vp, _u8p, C.c_size_t, C.c_uint32, vp, vp, vp, i64p]
    L.msm_bn254_g2_validate.argtypes = [vp, _u32p, C.c_uint32, _u8p, C.c_size_t, C.c_uint32, i64p]
    L.msm_bn254_g2_validate_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, i64p]
    L.msm_bn254_g1_validate.argtypes = [vp, _u32p, C.c_uint32, _u8p, C.c_size_t, i64p]
    L.msm_bn254_fr_root_of_unity.argtypes = [C.c_uint32, _u32p]
    L.msm_bn254_fr_ntt_plan.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), _u32p]
    L.msm_bn254_fr_ntt_device.argtypes = [vp, vp, C.c_uint32, C.c_size_t, C.c_uint32, _u32p, vp]
    L.msm_bn254_fr_ntt.argtypes = [vp, _u32p, _u32p, C.c_uint32, C.c_size_t, C.c_uint32, _u32p]
    L.msm_bn254_fr_mul_sub_scale_device.argtypes = [vp, vp, vp, vp, _u32p, vp, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_fr_r1cs_plan.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(R1csInfo)]
    L.msm_bn254_fr_r1cs_upload.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.msm_bn254_fr_r1cs_info.argtypes = [vp, C.POINTER(R1csInfo)]
    L.msm_bn254_fr_r1cs_eval_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp]
    L.msm_bn254_fr_r1cs_eval.argtypes = [vp, _u32p, C.c_size_t, _u32p, C.c_uint32]
    L.msm_bn254_g1_fixed_base_plan.argtypes = [C.c_uint32, C.POINTER(FixedBasePlan)]
    L.msm_bn254_g1_fixed_base_mul_device.argtypes = [vp, _u32p, C.c_uint32, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g1_fixed_base_mul.argtypes = [vp, _u32p, C.c_uint32, _u32p, C.c_size_t, C.c_uint32, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_g2_fixed_base_plan.argtypes = [C.c_uint32, C.POINTER(FixedBaseG2Plan)]
    L.msm_bn254_g2_fixed_base_mul_device.argtypes = [vp, _u32p, C.c_uint32, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g2_fixed_base_mul.argtypes = [vp, _u32p, C.c_uint32, _u32p, C.c_size_t, C.c_uint32, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_g1_pointwise_mul_plan.argtypes = [C.POINTER(PointwisePlan)]
    L.msm_bn254_g1_pointwise_mul_device.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g1_scale_device.argtypes = [vp, vp, vp, _u32p, C.c_size_t, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g1_pointwise_mul.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_g2_pointwise_mul_plan.argtypes = [C.POINTER(G2PointwisePlan)]
    L.msm_bn254_g2_pointwise_mul_device.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g2_scale_device.argtypes = [vp, vp, vp, _u32p, C.c_size_t, C.c_uint32, vp, vp, vp]
    L.msm_bn254_g2_pointwise_mul.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_g1_fft_plan.argtypes = [C.c_uint32, C.POINTER(G1FftPlan)]
    L.msm_bn254_g1_fft_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_g1_fft.argtypes = [vp, _u32p, C.c_uint32, _u8p, C.c_uint32, C.c_size_t, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_g2_fft_plan.argtypes = [C.c_uint32, C.POINTER(G2FftPlan)]
    L.msm_bn254_g2_fft_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_g2_fft.argtypes = [vp, _u32p, C.c_uint32, _u8p, C.c_uint32, C.c_size_t, C.c_uint32, _u32p, _u8p]
    L.msm_bn254_fr_vector_plan.argtypes = [C.POINTER(FrVectorPlan)]
    L.msm_bn254_fr_powers_device.argtypes = [vp, _u32p, _u32p, C.c_uint64, vp, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_fr_batch_inverse_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_fr_batch_inverse.argtypes = [vp, _u32p, _u32p, C.c_size_t, C.c_uint32]
    L.msm_bn254_fr_lagrange_device.argtypes = [vp, _u32p, C.c_uint32, vp, C.c_uint32, vp]
    L.msm_bn254_fr_lincomb_device.argtypes = [vp, vp, _u32p, vp, _u32p, vp, _u32p, vp, C.c_size_t, C.c_uint32, vp]
    L.msm_bn254_fr_scan_plan.argtypes = [C.c_size_t, C.POINTER(FrScanPlan)]
    L.msm_bn254_fr_poly_eval_device.argtypes = [vp, vp, C.c_size_t, _u32p, vp, C.c_uint32, vp]
    L.msm_bn254_fr_poly_div_linear_device.argtypes = [vp, vp, C.c_size_t, _u32p, vp, vp, C.c_uint32, vp]
    L.msm_bn254_fr_poly_div_linear.argtypes = [vp, _u32p, C.c_size_t, _u32p, _u32p, _u32p, C.c_uint32]
    L.msm_bn254_fr_running_product_device.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_uint32, vp]
    for name in ABI_SYMBOLS:
        f = getattr(L, name)
        if f.restype is C.c_int:  # default
            f.restype = C.c_int32
    # the structs above (Config, Plan, Timings) are those of ONE ABI: a library of another would be read / written past their ends
    have = int(L.msm_abi_version())
    if have != ABI_VERSION:
        raise MsmError(ERR_STATE, "library ABI %d, this binding is written against ABI %d (rebuild: make -C gpu-acceleration_amd/csrc)" % (have, ABI_VERSION))
    return L


def load_library():
    """dlopen the in-tree libmsm_hip.so (the PRODUCT); fails loudly if it was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MsmError(ERR_NO_DEVICE, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                      "(make -C gpu-acceleration_amd/csrc); there is no CPU fallback")
    _preload_torch()
    _lib = bind_product_abi(C.CDLL(LIB_PATH))
    return _lib


def _words(a, width):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a.reshape(-1, width)


def _p32(a):
    return a.ctypes.data_as(_u32p) if a is not None else None


class MsmResult:
    """One G1 result: Jacobian Montgomery words (what the Rust shim turns into G1Projective via
    Fq::new_unchecked, metal_msm.rs:228-241) and the canonical affine standard-form words."""

    def __init__(self, jac, aff, inf):
        self.jacobian_mont = jac
        self._aff = aff
        self.is_infinity = bool(inf)

    @property
    def affine_std(self):
        """canonical affine standard-form words; computed on first use (one field inversion on the host) when the call
        returned only the Jacobian point -- the reference's own result type (metal_msm.rs:228-241)"""
        if self._aff is None:
            self._aff = combine_partials(self.jacobian_mont.reshape(1, 24))._aff
        return self._aff

    def affine_ints(self):
        if self.is_infinity:
            return None
        to_int = lambda ws: sum(int(w) << (32 * i) for i, w in enumerate(ws.tolist()))
        return to_int(self.affine_std[:8]), to_int(self.affine_std[8:])


class G2Result:
    """One G2 result: Jacobian Montgomery words X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1 (48) and the canonical affine standard-form words
    x.c0 x.c1 y.c0 y.c1 (32)."""

    def __init__(self, jac, aff, inf):
        self.jacobian_mont = jac
        self._aff = aff
        self.is_infinity = bool(inf)

    @property
    def affine_std(self):
        if self._aff is None:
            self._aff = combine_partials_g2(self.jacobian_mont.reshape(1, 48))._aff
        return self._aff

    def affine_ints(self):
        """((x.c0, x.c1), (y.c0, y.c1)) as Python integers, None for the identity"""
        if self.is_infinity:
            return None
        w = [sum(int(v) << (32 * i) for i, v in enumerate(self.affine_std[8 * k:8 * k + 8].tolist())) for k in range(4)]
        return (w[0], w[1]), (w[2], w[3])


def combine_partials_g2(partials_jacobian_mont, want_affine=True, flags=0):
    """Fold G2 partial sums (k x 48 Jacobian Montgomery words) in order on the host (msm_bn254_g2_combine); flags 0 or FLAG_DETERMINISTIC."""
    p = _words(partials_jacobian_mont, 48)
    jac, aff, inf = np.zeros(48, np.uint32), (np.zeros(32, np.uint32) if want_affine else None), C.c_uint8(0)
    rc = load_library().msm_bn254_g2_combine(_p32(p), p.shape[0], flags, _p32(jac), _p32(aff), C.byref(inf))
    if rc != OK:
        raise MsmError(rc, "Empty input" if rc == ERR_EMPTY else f"G2 combine failed ({rc})")
    return G2Result(jac, aff, inf.value)


def plan(n, window_bits=0, flags=0, _lib=None):
    p = Plan()
    rc = (_lib or load_library()).msm_plan(n, window_bits, flags, C.byref(p))
    if rc != OK:
        raise MsmError(rc, "Empty input" if rc == ERR_EMPTY else f"msm_plan failed ({rc})")
    return p


def _fr_words(v):
    """a scalar-field element for the C ABI: None stays None, an int becomes its 8 little-endian words, words pass through"""
    if v is None:
        return None
    if isinstance(v, int):
        if not 0 <= v < 1 << 256:
            raise MsmError(ERR_BAD_ARG, "a field element is 256 bits")
        return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)
    return np.ascontiguousarray(v, dtype=np.uint32).reshape(8)


def fr_root_of_unity(log_n):
    """the primitive 2^log_n-th root of unity the transforms use, as an int (arkworks' / snarkjs' root; host only)"""
    out = np.zeros(8, np.uint32)
    rc = load_library().msm_bn254_fr_root_of_unity(log_n, _p32(out))
    if rc != OK:
        raise MsmError(rc, "log_n = %d: r - 1 has 28 factors of two" % log_n)
    return sum(int(w) << (32 * i) for i, w in enumerate(out.tolist()))


def ntt_plan(log_n):
    """the widths (bits) of the passes a transform of 2^log_n elements makes over global memory (host only)"""
    passes, radix = C.c_uint32(0), np.zeros(8, np.uint32)
    rc = load_library().msm_bn254_fr_ntt_plan(log_n, C.byref(passes), _p32(radix))
    if rc != OK:
        raise MsmError(rc, "log_n = %d: r - 1 has 28 factors of two" % log_n)
    return [int(t) for t in radix[:passes.value]]


def r1cs_coefs(coefs):
    """constraint-matrix entries for the C ABI: a R1CS_COEF_DTYPE array passes through; bytes (a zkey's coefficient section after its count) are
    viewed as records; an iterable of (matrix, row, col, value) with value an int < 2^256 or 8 words is packed"""
    if isinstance(coefs, np.ndarray) and coefs.dtype == R1CS_COEF_DTYPE:
        return np.ascontiguousarray(coefs)
    if isinstance(coefs, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(coefs), R1CS_COEF_DTYPE).copy()
    coefs = list(coefs)
    out = np.zeros(len(coefs), R1CS_COEF_DTYPE)
    for i, (m, r, c, v) in enumerate(coefs):
        out[i] = (m, r, c, _fr_words(v))
    return out


def r1cs_plan(coefs, num_rows, num_cols, log_n):
    """what MsmContext.r1cs_upload would build from these entries (host only: no context, no GPU), as a dict of msm_r1cs_info_t; the same
    validation, with the coefficient values taken as R1CS_COEF_STD"""
    a = r1cs_coefs(coefs)
    info = R1csInfo()
    lib = load_library()
    rc = lib.msm_bn254_fr_r1cs_plan(a.ctypes.data, a.shape[0], num_rows, num_cols, log_n, C.byref(info))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_fr_r1cs_plan failed ({rc})")
    return info.as_dict()


def transpose_r1cs_coefs(coefs):
    """the same entries with row and col swapped: uploaded with num_rows' = n_vars, num_cols' = 2^log_n, log_n' = ceil(log2 n_vars), an eval on
    the Lagrange vector gives [a_j(tau) | b_j(tau) | c_j(tau)] per variable j -- the QAP polynomials of a setup"""
    t = r1cs_coefs(coefs).copy()
    t["row"], t["col"] = t["col"].copy(), t["row"].copy()
    return t


def fr_vector_plan():
    """the inversion group and the elements one workgroup covers in the scalar-vector calls, as a dict of msm_fr_vector_plan_t (host only)"""
    p = FrVectorPlan()
    lib = load_library()
    rc = lib.msm_bn254_fr_vector_plan(C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_fr_vector_plan failed ({rc})")
    return p.as_dict()


def fr_scan_plan(n):
    """the chain of a lane, the elements of a workgroup, the kernel launches and the scratch bytes of a scalar-field scan over n elements, as a
    dict of msm_fr_scan_plan_t (host only: no context, no GPU)"""
    p = FrScanPlan()
    lib = load_library()
    rc = lib.msm_bn254_fr_scan_plan(n, C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_fr_scan_plan failed ({rc})")
    return p.as_dict()


def fixed_base_plan(window_bits=0):
    """the window table and the inversion group of a fixed-base multiplication with windows of window_bits (0: the default) as a dict of
    msm_fixed_base_plan_t (host only: no context, no GPU)"""
    p = FixedBasePlan()
    lib = load_library()
    rc = lib.msm_bn254_g1_fixed_base_plan(window_bits, C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g1_fixed_base_plan failed ({rc})")
    return p.as_dict()


def pointwise_mul_plan():
    """the inversion group, the positions of the ladder and the points a lane keeps in registers in the element-wise multiplication, as a dict of
    msm_pointwise_plan_t (host only: no context, no GPU)"""
    p = PointwisePlan()
    lib = load_library()
    rc = lib.msm_bn254_g1_pointwise_mul_plan(C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g1_pointwise_mul_plan failed ({rc})")
    return p.as_dict()


def g2_pointwise_mul_plan():
    """the same for the G2 element-wise multiplication, as a dict of msm_pointwise_g2_plan_t (host only: no context, no GPU)"""
    p = G2PointwisePlan()
    lib = load_library()
    rc = lib.msm_bn254_g2_pointwise_mul_plan(C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g2_pointwise_mul_plan failed ({rc})")
    return p.as_dict()


def g1_fft_plan(log_n):
    """the stages of a G1 group transform of 2^log_n points, those of them that run a ladder, the inversion group and the bytes of the twiddle
    table the context keeps for this size, as a dict of msm_g1_fft_plan_t (host only: no context, no GPU)"""
    p = G1FftPlan()
    lib = load_library()
    rc = lib.msm_bn254_g1_fft_plan(log_n, C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g1_fft_plan failed ({rc})")
    return p.as_dict()


def g2_fft_plan(log_n):
    """the same for the G2 group transform, as a dict of msm_g2_fft_plan_t: the table is the G1 transform's (host only: no context, no GPU)"""
    p = G2FftPlan()
    lib = load_library()
    rc = lib.msm_bn254_g2_fft_plan(log_n, C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g2_fft_plan failed ({rc})")
    return p.as_dict()


def fixed_base_g2_plan(window_bits=0):
    """the same for the G2 call, with the points of a chunk and the scratch array they go through, as a dict of msm_fixed_base_g2_plan_t
    (host only: no context, no GPU)"""
    p = FixedBaseG2Plan()
    lib = load_library()
    rc = lib.msm_bn254_g2_fixed_base_plan(window_bits, C.byref(p))
    if rc != OK:
        raise MsmError(rc, (lib.msm_last_error(None) or b"").decode() or f"msm_bn254_g2_fixed_base_plan failed ({rc})")
    return p.as_dict()


def combine_partials(partials_jacobian_mont, want_affine=True, flags=0):
    """Fold per-rank partial sums in fixed rank order (host arithmetic inside the library).
    want_affine=False skips the field inversion; MsmResult.affine_std then computes it on first use.
    flags=FLAG_DETERMINISTIC: the Jacobian words are the canonical Z = 1 representative (msm_bn254_g1_combine_flags) -- what the ranks of a
    one-process-per-GPU job fold with when their contexts carry the flag."""
    p = _words(partials_jacobian_mont, 24)
    jac, aff, inf = np.zeros(24, np.uint32), (np.zeros(16, np.uint32) if want_affine else None), C.c_uint8(0)
    rc = load_library().msm_bn254_g1_combine_flags(_p32(p), p.shape[0], flags, _p32(jac), _p32(aff), C.byref(inf))
    if rc != OK:
        raise MsmError(rc, "Empty input" if rc == ERR_EMPTY else f"combine failed ({rc})")
    return MsmResult(jac, aff, inf.value)


def compress_points(bases, form=FORM_STD, inf=None):
    """Host-side inverse of MsmContext.decompress: n x 16 coordinate words -> n x 32 bytes (no GPU needed)."""
    bases = _words(bases, 16)
    if bases.shape[0] == 0:
        raise MsmError(ERR_EMPTY, "Empty input")
    out = np.zeros(bases.shape[0] * 32, np.uint8)
    infp = None
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
        infp = inf.ctypes.data_as(_u8p)
    rc = load_library().msm_bn254_g1_compress(_p32(bases), form, infp, bases.shape[0], out.ctypes.data_as(_u8p))
    if rc != 0:
        raise MsmError(rc, "msm_bn254_g1_compress failed (%d)" % rc)
    return out.tobytes()


def compress_points_g2(bases, form=FORM_STD, inf=None):
    """Host-side inverse of MsmContext.decompress_g2: n x 32 coordinate words (x.c0, x.c1, y.c0, y.c1) -> n x 64 bytes, the images of ark-serialize 0.4
    G2Affine::serialize_compressed (no GPU needed)."""
    bases = _words(bases, 32)
    if bases.shape[0] == 0:
        raise MsmError(ERR_EMPTY, "Empty input")
    out = np.zeros(bases.shape[0] * 64, np.uint8)
    infp = None
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
        infp = inf.ctypes.data_as(_u8p)
    rc = load_library().msm_bn254_g2_compress(_p32(bases), form, infp, bases.shape[0], out.ctypes.data_as(_u8p))
    if rc != 0:
        raise MsmError(rc, "msm_bn254_g2_compress failed (%d)" % rc)
    return out.tobytes()


class MsmContext:
    """Persistent engine context (replaces MetalMSMPipeline, rebuilt per call in the reference)."""

    _loader = staticmethod(lambda: load_library())  # testhooks.HooksContext runs the same class on the hooks build

    def __init__(self, device=-1, window_bits=0, flags=0, max_points=0, stream_chunk_log2=0, batch_layout=BATCH_LAYOUT_AUTO, host_threads=0):
        self._lib = self._loader()
        cfg = Config(device, window_bits, flags, stream_chunk_log2, max_points, batch_layout, host_threads)
        h = C.c_void_p()
        rc = self._lib.msm_ctx_create(C.byref(cfg), C.byref(h))
        if rc != OK:
            raise MsmError(rc, (self._lib.msm_last_error(None) or b"").decode())
        self._h = h
        self.window_bits, self.flags = window_bits, flags
        # the device-pointer calls (the bench's timed call) write into one persistent buffer whose ctypes pointers are made once: building two numpy
        # arrays and their ctypes views cost 3 us per call, a copy of 96 bytes 0.2 (the C side serialises a context's calls; this lock covers the copy)
        import threading
        self._jbuf = np.zeros(24, np.uint32)
        self._jptr, self._oi = _p32(self._jbuf), C.c_uint8(0)
        self._oiref, self._olock = C.byref(self._oi), threading.Lock()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.msm_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != OK:
            raise MsmError(rc, (self._lib.msm_last_error(self._h) or b"").decode() or f"status {rc}")

    def _outs(self):
        return np.zeros(24, np.uint32), np.zeros(16, np.uint32), C.c_uint8(0)

    # -- the drop-in call ---------------------------------------------------------------------
    def msm(self, bases, scalars, form=FORM_STD, inf=None):
        bases, scalars = _words(bases, 16), _words(scalars, 8)
        if bases.shape[0] == 0 or scalars.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")  # metal_msm.rs:647-649
        n = min(bases.shape[0], scalars.shape[0])  # metal_msm.rs:652-656
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = inf.ctypes.data_as(_u8p)
        jac, aff, oi = self._outs()
        self._check(self._lib.msm_bn254_g1(self._h, _p32(bases), form, infp, _p32(scalars), n, _p32(jac), _p32(aff),
                                           C.byref(oi)))
        return MsmResult(jac, aff, oi.value)

    def msm_arkworks(self, raw_structs, stride, x_off, y_off, inf_off, scalars_mont):
        """Zero-copy path of the Rust shim: `raw_structs` is the byte image of a [G1Affine] slice, scalars are Fr
        Montgomery words; both go to the GPU untouched."""
        raw = np.ascontiguousarray(raw_structs, dtype=np.uint8).reshape(-1)
        sc = _words(scalars_mont, 8)
        n = min(raw.size // stride, sc.shape[0])
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        jac, aff, oi = self._outs()
        self._check(self._lib.msm_bn254_g1_arkworks(self._h, raw.ctypes.data_as(C.c_void_p), stride, x_off, y_off,
                                                    inf_off if inf_off is not None else C.c_size_t(-1).value, _p32(sc), n,
                                                    _p32(jac), _p32(aff), C.byref(oi)))
        return MsmResult(jac, aff, oi.value)

    def upload_bases(self, bases, form=FORM_STD, inf=None):
        bases = _words(bases, 16)
        if bases.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = inf.ctypes.data_as(_u8p)
        self._check(self._lib.msm_bn254_g1_upload_bases(self._h, _p32(bases), form, infp, bases.shape[0]))

    @staticmethod
    def _images(images, size=32):
        buf = np.frombuffer(images, dtype=np.uint8) if isinstance(images, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(images, dtype=np.uint8).reshape(-1)
        if buf.size == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        if buf.size % size:
            raise MsmError(ERR_BAD_ARG, "compressed %s images are %d bytes each" % ("G1Affine" if size == 32 else "G2Affine", size))
        return np.ascontiguousarray(buf)

    def decompress(self, images):
        """arkworks-0.4 `serialize_compressed` G1Affine images (n x 32 bytes) -> (xy Montgomery words n x 16, inf n).
        The square roots run on the GPU.  An image that does not decode raises MsmError(ERR_INVALID_DATA) with
        .first_invalid set (arkworks: SerializationError::InvalidData)."""
        buf = self._images(images)
        n = buf.size // 32
        xy = np.zeros((n, 16), np.uint32)
        inf = np.zeros(n, np.uint8)
        bad = C.c_int64(-1)
        rc = self._lib.msm_bn254_g1_decompress(self._h, buf.ctypes.data_as(_u8p), n, _p32(xy), inf.ctypes.data_as(_u8p), C.byref(bad))
        self._check_invalid(rc, bad)
        return xy, inf

    def upload_compressed(self, images):
        """Decode compressed images straight into the resident-bases set (then msm_resident)."""
        buf = self._images(images)
        bad = C.c_int64(-1)
        rc = self._lib.msm_bn254_g1_upload_compressed(self._h, buf.ctypes.data_as(_u8p), buf.size // 32, C.byref(bad))
        self._check_invalid(rc, bad)

    def _check_invalid(self, rc, bad):
        if rc == ERR_INVALID_DATA:
            e = MsmError(rc, (self._lib.msm_last_error(self._h) or b"invalid data").decode())
            e.first_invalid = int(bad.value)
            raise e
        self._check(rc)

    def msm_resident(self, scalars):
        scalars = _words(scalars, 8)
        if scalars.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        jac, aff, oi = self._outs()
        self._check(self._lib.msm_bn254_g1_resident(self._h, _p32(scalars), scalars.shape[0], _p32(jac), _p32(aff),
                                                    C.byref(oi)))
        return MsmResult(jac, aff, oi.value)

    def msm_resident_device(self, d_scalars_ptr, n, stream=None):
        """scalars already in HBM (raw device pointer) against the resident bases and, if the context has one, their window table"""
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        jac, _, oi = self._outs()
        self._check(self._lib.msm_bn254_g1_resident_device(self._h, d_scalars_ptr, n, stream, _p32(jac), None, C.byref(oi)))
        return MsmResult(jac, None, oi.value)

    def msm_resident_batch(self, scalar_vectors, want_affine=True):
        """several scalar vectors against the resident bases, two MSMs in flight (how provers call MSM): list of MsmResult"""
        vecs = [_words(s, 8) for s in scalar_vectors]
        if not vecs or any(v.shape[0] == 0 for v in vecs):
            raise MsmError(ERR_EMPTY, "Empty input")
        n = min(v.shape[0] for v in vecs)
        k = len(vecs)
        ptrs = (_u32p * k)(*[_p32(v) for v in vecs])
        jac = np.zeros((k, 24), np.uint32)
        aff = np.zeros((k, 16), np.uint32) if want_affine else None
        inf = np.zeros(k, np.uint8)
        self._check(self._lib.msm_bn254_g1_resident_batch(self._h, ptrs, n, k, _p32(jac), _p32(aff), inf.ctypes.data_as(_u8p)))
        return [MsmResult(jac[i], aff[i] if want_affine else None, inf[i]) for i in range(k)]

    def tune_batch(self, scalar_vectors, reps=0):
        """explicit, opt-in measurement of the batch layout on this context as the process is now (msm_tune_batch): returns
        (chosen MSM_BATCH_LAYOUT_*, {layout: ms per MSM}); AUTO contexts use the choice until the next upload"""
        vecs = [_words(s, 8) for s in scalar_vectors]
        if len(vecs) < 2 or any(v.shape[0] == 0 for v in vecs):
            raise MsmError(ERR_BAD_ARG, "tune_batch needs at least two non-empty scalar vectors")
        n = min(v.shape[0] for v in vecs)
        k = len(vecs)
        ptrs = (_u32p * k)(*[_p32(v) for v in vecs])
        chosen, ms = C.c_uint32(0), (C.c_double * 3)()
        self._check(self._lib.msm_tune_batch(self._h, ptrs, n, k, reps, C.byref(chosen), ms))
        return int(chosen.value), {BATCH_LAYOUT_ONE_STREAM: ms[0], BATCH_LAYOUT_ONE_STREAM_REDUCE: ms[1], BATCH_LAYOUT_TWO_STREAMS: ms[2]}

    def msm_device(self, d_bases_ptr, d_scalars_ptr, n, d_inf_ptr=None, stream=None):
        """All operands already in HBM (raw device pointers, e.g. torch.Tensor.data_ptr())."""
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        with self._olock:
            rc = self._lib.msm_bn254_g1_device(self._h, d_bases_ptr, d_inf_ptr, d_scalars_ptr, n, stream, self._jptr, None, self._oiref)
            if rc != OK:
                self._check(rc)
            return MsmResult(self._jbuf.copy(), None, self._oi.value)  # affine words on demand (MsmResult.affine_std)

    # -- BN254 G2 (the Groth16 B query) --------------------------------------------------------
    def msm_g2(self, bases, scalars, form=FORM_STD, inf=None):
        """bases: n x 32 words (x.c0, x.c1, y.c0, y.c1), scalars: n x 8 words standard form; lengths truncate to the shorter one as msm() does."""
        bases, scalars = _words(bases, 32), _words(scalars, 8)
        if bases.shape[0] == 0 or scalars.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        n = min(bases.shape[0], scalars.shape[0])
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = inf.ctypes.data_as(_u8p)
        jac, aff, oi = np.zeros(48, np.uint32), np.zeros(32, np.uint32), C.c_uint8(0)
        self._check(self._lib.msm_bn254_g2(self._h, _p32(bases), form, infp, _p32(scalars), n, _p32(jac), _p32(aff), C.byref(oi)))
        return G2Result(jac, aff, oi.value)

    def msm_g2_device(self, d_bases_ptr, d_scalars_ptr, n, d_inf_ptr=None, stream=None):
        """All operands already in HBM (raw device pointers): bases n x 32 Montgomery words, scalars n x 8 words."""
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        jac, oi = np.zeros(48, np.uint32), C.c_uint8(0)
        self._check(self._lib.msm_bn254_g2_device(self._h, d_bases_ptr, d_inf_ptr, d_scalars_ptr, n, stream, _p32(jac), None, C.byref(oi)))
        return G2Result(jac, None, oi.value)  # affine words on demand (G2Result.affine_std)

    # -- G2 bases from outside: compressed images, curve and subgroup checks (the square roots and [r]P = O run on the GPU) --------
    def decompress_g2(self, images, checks=0):
        """ark-serialize 0.4 `serialize_compressed` G2Affine images (n x 64 bytes) -> (xy Montgomery words n x 32, inf n).  checks: 0 or
        G2_CHECK_SUBGROUP (the curve check is inherent).  An invalid image raises MsmError(ERR_INVALID_DATA) with .first_invalid set; the message
        says "decode", "curve" or "subgroup"."""
        buf = self._images(images, 64)
        n = buf.size // 64
        xy, inf, bad = np.zeros((n, 32), np.uint32), np.zeros(n, np.uint8), C.c_int64(-1)
        rc = self._lib.msm_bn254_g2_decompress(self._h, buf.ctypes.data_as(_u8p), n, checks, _p32(xy), inf.ctypes.data_as(_u8p), C.byref(bad))
        self._check_invalid(rc, bad)
        return xy, inf

    def decompress_g2_device(self, images, d_out_ptr, d_inf_ptr, checks=0, stream=None):
        """the same into caller-owned device memory (raw pointers: n x 128 bytes and n bytes) -- what msm_g2_device takes; returns n"""
        buf = self._images(images, 64)
        n, bad = buf.size // 64, C.c_int64(-1)
        rc = self._lib.msm_bn254_g2_decompress_device(self._h, buf.ctypes.data_as(_u8p), n, checks, d_out_ptr, d_inf_ptr, stream, C.byref(bad))
        self._check_invalid(rc, bad)
        return n

    @staticmethod
    def _inf_ptr(inf):
        if inf is None:
            return None, None
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
        return inf, inf.ctypes.data_as(_u8p)

    def validate_g2(self, bases, form=FORM_STD, inf=None, checks=G2_CHECK_SUBGROUP):
        """n x 32 coordinate words: every component < p and the point on the twist (G2_CHECK_CURVE), in the subgroup of order r (G2_CHECK_SUBGROUP,
        which implies the former).  Returns None; an invalid point raises MsmError(ERR_INVALID_DATA) with .first_invalid set."""
        bases = _words(bases, 32)
        if bases.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        inf, infp = self._inf_ptr(inf)
        bad = C.c_int64(-1)
        self._check_invalid(self._lib.msm_bn254_g2_validate(self._h, _p32(bases), form, infp, bases.shape[0], checks, C.byref(bad)), bad)

    def validate_g2_device(self, d_bases_ptr, n, d_inf_ptr=None, checks=G2_CHECK_SUBGROUP, stream=None):
        """the same on n x 32 Montgomery words already in HBM (raw device pointers)"""
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        bad = C.c_int64(-1)
        self._check_invalid(self._lib.msm_bn254_g2_validate_device(self._h, d_bases_ptr, d_inf_ptr, n, checks, stream, C.byref(bad)), bad)

    def validate_g1(self, bases, form=FORM_STD, inf=None):
        """n x 16 coordinate words of G1 points: coordinates < p and y^2 = x^3 + 3 (the cofactor is 1: nothing else to check)"""
        bases = _words(bases, 16)
        if bases.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        inf, infp = self._inf_ptr(inf)
        bad = C.c_int64(-1)
        self._check_invalid(self._lib.msm_bn254_g1_validate(self._h, _p32(bases), form, infp, bases.shape[0], C.byref(bad)), bad)

    # -- BN254 scalar field: transforms in HBM (the H scalars of a Groth16 proof) ---------------------
    def ntt(self, values, log_n, batch=1, flags=0, coset=None, out=None):
        """host arrays: batch x 2^log_n elements of 8 words, natural order in and out; flags NTT_*; coset: generator g (int or 8 words,
        standard form) or None.  Returns the (batch * n) x 8 result: a new array, or `out` (a contiguous uint32 array, which may be `values`
        itself: the call then works in place)."""
        a = _words(values, 8)
        if a.shape[0] == 0 or batch == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        if 0 <= log_n <= 28 and a.shape[0] != batch << log_n:
            raise MsmError(ERR_BAD_ARG, "%d elements given, batch x 2^log_n = %d" % (a.shape[0], batch << log_n))
        if out is None:
            out = np.zeros_like(a)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.size == a.size):
                raise MsmError(ERR_BAD_ARG, "out must be a contiguous uint32 array of the input's size")
            out = out.reshape(-1, 8)
        g = _fr_words(coset)
        self._check(self._lib.msm_bn254_fr_ntt(self._h, _p32(a), _p32(out), log_n, batch, flags, _p32(g)))
        return out

    def ntt_device(self, d_ptr, log_n, batch=1, flags=0, coset=None, stream=None):
        """in place on batch x 2^log_n elements already in HBM (raw device pointer); enqueued on `stream` (None: the context's)"""
        self._check(self._lib.msm_bn254_fr_ntt_device(self._h, d_ptr, log_n, batch, flags, _p32(_fr_words(coset)), stream))

    def fr_mul_sub_scale_device(self, d_a, d_b, d_c, d_out, n, k=None, flags=0, stream=None):
        """out[i] = (a[i] * b[i] - c[i]) * k on raw device pointers; d_c None: no subtrahend; k None: 1; d_out may alias an input"""
        self._check(self._lib.msm_bn254_fr_mul_sub_scale_device(self._h, d_a, d_b, d_c, _p32(_fr_words(k)), d_out, n, flags, stream))

    # -- BN254 scalar field: rows of the constraint matrices times the witness ([a | b | c] made in HBM) ---
    def r1cs_upload(self, coefs, num_rows, num_cols, log_n, coef_form=R1CS_COEF_STD):
        """make up to three constraint matrices (matrix 0, 1, 2 = A, B, C; num_rows x num_cols) resident, replacing earlier ones; the evals are
        laid out over 2^log_n >= num_rows rows.  coefs: see r1cs_coefs.  Returns what was built (msm_r1cs_info_t as a dict)."""
        a = r1cs_coefs(coefs)
        self._check(self._lib.msm_bn254_fr_r1cs_upload(self._h, a.ctypes.data, a.shape[0], coef_form, num_rows, num_cols, log_n))
        return self.r1cs_info()

    def r1cs_info(self):
        info = R1csInfo()
        self._check(self._lib.msm_bn254_fr_r1cs_info(self._h, C.byref(info)))
        return info.as_dict()

    def r1cs_eval_device(self, d_witness, n_witness, d_out, flags=0, stream=None):
        """raw device pointers: n_witness x 8 witness words in, 3 x 2^log_n x 8 words [a | b | c] out; flags NTT_IN_MONT / NTT_OUT_MONT /
        R1CS_C_FROM_AB; enqueued on `stream` (None: the context's)"""
        self._check(self._lib.msm_bn254_fr_r1cs_eval_device(self._h, d_witness, n_witness, d_out, flags, stream))

    def r1cs_eval(self, witness, log_n, flags=0):
        """host arrays: the witness (num_cols x 8 words) -> the (3 * 2^log_n) x 8 words [a | b | c]; log_n as uploaded"""
        w = _words(witness, 8)
        out = np.zeros((3 << log_n, 8), np.uint32)
        self._check(self._lib.msm_bn254_fr_r1cs_eval(self._h, _p32(w), w.shape[0], _p32(out), flags))
        return out

    # -- BN254 scalar field: the scalars of a setup made in HBM (what the fixed-base calls read); nothing is kept on the context ---
    def fr_powers_device(self, base, d_out, n, scale=None, first=0, flags=0, stream=None):
        """out[i] = scale * base^(first + i) on a raw device pointer; base, scale: ints or 8 standard-form words (scale None: 1); flags
        NTT_OUT_MONT; enqueued on `stream` (None: the context's)"""
        self._check(self._lib.msm_bn254_fr_powers_device(self._h, _p32(_fr_words(base)), _p32(_fr_words(scale)), first, d_out, n, flags, stream))

    def fr_batch_inverse_device(self, d_in, d_out, n, flags=0, stream=None):
        """out[i] = 1 / in[i] on raw device pointers (0 stays 0; d_out may be d_in); flags NTT_IN_MONT / NTT_OUT_MONT"""
        self._check(self._lib.msm_bn254_fr_batch_inverse_device(self._h, d_in, d_out, n, flags, stream))

    def fr_batch_inverse(self, values, flags=0, out=None):
        """host arrays: n x 8 words -> their inverses, a new array or `out` (a contiguous uint32 array, which may be `values` itself)"""
        a = _words(values, 8)
        if out is None:
            out = np.zeros_like(a)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.size == a.size):
                raise MsmError(ERR_BAD_ARG, "out must be a contiguous uint32 array of the input's size")
            out = out.reshape(-1, 8)
        self._check(self._lib.msm_bn254_fr_batch_inverse(self._h, _p32(a), _p32(out), a.shape[0], flags))
        return out

    def fr_lagrange_device(self, tau, log_n, d_out, flags=0, stream=None):
        """out[i] = L_i(tau) over the transforms' domain of 2^log_n points on a raw device pointer; tau: an int or 8 standard-form words; flags
        NTT_OUT_MONT"""
        self._check(self._lib.msm_bn254_fr_lagrange_device(self._h, _p32(_fr_words(tau)), log_n, d_out, flags, stream))

    def fr_lincomb_device(self, d_a, d_out, n, ka=None, d_b=None, kb=None, d_c=None, kc=None, flags=0, stream=None):
        """out[i] = ka a[i] + kb b[i] + kc c[i] on raw device pointers; d_b / d_c None: no such term; a coefficient None: 1; d_out may alias an
        input; flags NTT_IN_MONT / NTT_OUT_MONT"""
        self._check(self._lib.msm_bn254_fr_lincomb_device(self._h, d_a, _p32(_fr_words(ka)), d_b, _p32(_fr_words(kb)), d_c, _p32(_fr_words(kc)),
                                                          d_out, n, flags, stream))

    @staticmethod
    def fr_vector_plan():
        return fr_vector_plan()

    # -- BN254 scalar field: scans; the context keeps one array of block aggregates and the event behind the latest call ---
    def fr_poly_eval_device(self, d_coeffs, n, z, d_value, flags=0, stream=None):
        """d_value[0..8) = sum_i c[i] z^i on raw device pointers; z: an int or 8 standard-form words; flags NTT_IN_MONT / NTT_OUT_MONT; enqueued
        on `stream` (None: the context's)"""
        self._check(self._lib.msm_bn254_fr_poly_eval_device(self._h, d_coeffs, n, _p32(_fr_words(z)), d_value, flags, stream))

    def fr_poly_div_linear_device(self, d_coeffs, n, z, d_quot, d_rem=None, flags=0, stream=None):
        """p = q (X - z) + p(z) on raw device pointers: n elements q (q[n - 1] = 0) at d_quot, which may be d_coeffs, and p(z) at d_rem (8
        words; None: not written); flags NTT_IN_MONT / NTT_OUT_MONT"""
        self._check(self._lib.msm_bn254_fr_poly_div_linear_device(self._h, d_coeffs, n, _p32(_fr_words(z)), d_quot, d_rem, flags, stream))

    def fr_poly_div_linear(self, coeffs, z, flags=0, out=None):
        """host arrays: n x 8 words -> (the n x 8 words of the quotient, the 8 words of p(z)); the quotient is a new array or `out` (a contiguous
        uint32 array, which may be `coeffs` itself)"""
        a = _words(coeffs, 8)
        if out is None:
            out = np.zeros_like(a)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.size == a.size):
                raise MsmError(ERR_BAD_ARG, "out must be a contiguous uint32 array of the input's size")
            out = out.reshape(-1, 8)
        rem = np.zeros(8, np.uint32)
        self._check(self._lib.msm_bn254_fr_poly_div_linear(self._h, _p32(a), a.shape[0], _p32(_fr_words(z)), _p32(out), _p32(rem), flags))
        return out, rem

    def fr_running_product_device(self, d_in, d_out, n, d_total=None, flags=0, stream=None):
        """out[i] = in[0] .. in[i] on raw device pointers (with FR_SCAN_EXCLUSIVE: out[0] = 1, out[i] = in[0] .. in[i - 1]); the product of all
        n at d_total (8 words; None: not written); d_out may be d_in; flags NTT_IN_MONT / NTT_OUT_MONT / FR_SCAN_EXCLUSIVE"""
        self._check(self._lib.msm_bn254_fr_running_product_device(self._h, d_in, d_out, n, d_total, flags, stream))

    @staticmethod
    def fr_scan_plan(n):
        return fr_scan_plan(n)

    # -- the host-array forms of the fixed-base and the element-wise calls; words: 16 per G1 point, 32 per G2 point; fn: the library's function ---
    def _fixed_base_host(self, words, fn, base, scalars, form, window_bits, flags):
        b, k = _words(base, words), _words(scalars, 8)
        xy, inf = np.zeros((k.shape[0], words), np.uint32), np.zeros(k.shape[0], np.uint8)
        self._check(fn(self._h, _p32(b), form, _p32(k), k.shape[0], window_bits, flags, _p32(xy), inf.ctypes.data_as(_u8p)))
        return xy, inf

    def _pointwise_host(self, words, fn, bases, scalars, form, inf, flags):
        b, k = _words(bases, words), _words(scalars, 8)
        if b.shape[0] != k.shape[0]:
            raise MsmError(ERR_BAD_ARG, "as many scalars as bases")
        xy, out_inf = np.zeros((k.shape[0], words), np.uint32), np.zeros(k.shape[0], np.uint8)
        inf, inf_p = self._inf_ptr(inf)
        if inf is not None and inf.size != k.shape[0]:
            raise MsmError(ERR_BAD_ARG, "as many infinity bytes as bases")
        self._check(fn(self._h, _p32(b), form, inf_p, _p32(k), k.shape[0], flags, _p32(xy), out_inf.ctypes.data_as(_u8p)))
        return xy, out_inf

    # -- BN254 G1 fixed base: out[i] = k_i * P, one base, n affine points (the queries of a setup made in HBM) ---
    def fixed_base_mul(self, base, scalars, form=FORM_STD, window_bits=0, flags=0):
        """host arrays: the base (16 words x, y in `form`) and n x 8 scalar words (any 256-bit patterns; flags NTT_IN_MONT: arkworks Fr.0 words)
        -> (n x 16 words xy, n bytes inf); the coordinates are arkworks Montgomery words, standard form with FB_OUT_STD"""
        return self._fixed_base_host(16, self._lib.msm_bn254_g1_fixed_base_mul, base, scalars, form, window_bits, flags)

    def fixed_base_mul_device(self, base, d_scalars, n, d_out_xy, d_out_inf, form=FORM_STD, window_bits=0, flags=0, stream=None):
        """raw device pointers: n x 8 scalar words in, n x 16 words xy and n bytes inf out; the base is a host array; enqueued on `stream`
        (None: the context's)"""
        b = _words(base, 16)
        self._check(self._lib.msm_bn254_g1_fixed_base_mul_device(self._h, _p32(b), form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf,
                                                                 stream))

    # -- BN254 G2 fixed base: out[i] = k_i * Q (the B2 query of a setup); the base is checked on the host: on the twist, and in G2 ---
    def fixed_base_g2_mul(self, base, scalars, form=FORM_STD, window_bits=0, flags=0):
        """host arrays: the base (32 words x.c0, x.c1, y.c0, y.c1 in `form`) and n x 8 scalar words (flags NTT_IN_MONT: arkworks Fr.0 words)
        -> (n x 32 words xy, n bytes inf); the coordinates are arkworks Montgomery words, standard form with FB_OUT_STD"""
        return self._fixed_base_host(32, self._lib.msm_bn254_g2_fixed_base_mul, base, scalars, form, window_bits, flags)

    def fixed_base_g2_mul_device(self, base, d_scalars, n, d_out_xy, d_out_inf, form=FORM_STD, window_bits=0, flags=0, stream=None):
        """raw device pointers: n x 8 scalar words in, n x 32 words xy and n bytes inf out (what msm_g2_device takes); the base is a host
        array; enqueued on `stream` (None: the context's)"""
        b = _words(base, 32)
        self._check(self._lib.msm_bn254_g2_fixed_base_mul_device(self._h, _p32(b), form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf,
                                                                 stream))

    # -- BN254 G1 element-wise: out[i] = k_i * P_i, n points each with its own scalar (or all with one): the update of an existing setup ---
    def pointwise_mul(self, bases, scalars, form=FORM_STD, inf=None, flags=0):
        """host arrays: n x 16 base words (x, y in `form`), n x 8 scalar words (any 256-bit patterns; flags NTT_IN_MONT: arkworks Fr.0 words) and
        optionally n infinity bytes -> (n x 16 words xy, n bytes inf); the coordinates are arkworks Montgomery words, standard form with
        FB_OUT_STD.  The bases are not validated (validate_g1 does that)"""
        return self._pointwise_host(16, self._lib.msm_bn254_g1_pointwise_mul, bases, scalars, form, inf, flags)

    def pointwise_mul_device(self, d_bases, d_scalars, n, d_out_xy, d_out_inf, d_inf=None, flags=0, stream=None):
        """raw device pointers: n x 16 base words, n x 8 scalar words and optionally n infinity bytes in, n x 16 words xy and n bytes inf out;
        d_out_xy may be d_bases and d_out_inf may be d_inf (in place); flags NTT_IN_MONT / FB_OUT_STD / PM_BASES_STD; enqueued on `stream`
        (None: the context's); nothing is kept on the context"""
        self._check(self._lib.msm_bn254_g1_pointwise_mul_device(self._h, d_bases, d_inf, d_scalars, n, flags, d_out_xy, d_out_inf, stream))

    def scale_device(self, d_bases, k, n, d_out_xy, d_out_inf, d_inf=None, flags=0, stream=None):
        """out[i] = k * P_i for ONE scalar k (an int or 8 standard-form words, read modulo r) on raw device pointers; flags FB_OUT_STD /
        PM_BASES_STD; otherwise as pointwise_mul_device"""
        self._check(self._lib.msm_bn254_g1_scale_device(self._h, d_bases, d_inf, _p32(_fr_words(k)), n, flags, d_out_xy, d_out_inf, stream))

    @staticmethod
    def pointwise_mul_plan():
        return pointwise_mul_plan()

    # -- BN254 G2 element-wise: out[i] = k_i * Q_i on records of 32 words (x.c0, x.c1, y.c0, y.c1): the G2 half of a ceremony update ---------
    def g2_pointwise_mul(self, bases, scalars, form=FORM_STD, inf=None, flags=0):
        """host arrays: n x 32 base words (in `form`), n x 8 scalar words (any 256-bit patterns; flags NTT_IN_MONT: arkworks Fr.0 words) and
        optionally n infinity bytes -> (n x 32 words xy, n bytes inf); the components are arkworks Montgomery words, standard form with
        FB_OUT_STD.  The bases must be points of G2 and are not validated (validate_g2 with G2_CHECK_SUBGROUP does that)"""
        return self._pointwise_host(32, self._lib.msm_bn254_g2_pointwise_mul, bases, scalars, form, inf, flags)

    def g2_pointwise_mul_device(self, d_bases, d_scalars, n, d_out_xy, d_out_inf, d_inf=None, flags=0, stream=None):
        """raw device pointers: n x 32 base words, n x 8 scalar words and optionally n infinity bytes in, n x 32 words xy and n bytes inf out;
        d_out_xy may be d_bases and d_out_inf may be d_inf (in place); flags NTT_IN_MONT / FB_OUT_STD / PM_BASES_STD; enqueued on `stream`
        (None: the context's); nothing is kept on the context"""
        self._check(self._lib.msm_bn254_g2_pointwise_mul_device(self._h, d_bases, d_inf, d_scalars, n, flags, d_out_xy, d_out_inf, stream))

    def g2_scale_device(self, d_bases, k, n, d_out_xy, d_out_inf, d_inf=None, flags=0, stream=None):
        """out[i] = k * Q_i for ONE scalar k (an int or 8 standard-form words, read modulo r) on raw device pointers; flags FB_OUT_STD /
        PM_BASES_STD; otherwise as g2_pointwise_mul_device"""
        self._check(self._lib.msm_bn254_g2_scale_device(self._h, d_bases, d_inf, _p32(_fr_words(k)), n, flags, d_out_xy, d_out_inf, stream))

    @staticmethod
    def g2_pointwise_mul_plan():
        return g2_pointwise_mul_plan()

    # -- BN254 G1 group transform: the DFT over points, in place; the inverse makes the Lagrange basis L_i(tau) * G from tau^j * G --------------
    def g1_fft(self, xy, log_n, form=FORM_STD, inf=None, batch=1, flags=0, out_xy=None, out_inf=None):
        """host arrays: batch * 2^log_n x 16 words (x, y in `form`) and optionally as many infinity bytes -> (xy, inf) of the transform, natural
        order in and out; flags NTT_INVERSE (1/n included) / FB_OUT_STD (default: arkworks Montgomery words).  out_xy / out_inf: contiguous
        arrays to write into; out_xy may be xy and out_inf may be inf (in place).  The points are not validated"""
        a = _words(xy, 16)
        n = batch << log_n
        if a.shape[0] != n:
            raise MsmError(ERR_BAD_ARG, "batch * 2^log_n points")
        inf, inf_p = self._inf_ptr(inf)
        if inf is not None and inf.size != n:
            raise MsmError(ERR_BAD_ARG, "as many infinity bytes as points")
        if out_xy is None:
            out_xy = np.zeros((n, 16), np.uint32)
        if out_inf is None:
            out_inf = np.zeros(n, np.uint8)
        for o, dt, size in ((out_xy, np.uint32, n * 16), (out_inf, np.uint8, n)):
            if not (isinstance(o, np.ndarray) and o.dtype == dt and o.flags.c_contiguous and o.flags.writeable and o.size == size):
                raise MsmError(ERR_BAD_ARG, "the output arrays are contiguous, writeable, uint32 resp. uint8, of the input's size")
        self._check(self._lib.msm_bn254_g1_fft(self._h, _p32(a), form, inf_p, log_n, batch, flags, _p32(out_xy), out_inf.ctypes.data_as(_u8p)))
        return out_xy, out_inf

    def g1_fft_device(self, d_xy, d_inf, log_n, batch=1, flags=0, stream=None):
        """raw device pointers, in place: batch arrays of 2^log_n x 16 words and batch * 2^log_n infinity bytes (required); flags NTT_INVERSE /
        PM_BASES_STD / FB_OUT_STD; enqueued on `stream` (None: the context's).  The context keeps the twiddle table of every log_n it has seen"""
        self._check(self._lib.msm_bn254_g1_fft_device(self._h, d_xy, d_inf, log_n, batch, flags, stream))

    @staticmethod
    def g1_fft_plan(log_n):
        return g1_fft_plan(log_n)

    # -- BN254 G2 group transform: the same over G2 records; the inverse makes L_i(tau) * H from the tauG2 section tau^j * H -------------------
    def g2_fft(self, xy, log_n, form=FORM_STD, inf=None, batch=1, flags=0, out_xy=None, out_inf=None):
        """host arrays: batch * 2^log_n x 32 words (x.c0 x.c1 y.c0 y.c1 in `form`) and optionally as many infinity bytes -> (xy, inf) of the
        transform, natural order in and out; flags NTT_INVERSE (1/n included) / FB_OUT_STD (default: arkworks Montgomery words).  out_xy /
        out_inf: contiguous arrays to write into; out_xy may be xy and out_inf may be inf (in place).  The points must be points of G2 and
        are not validated"""
        a = _words(xy, 32)
        n = batch << log_n
        if a.shape[0] != n:
            raise MsmError(ERR_BAD_ARG, "batch * 2^log_n points")
        inf, inf_p = self._inf_ptr(inf)
        if inf is not None and inf.size != n:
            raise MsmError(ERR_BAD_ARG, "as many infinity bytes as points")
        if out_xy is None:
            out_xy = np.zeros((n, 32), np.uint32)
        if out_inf is None:
            out_inf = np.zeros(n, np.uint8)
        for o, dt, size in ((out_xy, np.uint32, n * 32), (out_inf, np.uint8, n)):
            if not (isinstance(o, np.ndarray) and o.dtype == dt and o.flags.c_contiguous and o.flags.writeable and o.size == size):
                raise MsmError(ERR_BAD_ARG, "the output arrays are contiguous, writeable, uint32 resp. uint8, of the input's size")
        self._check(self._lib.msm_bn254_g2_fft(self._h, _p32(a), form, inf_p, log_n, batch, flags, _p32(out_xy), out_inf.ctypes.data_as(_u8p)))
        return out_xy, out_inf

    def g2_fft_device(self, d_xy, d_inf, log_n, batch=1, flags=0, stream=None):
        """raw device pointers, in place: batch arrays of 2^log_n x 32 words and batch * 2^log_n infinity bytes (required); flags NTT_INVERSE /
        PM_BASES_STD / FB_OUT_STD; enqueued on `stream` (None: the context's).  The twiddle tables are those g1_fft_device keeps"""
        self._check(self._lib.msm_bn254_g2_fft_device(self._h, d_xy, d_inf, log_n, batch, flags, stream))

    @staticmethod
    def g2_fft_plan(log_n):
        return g2_fft_plan(log_n)

    def set_stage_timing(self, enabled=True):
        self._check(self._lib.msm_set_stage_timing(self._h, int(bool(enabled))))

    def timings(self):
        t = Timings()
        self._check(self._lib.msm_get_timings(self._h, C.byref(t)))
        return t.as_dict()

    def set_kernel_timing(self, every_n):
        """every `every_n`-th launch of the accumulate kernel carries its pair of hipEvents (0 = none: the default; 1 = all: ~11 us more per MSM); accumulate_kernel_stats() and timings()["accumulate_ms"] see the timed launches only"""
        self._check(self._lib.msm_set_kernel_timing(self._h, every_n))

    def accumulate_kernel_stats(self):
        avg, cnt = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.msm_get_accumulate_kernel_stats(self._h, C.byref(avg), C.byref(cnt)))
        return avg.value, cnt.value

    def reset_kernel_stats(self):
        self._lib.msm_reset_kernel_stats(self._h)

    def clock_stats(self):
        """clock probe of k_accumulate since the last reset_kernel_stats: {"sclk_ghz": shader clock the kernel sustained,
        "cycles_per_addition": shader cycles of one wavefront per mixed addition, "samples": launches sampled}"""
        ghz, cpa, cnt = C.c_double(0), C.c_double(0), C.c_uint64(0)
        self._check(self._lib.msm_get_clock_stats(self._h, C.byref(ghz), C.byref(cpa), C.byref(cnt)))
        return {"sclk_ghz": ghz.value, "cycles_per_addition": cpa.value, "samples": cnt.value}


class MsmMulti:
    """One MSM over several GPUs of ONE process (include/msm_hip.h "multi-GPU"): contiguous point-range shards, one context
    and one host thread per device, partials exchanged with RCCL (all-gather of 24 words + fold in rank order) or folded on
    the host.  Same call signatures as MsmContext."""

    def __init__(self, devices=None, window_bits=0, flags=0, stream_chunk_log2=0, exchange=EXCHANGE_AUTO, host_threads=0, _lib=None):
        self._lib = _lib or load_library()
        cfg = Config(-1, window_bits, flags, stream_chunk_log2, 0, 0, host_threads)
        h = C.c_void_p()
        if devices is None:
            rc = self._lib.msm_multi_create(None, 0, C.byref(cfg), exchange, C.byref(h))
        else:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self._lib.msm_multi_create(arr, len(devices), C.byref(cfg), exchange, C.byref(h))
        if rc != OK:
            raise MsmError(rc, (self._lib.msm_multi_last_error(None) or b"").decode())
        self._h = h
        self.num_devices = int(self._lib.msm_multi_num_devices(h))
        self.exchange = int(self._lib.msm_multi_exchange(h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.msm_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != OK:
            raise MsmError(rc, (self._lib.msm_multi_last_error(self._h) or b"").decode() or f"status {rc}")

    def msm(self, bases, scalars, form=FORM_STD, inf=None):
        bases, scalars = _words(bases, 16), _words(scalars, 8)
        if bases.shape[0] == 0 or scalars.shape[0] == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        n = min(bases.shape[0], scalars.shape[0])
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = inf.ctypes.data_as(_u8p)
        jac, aff, oi = np.zeros(24, np.uint32), np.zeros(16, np.uint32), C.c_uint8(0)
        self._check(self._lib.msm_bn254_g1_multi(self._h, _p32(bases), form, infp, _p32(scalars), n, _p32(jac), _p32(aff), C.byref(oi)))
        return MsmResult(jac, aff, oi.value)

    def msm_arkworks(self, raw_structs, stride, x_off, y_off, inf_off, scalars_mont):
        raw = np.ascontiguousarray(raw_structs, dtype=np.uint8).reshape(-1)
        sc = _words(scalars_mont, 8)
        n = min(raw.size // stride, sc.shape[0])
        if n == 0:
            raise MsmError(ERR_EMPTY, "Empty input")
        jac, aff, oi = np.zeros(24, np.uint32), np.zeros(16, np.uint32), C.c_uint8(0)
        self._check(self._lib.msm_bn254_g1_multi_arkworks(self._h, raw.ctypes.data_as(C.c_void_p), stride, x_off, y_off,
                                                          inf_off if inf_off is not None else C.c_size_t(-1).value, _p32(sc), n,
                                                          _p32(jac), _p32(aff), C.byref(oi)))
        return MsmResult(jac, aff, oi.value)

    def msm_device(self, d_bases_ptrs, d_scalars_ptrs, counts, d_inf_ptrs=None):
        """shard g already sits in device g's HBM: raw device pointers and point counts per device"""
        G = self.num_devices
        assert len(d_bases_ptrs) == G and len(d_scalars_ptrs) == G and len(counts) == G
        vpa = C.c_void_p * G
        pb, ps = vpa(*d_bases_ptrs), vpa(*d_scalars_ptrs)
        pi = vpa(*d_inf_ptrs) if d_inf_ptrs is not None else None
        cn = (C.c_size_t * G)(*counts)
        jac, oi = np.zeros(24, np.uint32), C.c_uint8(0)
        self._check(self._lib.msm_bn254_g1_multi_device(self._h, pb, pi, ps, cn, _p32(jac), None, C.byref(oi)))
        return MsmResult(jac, None, oi.value)

    def timings(self, g=0):
        t = Timings()
        self._check(self._lib.msm_multi_get_timings(self._h, g, C.byref(t)))
        return t.as_dict()

    def exchange_stats(self):
        """(exchange ms of rank 0, [wall-clock ms of every rank's local MSM]) of the last call"""
        ex = C.c_float(0)
        sh = (C.c_float * self.num_devices)()
        self._check(self._lib.msm_multi_get_exchange_stats(self._h, C.byref(ex), sh, self.num_devices))
        return float(ex.value), [float(v) for v in sh]

    def set_kernel_timing(self, every_n):
        self._check(self._lib.msm_multi_set_kernel_timing(self._h, every_n))

    def clock_stats(self, g=0):
        """msm_get_clock_stats of rank g's context: {"sclk_ghz", "cycles_per_addition", "samples"}"""
        a, b, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
        self._check(self._lib.msm_multi_get_clock_stats(self._h, g, C.byref(a), C.byref(b), C.byref(n)))
        return {"sclk_ghz": a.value, "cycles_per_addition": b.value, "samples": n.value}

    def exchange_probe(self):
        """(rccl ms, host-fold ms) per exchange that EXCHANGE_AUTO measured when the handle was created; (0, 0) = nothing was probed"""
        a, b = C.c_float(0), C.c_float(0)
        self._check(self._lib.msm_multi_get_exchange_probe(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)


_default_ctx = None


def default_context():
    """Process-global lazily created context, as the Rust shim keeps."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = MsmContext()
    return _default_ctx


def hip_variable_base_msm(bases, scalars, form=FORM_STD, inf=None):
    """Drop-in for metal_variable_base_msm(&bases, &scalars) (metal_msm.rs:642-695)."""
    return default_context().msm(bases, scalars, form, inf)


def hip_variable_base_msm_g2(bases, scalars, form=FORM_STD, inf=None):
    """The G2 counterpart on the process-global context (the Groth16 B query)."""
    return default_context().msm_g2(bases, scalars, form, inf)


metal_variable_base_msm = hip_variable_base_msm  # the reference's own name, kept as an alias
