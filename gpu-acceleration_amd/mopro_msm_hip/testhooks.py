"""Test, benchmark and calibration hooks (include/msm_hip_testhooks.h) -- NOT part of the product.

They live in a second build of the same sources, gpu-acceleration_amd/libmsm_hip_hooks.so (-DMSM_HIP_TEST_HOOKS), which also
contains the whole engine: a HooksContext is an MsmContext on that build plus the hooks.  Users: tests/, bench.py (input
generation, multiplier calibration), tools/.  The product library libmsm_hip.so exports none of these symbols.
"""
import ctypes as C
import os

import numpy as np

from . import (ERR_NO_DEVICE, FLAG_NO_GLV, MsmContext, MsmError, _p32, _preload_torch, _u8p, _u32p, _words, bind_product_abi, plan)

_HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS_LIB_PATH = os.environ.get("MSM_HIP_HOOKS_LIB") or os.path.join(os.path.dirname(_HERE), "libmsm_hip_hooks.so")

HOOK_SYMBOLS = [
    "msm_bn254_g1_generate_device", "msm_bn254_generate_scalars_host", "msm_test_fp_op", "msm_test_g1_op",
    "msm_test_decompose", "msm_calibrate", "msm_test_stage_dump", "msm_test_abandon_after_sort",
    "msm_probe_wide_level", "msm_probe_launch_chain", "msm_probe_empty_launch", "msm_test_get_list_counts", "msm_probe_reduce_bits",
    "msm_test_g2_sqrt", "msm_test_ntt_set_tile_log2", "msm_test_g2_op", "msm_test_g1_raw_op",
    "msm_test_fr_raw_op", "msm_test_fq_raw_op", "msm_test_fq2_raw_op", "msm_test_fr_scan_set_chain",
]
OP_G2_MADD, OP_G2_ADD, OP_G2_DBL = 0, 1, 2  # MSM_OP_G2_* of include/msm_hip_testhooks.h
# MSM_OP_G1_RAW_* of include/msm_hip_testhooks.h
(OP_G1_RAW_MADD, OP_G1_RAW_MADD_NEG_RAW, OP_G1_RAW_MADD_M256, OP_G1_RAW_MADD_M256_NEG, OP_G1_RAW_ADD, OP_G1_RAW_DBL, OP_G1_RAW_ADD_WIDE_LDS,
 OP_G1_RAW_ADD_WIDE_HBM) = range(8)
G1_RAW_B_WORDS = {OP_G1_RAW_MADD: 18, OP_G1_RAW_MADD_NEG_RAW: 18, OP_G1_RAW_MADD_M256: 16, OP_G1_RAW_MADD_M256_NEG: 16, OP_G1_RAW_ADD: 36,
                  OP_G1_RAW_DBL: 0, OP_G1_RAW_ADD_WIDE_LDS: 36, OP_G1_RAW_ADD_WIDE_HBM: 36}  # words per element of b
# MSM_OP_FR_RAW_* of include/msm_hip_testhooks.h
FR_RAW_OPS = ("MUL", "ADD", "SUB2", "SUB3", "SUB7", "SUB8", "NORMALIZE", "REDUCE_LT2R", "CANONICAL", "UNPACK", "PACK", "FROM_STD", "TO_STD", "POW_U32",
              "INV")
(OP_FR_RAW_MUL, OP_FR_RAW_ADD, OP_FR_RAW_SUB2, OP_FR_RAW_SUB3, OP_FR_RAW_SUB7, OP_FR_RAW_SUB8, OP_FR_RAW_NORMALIZE, OP_FR_RAW_REDUCE_LT2R,
 OP_FR_RAW_CANONICAL, OP_FR_RAW_UNPACK, OP_FR_RAW_PACK, OP_FR_RAW_FROM_STD, OP_FR_RAW_TO_STD, OP_FR_RAW_POW_U32, OP_FR_RAW_INV) = range(15)
FR_RAW_NEEDS_B = (OP_FR_RAW_MUL, OP_FR_RAW_ADD, OP_FR_RAW_SUB2, OP_FR_RAW_SUB3, OP_FR_RAW_SUB7, OP_FR_RAW_SUB8, OP_FR_RAW_POW_U32)
# MSM_OP_FQ_RAW_* / MSM_OP_FQ2_RAW_* of include/msm_hip_testhooks.h: op = kind | K << 8
FQ_RAW_KINDS = ("MUL", "SQR", "MUL_ADD", "ADD", "DBL", "SUB", "NEG", "SUB_B_2C", "NORMALIZE", "REDUCE_LT2P", "CANONICAL", "INV", "IS_ZERO_LT2P", "UNPACK",
                "UNPACK_SHL5", "FROM_MONT256", "FROM_STD", "PACK", "TO_MONT256", "TO_STD", "MUL_NEG_RAW2", "NORMALIZE_NEG_RAW2", "SUB6_NEG_RAW4", "Y3")
FQ_RAW_ARITY = {"MUL": 2, "ADD": 2, "SUB": 2, "MUL_NEG_RAW2": 2, "SUB6_NEG_RAW4": 2, "SUB_B_2C": 3, "MUL_ADD": 4, "Y3": 5}  # records; the rest 1
FQ_RAW_K = {"SUB": (2, 3, 4, 5, 6, 7, 8), "NEG": (2, 3, 4, 6), "Y3": (3, 6)}  # the pad multiples instantiated; the other kinds take K = 0
FQ2_RAW_KINDS = ("MUL", "SQR", "SUB", "NEG", "ADD", "DBL", "MUL_FP", "IS_ZERO_LT2P", "IS_ZERO_ANY", "NEG_RAW6_MUL_ONE", "NEG_RAW6_MUL_FP", "CONJ")
FQ2_RAW_WORDS = {"MUL": 36, "SUB": 36, "ADD": 36, "MUL_FP": 27, "NEG_RAW6_MUL_FP": 27}  # words of an element; the rest 18
FQ2_RAW_K = {"MUL": (3, 4, 6, 7, 9, 10, 13, 15, 16, 17), "SQR": (3, 5, 6, 12, 13, 15, 16, 17), "SUB": (2, 3, 4, 5, 6, 7, 8, 9, 12, 13), "NEG": (2, 8),
             "CONJ": (9, 13)}


def fq_raw_op(kind, k=0):
    """the op word of msm_test_fq_raw_op: kind (a name of FQ_RAW_KINDS) | K << 8"""
    return FQ_RAW_KINDS.index(kind) | k << 8


def fq2_raw_op(kind, k=0):
    return FQ2_RAW_KINDS.index(kind) | k << 8


def _raw_words(op, kinds, ks, words_of):
    """the words of an element of `op`, ValueError for a kind or a K that is not instantiated"""
    kind, k = op & 0xFF, op >> 8
    if not 0 <= kind < len(kinds) or k not in ks.get(kinds[kind], (0,)):
        raise ValueError(f"unknown raw op {op} (kind {kind}, K {k})")
    return words_of(kinds[kind])


def _elements(operands, words):
    """n x words: a row of another width (a record missing, or one too many) is refused instead of being reshaped into other elements"""
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != words:
        raise ValueError(f"operands must be n x {words} words, got {a.shape}")
    return a


_lib = None


def hooks_plan(n, window_bits=0, flags=0):
    """msm_plan of the HOOKS build: the one that reads the test / A-B knobs (MSM_HIP_GLV_MAX_LOG2, MSM_HIP_TABLE_* ...); the product's reads none"""
    return plan(n, window_bits, flags, _lib=load_hooks_library())


def load_hooks_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HOOKS_LIB_PATH):
        raise MsmError(ERR_NO_DEVICE, f"{HOOKS_LIB_PATH} not built: make -C gpu-acceleration_amd/csrc hooks")
    _preload_torch()
    L = bind_product_abi(C.CDLL(HOOKS_LIB_PATH))
    vp = C.c_void_p
    L.msm_bn254_g1_generate_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_size_t, vp, vp]
    L.msm_bn254_generate_scalars_host.argtypes = [C.c_uint64, C.c_size_t, C.c_int, _u32p]
    L.msm_test_fp_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, _u32p, C.c_size_t]
    L.msm_test_g1_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, _u32p, C.c_size_t]
    L.msm_test_g2_sqrt.argtypes = [vp, _u32p, _u8p, _u32p, _u8p, C.c_size_t]
    L.msm_test_g2_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, _u32p, C.c_size_t]
    L.msm_test_g1_raw_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, _u32p, C.c_size_t]
    L.msm_test_fr_raw_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, _u32p, C.c_size_t]
    L.msm_test_fq_raw_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, C.c_size_t]
    L.msm_test_fq2_raw_op.argtypes = [vp, C.c_uint32, _u32p, _u32p, C.c_size_t]
    L.msm_test_decompose.argtypes = [vp, _u32p, C.c_size_t, C.c_uint32, C.POINTER(C.c_int32)]
    L.msm_test_abandon_after_sort.argtypes = [vp, _u32p, C.c_size_t]
    L.msm_calibrate.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.msm_probe_wide_level.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_longlong)]
    L.msm_probe_launch_chain.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.msm_probe_empty_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.msm_test_get_list_counts.argtypes = [vp, _u32p]
    L.msm_test_ntt_set_tile_log2.argtypes = [vp, C.c_uint32]
    L.msm_test_fr_scan_set_chain.argtypes = [vp, C.c_uint32]
    L.msm_probe_reduce_bits.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.msm_test_stage_dump.argtypes = [vp, _u32p, C.c_uint32, _u8p, _u32p, C.c_size_t, _u32p, _u32p, _u32p, _u32p, _u32p,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _u32p]
    for name in HOOK_SYMBOLS:
        getattr(L, name).restype = C.c_int32
    _lib = L
    return L


def generate_scalars_host(seed, n, nonzero=False):
    """element i of SplitMix64 stream `seed` reduced below r -- the k_i / s_i of the synthetic instances, on the host"""
    out = np.zeros((n, 8), np.uint32)
    load_hooks_library().msm_bn254_generate_scalars_host(seed, n, int(nonzero), _p32(out))
    return out


class StageDump:
    """intermediates of one pipeline run (msm_test_stage_dump)"""


class HooksContext(MsmContext):
    """MsmContext on the hooks build + the hooks themselves"""
    _loader = staticmethod(lambda: load_hooks_library())

    def generate_device(self, base_seed, scalar_seed, n, d_bases_ptr, d_scalars_ptr):
        """synthetic instance straight into device memory: bases k_i*G (Montgomery words), scalars s_i (counterpart of
        test_utils::generate_random_bases_and_scalars, metal_msm.rs:698-731)"""
        self._check(self._lib.msm_bn254_g1_generate_device(self._h, base_seed, scalar_seed, n, d_bases_ptr, d_scalars_ptr))

    # -- device-math unit-test hooks -----------------------------------------------------------
    def test_fp_op(self, op, a, b=None):
        a = _words(a, 8)
        b = _words(b, 8) if b is not None else None
        out = np.zeros_like(a)
        self._check(self._lib.msm_test_fp_op(self._h, op, _p32(a), _p32(b), _p32(out), a.shape[0]))
        return out

    def test_g1_op(self, op, a, b=None):
        a = _words(a, 24)
        b = _words(b, 16 if op in (0, 4, 5) else 24) if b is not None else None  # (0, 4, 5: mixed additions, b affine)
        out = np.zeros_like(a)
        self._check(self._lib.msm_test_g1_op(self._h, op, _p32(a), _p32(b), _p32(out), a.shape[0]))
        return out

    def test_g2_sqrt(self, a_std, want_larger):
        """k_g2_decompress's root-and-sign routine on Fq2 values (n x 16 standard-form words): (roots n x 16 standard-form words, ok n bytes)"""
        a = _words(a_std, 16)
        want = np.ascontiguousarray(want_larger, dtype=np.uint8)
        out, ok = np.zeros_like(a), np.zeros(a.shape[0], np.uint8)
        self._check(self._lib.msm_test_g2_sqrt(self._h, _p32(a), want.ctypes.data_as(_u8p), _p32(out), ok.ctypes.data_as(_u8p), a.shape[0]))
        return out, ok

    def test_g2_op(self, op, a, b=None):
        """the G2 group law on raw limb records (msm_test_g2_op): a n x 72 limbs (XYZZ over Fq2, 9 x 29-bit limbs per component, internal domain, any
        representative within the bounds of ec_g2_bn254.hpp), b n x 36 (OP_G2_MADD: affine), n x 72 (OP_G2_ADD) or None (OP_G2_DBL) -> n x 72 limbs,
        exactly what the device stored"""
        if op not in (OP_G2_MADD, OP_G2_ADD, OP_G2_DBL):
            raise ValueError(f"unknown G2 op {op}")
        a = _words(a, 72)
        if op == OP_G2_DBL:
            b = None
        else:  # the C hook reads n records of b: a missing or shorter b must not reach it
            if b is None:
                raise ValueError("OP_G2_MADD / OP_G2_ADD need b")
            b = _words(b, 36 if op == OP_G2_MADD else 72)
            if b.shape[0] != a.shape[0]:
                raise ValueError(f"a holds {a.shape[0]} records, b {b.shape[0]}")
        out = np.zeros_like(a)
        self._check(self._lib.msm_test_g2_op(self._h, op, _p32(a), _p32(b), _p32(out), a.shape[0]))
        return out

    def test_g1_raw_op(self, op, a, b=None):
        """the G1 group law on raw limb records (msm_test_g1_raw_op): a n x 36 limbs (X, Y, ZZ, ZZZ, 9 x 29-bit limbs each, internal domain, any
        representative within the bounds of ec_bn254.hpp), b n x G1_RAW_B_WORDS[op] words (18 limbs x, y: the mixed additions; 16 words of any
        value: the M256 ones; a second record: the additions; None: OP_G1_RAW_DBL) -> n x 36 limbs, exactly what the device stored"""
        if op not in G1_RAW_B_WORDS:
            raise ValueError(f"unknown raw G1 op {op}")
        a = _words(a, 36)
        if op == OP_G1_RAW_DBL:
            b = None
        else:  # the C hook reads n records of b: a missing or shorter b must not reach it
            if b is None:
                raise ValueError("every raw G1 op but OP_G1_RAW_DBL needs b")
            b = _words(b, G1_RAW_B_WORDS[op])
            if b.shape[0] != a.shape[0]:
                raise ValueError(f"a holds {a.shape[0]} records, b {b.shape[0]}")
        out = np.zeros_like(a)
        self._check(self._lib.msm_test_g1_raw_op(self._h, op, _p32(a), _p32(b), _p32(out), a.shape[0]))
        return out

    def test_fr_raw_op(self, op, a, b=None):
        """the scalar field on raw limb records (msm_test_fr_raw_op): a n x 9 words (9 x 29-bit limbs, any representative fr_bn254.hpp allows for
        the operation; the 8 words of a 256-bit pattern and an ignored ninth for OP_FR_RAW_UNPACK / _FROM_STD), b n x 9 words for the operations of
        FR_RAW_NEEDS_B (a second record; OP_FR_RAW_POW_U32: the exponent in b[i][0]) -> n x 9 words, exactly what the device stored (word 8 is 0
        where the function writes 8 words: OP_FR_RAW_PACK / _TO_STD)"""
        if op not in range(len(FR_RAW_OPS)):
            raise ValueError(f"unknown raw Fr op {op}")
        a = _words(a, 9)
        if op not in FR_RAW_NEEDS_B:
            b = None
        else:  # the C hook reads n records of b: a missing or shorter b must not reach it
            if b is None:
                raise ValueError("MUL, ADD, SUB<K> and POW_U32 need b")
            b = _words(b, 9)
            if b.shape[0] != a.shape[0]:
                raise ValueError(f"a holds {a.shape[0]} records, b {b.shape[0]}")
        out = np.zeros_like(a)
        self._check(self._lib.msm_test_fr_raw_op(self._h, op, _p32(a), _p32(b), _p32(out), a.shape[0]))
        return out

    def test_fq_raw_op(self, op, operands):
        """the base field on raw limb records (msm_test_fq_raw_op): op = fq_raw_op(kind, K); operands n x (ARITY * 9) words, the records of an
        element one after the other (9 x 29-bit limbs each, any representative fp_bn254.hpp allows for the operation; the 8 words of a 256-bit
        pattern and an ignored ninth for UNPACK, UNPACK_SHL5, FROM_MONT256, FROM_STD) -> n x 9 words, exactly what the device stored (word 8 is 0
        where the function writes 8 words: PACK, TO_MONT256, TO_STD)"""
        words = _raw_words(op, FQ_RAW_KINDS, FQ_RAW_K, lambda kind: 9 * FQ_RAW_ARITY.get(kind, 1))
        a = _elements(operands, words)  # the C hook reads n x words: a shorter row must not reach it
        out = np.zeros((a.shape[0], 9), np.uint32)
        self._check(self._lib.msm_test_fq_raw_op(self._h, op, _p32(a), _p32(out), a.shape[0]))
        return out

    def test_fq2_raw_op(self, op, operands):
        """Fq2 on raw limb records (msm_test_fq2_raw_op): op = fq2_raw_op(kind, K); operands n x FQ2_RAW_WORDS words (records of 18 words c0 c1;
        the Fq operand of MUL_FP / NEG_RAW6_MUL_FP is 9 words) -> n x 18 words, exactly what the device stored"""
        words = _raw_words(op, FQ2_RAW_KINDS, FQ2_RAW_K, lambda kind: FQ2_RAW_WORDS.get(kind, 18))
        a = _elements(operands, words)
        out = np.zeros((a.shape[0], 18), np.uint32)
        self._check(self._lib.msm_test_fq2_raw_op(self._h, op, _p32(a), _p32(out), a.shape[0]))
        return out

    def ntt_set_tile_log2(self, tile_log2):
        """the LDS tile (log2 elements) of the transforms that follow on this context: 4 or 10; 0 = the plan's own"""
        self._check(self._lib.msm_test_ntt_set_tile_log2(self._h, tile_log2))

    def fr_scan_set_chain(self, chain):
        """the elements per lane of the scalar-field scans that follow on this context: 1 or 8; 0 = the plan's own"""
        self._check(self._lib.msm_test_fr_scan_set_chain(self._h, chain))

    def abandon_after_sort(self, scalars):
        """decomposition + sort + piece plan of an MSM on `scalars`, then the failure a copy / event wait in front of the accumulation would be:
        raises MsmError(ERR_HIP); the context is left as that failure leaves it"""
        scalars = _words(scalars, 8)
        self._check(self._lib.msm_test_abandon_after_sort(self._h, _p32(scalars), scalars.shape[0]))

    def calibrate(self):
        """(v_mad_u64_u32 per second, field multiplications per second) this device sustains -- two ~1 ms micro-kernels."""
        a, b = C.c_double(0), C.c_double(0)
        self._check(self._lib.msm_calibrate(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def probe_wide_level(self, threads, m, iters, mode):
        """one workgroup, `iters` pairwise levels over m records in LDS (msm_probe_wide_level): 18 counters, see include/msm_hip_testhooks.h"""
        out = (C.c_longlong * 18)()
        self._check(self._lib.msm_probe_wide_level(self._h, threads, m, iters, mode, out))
        return [int(v) for v in out]

    def probe_empty_launch(self, blocks, threads, lds_kb, launches=200):
        """microseconds per dependent launch of an empty kernel of blocks x threads with lds_kb of static LDS per workgroup"""
        us = C.c_double(0)
        self._check(self._lib.msm_probe_empty_launch(self._h, blocks, threads, lds_kb, launches, C.byref(us)))
        return us.value

    def probe_reduce_bits(self, parts, launches=100):
        """microseconds per launch of k_reduce_bits_wide<parts> on the 2^20 shape (bit 0 staging, 1 tree, 2 final conversion)"""
        us = C.c_double(0)
        self._check(self._lib.msm_probe_reduce_bits(self._h, parts, launches, C.byref(us)))
        return us.value

    def list_counts(self):
        """{"long", "mid", "pieces", "partials", "mid2"}: the list counters the last sort chain / accumulation left on the device"""
        out = np.zeros(5, np.uint32)
        self._check(self._lib.msm_test_get_list_counts(self._h, _p32(out)))
        return dict(zip(("long", "mid", "pieces", "partials", "mid2"), (int(v) for v in out)))

    def probe_launch_chain(self, n_adds, launches):
        """microseconds per dependent launch of k_pair_level_wide over n_adds additions (0: an empty kernel)"""
        us = C.c_double(0)
        self._check(self._lib.msm_probe_launch_chain(self._h, n_adds, launches, C.byref(us)))
        return us.value

    def test_decompose(self, scalars, window_bits=0):
        scalars = _words(scalars, 8)
        n = scalars.shape[0]
        p = hooks_plan(n, window_bits or self.window_bits, self.flags | FLAG_NO_GLV)  # the hook returns the plain 254-bit digits
        out = np.zeros((p.num_windows, n), np.int32)
        self._check(self._lib.msm_test_decompose(self._h, _p32(scalars), n, window_bits, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def stage_dump(self, bases, scalars, form=0, inf=None, want_buckets=True):
        """run the pipeline once and return every stage's intermediates (counterpart of the reference's per-kernel tests)"""
        bases, scalars = _words(bases, 16), _words(scalars, 8)
        n = min(bases.shape[0], scalars.shape[0])
        p = hooks_plan(n, self.window_bits, self.flags)
        W, nb, nv = p.num_windows, p.num_buckets, int(p.virtual_points)
        kb = nb.bit_length() - 1
        d = StageDump()
        d.plan, d.W, d.nb, d.nv, d.kb = p, W, nb, nv, kb
        # bucket arrays (= windows without a window table), table factor, pseudo-windows of the reduction (arrays above 2^17 buckets)
        d.V, d.tf = int(p.bucket_arrays), int(p.table_factor)
        d.pw_bits = kb - 16 if kb > 17 else 0
        d.rkb = kb - d.pw_bits
        d.digits = np.zeros((W, nv), np.uint32)
        d.offsets = np.zeros(d.V * nb + 1, np.uint32)
        d.sorted = np.zeros(W * nv, np.uint32)
        d.buckets = np.zeros((d.V * nb, 24), np.uint32) if want_buckets else None
        d.bit_sums = np.zeros((d.V << d.pw_bits, d.rkb + 1, 24), np.uint32)
        d.jacobian = np.zeros(24, np.uint32)
        sp, bi = C.c_uint32(0), C.c_uint32(0)
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = inf.ctypes.data_as(_u8p)
        self._check(self._lib.msm_test_stage_dump(self._h, _p32(bases), form, infp, _p32(scalars), n, _p32(d.digits), _p32(d.offsets),
                                                  _p32(d.sorted), _p32(d.buckets) if want_buckets else None, _p32(d.bit_sums),
                                                  C.byref(sp), C.byref(bi), _p32(d.jacobian)))
        d.sort_path, d.big_items = int(sp.value), int(bi.value)
        return d
