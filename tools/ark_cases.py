"""Inputs of the arkworks struct-array entry (msm_bn254_g1_arkworks) as the tests build them: the byte image of a [G1Affine] slice and Fr scalars in
Montgomery form.  Shared by tests/test_gpu_1_parity.py and tests/test_gpu_21_context_state.py."""
import numpy as np

from oracle import bn254_oracle as orc

R256 = 1 << 256


def ark_image(bases_std, inf, stride, x_off, y_off, inf_off, rng):
    """byte image of a [G1Affine] slice: Fq Montgomery limbs at x_off / y_off, `infinity` bool at inf_off, garbage in
    the padding (arkworks' identity is x = y = 0, infinity = true)"""
    n = bases_std.shape[0]
    img = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    for i in range(n):
        x = orc.words_to_int(bases_std[i, :8]) * R256 % orc.P
        y = orc.words_to_int(bases_std[i, 8:]) * R256 % orc.P
        if inf is not None and inf[i]:
            x = y = 0
        img[i, x_off:x_off + 32] = np.frombuffer(x.to_bytes(32, "little"), np.uint8)
        img[i, y_off:y_off + 32] = np.frombuffer(y.to_bytes(32, "little"), np.uint8)
        if inf_off is not None:
            img[i, inf_off] = 1 if (inf is not None and inf[i]) else 0
    return img


def ark_image_of_mont_words(bases_mont, inf, rng, stride=72):
    """the same image for bases that already are arkworks words (n x 16 Montgomery words), layout (stride, 0, 32, 64): no per-point Python work"""
    n = bases_mont.shape[0]
    img = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    img[:, :64] = np.ascontiguousarray(bases_mont, dtype=np.uint32).view(np.uint8).reshape(n, 64)
    img[:, 64] = 0
    if inf is not None:
        flagged = np.asarray(inf) != 0
        img[flagged, :64] = 0
        img[flagged, 64] = 1
    return img


def fr_mont(scalars):
    """standard-form Fr words (n x 8) -> arkworks Montgomery words"""
    return np.stack([orc.int_to_words(orc.words_to_int(s) * R256 % orc.R_ORDER) for s in scalars])
