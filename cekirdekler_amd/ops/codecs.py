"""The element formats of the GEMM operands as numpy codecs: bf16, OCP e4m3fn
and e2m1 bit patterns, E8M0 scale bytes, the e2m1 nibble packing, and the two
OCP Microscaling block formats built from them (MXFP8, MXFP4).  Pure numpy;
the executable specification the kernels and the device quantisers are held
against."""
from __future__ import annotations

import numpy as np

MX_BLOCK = 32  # elements per scale along K


def to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 → bf16 bit patterns (round to nearest even), as uint16.  A NaN
    stays a NaN: its sign and top 7 payload bits are kept and the quiet bit is
    set (the rounding increment would carry a NaN with a low payload into
    ±Inf or ±0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> 16) | np.uint32(0x0040)).astype(np.uint16), r)


def from_bf16_bits(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def _fp8_e4m3_table() -> np.ndarray:
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e - 7.0))
    v[(c & 0x7F) == 0x7F] = np.nan
    return np.where(c & 0x80, -v, v).astype(np.float32)


_FP8_E4M3 = _fp8_e4m3_table()
FP8_E4M3_EMAX = 8  # exponent of e4m3's largest binade (256, 448)


def to_fp8_e4m3_bits(x: np.ndarray) -> np.ndarray:
    """fp32 → OCP e4m3fn bit patterns, as uint8: round to nearest even
    (subnormals included: the smallest is 2⁻⁹), NaN → ``0x7F``, the sign of
    zero kept.  Finite values beyond ±448 and ±inf SATURATE to ±448
    (``0x7E`` / ``0xFE``); torch's CPU conversion turns what rounds past 448
    into NaN instead, and agrees bit for bit everywhere else."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    sign = ((u >> 24) & np.uint32(0x80)).astype(np.uint8)
    # normal range: nearest even at 3 mantissa bits, exponent rebiased 127 → 7
    norm = ((a + np.uint32(0x7FFFF) + ((a >> 20) & np.uint32(1))) >> 20).astype(np.int64) - (120 << 3)
    # below 2⁻⁶: units of 2⁻⁹ (8 units = code 0x08 = 2⁻⁶, the first normal)
    small = a < np.uint32(0x3C800000)
    sub = np.rint(np.where(small, a, np.uint32(0)).view(np.float32) * np.float32(512.0)).astype(np.int64)
    code = np.where(small, sub, norm)
    code = np.where(a >= np.uint32(0x43E00000), 0x7E, code).astype(np.uint8) | sign  # |x| >= 448, inf
    return np.where(a > np.uint32(0x7F800000), np.uint8(0x7F), code).astype(np.uint8)


def from_fp8_e4m3_bits(b: np.ndarray) -> np.ndarray:
    """OCP e4m3fn bit patterns (uint8) → fp32 (``0x7F`` / ``0xFF`` → NaN)."""
    return _FP8_E4M3[np.asarray(b, dtype=np.uint8)]


def e8m0_to_f64(scales: np.ndarray) -> np.ndarray:
    """E8M0 scale bytes → float64 ``2^(byte − 127)``, exact (``0xFF`` → NaN)."""
    s = np.asarray(scales, dtype=np.uint8)
    return np.where(s == 0xFF, np.nan, np.ldexp(1.0, s.astype(np.int64) - 127))


# OCP e2m1 (MXFP4's element): code s e e m
_FP4_E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                      -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], np.float32)
# the midpoints between neighbouring magnitudes; a value on midpoint i lies
# between codes i and i + 1 and goes to the even one
_FP4_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
FP4_E2M1_EMAX = 2  # exponent of e2m1's largest binade (4, 6)


def _f32_or_f64(x) -> np.ndarray:
    """``x`` contiguous, float64 if it came as float64 and float32 otherwise."""
    x = np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float64 if x.dtype == np.float64 else np.float32)


def to_fp4_e2m1_codes(x: np.ndarray) -> np.ndarray:
    """fp32 (or fp64) → OCP e2m1 codes 0..15, one per element, as uint8: bit
    layout ``s e e m``, codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6 and 8..15 their
    negatives (−0 kept).  Round to nearest even (a value halfway between two
    neighbours goes to the one whose mantissa bit is 0); finite values beyond
    ±6 and ±inf SATURATE to ±6.  e2m1 has no NaN: a NaN gives code 0."""
    x = _f32_or_f64(x)
    a = np.abs(x)
    code = np.zeros(x.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        for i, mid in enumerate(_FP4_MIDPOINTS):
            code += (a >= mid) if i % 2 else (a > mid)
    nan = np.isnan(x)
    return np.where(nan, np.uint8(0), code | (np.signbit(x).astype(np.uint8) << 3)).astype(np.uint8)


def from_fp4_e2m1_codes(c: np.ndarray) -> np.ndarray:
    """OCP e2m1 codes (uint8, 0..15, one per element) → fp32, by table."""
    c = np.asarray(c, dtype=np.uint8)
    if c.size and int(c.max()) > 15:
        raise ValueError("e2m1 codes are 0..15")
    return _FP4_E2M1[c]


def pack_fp4(codes: np.ndarray) -> np.ndarray:
    """e2m1 codes ``[..., K]`` (0..15) → packed bytes ``[..., K/2]``: element
    ``2i`` in bits 0–3 of byte ``i``, element ``2i + 1`` in bits 4–7 (the
    public layout of every fp4x2 array)."""
    c = np.asarray(codes, dtype=np.uint8)
    if c.shape[-1] % 2:
        raise ValueError(f"the last axis ({c.shape[-1]}) must be even")
    if c.size and int(c.max()) > 15:
        raise ValueError("e2m1 codes are 0..15")
    return (c[..., 0::2] | (c[..., 1::2] << 4)).astype(np.uint8)


def unpack_fp4(packed: np.ndarray) -> np.ndarray:
    """Inverse of :func:`pack_fp4`: bytes ``[..., K/2]`` → codes ``[..., K]``."""
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack((p & 15, p >> 4), axis=-1).reshape(p.shape[:-1] + (2 * p.shape[-1],))


def _mx_blocks(x: np.ndarray, block: int, emax: int):
    """The block step of :func:`to_mxfp8` and :func:`to_mxfp4`: ``x`` in
    float64 blocks ``[..., K/block, block]``, and per block the shared
    exponent ``floor(log2(max |x| over the block's finite values)) − emax``,
    clamped to [−127, 127] and 0 for a block without a finite nonzero value
    (``emax``: the exponent of the element format's largest binade)."""
    K = x.shape[-1]
    xb = x.reshape(x.shape[:-1] + (K // block, block)).astype(np.float64)
    amax = np.where(np.isfinite(xb), np.abs(xb), 0.0).max(axis=-1)
    _, ex = np.frexp(amax)  # amax = m · 2^ex, 0.5 <= m < 1: floor(log2 amax) = ex − 1
    return xb, np.clip(np.where(amax > 0, ex.astype(np.int64) - 1 - emax, 0), -127, 127)


def _mx_scaled(v: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """Decoded elements ``v`` (``[..., K]``) times their blocks' E8M0 scales
    (``[..., K/block]``), the product taken in float64, as float32."""
    nb = scales.shape[-1]
    vb = v.astype(np.float64).reshape(scales.shape + (v.shape[-1] // nb,))
    with np.errstate(over="ignore", invalid="ignore"):
        return (vb * e8m0_to_f64(scales)[..., None]).astype(np.float32).reshape(v.shape)


def to_mxfp8(x: np.ndarray, block: int = MX_BLOCK):
    """OCP Microscaling (MX v1.0) MXFP8 along the last axis: ``(codes uint8
    [..., K], scales uint8 [..., K/block])``.  Per block the shared exponent is
    ``e = floor(log2(max |x| over the block's finite values)) − 8`` (8: the
    exponent of e4m3's largest binade), clamped to [−127, 127], the scale byte
    ``e + 127`` and the elements ``to_fp8_e4m3_bits(x · 2^−e)``: round to
    nearest even, saturating, so scaled values in (448, 512) become ±448.  A
    block without a finite nonzero value gets byte 127; NaN → ``0x7F`` without
    a say in the scale; ±inf → ±448.  ``0xFF`` (E8M0 NaN) is never produced.
    ``x`` is taken as float32 (float64 is kept for the scale and the scaling,
    the element rounding then goes through float32)."""
    x = _f32_or_f64(x)
    K = x.shape[-1]
    if block <= 0 or K % block:
        raise ValueError(f"the last axis ({K}) must be a multiple of the block ({block})")
    xb, e = _mx_blocks(x, block, FP8_E4M3_EMAX)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = np.ldexp(xb, -e[..., None]).astype(np.float32)
    return to_fp8_e4m3_bits(scaled).reshape(x.shape), (e + 127).astype(np.uint8)


def from_mxfp8(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """MXFP8 → float32: ``e4m3(code) · 2^(scale − 127)`` with one scale per
    ``K / scales.shape[-1]`` elements of the last axis.  (The product is taken
    in float64; what float32 cannot hold rounds, overflows or underflows.)"""
    return _mx_scaled(from_fp8_e4m3_bits(np.asarray(codes, np.uint8)), np.asarray(scales, np.uint8))


def to_mxfp4(x: np.ndarray, block: int = MX_BLOCK):
    """OCP Microscaling (MX v1.0) MXFP4 along the last axis: ``(packed uint8
    [..., K/2], scales uint8 [..., K/block])``, the elements packed as
    :func:`pack_fp4` does.  Per block the shared exponent is ``e = floor(log2(max
    |x| over the block's finite values)) − 2`` (2: the exponent of e2m1's
    largest binade), clamped to [−127, 127], the scale byte ``e + 127`` and the
    elements ``to_fp4_e2m1_codes(x · 2^−e)``: round to nearest even,
    saturating, so scaled values in (6, 8) become ±6.  A block without a
    finite nonzero value gets byte 127; ±inf → ±6 without a say in the scale.

    NaN: e2m1 has no NaN code, so a NaN cannot stay in its element.  A block
    that contains a NaN gets the scale byte ``0xFF`` (E8M0 NaN), which makes
    the WHOLE block NaN in OCP MX (:func:`from_mxfp4`, the kernels); its NaN
    elements get code 0 and its other elements the codes they would have had.
    (:func:`to_mxfp8` never produces ``0xFF``: e4m3 has a NaN of its own.)

    The scaling and the element rounding are done in float64, where both are
    exact for float32 and float64 input alike."""
    x = _f32_or_f64(x)
    K = x.shape[-1]
    if block <= 0 or block % 2 or K % block:
        raise ValueError(f"the last axis ({K}) must be a multiple of the block ({block}), the block even")
    xb, e = _mx_blocks(x, block, FP4_E2M1_EMAX)
    with np.errstate(over="ignore", invalid="ignore"):
        codes = to_fp4_e2m1_codes(np.ldexp(xb, -e[..., None]))
    scales = np.where(np.isnan(xb).any(axis=-1), 0xFF, e + 127).astype(np.uint8)
    return pack_fp4(codes.reshape(x.shape)), scales


def from_mxfp4(packed: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """MXFP4 → float32: ``e2m1(code) · 2^(scale − 127)`` with one scale per
    ``K / scales.shape[-1]`` elements of the last axis, K twice the packed
    length; a scale byte ``0xFF`` makes its whole block NaN.  (The product is
    taken in float64; what float32 cannot hold rounds, overflows or underflows.)"""
    return _mx_scaled(from_fp4_e2m1_codes(unpack_fp4(packed)), np.asarray(scales, np.uint8))
