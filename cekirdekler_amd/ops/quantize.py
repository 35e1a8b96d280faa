"""MXFP8 quantisation on the device (``kernels/mx_quantize.hip``): fp32 or
bf16 in device memory in, OCP e4m3fn codes plus one E8M0 scale byte per block
of 32 out, and the scales once more in the packed layout the MXFP8 GEMM
kernels read.  The result is :func:`cekirdekler_amd.ops.codecs.to_mxfp8`'s bit
for bit (:func:`mxfp8_reference`); :func:`mxfp8_kernel_model` is the kernels'
algorithm in integer and float32 numpy operations, the executable
specification the host tests hold against the float64 codec.

The input is ``[rows][K]`` row-major with K % 32 = 0, so it is a flat
sequence of ``rows·K/32`` blocks and work item i owns block i: the quantise
compute is range-partitioned by blocks (local size 64, a work-group owns 2048
consecutive elements), every device's slice of the codes and of the row-major
scales is contiguous, and on several devices both are gathered device to
device so that every replica is whole.  The packed layout is K-tile-major,
not contiguous per row slice: a second compute (one work item per packed
dword) builds it from the whole row-major scales.

MXFP4 (``kernels/mx4_quantize.hip``, :class:`MxFp4Quantizer`,
:func:`mxfp4_reference`, :func:`mxfp4_kernel_model`) is the same machinery
with e2m1 codes, two per byte, and :func:`cekirdekler_amd.ops.codecs.to_mxfp4`
as the codec; its scales go through the same pack kernel.
"""
from __future__ import annotations

import numpy as np

from ..arrays import ClArray
from ..cruncher import ClComputeError, ClNumberCruncher
from .codecs import FP4_E2M1_EMAX, FP8_E4M3_EMAX, MX_BLOCK, from_bf16_bits, pack_fp4, to_mxfp4, to_mxfp8
from .library import LIBRARY, library
from .tiling import pack_mx_scales

QUANTIZE_KERNELS = {"float32": "cek_mx_quantize_f32", "bfloat16": "cek_mx_quantize_bf16"}
QUANTIZE4_KERNELS = {"float32": "cek_mx4_quantize_f32", "bfloat16": "cek_mx4_quantize_bf16"}
PACK_KERNEL = "cek_mx_pack_scales"
LOCAL = 64  # work items (= blocks) per work-group
_SRC_NAMES = {"float32": "float32", "float": "float32", "f32": "float32", "bfloat16": "bfloat16", "bf16": "bfloat16"}


def _src_name(src) -> str:
    key = _SRC_NAMES.get(src.lower()) if isinstance(src, str) else None
    if key is None:
        raise ValueError(f"src must be 'float32' or 'bfloat16' (got {src!r})")
    return key


def _reference(codec, x) -> tuple:
    """``codec`` of the float32 input, or of the decoded values of bf16 bit
    patterns (a uint16 array or a bf16 :class:`ClArray`)."""
    if isinstance(x, ClArray):
        x = x.array
    x = np.asarray(x)
    return codec(from_bf16_bits(x) if x.dtype == np.uint16 else x.astype(np.float32, copy=False))


def mxfp8_reference(x) -> tuple:
    """What the quantise kernels compute: :func:`to_mxfp8` of the float32
    input, or of the decoded values of bf16 bit patterns (a uint16 array or a
    bf16 :class:`ClArray`): ``(codes, scales)``, blocks along the last axis."""
    return _reference(to_mxfp8, x)


def e4m3_convert_model(y: np.ndarray) -> np.ndarray:
    """gfx950's fp8 conversion of float32 ``y`` as the GPU tier found it
    (profiles/quantize_mxfp8.md), uint32 codes under the sign of ``y``: round
    to nearest even at 3 mantissa bits, below 2^-6 in units of 2^-9 (the bit
    rounding of ``aux_functions.py``'s ``cek_f32_to_fp8_e4m3``), and whatever
    rounds past 448, inf and NaN as the all-ones code 0x7f."""
    u = np.ascontiguousarray(y, np.float32).view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    s = (u >> np.uint32(24)) & np.uint32(0x80)
    c = np.minimum(a, np.uint32(0x43F00000))  # 480, where 0x7f would lie: the normal path gives 0x7f
    norm = ((c + np.uint32(0x7FFFF) + ((c >> np.uint32(20)) & np.uint32(1))) >> np.uint32(20)) - np.uint32(120 << 3)
    sub = (c.view(np.float32) * np.float32(512.0) + np.float32(8388608.0)).view(np.uint32) & np.uint32(15)
    return np.where(c < np.uint32(0x3C800000), sub, norm) | s


def _model_blocks(x, src: str, emax: int) -> tuple:
    """The kernel models' common start: ``x`` as uint32 bit patterns in blocks
    of 32 (``[blocks][32]``), their keys ``|x| bits + 2^23`` as int32, and per
    block the scale byte ``max(E − emax, 0)`` from the exponent field E of the
    finite |x| maximum (127 when that is zero or nothing is finite; ``emax``:
    the exponent of the element format's largest binade) and the float32
    multiplier ``2^-e``, bits ``(254 − byte) << 23``."""
    src = _src_name(src)
    x = np.asarray(x)
    if src == "bfloat16":
        if x.dtype != np.uint16:
            raise ValueError("bfloat16 input is given as uint16 bit patterns")
        u = x.astype(np.uint32) << np.uint32(16)
    else:
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if u.shape[-1] % MX_BLOCK:
        raise ValueError(f"the last axis ({u.shape[-1]}) must be a multiple of the block ({MX_BLOCK})")
    ub = np.ascontiguousarray(u).reshape(-1, MX_BLOCK)
    key = ((ub & np.uint32(0x7FFFFFFF)) + np.uint32(0x00800000)).view(np.int32)
    amax = (np.maximum(key.max(axis=1), np.int32(0x00800000)) - np.int32(0x00800000)).astype(np.uint32)
    field = (amax >> np.uint32(23)).astype(np.int32)
    sb = np.where(amax == 0, 127, np.maximum(field - emax, 0)).astype(np.uint32)
    mult = ((np.uint32(254) - sb) << np.uint32(23)).view(np.float32)
    return x, ub, key, sb, mult


def mxfp8_kernel_model(x, src: str = "float32") -> tuple:
    """``kernels/mx_quantize.hip`` step by step, in uint32 and float32
    operations only.  Per block: the maximum of the keys ``|x| bits + 2^23``
    as signed integers (inf and NaN are negative there, so it is the maximum
    over the finite values), the scale byte ``max(E − 8, 0)`` from that
    maximum's exponent field E (127 when it is zero or nothing is finite).
    Per element: the conversion of ``x · 2^-e`` (:func:`e4m3_convert_model`;
    one float32 multiply by ``2^-e``, bits ``(254 − byte) << 23``, always a
    normal number — the product is exact unless it underflows, where the code
    is a signed zero like the instruction's, which scales and rounds once),
    then the kernels' repair: an all-ones code becomes 0x7e under its sign
    (saturation) unless the input was a NaN, which loses its sign.  ``x``:
    float32 values, or bf16 bit patterns (uint16) with ``src="bfloat16"``;
    blocks of 32 along the last axis.  Returns ``(codes uint8 like x, scales
    uint8 [..., K/32])``."""
    x, ub, key, sb, mult = _model_blocks(x, src, FP8_E4M3_EMAX)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w = e4m3_convert_model(ub.view(np.float32) * mult[:, None])
    nan = (np.uint32(0x80000000) - key.view(np.uint32)).view(np.int32) < 0
    full = (w & np.uint32(0x7F)) == np.uint32(0x7F)
    codes = np.where(nan, np.uint32(0x7F), np.where(full, w - np.uint32(1), w))
    return codes.astype(np.uint8).reshape(x.shape), sb.astype(np.uint8).reshape(x.shape[:-1] + (-1,))


def mxfp4_reference(x) -> tuple:
    """What the MXFP4 quantise kernels compute: :func:`to_mxfp4` of the
    float32 input, or of the decoded values of bf16 bit patterns (a uint16
    array or a bf16 :class:`ClArray`): ``(packed codes [..., K/2], scales)``,
    blocks along the last axis."""
    return _reference(to_mxfp4, x)


def e2m1_convert_model(y: np.ndarray) -> np.ndarray:
    """gfx950's fp4 conversion of float32 ``y`` as the GPU tier found it
    (profiles/quantize_mxfp4.md), uint32 codes 0..15 under the sign of ``y``:
    round to nearest even at one mantissa bit, below 1 in units of 0.5, and
    whatever lies beyond 6, inf and NaN included, as the largest code 7."""
    u = np.ascontiguousarray(y, np.float32).view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    s = (u >> np.uint32(28)) & np.uint32(8)
    c = np.minimum(a, np.uint32(0x40C00000))  # 6
    norm = ((c + np.uint32(0x1FFFFF) + ((c >> np.uint32(22)) & np.uint32(1))) >> np.uint32(22)) - np.uint32(126 << 1)
    sub = (c.view(np.float32) * np.float32(2.0) + np.float32(8388608.0)).view(np.uint32) & np.uint32(3)
    return np.where(c < np.uint32(0x3F800000), sub, norm) | s


def mxfp4_kernel_model(x, src: str = "float32") -> tuple:
    """``kernels/mx4_quantize.hip`` step by step, in uint32 and float32
    operations only.  Per block: the maximum of the keys as in
    :func:`mxfp8_kernel_model`, the scale byte ``max(E − 2, 0)`` from that
    maximum's exponent field E (127 when it is zero or nothing is finite).
    Per element: the conversion of ``x · 2^-e`` (:func:`e2m1_convert_model`;
    one float32 multiply by ``2^-e``, bits ``(254 − byte) << 23``, always a
    normal number — the product is exact unless it underflows, far below
    e2m1's round-to-zero boundary 0.25, where the code is a signed zero), then
    the NaN rule: a NaN element gets code 0 without a sign and its block the
    byte ``0xFF``, the block's other elements keep their codes.  ``x``:
    float32 values, or bf16 bit patterns (uint16) with ``src="bfloat16"``;
    blocks of 32 along the last axis.  Returns ``(packed codes uint8 [...,
    K/2], scales uint8 [..., K/32])`` like :func:`to_mxfp4`."""
    x, ub, key, sb, mult = _model_blocks(x, src, FP4_E2M1_EMAX)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w = e2m1_convert_model(ub.view(np.float32) * mult[:, None])
    nan = (np.uint32(0x80000000) - key.view(np.uint32)).view(np.int32) < 0
    codes = np.where(nan, np.uint32(0), w).astype(np.uint8).reshape(x.shape)
    sb = np.where(nan.any(axis=1), np.uint32(0xFF), sb)
    return pack_fp4(codes), sb.astype(np.uint8).reshape(x.shape[:-1] + (-1,))


def relu_model(x: np.ndarray) -> np.ndarray:
    """The GEMM epilogue's ReLU (``kernels/gemm8_out.h``) on float32 bit
    patterns, in integer operations: ``x > 0`` and every NaN stay as they
    are, everything else (``-0`` included) becomes ``+0``."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    keep = (u.view(np.int32) > 0) | ((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000))
    return np.where(keep, u, np.uint32(0)).view(np.float32)


def bf16_bits_model(x: np.ndarray) -> np.ndarray:
    """The epilogue's fp32 → bf16 on bit patterns: round to nearest even on
    the integer, a NaN keeps its high half and gets the quiet bit."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint16)


def gemm_out_model(c: np.ndarray, out: str, act: str | None = None) -> tuple:
    """The output-mode epilogue of the MX GEMMs (``kernels/gemm8_out.h``)
    step by step on the fp32 ``[M][N]`` values the plain kernel would store:
    the activation, then the conversion of ``out`` (``"bfloat16"``: the
    integer rounding; ``"mxfp8"`` / ``"mxfp4"``: the quantise kernels' models,
    blocks of 32 along N), then the pack of the scales.  Returns ``(Y, SY,
    packed)``: bf16 bit patterns ``[M][N]`` with ``None, None``, or the codes
    (``[M][N]``, MXFP4 ``[M][N/2]``), the scale bytes ``[M][N/32]`` and
    :func:`~cekirdekler_amd.ops.tiling.pack_mx_scales` of them."""
    c = np.ascontiguousarray(c, np.float32)
    if act not in (None, "relu"):
        raise ValueError(f"act must be None or 'relu' (got {act!r})")
    if act == "relu":
        c = relu_model(c)
    if out == "bfloat16":
        return bf16_bits_model(c), None, None
    if out not in ("mxfp8", "mxfp4"):
        raise ValueError(f"out must be 'bfloat16', 'mxfp8' or 'mxfp4' (got {out!r})")
    codes, scales = (mxfp8_kernel_model if out == "mxfp8" else mxfp4_kernel_model)(c)
    return codes, scales, pack_mx_scales(scales)


_FLAGS = ("read", "partial_read", "write", "elements_per_work_item", "gather_resident")


class _MxQuantizer:
    """What :class:`MxFp8Quantizer` and :class:`MxFp4Quantizer` share: the
    argument checks, the arrays and the two computes.  A format names its
    quantise kernels, the libraries they and the pack kernel come from, the
    dtype of its codes and how many elements a code byte holds."""

    KERNELS: dict
    LIBS: tuple
    CODES_DTYPE: str
    PER_BYTE = 1

    def __init__(self, rows: int, K: int, src: str = "float32", devices=None,
                 cruncher: ClNumberCruncher | None = None, codes: ClArray | None = None,
                 scales: ClArray | None = None, packed: ClArray | None = None, x: ClArray | None = None):
        self.src = _src_name(src)
        rows, K = int(rows), int(K)
        if rows <= 0 or K <= 0 or K % MX_BLOCK:
            raise ValueError(f"rows and K must be positive and K % {MX_BLOCK} = 0 (got {rows}, {K})")
        self.rows, self.K = rows, K
        self.blocks = rows * K // MX_BLOCK
        if self.blocks % LOCAL:
            raise ValueError(f"the number of blocks rows*K/{MX_BLOCK} ({self.blocks}) must be a multiple of {LOCAL}")
        self.kernel = self.KERNELS[self.src]
        self.has_packed = rows % 64 == 0 and K % 128 == 0
        n = rows * K
        want = [("x", x, n, np.float32 if self.src == "float32" else np.uint16),
                ("codes", codes, n // self.PER_BYTE, np.uint8), ("scales", scales, self.blocks, np.uint8)]
        if self.has_packed:
            want.append(("packed", packed, n // 128, np.uint32))
        elif packed is not None:
            raise ValueError(f"packed scales need rows % 64 = 0 and K % 128 = 0 (got {rows}, {K})")
        for name, arr, length, dt in want:
            if arr is not None and (not isinstance(arr, ClArray) or arr.N != length or arr.array.dtype != dt):
                raise ValueError(f"{name} must be a ClArray of {length} {np.dtype(dt).name} elements")
        self.cr = cruncher or ClNumberCruncher(devices, "", prebuilt=library(*self.LIBS))
        have = {k.split(":")[0] for k in self.cr.kernel_names}
        for lib in self.LIBS:
            missing = [k for k in LIBRARY[lib] if k not in have]
            if missing:
                raise ClComputeError(f"the cruncher has no kernel {missing[0]!r}: it was built without "
                                     f"library({lib!r})")
        self.X = x if x is not None else ClArray(n, "float32" if self.src == "float32" else "bfloat16")
        self.codes = codes if codes is not None else ClArray(n // self.PER_BYTE, self.CODES_DTYPE)
        self.scales = scales if scales is not None else ClArray(self.blocks, np.uint8)
        self.packed = None
        if self.has_packed:
            self.packed = packed if packed is not None else ClArray(n // 128, np.uint32)
        self.dims = ClArray(np.array([rows, K], np.int32))
        self.records = []

    def _arrays(self) -> list:
        return [a for a in (self.X, self.codes, self.scales, self.packed, self.dims) if a is not None]

    def run(self, compute_id: int = 7001, upload: bool = True, download: bool = True, pack: bool = True,
            pack_compute_id: int | None = None) -> None:
        """One ``compute()`` of the quantise kernel over the blocks, then, with
        ``pack`` and a packed array, one of the pack kernel over the packed
        dwords under ``pack_compute_id`` (default ``compute_id + 1``).
        ``upload=False``: X is resident already (an earlier call, or another
        kernel wrote it).  ``download=False``: the outputs stay in device
        memory.  On several devices the outputs are gathered device to device:
        every device holds all of them afterwards, and the pack compute reads
        the scales as a resident whole.  ``records`` holds the computes'
        ``last_record()`` afterwards (quantise, then pack)."""
        saved = [(a, [getattr(a, f) for f in _FLAGS]) for a in self._arrays()]
        gather = self.cr.number_of_devices > 1
        try:
            for a, epw, rd, wr, ga in ((self.X, MX_BLOCK, upload, False, False),
                                       (self.codes, MX_BLOCK // self.PER_BYTE, False, download, gather),
                                       (self.scales, 1, False, download, gather)):
                a.partial_read = False
                a.read, a.write, a.elements_per_work_item, a.gather_resident = rd, wr, epw, ga
            self.X.next_param(self.codes, self.scales).compute(self.cr, compute_id, self.kernel, self.blocks, LOCAL)
            self.records = [self.cr.last_record()]
            if pack and self.packed is not None:
                self.scales.write = self.scales.gather_resident = False
                self.dims.partial_read = self.dims.write = self.dims.gather_resident = False
                self.dims.read = True  # 8 bytes: every device has them whatever the split was before
                p = self.packed
                p.partial_read = p.read = False
                p.write, p.elements_per_work_item, p.gather_resident = download, 1, gather
                self.dims.next_param(self.scales, p).compute(
                    self.cr, compute_id + 1 if pack_compute_id is None else pack_compute_id, PACK_KERNEL,
                    p.N, LOCAL)
                self.records.append(self.cr.last_record())
        finally:
            for a, flags in saved:
                for f, v in zip(_FLAGS, flags):
                    setattr(a, f, v)


class MxFp8Quantizer(_MxQuantizer):
    """``[rows][K]`` fp32 or bf16 → MXFP8 through ``compute()``.

    ``X`` (``rows·K`` of the source type; bf16 as the uint16-storage bf16
    ClArray) is the input, ``codes`` (``"float8_e4m3fn"``), ``scales`` (uint8,
    ``rows·K/32``, row-major) and ``packed`` (uint32, ``rows·K/128``, the
    layout of :func:`~cekirdekler_amd.ops.tiling.pack_mx_scales`) the outputs;
    ``packed`` exists when rows % 64 = 0 and K % 128 = 0 and is None
    otherwise.  Arrays passed in are adopted (``x``: an input that already
    lives in a ClArray, e.g. another kernel's output); their transfer flags
    are as they were when :meth:`run` returns.

    The number of blocks ``rows·K/32`` must be a multiple of 64."""

    KERNELS = QUANTIZE_KERNELS
    LIBS = ("mx_quantize",)
    CODES_DTYPE = "float8_e4m3fn"


class MxFp4Quantizer(_MxQuantizer):
    """``[rows][K]`` fp32 or bf16 → MXFP4 through ``compute()``
    (``kernels/mx4_quantize.hip``), bit for bit
    :func:`~cekirdekler_amd.ops.codecs.to_mxfp4`: :class:`MxFp8Quantizer` with
    ``codes`` a ``"float4_e2m1fn_x2"`` array of ``rows·K/2`` bytes (two
    elements per byte, :func:`~cekirdekler_amd.ops.codecs.pack_fp4`).  A block
    with a NaN has the scale byte ``0xFF``.  The pack compute is the MXFP8
    one, so the cruncher needs ``library("mx4_quantize", "mx_quantize")``."""

    KERNELS = QUANTIZE4_KERNELS
    LIBS = ("mx4_quantize", "mx_quantize")
    CODES_DTYPE = "float4_e2m1fn_x2"
    PER_BYTE = 2
