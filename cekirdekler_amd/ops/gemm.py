"""Range-partitioned GEMMs: bf16 (the "SGEMM 8192² bf16" config of
BASELINE.json), fp32 on the fp32 matrix cores, fp8 (OCP e4m3fn), MXFP8
(e4m3fn with one E8M0 scale per block of 32), MXFP4 (e2m1, two per byte,
with the same scales) and the mixed MXFP8 × MXFP4 form (8-bit A, 4-bit B).

``C = A · Bᵀ`` with A ``[M][K]`` and Bt ``[N][K]`` bf16 row-major, C fp32 in
tile-major layout (see ``kernels/sgemm_bf16.hip``).  The global range is one
work-group per output tile, so the load balancer splits the problem across
devices in whole tiles and each device's C slice is one contiguous range
(``elements_per_work_item = BM·BN / local``).

``resident=True`` keeps A and B on the devices after the first upload and
leaves C in device memory (the BASELINE "device-resident" number);
``resident=False`` is the reference's host-resident semantics: A and B are
uploaded and every device downloads its C slice on each call.

The element codecs live in ``ops/codecs.py`` and the C-tile and scale layouts
in ``ops/tiling.py``; both are imported here by name, so this module remains
the import path for all of them.
"""
from __future__ import annotations

import weakref
from typing import Callable, NamedTuple

import numpy as np

from ..arrays import ClArray
from ..cruncher import ClComputeError, ClNumberCruncher
from .codecs import (FP4_E2M1_EMAX, MX_BLOCK, e8m0_to_f64, from_bf16_bits, from_fp4_e2m1_codes,  # noqa: F401
                     from_fp8_e4m3_bits, from_mxfp4, from_mxfp8, pack_fp4, to_bf16_bits, to_fp4_e2m1_codes,
                     to_fp8_e4m3_bits, to_mxfp4, to_mxfp8, unpack_fp4)
from .library import library
from .quantize import LOCAL as QUANTIZE_LOCAL, PACK_KERNEL, MxFp4Quantizer, MxFp8Quantizer, _src_name
from .tiling import pack_mx_scales, rows_to_tile, tile_coords, tile_to_rows, unpack_mx_scales, untile  # noqa: F401

# tile name -> (BM, BN, work-group size, kernel).  The production tiles and
# at most two tested alternates per dtype; every variant measured and dropped
# in rounds 1-2 is in git history, with its numbers in profiles/gemm_*.md.
TILES = {
    # balanced-DMA ping-pong (G0 stages A, G1 stages Bt two K-tiles ahead):
    # the full-problem tile, one branch-free K loop per wave group (1.55-1.57 PF
    # at 8192³ where its reference tile 256x256pb0 runs 1.51;
    # profiles/gemm_flat_loop.md)
    "256x256pb": (256, 256, 512, "cek_sgemm_bf16_256x256pb"),
    # the same kernel with C row-major [M][N] (an LDS turn-around per wave in
    # the epilogue): the layout hipBLASLt writes, for like-for-like numbers;
    # device-resident computes only (a device's slice of C is one block of
    # rows only when its tile range is whole tile groups)
    "256x256pbr": (256, 256, 512, "cek_sgemm_bf16_256x256pbr"),
    # uneven split-K = 2 (the helper runs `exchange_shift` K-tiles fewer and
    # hands its whole partial to the owner while the owner still multiplies):
    # the 8-GPU slice (1024 rows of 8192², 128 tiles for 256 CUs).  The
    # hand-over is co-residency-safe: an owner whose helper is late claims
    # the hand-over and multiplies the helper's K-range itself.
    "256x256pbw": (256, 256, 512, "cek_sgemm_bf16_256x256pb_sw"),
    # the same, row halves exchanged at the end: the helper hands over its
    # partial of the owner's half, the owner hands back its partial of the
    # helper's half, each stores one half of C (384 KiB of tail traffic on
    # the owner instead of 512)
    "256x256pbh": (256, 256, 512, "cek_sgemm_bf16_256x256pb_sh"),
    # halves exchanged with an even split: the owner hands its partial back
    # before it waits for the helper's, so both partial stores are in flight
    # together and both sides end their loops together
    "256x256pbs": (256, 256, 512, "cek_sgemm_bf16_256x256pb_ss"),
    # 256×128 fallbacks (twice the tiles): even chunk-split DMA, three stages / balanced DMA
    "256x128pe": (256, 128, 512, "cek_sgemm_bf16_256x128pe"),
    "256x128pb": (256, 128, 512, "cek_sgemm_bf16_256x128pb"),
    # reference structures: one LDS stage in flight / ping-pong wave groups
    # (the latter with a last-arriver split-K variant)
    "256x256": (256, 256, 512, "cek_sgemm_bf16_256x256"),
    "256x256pp": (256, 256, 512, "cek_sgemm_bf16_256x256pp"),
    # small problems: 2 blocks per CU
    "128x128": (128, 128, 256, "cek_sgemm_bf16_128x128"),
}

# Reference tiles: kernels kept to measure and check a production tile
# against, accepted by GemmBf16(tile=...) like the tiles above but not part of
# the tile set.  256x256pb0 is 256x256pb with the K loop written once for
# both wave groups (the loop 256x256pb had before its flat loops): C is the
# same to the bit (tests/test_gpu_gemm_flat_loop.py), and tools/scale_probe.py
# and tools/microbench/gemm_loop measure against it.
REFERENCE_TILES = {"256x256pb0": (256, 256, 512, "cek_sgemm_bf16_256x256pb0")}
REFERENCE_TILE_WAVES = {"256x256pb0": (2, 4, 8, 4)}

GEMM_LIBS = ("sgemm_bf16",)

# Wave geometry of every bf16 tile (WM × WN waves, FM × FN 16×16 fragments
# each): the kernels store a C tile in fragment order (one dwordx4 per lane
# per fragment), which tile_to_rows / rows_to_tile convert.
TILE_WAVES = {
    "256x256pb": (2, 4, 8, 4), "256x256pbr": (2, 4, 8, 4), "256x256pbw": (2, 4, 8, 4), "256x256pbh": (2, 4, 8, 4), "256x256pbs": (2, 4, 8, 4), "256x256": (2, 4, 8, 4), "256x256pp": (2, 4, 8, 4),
    "256x128pe": (4, 2, 4, 4), "256x128pb": (4, 2, 4, 4), "128x128": (2, 2, 4, 4),
}


# fp32 tiles (kernels/sgemm_f32.hip): v_mfma_f32_16x16x4_f32, BK = 32
F32_TILES = {
    # production: register-direct, 8 waves of 128×64 — fragments loaded
    # global → VGPR, no LDS, no barrier — with the next block's loads spread
    # evenly over the current block's MFMA groups (152.8 TF at 8192³ vs
    # hipBLASLt 152.8 on one box, 152.0 / 151.7 vs 152.0 on another, where
    # the first-half spread g8h ran 151.2 / 150.6; profiles/round4_session5.md,
    # round4_session6.md)
    "256x256g8i": (256, 256, 512, "cek_sgemm_f32_256x256g8i"),
    # the same loads spread over the first half / quarter of the groups
    "256x256g8h": (256, 256, 512, "cek_sgemm_f32_256x256g8h"),
    "256x256g8q": (256, 256, 512, "cek_sgemm_f32_256x256g8q"),
    # burst loads ahead of each block's MFMAs (151.4 TF vs hipBLASLt 153.4 on
    # another box, 256x256ir 138.6 there)
    "256x256g8": (256, 256, 512, "cek_sgemm_f32_256x256g8"),
    # LDS-staged: k block 1's fragment reads between block 0's MFMA groups
    # (146-147 TF at 8192³ on earlier boxes)
    "256x256ir": (256, 256, 512, "cek_sgemm_f32_256x256ir"),
    # alternates: the barrier ahead of the last MFMA groups; v_mfma_f32_32x32x2_f32
    "256x256ib7": (256, 256, 512, "cek_sgemm_f32_256x256ib7"),
    "256x256w": (256, 256, 512, "cek_sgemm_f32_256x256w"),
    # 256×128: every LDS-DMA piece within the first k block's MFMAs
    "256x128ie": (256, 128, 512, "cek_sgemm_f32_256x128ie"),
    # plain one-stage-in-flight structures
    "256x256": (256, 256, 512, "cek_sgemm_f32_256x256"),
    "256x128": (256, 128, 512, "cek_sgemm_f32_256x128"),
    # register-direct: fragments global → VGPR, no LDS, no barrier; 4 waves
    # of 128×128 (one per SIMD) or 8 of 128×64; t = phases ordered by
    # fragment ties instead of scheduling barriers
    "256x256g": (256, 256, 256, "cek_sgemm_f32_256x256g"),
    "256x256gt": (256, 256, 256, "cek_sgemm_f32_256x256gt"),
    "256x256gh": (256, 256, 256, "cek_sgemm_f32_256x256gh"),  # 4-wave form of g8h
    "256x256g8t": (256, 256, 512, "cek_sgemm_f32_256x256g8t"),
    "128x128": (128, 128, 256, "cek_sgemm_f32_128x128"),
}

# fp8 e4m3fn tiles (kernels/sgemm_fp8.hip): BK = 128, C in fragment order
# like the bf16 tiles.  No split-K or exchange variants.  Throughput at 8192³
# beside the bf16 256x256pb of the same run (1487 TF/s): profiles/gemm_fp8.md.
FP8_TILES = {
    # the bf16 production structure (balanced-DMA ping-pong) with four
    # v_mfma_f32_16x16x32_fp8_fp8 steps per K-tile, the bf16 matrix rate:
    # 1997 TF/s (1.34× bf16: half the staging bytes and barriers per flop)
    "256x256pb": (256, 256, 512, "cek_sgemm_fp8_256x256pb"),
    # the same with v_mfma_scale_f32_16x16x128_f8f6f4 at unit scales, one
    # instruction per fragment pair and K-tile, the fp8 matrix rate:
    # 2751 TF/s (1.85× bf16), the GemmFp8 default
    "256x256pbx": (256, 256, 512, "cek_sgemm_fp8_256x256pbx"),
    # one LDS stage in flight, 4 waves, the simple kernel the others are
    # judged against: 1709 TF/s (1.15× bf16)
    "128x128": (128, 128, 256, "cek_sgemm_fp8_128x128"),
}
FP8_TILE_WAVES = {"256x256pb": (2, 4, 8, 4), "256x256pbx": (2, 4, 8, 4), "128x128": (2, 2, 4, 4)}

# MXFP8 tiles (kernels/sgemm_mxfp8.hip): the fp8 structures with E8M0 block
# scales applied by v_mfma_scale_f32_16x16x128_f8f6f4.  Throughput beside the
# unit-scale fp8 256x256pbx of the same run: profiles/gemm_mxfp8.md.
MXFP8_TILES = {
    # balanced-DMA ping-pong, packed scales global → VGPR one K-tile ahead:
    # the GemmMxFp8 default
    "256x256pbx": (256, 256, 512, "cek_sgemm_mxfp8_256x256pbx"),
    # one LDS stage in flight, 4 waves: the simple kernel the other is judged against
    "128x128": (128, 128, 256, "cek_sgemm_mxfp8_128x128"),
}
MXFP8_TILE_WAVES = {"256x256pbx": (2, 4, 8, 4), "128x128": (2, 2, 4, 4)}

# MXFP4 tiles (kernels/sgemm_mxfp4.hip): the MXFP8 structures with e2m1
# operands, two per byte, a K-tile of 128 B = 256 k as two scaled
# instructions.  Throughput beside the MXFP8 256x256pbx of the same run:
# profiles/gemm_mxfp4.md.
MXFP4_TILES = {
    # balanced-DMA ping-pong, packed scales global → VGPR one K-tile ahead:
    # the GemmMxFp4 default
    "256x256pbx": (256, 256, 512, "cek_sgemm_mxfp4_256x256pbx"),
    # one LDS stage in flight, 4 waves: the simple kernel the other is judged against
    "128x128": (128, 128, 256, "cek_sgemm_mxfp4_128x128"),
}
MXFP4_TILE_WAVES = {"256x256pbx": (2, 4, 8, 4), "128x128": (2, 2, 4, 4)}

# Output modes of the MX GEMMs (kernels/sgemm_mx_out.hip): (operand format,
# tile, out) -> kernel.  The loop is the plain tile's, so the fp32 values that
# are converted are the plain kernel's C bit for bit; Y is row-major [M][N].
MX_OUTPUTS = ("bfloat16", "mxfp8", "mxfp4")
MX_OUT_KERNELS = {(fmt, tile, out): f"cek_sgemm_{fmt}_{tile}_{'bf16' if out == 'bfloat16' else out}"
                  for fmt, tiles in (("mxfp8", MXFP8_TILES), ("mxfp4", MXFP4_TILES))
                  for tile in tiles for out in MX_OUTPUTS}
MX_OUT_LIB = "sgemm_mx_out"
# the pack compute of an output-mode call runs under the call's compute id plus this
MX_OUT_PACK_ID = 0x4D70
MX_ACTIVATIONS = {None: 0, "relu": 1}  # dims[5]


class MxFormat(NamedTuple):
    """An MX operand format: what an MX GEMM states per operand
    (``OPERANDS``), and what an ``"mxfp8"`` / ``"mxfp4"`` output mode stores,
    an output being the next layer's operand."""
    name: str  # the output mode of a producer whose Y is such an operand
    dtype: str  # storage dtype of the codes
    per_item: int  # elements per storage item
    encode: Callable  # [rows][K] fp32 values -> (what the operand stores, scale bytes)
    decode: Callable  # (codes, scale bytes) -> values
    quantizer: type  # the same conversion on the devices (ops/quantize.py)
    base_id: int  # compute id of its quantise compute for A; +2 for B, +1 for the pack that follows


MXFP8 = MxFormat("mxfp8", "float8_e4m3fn", 1, to_mxfp8, from_mxfp8, MxFp8Quantizer, 0x4D58)
MXFP4 = MxFormat("mxfp4", "float4_e2m1fn_x2", 2, to_mxfp4, from_mxfp4, MxFp4Quantizer, 0x4D60)
MX_FORMATS = {f.name: f for f in (MXFP8, MXFP4)}

# Mixed MXFP8 × MXFP4 tiles (kernels/sgemm_mxf8f4.hip): A e4m3fn, Bt e2m1, a
# K-tile of 256 k as two scaled instructions with one format per operand.
# Throughput beside the MXFP8 256x256pbx of the same run: profiles/gemm_mxf8f4.md.
MXF8F4_TILES = {
    # balanced-DMA ping-pong, byte for byte the MXFP8 256x256pbx loop (A's
    # K-tile is 256 B per row, so the tile has half the rows): the GemmMxFp8Fp4 default
    "128x256pbx": (128, 256, 512, "cek_sgemm_mxf8f4_128x256pbx"),
    # one LDS stage in flight, 4 waves: the simple kernel the other is judged against
    "128x128": (128, 128, 256, "cek_sgemm_mxf8f4_128x128"),
}
MXF8F4_TILE_WAVES = {"128x256pbx": (2, 4, 4, 4), "128x128": (2, 2, 4, 4)}
# their output modes (kernels/sgemm_mxf8f4_out.hip), keyed like MX_OUT_KERNELS
MXF8F4_OUT_KERNELS = {("mxf8f4", tile, out): f"cek_sgemm_mxf8f4_{tile}_{'bf16' if out == 'bfloat16' else out}"
                      for tile in MXF8F4_TILES for out in MX_OUTPUTS}
MXF8F4_OUT_LIB = "sgemm_mxf8f4_out"

# tiles whose kernel stores C row-major ([M][N]) instead of tile-major
ROW_MAJOR_TILES = {"256x256pbr"}
# tiles with a split-K kernel variant ("<kernel>_sk", arrays + W + counters)
SPLIT_K_TILES = {"256x256pp", "256x256pb"}
# tiles whose kernel always runs two K-splits with a hand-over (flag words per tile)
EXCHANGE_TILES = {"256x256pbw": 4, "256x256pbh": 4, "256x256pbs": 4}
# K-tile deficit of the helper split (dims[5]): it hands its whole partial
# over and leaves while the owner still multiplies
EXCHANGE_SHIFT = {"256x256pbw": 4, "256x256pbh": 4, "256x256pbs": 0}


def decode_operand(arr: ClArray) -> np.ndarray:
    """The host array of a GEMM operand as numbers: bf16, fp8 and fp4x2 arrays
    hold bit patterns (``is_fp8``; ``is_fp4``: two e2m1 codes per byte, so the
    result is twice as long as the array; ``is_bf16`` or plain uint16
    storage), every other array its values."""
    x = arr.array
    if getattr(arr, "is_fp4", False):
        return from_fp4_e2m1_codes(unpack_fp4(x))
    if getattr(arr, "is_fp8", False):
        return from_fp8_e4m3_bits(x)
    return from_bf16_bits(x) if getattr(arr, "is_bf16", False) or x.dtype == np.uint16 else x


class GemmBf16:
    # What a format states; the constructor below does the rest for all five.
    TILE_TABLE = TILES
    TILE_GEOM = TILE_WAVES  # tile -> wave geometry (C tiles in fragment order); None: C tiles row-major
    K_MULTIPLE = 64
    POSITIVE_DIMS = False  # the 8-bit and 4-bit classes also refuse M, N, K <= 0
    LIBS = GEMM_LIBS
    OPERAND_DTYPE = "bfloat16"
    PER_ITEM = 1  # elements per storage item of A / B
    _encode = staticmethod(to_bf16_bits)  # fp32 values -> what A / B store

    def __init__(self, M: int, N: int, K: int, devices=None, tile: str = "256x256",
                 cruncher: ClNumberCruncher | None = None, fill: str = "random", seed: int = 0,
                 group_m: int = 4, split_k: int = 1, wave_granularity: bool | None = None,
                 exchange_shift: int | None = None, handover_spin_limit: int = 0):
        # split-K, exchange, row-major C and reference tiles are variants of the bf16 tiles alone
        bf16 = self.TILE_TABLE is TILES
        reference = bf16 and tile in REFERENCE_TILES
        BM, BN, L, kname = REFERENCE_TILES[tile] if reference else self.TILE_TABLE[tile]
        self.tile = tile
        if M % BM or N % BN or K % self.K_MULTIPLE or (self.POSITIVE_DIMS and min(M, N, K) <= 0):
            raise ValueError(f"M%{BM}, N%{BN} and K%{self.K_MULTIPLE} must be 0"
                             + (" and M, N, K positive" if self.POSITIVE_DIMS else "") + f" (got {M},{N},{K})")
        if split_k > 1:
            if tile not in SPLIT_K_TILES:
                raise ValueError(f"split-K is available for tiles {sorted(SPLIT_K_TILES)}")
            if (K // 64) % split_k:
                raise ValueError(f"K/64 ({K // 64}) must be divisible by split_k ({split_k})")
            kname = kname + "_sk"
        self.exchange = bf16 and tile in EXCHANGE_TILES
        shift = 0
        if self.exchange:
            if (K // 64) % 2:
                raise ValueError(f"K/64 ({K // 64}) must be even for tile {tile}")
            split_k = 2
            if tile in EXCHANGE_SHIFT:
                shift = EXCHANGE_SHIFT[tile] if exchange_shift is None else int(exchange_shift)
                shift = max(0, min(shift, K // 128 - 1))  # the helper keeps >= 1 K-tile
        self.exchange_shift = shift
        self.M, self.N, self.K, self.BM, self.BN, self.L, self.kernel = M, N, K, BM, BN, L, kname
        self.geom = REFERENCE_TILE_WAVES[tile] if reference else self.TILE_GEOM[tile] if self.TILE_GEOM else None
        self.row_major_c = bf16 and tile in ROW_MAJOR_TILES
        self.split_k = max(1, int(split_k))
        self.tiles = (M // BM) * (N // BN)
        self.global_range = self.tiles * self.split_k * L
        self.cr = cruncher or ClNumberCruncher(devices, "", prebuilt=library(*self.LIBS))
        self.group_m = group_m
        # dims[7]: the owner's wait for the helper's partial, in polls (0: the
        # kernel default, 65536; -1: the owner claims at once and the helper
        # waits for that claim, so every owner falls back; -2 (halves tile):
        # the helper claims the hand-back at once — forced fall-backs)
        self.dims = ClArray(np.array([M, N, K, group_m, self.split_k, shift, 0, int(handover_spin_limit)], np.int32))
        self.dims.write = False
        self.A = ClArray(M * K // self._per_item("A"), self._operand_dtype("A"))
        self.B = ClArray(N * K // self._per_item("B"), self._operand_dtype("B"))
        scales = self._alloc_scales()
        for a in (self.A, self.B, *scales):
            a.write = False
        self._alloc_output()
        self.extra = []
        if self.split_k > 1:
            # per-work-group partial tiles (device-only scratch: never transferred;
            # np.empty leaves the host pages untouched) and per-tile arrival counters
            # (exchange tiles: one tile of partial halves per tile, two ready
            # flags per tile and a spin-timeout counter at the end)
            wtiles = self.tiles if self.exchange else self.tiles * self.split_k
            self.W = ClArray(np.empty(wtiles * BM * BN, np.float32))
            self.W.read = self.W.write = False
            nflags = EXCHANGE_TILES[tile] * self.tiles + 1 if self.exchange else self.tiles
            self.counters = ClArray(np.zeros(nflags, np.int32))
            self.counters.write = False
            self.extra = [self.W, self.counters]
        if fill == "random":
            self._fill_random(np.random.default_rng(seed))
        self._uploaded = False
        self.wave_granularity = wave_granularity
        self._orders = {}  # compute id -> shell panels of its tile order (0: grouped)

    def _operand_dtype(self, name: str):
        """Storage dtype of operand ``name`` (``"A"`` / ``"B"``); the MX
        classes read it, like the next, from the operand's :class:`MxFormat`."""
        return self.OPERAND_DTYPE

    def _per_item(self, name: str) -> int:
        """Elements per storage item of operand ``name``."""
        return self.PER_ITEM

    def _alloc_scales(self) -> tuple:
        """Allocate what a format keeps beside ``A`` and ``B`` (the MX formats:
        their scale arrays); returns those of them the kernels only read."""
        return ()

    def _alloc_output(self) -> None:
        """Allocate what the kernel writes: C, one contiguous slice per device."""
        self.C = ClArray(self.M * self.N, np.float32)
        self.C.read = False
        self.C.elements_per_work_item = self.BM * self.BN // (self.L * self.split_k)

    def _output_flags(self, resident: bool) -> None:
        """Transfer flags of the written arrays for one call."""
        self.C.write = not resident

    def _after_compute(self, compute_id: int, resident: bool) -> None:
        """What a format runs behind the GEMM compute of a call."""

    def _fill_random(self, rng) -> None:
        """Uniform [−1, 1) values in the operands' format, A then B."""
        self.A.array[:] = self._encode(rng.uniform(-1, 1, self.M * self.K).astype(np.float32))
        self.B.array[:] = self._encode(rng.uniform(-1, 1, self.N * self.K).astype(np.float32))

    def granularity(self) -> int:
        """Balancer unit in work items.  One tile (all its K-splits) by
        default.  On identical GPUs whose slices are whole waves of tiles
        (``work-groups % CUs == 0`` and at least one wave per device), the unit
        is one wave: one work-group per CU.  With 256 CUs and exactly one
        wave of tiles per device (8192² at 4 or 8 GPUs), a one-tile step would
        let timing noise hand a device 257 tiles, which costs it a second
        round of tiles and doubles its time.  A split in whole waves cannot do
        that.  ``wave_granularity`` forces the choice (None = auto)."""
        tile_unit = self.L * self.split_k
        devs = [d for d in self.cr.devices]
        if self.wave_granularity is False or not devs:
            return tile_unit
        cus = {d.compute_units for d in devs}
        gpus = all(d.is_gpu for d in devs)
        if self.wave_granularity is None and not (gpus and len(cus) == 1):
            return tile_unit
        cu = min(cus)
        groups = self.tiles * self.split_k
        ndev = self.cr.number_of_devices or len(devs)
        if cu <= 0 or groups % cu or groups // cu < ndev:
            return tile_unit
        # a wave of tiles must keep a tile's K-splits together
        return cu * self.L if cu % self.split_k == 0 else tile_unit

    @property
    def flops(self) -> float:
        return 2.0 * self.M * self.N * self.K

    def _row_items(self) -> int:
        """Storage items of one operand row in ``A`` / ``B``: K, one per
        element (GemmMxFp4: K/2 bytes of two elements each)."""
        return self.K // self._per_item("A")

    def _group_work_items(self) -> int:
        """Work items of one tile group (``group_m`` tile rows × every tile
        column): the unit whose A rows form one contiguous panel."""
        return self.group_m * (self.N // self.BN) * self.L * self.split_k

    def can_stream(self) -> bool:
        """Host-resident streaming needs whole tile groups (A row panels) per
        blob and an integral A panel per work item."""
        ntm, ntn = self.M // self.BM, self.N // self.BN
        per_wi = self.BM * self._row_items()
        return (self.split_k == 1 and ntm % self.group_m == 0
                and per_wi % (ntn * self.L) == 0)

    def run(self, compute_id: int = 1, resident: bool = True, stream_blobs: int = 0,
            stream_event: bool = True) -> None:
        """One GEMM through compute().  ``resident``: A/B stay on the devices
        after the first call and C stays in device memory.  ``stream_blobs``
        (host-resident only): run the call through the event-driven
        read/compute/write pipeline (Cores.cs:1197-1367) in that many blobs
        per device — B is a full read, A goes up one row panel per blob
        (``partial``) and every blob's C tiles come down while later blobs'
        panels upload and compute, on the two half-pipelines' streams."""
        if self.row_major_c and not resident:
            raise ValueError("row-major C tiles run device-resident computes only")
        if self.split_k > 1 and self.cr.enqueue_mode and self.cr.enqueue_mode_async_enable:
            # computes on async queues run concurrently; two launches of one
            # split-K GEMM would share its partial tiles and hand-over words
            raise ClComputeError("split-K / exchange GEMM tiles cannot run on async enqueue queues "
                                 "(concurrent launches would share the partial-tile workspace); "
                                 "use a single-pass tile such as 256x256pb")
        first = not self._uploaded
        self._orders[compute_id] = 0
        streamed = bool(stream_blobs) and not resident
        if streamed and not self.can_stream():
            raise ValueError("stream_blobs needs split_k == 1, whole tile groups and an integral A panel "
                             "per work item")
        for a in self._inputs(first or not resident):
            a.read = first or not resident
        self.A.partial_read = streamed
        # an A row panel of one tile group spans group_m·BM rows; per work item
        panel = self.BM * self._row_items()
        self.A.elements_per_work_item = panel // ((self.N // self.BN) * self.L) if streamed else 1
        if self.split_k > 1:
            self.counters.read = first  # zeroed once; the kernel re-arms them
        self._output_flags(resident)
        gran = self.granularity()
        if streamed:
            gran = self._group_work_items()
        self.dims.next_param(*self._params()).compute(
            self.cr, compute_id, self.kernel, self.global_range, self.L,
            pipeline=streamed, pipeline_type=stream_event, pipeline_blobs=max(1, stream_blobs),
            granularity=gran)
        self._uploaded = True
        self._after_compute(compute_id, resident)

    def _inputs(self, upload: bool) -> tuple:
        """The arrays a call reads (``upload``: this call sends them to the devices)."""
        return self.dims, self.A, self.B

    def _params(self) -> tuple:
        """The kernel's array parameters after ``dims``, in its order."""
        return (self.A, self.B, self.C, *self.extra)

    def _operand(self, name: str) -> np.ndarray:
        """Operand ``"A"`` (``[M][K]``) or ``"B"`` (``[N][K]``) as the numbers
        the kernel multiplies: what every host reference is computed from."""
        arr, rows = (self.A, self.M) if name == "A" else (self.B, self.N)
        return decode_operand(arr).reshape(rows, self.K)

    def _operand_t(self, name: str, device):
        """:meth:`_operand` as a float64 torch tensor on ``device``."""
        import torch

        arr, rows = (self.A, self.M) if name == "A" else (self.B, self.N)
        x = arr.array
        if getattr(arr, "is_fp4", False):
            # two e2m1 codes per byte, low nibble first, decoded by table on the device
            p = torch.from_numpy(x).to(device)
            codes = torch.stack((p & 15, p >> 4), dim=-1).reshape(rows, self.K).long()
            del p
            table = from_fp4_e2m1_codes(np.arange(16, dtype=np.uint8)).astype(np.float64)
            return torch.from_numpy(table).to(device)[codes]
        if getattr(arr, "is_fp8", False):
            # e4m3fn bit patterns, decoded on the host (every e4m3 value is exact in bf16)
            t = torch.from_numpy(x).view(torch.float8_e4m3fn).to(torch.bfloat16).to(device)
        elif x.dtype == np.uint16:  # bf16 bit patterns
            t = torch.from_numpy(x.view(np.int16)).to(device).view(torch.bfloat16)
        else:
            t = torch.from_numpy(x).to(device)
        return t.reshape(rows, self.K).double()

    def shell_bounds(self, panels: int, split_last: int = 0):
        """Work-item bounds of the square shells (blob s = shell s) and the
        per-blob row panels of A and B, for :meth:`run_shells`.  The last
        ``split_last`` shells become two blobs each, ``R_s`` (which uploads
        panels A_s and B_s) and ``C_s`` (no upload), so ``R_s``'s C tiles
        come down while ``C_s`` multiplies: the call's tail after the last
        upload is ``C_s`` alone."""
        P = int(panels)
        if self.split_k != 1:
            raise ValueError("shell streaming runs single-pass tiles (split_k == 1)")
        if P < 1 or self.M % P or self.N % P or (self.M // P) % self.BM or (self.N // P) % self.BN:
            raise ValueError(f"M and N must split into {P} panels of whole {self.BM}x{self.BN} tiles")
        pm, pn = self.M // P // self.BM, self.N // P // self.BN
        a_rows, b_rows = self.M // P, self.N // P
        unit = pm * pn * self.L  # work items of one panel × panel block
        bounds, a_sl, b_sl = [0], [], []
        for k in range(P):
            a_panel, b_panel = (k * a_rows * self.K, a_rows * self.K), (k * b_rows * self.K, b_rows * self.K)
            if k >= P - int(split_last) and k > 0:
                bounds += [(k * k + k + 1) * unit, (k + 1) * (k + 1) * unit]  # R_k, then C_k
                a_sl += [a_panel, (0, 0)]
                b_sl += [b_panel, (0, 0)]
            else:
                bounds.append((k + 1) * (k + 1) * unit)
                a_sl.append(a_panel)
                b_sl.append(b_panel)
        return bounds, a_sl, b_sl

    def run_shells(self, panels: int = 16, compute_id: int = 2, split_last: int = 0) -> None:
        """One host-resident call through ``compute()``: the event-driven
        read/compute/write pipeline with explicit, uneven blobs — blob s is
        square shell s (``R_s = A_s·B[0..s]ᵀ`` then ``C_s = A[0..s-1]·B_sᵀ``,
        the kernels' shell tile order, ``dims[6] = panels``), A and B go up
        one row panel per blob (``ClArray.blob_slices``) on the upload stream
        and every shell's C comes down (one contiguous range) while later
        panels go up.  The first kernels need two panels instead of all of
        B.  One device holds the range (several: the plain path)."""
        bounds, a_sl, b_sl = self.shell_bounds(panels, split_last)
        if getattr(self, "_dims_shell", None) is None or int(self._dims_shell.array[6]) != panels:
            d = self.dims.array.copy()
            d[6] = panels
            self._dims_shell = ClArray(d)
            self._dims_shell.write = False
        self._orders[compute_id] = int(panels)
        saved = [(a.read, a.partial_read, a.blob_slices) for a in (self.A, self.B)]
        try:
            for a, sl in ((self.A, a_sl), (self.B, b_sl)):
                a.partial_read = True
                a.blob_slices = sl
            self.C.write = True
            self._dims_shell.read = True
            self._dims_shell.next_param(self.A, self.B, self.C).compute(
                self.cr, compute_id, self.kernel, self.global_range, self.L, pipeline=True,
                pipeline_blobs=bounds, granularity=self.granularity())
        finally:
            for a, (r, pr, bs) in zip((self.A, self.B), saved):
                a.partial_read, a.blob_slices = pr, bs
                a.read = r
        self._uploaded = False  # the device copies of A/B were streamed, not kept whole

    def run_host_shells(self, panels: int = 8, device: int = 0) -> None:
        """One host-resident call streamed in square shells
        (``Cores::gemm_host_shells``, ``csrc/shell_gemm.cpp``): A and B go up
        in ``panels`` row panels each (A0 B0 A1 B1 …), shell s's two GEMMs
        (``A_s·B[0..s]ᵀ`` and ``A[0..s-1]·B_sᵀ``) run once panels s have
        landed, and each shell's C comes down while later panels go up.
        Unlike the 1-D blob pipeline, the first kernels need only two panels
        instead of all of B.  One GPU of the cruncher; the host C is in shell
        layout (:meth:`shells_result`)."""
        if self.split_k != 1:
            raise ValueError("shell streaming runs single-pass tiles (split_k == 1)")
        pm, pn = self.M // max(1, panels), self.N // max(1, panels)
        if panels < 1 or self.M % panels or self.N % panels or pm % self.BM or pn % self.BN:
            raise ValueError(f"M and N must split into {panels} panels of whole {self.BM}x{self.BN} tiles")
        self.cr.cores.gemm_host_shells(device, self.kernel, self.A._spec(), self.B._spec(), self.C._spec(),
                                       self.M, self.N, self.K, panels, self.group_m, self.BM, self.BN, self.L)

    def shells_result(self, panels: int = 8) -> np.ndarray:
        """Row-major fp32 C from the host C of :meth:`run_host_shells`
        (shell by shell: ``R_s`` then ``C_s``, each tile-major)."""
        pm, pn = self.M // panels, self.N // panels
        out = np.empty((self.M, self.N), np.float32)
        c, off = self.C.array, 0
        for s in range(panels):
            m, n = pm, (s + 1) * pn
            out[s * pm:(s + 1) * pm, :n] = untile(c[off:off + m * n], m, n, self.BM, self.BN, self.group_m, self.geom)
            off += m * n
            if s:
                m, n = s * pm, pn
                out[:s * pm, s * pn:(s + 1) * pn] = untile(c[off:off + m * n], m, n, self.BM, self.BN, self.group_m, self.geom)
                off += m * n
        return out

    def verify_shells(self, panels: int = 8, samples: int = 16, seed: int = 2) -> float:
        """Max relative error of sampled 256-row × 256-column blocks of
        :meth:`shells_result` against a float64 host product."""
        c = self.shells_result(panels)
        a = self._operand("A")
        b = self._operand("B")
        rng = np.random.default_rng(seed)
        worst = 0.0
        for _ in range(samples):
            r = int(rng.integers(0, self.M // 256)) * 256
            q = int(rng.integers(0, self.N // 256)) * 256
            ref = a[r:r + 256].astype(np.float64) @ b[q:q + 256].astype(np.float64).T
            worst = max(worst, float(np.abs(c[r:r + 256, q:q + 256] - ref).max() / max(np.abs(ref).max(), 1e-30)))
        return worst

    def verify_shells_full(self, panels: int = 8, device=None) -> tuple:
        """Every element of :meth:`shells_result` against a float64 product
        computed by torch on ``device``: ``(max_rel_err, blocks_checked)``,
        the error per BM×BN block relative to that block's ``max |ref|``."""
        import torch

        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else (
                torch.device("cpu"))
        c = torch.from_numpy(self.shells_result(panels)).to(device)
        ref = self._reference_t(device)
        ntm, ntn = self.M // self.BM, self.N // self.BN
        got = c.view(ntm, self.BM, ntn, self.BN).double()
        want = ref.view(ntm, self.BM, ntn, self.BN)
        err = (got - want).abs().amax(dim=(1, 3)) / want.abs().amax(dim=(1, 3)).clamp_min(1e-30)
        return float(err.max()), ntm * ntn

    def _reference_t(self, device):
        """C = A·Bᵀ in float64 on a torch device (row-major [M][N])."""
        return self._operand_t("A", device) @ self._operand_t("B", device).T

    def result(self, download: bool = True) -> np.ndarray:
        """Row-major fp32 C (downloads every device's slice when resident)."""
        if download:
            rng = self.cr.ranges(self.cr._cores.last_compute_id)
            refs = self.cr.references(self.cr._cores.last_compute_id)
            e = self.C.elements_per_work_item
            for dev in range(self.cr._cores.num_devices):
                g = self.cr._cores.global_base + dev
                lo, n = refs[g] * e, rng[g] * e
                self._download_slice(dev, lo, n)
        if self.row_major_c:
            return self.C.array.reshape(self.M, self.N).copy()
        return untile(self.C.array, self.M, self.N, self.BM, self.BN, self.group_m, self.geom,
                      self._orders.get(self.cr._cores.last_compute_id, 0))

    def tile_block(self, flat: np.ndarray) -> np.ndarray:
        """One C tile as stored (``BM·BN`` floats) → row-major ``[BM][BN]``."""
        return flat.reshape(self.BM, self.BN) if self.geom is None else tile_to_rows(flat, self.geom)

    def handover_fallbacks(self) -> int:
        """Exchange tiles only: how many owners found their helper's partial
        missing after the bounded wait and multiplied the helper's K-range
        themselves (summed over devices and calls).  C is correct either way;
        a nonzero count means the GPU was shared (helpers not co-resident)
        and those tiles ran at half speed."""
        if not self.exchange:
            return 0
        total = 0
        for dev in range(self.cr._cores.num_devices):
            self.cr.download(self.counters, dev)
            total += int(self.counters.array[-1])
        return total

    spin_timeouts = handover_fallbacks  # round-3 name

    def verify(self, compute_id: int = 1, tiles_per_device: int = 8, seed: int = 1,
               host: bool = False) -> float:
        """Max relative error of the device-resident C of ``compute_id``
        against a float64 host product, over sampled output tiles of this
        process's devices' ranges: the first and last tile of each range plus
        random ones.  Relative to ``max |ref|`` of each tile.  Downloads each
        local device's C replica (device memory is not changed).
        ``host=True`` checks the host C instead (a host-resident call's
        downloaded slices), without downloading."""
        ranges = self.cr.ranges(compute_id)
        refs = self.cr.references(compute_id)
        unit = self.L * self.split_k
        a = self._operand("A")
        b = self._operand("B")
        rng = np.random.default_rng(seed)
        saved = self.C.array.copy()
        worst = 0.0
        tile = self.BM * self.BN
        for dev in range(self.cr._cores.num_devices):
            g = self.cr._cores.global_base + dev
            t0, nt = refs[g] // unit, ranges[g] // unit
            if nt == 0:
                continue
            if not host:
                self.cr.download(self.C, dev)
            picks = {t0, t0 + nt - 1}
            picks.update((t0 + rng.choice(nt, size=min(nt, tiles_per_device), replace=False)).tolist())
            picks = np.array(sorted(picks))
            tm, tn = tile_coords(picks, self.M, self.N, self.BM, self.BN, self.group_m,
                                 self._orders.get(compute_id, 0))
            for t, r, c in zip(picks, tm, tn):
                if self.row_major_c:
                    got = self.C.array.reshape(self.M, self.N)[r * self.BM:(r + 1) * self.BM,
                                                               c * self.BN:(c + 1) * self.BN].astype(np.float64)
                else:
                    got = self.tile_block(self.C.array[t * tile:(t + 1) * tile]).astype(np.float64)
                ref = (a[r * self.BM:(r + 1) * self.BM].astype(np.float64)
                       @ b[c * self.BN:(c + 1) * self.BN].astype(np.float64).T)
                worst = max(worst, float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-30)))
        self.C.array[:] = saved
        return worst

    def verify_full(self, compute_id: int = 1, host: bool = False, device=None) -> tuple:
        """Whole-output check: EVERY C tile this process's devices own under
        the split of ``compute_id``, against a float64 product computed by
        torch on ``device`` (default: torch's current GPU, else the CPU).
        Each local device's C replica is downloaded (``host=True``: the host C
        of a host-resident call is checked as it is), untiled on ``device``
        and compared tile by tile.  Returns ``(max_rel_err, tiles_checked)``;
        the error of a tile is ``max |C - ref| / max |ref|`` over the tile."""
        import torch

        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else (
                torch.device("cpu"))
        M, N, BM, BN = self.M, self.N, self.BM, self.BN
        ntm, ntn = M // BM, N // BN
        ref = self._reference_t(device)  # [M][N] float64
        ref_tiles = ref.view(ntm, BM, ntn, BN).permute(0, 2, 1, 3)  # [ntm][ntn][BM][BN]
        del ref
        ranges = self.cr.ranges(compute_id)
        refs = self.cr.references(compute_id)
        unit = self.L * self.split_k
        saved = self.C.array.copy()
        worst, checked = 0.0, 0
        try:
            for dev in range(self.cr._cores.num_devices):
                g = self.cr._cores.global_base + dev
                t0, nt = refs[g] // unit, ranges[g] // unit
                if nt == 0:
                    continue
                if not host:
                    self.cr.download(self.C, dev)
                tm, tn = tile_coords(np.arange(t0, t0 + nt), M, N, BM, BN, self.group_m,
                                     self._orders.get(compute_id, 0))
                tm_t = torch.from_numpy(np.asarray(tm, np.int64)).to(device)
                tn_t = torch.from_numpy(np.asarray(tn, np.int64)).to(device)
                c = torch.from_numpy(self.C.array).to(device)
                if self.row_major_c:
                    got = c.view(ntm, BM, ntn, BN).permute(0, 2, 1, 3)[tm_t, tn_t]
                else:
                    flat = c.view(-1, BM * BN)[t0:t0 + nt]
                    if self.geom is None:
                        got = flat.view(nt, BM, BN)
                    else:
                        WM, WN, FM, FN = self.geom
                        got = flat.view(nt, WM, WN, FM, FN, 4, 16, 4).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(nt, BM, BN)
                want = ref_tiles[tm_t, tn_t]
                err = (got.double() - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2)).clamp_min(1e-30)
                worst = max(worst, float(err.max()))
                checked += nt
                del c, got, want, err
        finally:
            self.C.array[:] = saved
        return worst, checked

    def _download_slice(self, dev: int, lo: int, n: int) -> None:
        # a sub-view ClArray sharing the same uid would alias buffers; the
        # native download copies the whole replica, slice afterwards
        tmp = np.empty_like(self.C.array)
        saved = self.C.array.copy()
        self.cr.download(self.C, dev)
        tmp[:] = self.C.array
        self.C.array[:] = saved
        self.C.array[lo:lo + n] = tmp[lo:lo + n]

    def reference(self, rows: slice = slice(None)) -> np.ndarray:
        a = self._operand("A")[rows].astype(np.float64)
        b = self._operand("B").astype(np.float64)
        return a @ b.T


class GemmF32(GemmBf16):
    """``C = A · Bᵀ`` in fp32 on the fp32 matrix cores (``v_mfma_f32_16x16x4_f32``):
    A ``[M][K]``, Bt ``[N][K]`` and C fp32, C tile-major like :class:`GemmBf16`
    (same grouped tile order, so the same range partitioning and
    wave-quantized balancing apply)."""

    TILE_TABLE = F32_TILES
    TILE_GEOM = None  # the fp32 kernels store C tiles row-major
    K_MULTIPLE = 32
    LIBS = ("sgemm_f32",)
    OPERAND_DTYPE = np.float32
    _encode = staticmethod(lambda x: x)

    def __init__(self, M: int, N: int, K: int, devices=None, tile: str = "256x256g8i",
                 cruncher: ClNumberCruncher | None = None, fill: str = "random", seed: int = 0,
                 group_m: int = 4, wave_granularity: bool | None = None):
        super().__init__(M, N, K, devices, tile, cruncher, fill, seed, group_m, wave_granularity=wave_granularity)


class GemmFp8(GemmBf16):
    """``C = A · Bᵀ`` with OCP e4m3fn operands (one byte per element, half the
    device memory and transfer bytes of bf16) and fp32 accumulation and
    output: A ``[M][K]``, Bt ``[N][K]`` as ``ClArray(…, "float8_e4m3fn")``, C
    tile-major in fragment order like :class:`GemmBf16`, so the range
    partitioning, the streamed and shell paths and every ``verify`` apply
    unchanged.  ``fill="random"`` draws uniform [−1, 1) values and quantises
    them with :func:`to_fp8_e4m3_bits`.  K must be a multiple of 128.

    Numerics (measured, profiles/gemm8_specials.md): the NaN codes ``0x7F`` /
    ``0xFF`` poison exactly their row (A) or column (Bt) of C, 0·NaN
    included.  The sum over k is not a chain of fp32 additions: both fp8
    matrix instructions align the products of 8 neighbouring k to the largest
    of them and keep 14 bits, so a product more than 2^13 times smaller than
    a neighbour is dropped.  Data of a narrow range inside every such group
    (small integers, uniform random values) is summed as fp32 would."""

    TILE_TABLE = FP8_TILES
    TILE_GEOM = FP8_TILE_WAVES
    K_MULTIPLE = 128
    POSITIVE_DIMS = True
    LIBS = ("sgemm_fp8",)
    OPERAND_DTYPE = "float8_e4m3fn"
    _encode = staticmethod(to_fp8_e4m3_bits)

    def __init__(self, M: int, N: int, K: int, devices=None, tile: str = "256x256pbx",
                 cruncher: ClNumberCruncher | None = None, fill: str = "random", seed: int = 0,
                 group_m: int = 4, wave_granularity: bool | None = None):
        super().__init__(M, N, K, devices, tile, cruncher, fill, seed, group_m, wave_granularity=wave_granularity)


class GemmMxFp8(GemmBf16):
    """``C = (A∘SA) · (B∘SB)ᵀ`` in OCP MXFP8: e4m3fn elements (``A``, ``B`` as
    in :class:`GemmFp8`) with one E8M0 scale byte per 32 consecutive k, an
    element's value being ``e4m3(code) · 2^(scale − 127)``; fp32 accumulation
    and output, C tile-major in fragment order like :class:`GemmBf16`.

    ``SA`` (``M·K/32``) and ``SB`` (``N·K/32``) are the row-major uint8 scale
    arrays a user fills (:func:`to_mxfp8` produces codes and scales).  The
    kernels read them in a packed layout (:func:`pack_mx_scales`), kept in
    device-side arrays of this object and re-packed from ``SA`` / ``SB``
    whenever the operands are uploaded: on the first call, and on every
    ``resident=False`` call.  On several devices, and in streamed calls, the
    scale arrays go whole to every device.

    ``fill="random"`` draws uniform [−1, 1) values times ``2^u`` per block, u
    an integer uniform in [−12, 12], and quantises them with
    :func:`to_mxfp8`.  K must be a multiple of 128.  The shell paths are not
    available.

    Numerics (measured, profiles/gemm8_specials.md): a scale byte ``0xFF``
    makes its block NaN (OCP MX, :func:`e8m0_to_f64`) and with it the row or
    column of C, whatever the elements; the two scale exponents are added as
    integers before they meet the product, so byte 254 with byte 0 cancels
    exactly and 254 + 254 gives ±Inf; results in fp32's subnormal range are
    exact, nothing is flushed.  Element NaNs and the 14-bit sum over 8
    neighbouring k are as in :class:`GemmFp8`.

    :meth:`quantize` makes an operand from fp32 or bf16 data on the devices
    instead (``kernels/mx_quantize.hip``, the same bits as :func:`to_mxfp8`):
    codes, scales and packed scales stay resident and the next resident
    :meth:`run` uploads nothing for that operand; its host arrays are stale
    until :meth:`sync_operands`, which every host reference (``verify*``,
    ``reference``) calls first.

    Output modes (``kernels/sgemm_mx_out.hip``).  ``out="bfloat16"``,
    ``"mxfp8"`` or ``"mxfp4"`` makes the kernel store the next layer's operand
    instead of ``C``: ``Y``, row-major ``[M][N]`` (bf16 bit patterns, e4m3fn
    codes, or ``[M][N/2]`` packed e2m1) and, for the MX outputs, ``SY``
    (``[M][N/32]`` E8M0 bytes, blocks of 32 along N) and the packed scales
    ``Yp``, which a pack compute behind the GEMM makes from ``SY`` (compute id
    ``compute_id + MX_OUT_PACK_ID``; ``records`` holds both records).  The
    loop is the plain tile's, so what is converted is the plain kernel's C
    bit for bit, and the conversion is the host codec's bit for bit
    (:func:`~cekirdekler_amd.ops.quantize.gemm_out_model`).  ``act="relu"``
    (``x > 0 → x``, ``NaN → NaN``, all else ``→ +0``) is applied to the fp32
    accumulator first and needs an output mode.  ``Y`` and ``SY`` carry C's
    flags; being row-major, a device's range is a block of rows only in
    whole tile groups, so on several devices the split unit is one tile
    group, ``(M / BM) % group_m`` must be 0 and the outputs are keep-resident
    gathered; one device takes a ragged last group too.  :meth:`result`
    decodes what was stored; streaming and the shell paths raise
    ``ValueError``.  :meth:`take_operand` hands the output to the next GEMM."""

    TILE_TABLE = MXFP8_TILES
    TILE_GEOM = MXFP8_TILE_WAVES
    K_MULTIPLE = 128
    POSITIVE_DIMS = True
    LIBS = ("sgemm_mxfp8", "mx_quantize")
    OPERANDS = {"A": MXFP8, "B": MXFP8}  # the MX format of each operand

    FORMAT = "mxfp8"  # the key of OUT_KERNELS
    OUT_KERNELS = MX_OUT_KERNELS  # (FORMAT, tile, out) -> output-mode kernel, in library OUT_LIB
    OUT_LIB = MX_OUT_LIB

    def _operand_dtype(self, name: str):
        return self.OPERANDS[name].dtype

    def _per_item(self, name: str) -> int:
        return self.OPERANDS[name].per_item

    def __init__(self, M: int, N: int, K: int, devices=None, tile: str = "256x256pbx",
                 cruncher: ClNumberCruncher | None = None, fill: str = "random", seed: int = 0,
                 group_m: int = 4, wave_granularity: bool | None = None, out: str | None = None,
                 act: str | None = None):
        self._stale = set()  # operands made on the device whose host arrays are behind
        self._quantizers = {}
        self._taken = {}  # operand name -> the output-mode GEMM whose Y / SY / packed arrays it is
        self._consumers = []  # (weak reference to a GEMM that took this one's output, operand name)
        if out is not None and out not in MX_OUTPUTS:
            raise ValueError(f"out must be None or one of {MX_OUTPUTS} (got {out!r})")
        if act not in MX_ACTIVATIONS:
            raise ValueError(f"act must be None or 'relu' (got {act!r})")
        if act is not None and out is None:
            raise ValueError("act needs an output mode (out=...): the plain kernels store the accumulator as it is")
        self.out, self.act = out, act
        if out is not None:
            self.LIBS = type(self).LIBS + (self.OUT_LIB,)
        super().__init__(M, N, K, devices, tile, cruncher, fill, seed, group_m, wave_granularity=wave_granularity)
        if out is None:
            return
        self.kernel = self.OUT_KERNELS[self.FORMAT, tile, out]
        self.dims.array[5] = MX_ACTIVATIONS[act]
        if self.cr.number_of_devices > 1 and (M // self.BM) % max(1, group_m):
            raise ValueError(f"an output mode on several devices needs whole tile groups: (M / {self.BM}) = "
                             f"{M // self.BM} must be a multiple of group_m ({group_m})")

    def _alloc_output(self) -> None:
        if self.out is None:
            return super()._alloc_output()
        # Y row-major [M][N] in the output's format, for the MX outputs with
        # its row-major scales SY [M][N/32] and their packed form: the trio of
        # an A / B operand with K = N.  Per work item: a tile's share, under
        # which a device's range of whole tile groups is one block of rows.
        n, per_tile = self.M * self.N, self.BM * self.BN
        self.C = None
        self.SY = self.Yp = None
        fmt = MX_FORMATS.get(self.out)  # None: bf16
        self.Y = ClArray(n // fmt.per_item, fmt.dtype) if fmt else ClArray(n, "bfloat16")
        self._out_epw = [(self.Y, per_tile * self.Y.N // n // self.L)]
        if fmt:
            self.SY = ClArray(n // MX_BLOCK, np.uint8)
            self.Yp = ClArray(n // 128, np.uint32)
            self._dims_pack = ClArray(np.array([self.M, self.N], np.int32))
            self._out_epw.append((self.SY, per_tile // MX_BLOCK // self.L))
        for a, epw in self._out_epw:
            a.read = False
            a.elements_per_work_item = epw
        self.records = []

    def _output_flags(self, resident: bool) -> None:
        if self.out is None:
            return super()._output_flags(resident)
        gather = self.cr.number_of_devices > 1
        for a, epw in self._out_epw:
            a.read = a.partial_read = False
            a.write, a.elements_per_work_item, a.gather_resident = not resident, epw, gather

    def _after_compute(self, compute_id: int, resident: bool) -> None:
        if self.out is None:
            return
        self.records = [self.cr.last_record()]
        if self.Yp is not None:
            # the packed scales a consumer reads, from the whole resident SY
            # (the pack compute of _MxQuantizer.run)
            gather = self.cr.number_of_devices > 1
            d, p = self._dims_pack, self.Yp
            self.SY.write = self.SY.gather_resident = False
            self.SY.elements_per_work_item = 1
            d.read, d.write = True, False
            p.read = p.partial_read = False
            p.write, p.elements_per_work_item, p.gather_resident = not resident, 1, gather
            d.next_param(self.SY, p).compute(self.cr, compute_id + MX_OUT_PACK_ID, PACK_KERNEL, p.N, QUANTIZE_LOCAL)
            self.records.append(self.cr.last_record())
        for ref, name in self._consumers:  # their host copies of this output are behind again
            g = ref()
            if g is not None and g._taken.get(name) is self:
                g._stale.add(name)

    def granularity(self) -> int:
        """:meth:`GemmBf16.granularity`; an output mode on several devices
        splits in whole tile groups, so that every device's range is one block
        of rows of the row-major ``Y`` and ``SY``."""
        if self.out is not None and self.cr.number_of_devices > 1:
            return self._group_work_items()
        return super().granularity()

    def _alloc_scales(self) -> tuple:
        M, N, K = self.M, self.N, self.K
        self.SA = ClArray(np.full(M * K // MX_BLOCK, 127, np.uint8))  # 2^0
        self.SB = ClArray(np.full(N * K // MX_BLOCK, 127, np.uint8))
        # the packed scales the kernels read; run() fills them from SA / SB
        self._SAp = ClArray(np.zeros(M * K // 128, np.uint32))
        self._SBp = ClArray(np.zeros(N * K // 128, np.uint32))
        return self._SAp, self._SBp

    def _fill_random(self, rng) -> None:
        """Per operand, A then B: uniform [−1, 1) values times ``2^u`` per
        block, u an integer uniform in [−12, 12], quantised by the format."""
        K = self.K
        for name, arr, sc, rows in (("A", self.A, self.SA, self.M), ("B", self.B, self.SB, self.N)):
            x = rng.uniform(-1, 1, (rows, K // MX_BLOCK, MX_BLOCK))
            x = np.ldexp(x, rng.integers(-12, 13, (rows, K // MX_BLOCK, 1)))
            codes, scales = self.OPERANDS[name].encode(x.astype(np.float32).reshape(rows, K))
            arr.array[:] = codes.ravel()
            sc.array[:] = scales.ravel()

    def _inputs(self, upload: bool) -> tuple:
        # an operand quantised on the device is resident with its packed
        # scales: it is neither uploaded nor re-packed from its (stale) host arrays
        host = [n for n in ("A", "B") if n not in self._stale]
        if upload:  # the operands go up: the packed scales follow the public ones
            if "A" in host:
                self._SAp.array[:] = pack_mx_scales(self.SA.array.reshape(self.M, -1)).ravel()
            if "B" in host:
                self._SBp.array[:] = pack_mx_scales(self.SB.array.reshape(self.N, -1)).ravel()
        trio = {"A": (self.A, self._SAp), "B": (self.B, self._SBp)}
        return (self.dims, *(trio[n][0] for n in host), *(trio[n][1] for n in host))

    def _params(self) -> tuple:
        if self.out is not None:  # Y and, for the MX outputs, SY in C's place
            return (self.A, self.B, self._SAp, self._SBp, *(a for a, _ in self._out_epw))
        return self.A, self.B, self._SAp, self._SBp, self.C

    def run(self, compute_id: int = 1, resident: bool = True, stream_blobs: int = 0,
            stream_event: bool = True) -> None:
        """:meth:`GemmBf16.run`.  An operand quantised on the device
        (:meth:`quantize`) is used where it lies: a resident call uploads only
        the other operand (on its first call) and ``dims``; a host-resident
        call would send the stale host arrays and is refused until
        :meth:`sync_operands` has fetched them."""
        if self._stale and not resident:
            raise ValueError(f"operand(s) {sorted(self._stale)} were quantised on the device and the host arrays are "
                             "stale: call sync_operands() before a run(resident=False)")
        if self.out is not None and stream_blobs:
            raise ValueError("an output mode (out=...) has no streamed path: stream_blobs must be 0")
        if self.out is not None:
            have = {k.split(":")[0] for k in self.cr.kernel_names}
            for k in (self.kernel, PACK_KERNEL):
                if k not in have:
                    raise ClComputeError(f"the cruncher has no kernel {k!r}: it was built without "
                                         f"library({self.OUT_LIB!r}) or library('mx_quantize')")
        for name in self._taken:  # shared with their producer, which sets its own flags for its calls
            for a in ((self.A, self._SAp) if name == "A" else (self.B, self._SBp)):
                a.write = a.gather_resident = a.partial_read = False
                a.elements_per_work_item = 1
        super().run(compute_id, resident, stream_blobs, stream_event)

    def take_operand(self, name: str, producer: "GemmMxFp8") -> None:
        """Make the output of ``producer``, an MX GEMM with ``out`` equal to
        this class's format, operand ``name`` of this GEMM: ``Y`` / ``SY`` and
        the packed scales become ``A`` / ``SA`` (``B`` / ``SB``) and the packed
        array the kernels read — the same :class:`ClArray` objects on the same
        cruncher, so the resident replicas the producer wrote are the operand
        and nothing is copied.  The residency rules are :meth:`quantize`'s:
        the next resident :meth:`run` uploads nothing for the operand, its
        host arrays are stale (again after every call of the producer) until
        :meth:`sync_operands`, and ``run(resident=False)`` is refused while
        they are."""
        if name not in ("A", "B"):
            raise ValueError(f"operand name must be 'A' or 'B' (got {name!r})")
        out, fmt = getattr(producer, "out", None), self.OPERANDS[name].name
        if out != fmt:
            raise ValueError(f"format mismatch: {type(self).__name__} takes a producer with out={fmt!r} "
                             f"(got out={out!r})")
        rows = self.M if name == "A" else self.N
        if producer.M != rows:
            raise ValueError(f"rows mismatch: operand {name} has {rows} rows, the producer's M is {producer.M}")
        if producer.N != self.K:
            raise ValueError(f"K mismatch: this GEMM's K is {self.K}, the producer's N is {producer.N}")
        if producer.cr is not self.cr:
            raise ValueError("cruncher mismatch: producer and consumer must run on the same ClNumberCruncher")
        if name == "A":
            self.A, self.SA, self._SAp = producer.Y, producer.SY, producer.Yp
        else:
            self.B, self.SB, self._SBp = producer.Y, producer.SY, producer.Yp
        for k in [k for k in self._quantizers if k[0] == name]:  # they hold the arrays given up
            del self._quantizers[k]
        self._taken[name] = producer
        producer._consumers = [(r, n) for r, n in producer._consumers
                               if r() is not None and (r() is not self or n != name)]
        producer._consumers.append((weakref.ref(self), name))
        self._stale.add(name)

    def quantize(self, name: str, x, src: str | None = None, download: bool = False) -> None:
        """Quantise operand ``name`` (``"A"``: ``[M][K]``, ``"B"``: ``[N][K]``)
        to MXFP8 on the devices of this GEMM's cruncher
        (:class:`~cekirdekler_amd.ops.quantize.MxFp8Quantizer`, bit for bit
        :func:`to_mxfp8`): afterwards the codes, the row-major scales and the
        packed scales are resident on every device and the next resident
        :meth:`run` uses them without an upload.

        ``x``: a float32 numpy array (copied into a pinned array of this
        object and uploaded), bf16 bit patterns as a uint16 numpy array with
        ``src="bfloat16"``, or a float32 / bf16 :class:`ClArray`, whose
        ``read`` flag says whether it is uploaded (``False``: it is resident,
        e.g. another kernel of this cruncher wrote it).  ``download=True``
        also brings the codes and scales into ``A`` / ``SA`` (``B`` / ``SB``);
        otherwise the host arrays are stale until :meth:`sync_operands`.

        The quantizer is that of the operand's format (``OPERANDS``); its
        quantise and pack computes run under the format's ``base_id`` (A) or
        ``base_id + 2`` (B) and the id after it."""
        if name not in ("A", "B"):
            raise ValueError(f"operand name must be 'A' or 'B' (got {name!r})")
        fmt = self.OPERANDS[name]
        rows = self.M if name == "A" else self.N
        n = rows * self.K
        if isinstance(x, ClArray):
            given = "bfloat16" if x.is_bf16 else "float32" if x.array.dtype == np.float32 else None
            if given is None or (src is not None and _src_name(src) != given):
                raise ValueError(f"x must be a float32 or bfloat16 ClArray matching src (got {x.dtype_name}, src={src!r})")
            length, key, upload = x.N, (name, given, x.uid), x.read
        else:
            given = _src_name(src or "float32")
            x = np.asarray(x)
            if given == "bfloat16" and x.dtype != np.uint16:
                raise ValueError("a bfloat16 operand is given as uint16 bit patterns or as a bf16 ClArray")
            if given == "float32" and x.dtype != np.float32:
                raise ValueError(f"a float32 operand is given as a float32 array (got {x.dtype})")
            length, key, upload = x.size, (name, given, None), True
        if length != n:
            raise ValueError(f"operand {name} has {rows}x{self.K} = {n} elements (got {length})")
        q = self._quantizers.get(key)
        if q is None:
            for k in [k for k in self._quantizers if k[0] == name]:  # one quantizer (and input buffer) per operand
                del self._quantizers[k]
            codes, scales, packed = (self.A, self.SA, self._SAp) if name == "A" else (self.B, self.SB, self._SBp)
            q = fmt.quantizer(rows, self.K, given, cruncher=self.cr, codes=codes, scales=scales, packed=packed,
                              x=x if isinstance(x, ClArray) else None)
            self._quantizers[key] = q
        if not isinstance(x, ClArray):
            q.X.array[:] = x.reshape(-1)
        base = fmt.base_id + (0 if name == "A" else 2)  # compute ids of the quantise and pack computes
        q.run(compute_id=base, upload=upload, download=download, pack_compute_id=base + 1)
        for a in (q.codes, q.scales, q.packed):
            a.read = False  # resident: the next run() must not send the host copy
        if download:
            self._stale.discard(name)
        else:
            self._stale.add(name)

    def sync_operands(self) -> None:
        """Download the codes and row-major scales of every operand quantised
        on the device (from device 0, which holds them whole) into ``A`` /
        ``SA`` / ``B`` / ``SB`` and clear their stale mark."""
        for name in sorted(self._stale):
            for a in ((self.A, self.SA) if name == "A" else (self.B, self.SB)):
                self.cr.download(a, 0)
        self._stale.clear()

    def _scales(self, name: str) -> np.ndarray:
        """float64 ``[rows][K/32]`` scale factors of operand ``name``."""
        if self._stale:
            self.sync_operands()
        arr, rows = (self.SA, self.M) if name == "A" else (self.SB, self.N)
        return e8m0_to_f64(arr.array.reshape(rows, self.K // MX_BLOCK))

    def _operand(self, name: str) -> np.ndarray:
        """Dequantised operand, float64 (the product with the scale is exact there)."""
        if self._stale:
            self.sync_operands()
        x = super()._operand(name).astype(np.float64)
        return (x.reshape(-1, self.K // MX_BLOCK, MX_BLOCK) * self._scales(name)[..., None]).reshape(-1, self.K)

    def _operand_t(self, name: str, device):
        import torch

        if self._stale:
            self.sync_operands()
        x = super()._operand_t(name, device)
        sc = torch.from_numpy(self._scales(name)).to(device)
        return (x.view(-1, self.K // MX_BLOCK, MX_BLOCK) * sc[..., None]).view(-1, self.K)

    def result(self, download: bool = True) -> np.ndarray:
        """:meth:`GemmBf16.result`.  In an output mode: what was stored,
        decoded to fp32 row-major ``[M][N]`` (the MX outputs through
        :func:`from_mxfp8` / :func:`from_mxfp4`); ``download`` fetches ``Y``
        and ``SY`` from device 0, which holds them whole."""
        if self.out is None:
            return super().result(download)
        if download:
            for a, _ in self._out_epw:
                self.cr.download(a, 0)
        if self.out == "bfloat16":
            return from_bf16_bits(self.Y.array).reshape(self.M, self.N)
        fmt = MX_FORMATS[self.out]
        with np.errstate(over="ignore", invalid="ignore"):
            return fmt.decode(self.Y.array.reshape(self.M, self.N // fmt.per_item),
                              self.SY.array.reshape(self.M, self.N // MX_BLOCK)).astype(np.float32)

    def verify(self, compute_id: int = 1, tiles_per_device: int = 8, seed: int = 1, host: bool = False) -> float:
        """:meth:`GemmBf16.verify`.  In an output mode: ``max |Y − act(ref)| /
        max |ref|`` over the whole decoded output against the float64
        product, the output format's rounding included (of the order of 2^-9
        for bf16, 2^-4 for MXFP8, 2^-2 for MXFP4): a plausibility figure, not
        a check of the bits."""
        if self.out is None:
            return super().verify(compute_id, tiles_per_device, seed, host)
        got = self.result(download=not host).astype(np.float64)
        ref = self.reference()
        if self.act == "relu":
            ref = np.where(ref > 0, ref, np.where(np.isnan(ref), ref, 0.0))
        return float(np.nanmax(np.abs(got - ref)) / max(float(np.nanmax(np.abs(ref))), 1e-30))

    def verify_full(self, compute_id: int = 1, host: bool = False, device=None) -> tuple:
        if self.out is None:
            return super().verify_full(compute_id, host, device)
        return self.verify(compute_id, host=host), self.tiles

    def _no_shells(self, *a, **k):
        if self.out is not None:
            raise ValueError("an output mode (out=...) has no shell paths")
        raise NotImplementedError(f"{type(self).__name__} has no shell paths: the shell streamer "
                                  "(csrc/shell_gemm.cpp) passes no scales")

    run_shells = run_host_shells = verify_shells = verify_shells_full = _no_shells


class GemmMxFp4(GemmMxFp8):
    """``C = (A∘SA) · (B∘SB)ᵀ`` in OCP MXFP4: e2m1 elements, two per byte,
    with one E8M0 scale byte per 32 consecutive k, an element's value being
    ``e2m1(code) · 2^(scale − 127)``; fp32 accumulation and output, C
    tile-major in fragment order like :class:`GemmBf16`.

    ``A`` (``M·K/2`` bytes) and ``B`` (``N·K/2`` bytes) are
    ``ClArray(…, "float4_e2m1fn_x2")``: row-major ``[M][K/2]`` / ``[N][K/2]``,
    element ``2i`` of a row in bits 0–3 of its byte ``i`` and element
    ``2i + 1`` in bits 4–7 (:func:`pack_fp4`).  ``SA`` (``M·K/32``) and ``SB``
    (``N·K/32``) are the row-major uint8 scale arrays; :func:`to_mxfp4`
    produces both.  The kernels read the scales in the packed layout of
    :func:`pack_mx_scales`, kept in device-side arrays of this object and
    re-packed from ``SA`` / ``SB`` whenever the operands are uploaded, as in
    :class:`GemmMxFp8`.

    ``fill="random"`` is :class:`GemmMxFp8`'s draw (uniform [−1, 1) times
    ``2^u`` per block, u an integer uniform in [−12, 12]) through
    :func:`to_mxfp4`.  K must be a multiple of 256 (one K-tile of 128 bytes).
    ``flops`` counts ``2·M·N·K`` with K in elements.  The shell paths are not
    available.

    :meth:`quantize_operand` makes an operand from fp32 or bf16 data on the
    devices (``kernels/mx4_quantize.hip``, the same bits as :func:`to_mxfp4`),
    with the residency and stale-host-array rules of
    :meth:`GemmMxFp8.quantize`; :meth:`quantize` itself is not available here.

    Numerics: e2m1 has no NaN; a scale byte ``0xFF`` makes its block NaN
    (OCP MX) and with it the row or column of C.  profiles/gemm_mxfp4.md has
    what the single-instruction probe measured."""

    TILE_TABLE = MXFP4_TILES
    TILE_GEOM = MXFP4_TILE_WAVES
    FORMAT = "mxfp4"
    K_MULTIPLE = 256
    LIBS = ("sgemm_mxfp4", "mx4_quantize", "mx_quantize")
    OPERANDS = {"A": MXFP4, "B": MXFP4}
    PER_ITEM = MXFP4.per_item  # bytes of two elements each

    def quantize(self, *a, **k):
        raise NotImplementedError("GemmMxFp4 takes operands quantised on the host (to_mxfp4): on-device MXFP4 "
                                  "quantisation is a separate, later change")

    def quantize_operand(self, name: str, x, src: str | None = None, download: bool = False) -> None:
        """:meth:`GemmMxFp8.quantize` for MXFP4: quantise operand ``name``
        from ``x`` (a float32 numpy array, bf16 bit patterns as uint16 with
        ``src="bfloat16"``, or a float32 / bf16 :class:`ClArray` whose
        ``read`` flag says whether it is uploaded) on the devices of this
        GEMM's cruncher (:class:`~cekirdekler_amd.ops.quantize.MxFp4Quantizer`,
        bit for bit :func:`to_mxfp4`, a block with a NaN getting the scale
        byte ``0xFF``).  The packed codes, the row-major scales and the packed
        scales stay resident for the next resident :meth:`run`; the host
        arrays are stale until :meth:`sync_operands` unless ``download``."""
        GemmMxFp8.quantize(self, name, x, src, download)


class GemmMxFp8Fp4(GemmMxFp8):
    """``C = (A∘SA) · (B∘SB)ᵀ`` with MXFP8 activations against MXFP4 weights
    ("W4A8"): ``A`` ``[M][K]`` e4m3fn bytes (``ClArray(…, "float8_e4m3fn")``,
    as in :class:`GemmMxFp8`), ``B`` ``[N][K/2]`` packed e2m1
    (``ClArray(…, "float4_e2m1fn_x2")``, the low nibble the even k, as in
    :class:`GemmMxFp4`), ``SA`` (``M·K/32``) and ``SB`` (``N·K/32``) E8M0 scale
    bytes, one per 32 consecutive k; fp32 accumulation and output, C
    tile-major in fragment order like :class:`GemmBf16`.  B's device and
    upload bytes are half of :class:`GemmMxFp8`'s, and A keeps its 8 bits.

    Only this orientation exists (A 8-bit, B 4-bit): 4-bit A against 8-bit B is
    the same product transposed, ``(B∘SB) · (A∘SA)ᵀ = Cᵀ`` with the operands'
    roles exchanged.

    ``fill="random"`` is :class:`GemmMxFp8`'s draw through :func:`to_mxfp8`
    for A and :func:`to_mxfp4` for B.  K must be a multiple of 256 (one K-tile
    of 128 bytes of B).  Every host reference decodes each operand by its own
    format.  The shell paths are not available.

    ``quantize("A", x)`` runs :class:`~cekirdekler_amd.ops.quantize.MxFp8Quantizer`
    and ``quantize("B", x)`` :class:`~cekirdekler_amd.ops.quantize.MxFp4Quantizer`,
    with :meth:`GemmMxFp8.quantize`'s residency rules; ``take_operand("A", p)``
    needs ``p.out == "mxfp8"`` and ``take_operand("B", p)`` ``p.out ==
    "mxfp4"``.  ``out=`` and ``act=`` are :class:`GemmMxFp8`'s, through
    ``kernels/sgemm_mxf8f4_out.hip``.

    Numerics: profiles/gemm_mxf8f4.md has what the single-instruction probe of
    the mixed form measured; A's NaN codes and a scale byte ``0xFF`` poison
    their row or column of C as in the pure formats."""

    TILE_TABLE = MXF8F4_TILES
    TILE_GEOM = MXF8F4_TILE_WAVES
    FORMAT = "mxf8f4"  # the key of OUT_KERNELS; the operands' formats are OPERANDS'
    OUT_KERNELS = MXF8F4_OUT_KERNELS
    OUT_LIB = MXF8F4_OUT_LIB
    K_MULTIPLE = 256
    LIBS = ("sgemm_mxf8f4", "mx_quantize", "mx4_quantize")
    OPERANDS = {"A": MXFP8, "B": MXFP4}

    def __init__(self, M: int, N: int, K: int, devices=None, tile: str = "128x256pbx",
                 cruncher: ClNumberCruncher | None = None, fill: str = "random", seed: int = 0,
                 group_m: int = 4, wave_granularity: bool | None = None, out: str | None = None,
                 act: str | None = None):
        super().__init__(M, N, K, devices, tile, cruncher, fill, seed, group_m, wave_granularity, out, act)
