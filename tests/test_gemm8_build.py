"""What the compiler made of the byte-operand GEMM kernels (kernels/gemm8_tile.h
and the six files that instantiate it): no warning from those sources, and
per kernel, from the code object's metadata notes read with the ROCm
llvm-readelf, no private segment, no spill, the LDS size the tile table and
the operand formats give, and the register counts of the kernels as they were
before the tile function took its operands by format.  No instruction is
inspected."""
import os
import re
import subprocess

import pytest

from cekirdekler_amd import build_native as bn
from cekirdekler_amd.ops import gemm
from cekirdekler_amd.ops.library import LIBRARY, code_object

LLVM_BIN = os.path.join(bn.ROCM, "llvm", "bin")
KDIR = os.path.join(os.path.dirname(bn.__file__), "kernels")

# code object -> (tile table, bits per element of A, of Bt)
FILES = {
    "sgemm_fp8": (gemm.FP8_TILES, 8, 8),
    "sgemm_mxfp8": (gemm.MXFP8_TILES, 8, 8),
    "sgemm_mxfp4": (gemm.MXFP4_TILES, 4, 4),
    "sgemm_mxf8f4": (gemm.MXF8F4_TILES, 8, 4),
    "sgemm_mx_out": (None, None, None),  # the MXFP8 and MXFP4 tiles, by kernel name
    "sgemm_mxf8f4_out": (gemm.MXF8F4_TILES, 8, 4),
}

# kernel -> (.vgpr_count, .agpr_count, .sgpr_count), recorded from a build of
# the commit before this test (8176475), whose tile function took four booleans
REGISTERS = {
    "cek_sgemm_fp8_128x128": (108, 64, 49),
    "cek_sgemm_fp8_256x256pb": (232, 0, 49),
    "cek_sgemm_fp8_256x256pbx": (233, 0, 49),
    "cek_sgemm_mxfp8_128x128": (208, 64, 55),
    "cek_sgemm_mxfp8_256x256pbx": (239, 0, 55),
    "cek_sgemm_mxfp4_128x128": (208, 64, 57),
    "cek_sgemm_mxfp4_256x256pbx": (245, 0, 57),
    "cek_sgemm_mxf8f4_128x128": (252, 64, 57),
    "cek_sgemm_mxf8f4_128x256pbx": (191, 0, 63),
    "cek_sgemm_mxfp8_128x128_bf16": (212, 64, 57),
    "cek_sgemm_mxfp8_128x128_mxfp8": (212, 64, 60),
    "cek_sgemm_mxfp8_128x128_mxfp4": (212, 64, 60),
    "cek_sgemm_mxfp8_256x256pbx_bf16": (242, 0, 57),
    "cek_sgemm_mxfp8_256x256pbx_mxfp8": (242, 0, 60),
    "cek_sgemm_mxfp8_256x256pbx_mxfp4": (242, 0, 60),
    "cek_sgemm_mxfp4_128x128_bf16": (212, 64, 59),
    "cek_sgemm_mxfp4_128x128_mxfp8": (212, 64, 61),
    "cek_sgemm_mxfp4_128x128_mxfp4": (212, 64, 61),
    "cek_sgemm_mxfp4_256x256pbx_bf16": (248, 0, 59),
    "cek_sgemm_mxfp4_256x256pbx_mxfp8": (248, 0, 63),
    "cek_sgemm_mxfp4_256x256pbx_mxfp4": (248, 0, 63),
    "cek_sgemm_mxf8f4_128x128_bf16": (256, 64, 59),
    "cek_sgemm_mxf8f4_128x128_mxfp8": (256, 64, 61),
    "cek_sgemm_mxf8f4_128x128_mxfp4": (256, 64, 61),
    "cek_sgemm_mxf8f4_128x256pbx_bf16": (194, 0, 66),
    "cek_sgemm_mxf8f4_128x256pbx_mxfp8": (194, 0, 70),
    "cek_sgemm_mxf8f4_128x256pbx_mxfp4": (194, 0, 70),
}
KERNELS = [(lib, k) for lib in FILES for k in LIBRARY[lib]]


def lds_bytes(lib: str, kernel: str) -> int:
    """gemm8_lds_bytes of kernels/gemm8_tile.h from the tile table and the
    formats: rows of 128 B, Bt one row per tile column, A bits(A) / bits(Bt)
    sub-tiles; two whole stages, or (ping-pong) two A and three Bt buffers."""
    tiles, bits_a, bits_b = FILES[lib]
    if tiles is None:
        fmt = kernel.split("_")[2]
        tiles, bits_a, bits_b = {"mxfp8": (gemm.MXFP8_TILES, 8, 8), "mxfp4": (gemm.MXFP4_TILES, 4, 4)}[fmt]
    (tile, (bm, bn, _l, _k)), = [(t, v) for t, v in tiles.items()
                                 if kernel == v[3] or kernel.rsplit("_", 1)[0] == v[3]]
    a, b = bm * 128 * (bits_a // bits_b), bn * 128
    return 2 * a + 3 * b if "pb" in tile else 2 * (a + b)


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """kernel -> {key: value} of every kernel of the six code objects' gfx950 ELFs."""
    tmp, out = tmp_path_factory.mktemp("gemm8"), {}
    for lib in FILES:
        elf = str(tmp / (lib + ".elf"))
        subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--type=o", "--unbundle",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{bn.ARCH}", f"--input={code_object(lib)}",
                        f"--output={elf}"], check=True)
        notes = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", elf], check=True,
                               stdout=subprocess.PIPE, text=True).stdout
        # one entry of amdhsa.kernels per "  - " at list depth; its scalar keys sit at four spaces
        for entry in re.split(r"^  - ", notes, flags=re.M)[1:]:
            kv = dict(re.findall(r"^(?:    )?(\.\w+): +(\S+)$", entry, flags=re.M))
            if ".vgpr_count" in kv:
                out[kv[".name"]] = kv
    return out


def test_expected_lds_sizes():
    """The formula gives what the kernel files state: 64 KiB for the 128x128
    tiles of one format, 96 KiB for the mixed one, 160 KiB for every ping-pong tile."""
    for lib, k in KERNELS:
        want = 160 if "pb" in k else 96 if "mxf8f4" in k else 64
        assert lds_bytes(lib, k) == want * 1024, k


def test_every_kernel_is_described(metadata):
    assert sorted(metadata) == sorted(k for _, k in KERNELS) == sorted(REGISTERS) and len(KERNELS) == 27


@pytest.mark.parametrize("lib", FILES)
def test_sources_compile_without_warnings(lib):
    """The file's own command line, device-only and -fsyntax-only: nothing is
    reported from the .hip file or gemm8_tile.h."""
    src = os.path.join(KDIR, lib + ".hip")
    cmd = [a for a in bn.kernel_command(src, os.devnull)[:-2] if a != "--genco"]
    r = subprocess.run(cmd + ["--cuda-device-only", "-fsyntax-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout
    hits = [ln for ln in r.stdout.splitlines() if re.search(r"(gemm8_tile\.h|%s\.hip):\d+:\d+: (warning|error)" % lib, ln)]
    print(lib, len(hits), "warnings")
    assert not hits, "\n".join(hits[:10])


@pytest.mark.parametrize("lib,name", KERNELS)
def test_no_scratch_no_spill_lds_and_registers(metadata, lib, name):
    k = metadata[name]
    print(name, {key: k[key] for key in sorted(k) if key.endswith(("_count", "_size"))})
    assert int(k[".private_segment_fixed_size"]) == 0
    assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0
    assert int(k[".group_segment_fixed_size"]) == lds_bytes(lib, name)
    assert (int(k[".vgpr_count"]), int(k[".agpr_count"]), int(k[".sgpr_count"])) == REGISTERS[name]
