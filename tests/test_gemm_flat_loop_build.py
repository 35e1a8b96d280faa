"""What the compiler made of the bf16 GEMM kernels (kernels/sgemm_bf16.hip):
the code object's metadata notes, read with the ROCm llvm-readelf.  A ping-pong
kernel holds 128 accumulator and 96 fragment registers per lane; a loop that
needs a few address registers too many spills to scratch, and a spill inside
the K loop costs far more than any loop shape saves.  So: no private segment,
no spilled VGPR and at most 256 VGPRs, for every kernel of the library — and
the reference tile of the flat loops, 256x256pb0, is there."""
import os
import re
import subprocess

import pytest

from cekirdekler_amd import build_native as bn
from cekirdekler_amd.ops import gemm
from cekirdekler_amd.ops.library import LIBRARY, code_object

LLVM_BIN = os.path.join(bn.ROCM, "llvm", "bin")
KEYS = (".name", ".private_segment_fixed_size", ".vgpr_count", ".vgpr_spill_count")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> {key: value} of every kernel in sgemm_bf16.hsaco's gfx950 ELF."""
    elf = str(tmp_path_factory.mktemp("bf16") / "sgemm_bf16.elf")
    subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--type=o", "--unbundle",
                    f"--targets=hipv4-amdgcn-amd-amdhsa--{bn.ARCH}", f"--input={code_object('sgemm_bf16')}",
                    f"--output={elf}"], check=True)
    notes = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", elf], check=True,
                           stdout=subprocess.PIPE, text=True).stdout
    out = {}
    # one entry of amdhsa.kernels per "  - " at list depth; its scalar keys sit at four spaces
    for entry in re.split(r"^  - ", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^(?:    )?(\.\w+): +(\S+)$", entry, flags=re.M))
        if ".vgpr_count" in kv:
            out[kv[".name"]] = {k: kv[k] for k in KEYS}
    return out


def test_reference_tile_is_the_production_tile_under_another_kernel():
    """256x256pb0 stands beside TILES, not in it, and differs from 256x256pb
    in the kernel name alone."""
    assert "256x256pb0" not in gemm.TILES and "256x256pb0" not in gemm.TILE_WAVES
    assert gemm.REFERENCE_TILES["256x256pb0"][:3] == gemm.TILES["256x256pb"][:3]
    assert gemm.REFERENCE_TILES["256x256pb0"][3] == "cek_sgemm_bf16_256x256pb0" in LIBRARY["sgemm_bf16"]
    assert gemm.REFERENCE_TILE_WAVES["256x256pb0"] == gemm.TILE_WAVES["256x256pb"]


def test_every_library_kernel_is_described(kernels):
    assert sorted(kernels) == sorted(LIBRARY["sgemm_bf16"])
    assert "cek_sgemm_bf16_256x256pb0" in kernels


@pytest.mark.parametrize("name", LIBRARY["sgemm_bf16"])
def test_no_scratch_no_spill_at_most_256_vgprs(kernels, name):
    k = kernels[name]
    print(name, k)
    assert int(k[".private_segment_fixed_size"]) == 0
    assert int(k[".vgpr_spill_count"]) == 0
    assert int(k[".vgpr_count"]) <= 256
