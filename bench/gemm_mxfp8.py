"""MXFP8 GEMM tiles beside the unit-scale fp8 production tile, one GPU, one process.

Set-up and timing are bench/gemm_fp8.py's (its ``measure``: the balancer run
to its split, untimed computes until the clocks are up, W warm-up computes,
then K computes in enqueue mode on one queue between two device syncs; the
median of ROUNDS such rounds).  Order: GemmFp8 256x256pbx (every scale 1) at
8192³, every MXFP8 tile at 8192³, then the same at 1024×8192×8192.  The MXFP8
operands are the class's default data (block factors 2^-12 .. 2^12).  Every
run's whole output is checked against a float64 product of the dequantised
operands (``verify_full``) and must cover every tile.  Prints one JSON line;
``ratio_to_unit_scale`` is the MXFP8 tile's throughput over the unit-scale
kernel's of the same run and shape.

    python bench/gemm_mxfp8.py [--steps K] [--warmup W] [--size N]
"""
import argparse

from common import emit
from gemm_fp8 import ROUNDS, measure


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import MXFP8_TILES, GemmFp8, GemmMxFp8

    gpu = ck.ClPlatforms.all().gpus()[0]
    s = a.size
    res = {"bench": "gemm_mxfp8", "device": gpu.device(0).name,
           "timing": "enqueue mode, one queue (one GEMM in flight), median of %d rounds of %d" % (ROUNDS, a.steps)}
    for key, m in (("", s), ("_1024_rows", 1024)):
        unit = measure(GemmFp8, "256x256pbx", m, s, s, gpu, ("sgemm_fp8",), a.steps, a.warmup)
        res["fp8_unit_scale_256x256pbx" + key] = unit
        res["mxfp8" + key] = {}
        for tile in MXFP8_TILES:
            r = measure(GemmMxFp8, tile, m, s, s, gpu, ("sgemm_mxfp8",), a.steps, a.warmup)
            r["ratio_to_unit_scale"] = round(r["tflops"] / unit["tflops"], 3)
            res["mxfp8" + key][tile] = r
    res["ratio_to_unit_scale"] = res["mxfp8"]["256x256pbx"]["ratio_to_unit_scale"]
    emit(res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
