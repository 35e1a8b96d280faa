"""MXFP4 GEMM tiles beside the MXFP8 production tile, one GPU, one process.

Set-up and timing are bench/gemm_fp8.py's (its ``measure``: the balancer run
to its split, untimed computes until the clocks are up, W warm-up computes,
then K computes in enqueue mode on one queue between two device syncs; the
median of ROUNDS such rounds).  Order: GemmMxFp8 256x256pbx at N³ (N = 8192),
every MXFP4 tile at N³, then MXFP4 256x256pbx at N×N×2N.  That last shape has
the operand bytes, the K-tiles and the matrix-core cycles of MXFP8 at N³, so
its time per step over MXFP8's is the direct test of "the loop takes the same
time for twice the FLOPs".  The operands are the classes' default data (block
factors 2^-12 .. 2^12).  Every run's whole output is checked against a
float64 product of the dequantised operands (``verify_full``) and must cover
every tile.  Prints one JSON line with

    ratio_to_mxfp8             MXFP4 256x256pbx TFLOP/s at N³ over MXFP8's
    ms_ratio_k2_to_mxfp8       ms(MXFP4 at K = 2N) over ms(MXFP8 at K = N)

both against the MXFP8 kernel of the same run.

    python bench/gemm_mxfp4.py [--steps K] [--warmup W] [--size N]
"""
import argparse
import sys

from common import emit
from gemm_fp8 import ROUNDS, measure


def _progress(r) -> None:
    """One line per finished measurement on stderr: the host-side MXFP4
    quantisation of 8192 × 16384 operands alone takes a while."""
    print("%s %s: %.4f ms, %.1f TFLOP/s" % (r["tile"], r["shape"], r["ms"], r["tflops"]), file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import MXFP4_TILES, GemmMxFp4, GemmMxFp8

    gpu = ck.ClPlatforms.all().gpus()[0]
    s = a.size
    res = {"bench": "gemm_mxfp4", "device": gpu.device(0).name,
           "timing": "enqueue mode, one queue (one GEMM in flight), median of %d rounds of %d" % (ROUNDS, a.steps)}
    base = measure(GemmMxFp8, "256x256pbx", s, s, s, gpu, ("sgemm_mxfp8", "mx_quantize"), a.steps, a.warmup)
    res["mxfp8_256x256pbx"] = base
    _progress(base)
    res["mxfp4"] = {}
    for tile in MXFP4_TILES:
        r = measure(GemmMxFp4, tile, s, s, s, gpu, ("sgemm_mxfp4",), a.steps, a.warmup)
        r["ratio_to_mxfp8"] = round(r["tflops"] / base["tflops"], 3)
        res["mxfp4"][tile] = r
        _progress(r)
    k2 = measure(GemmMxFp4, "256x256pbx", s, s, 2 * s, gpu, ("sgemm_mxfp4",), a.steps, a.warmup)
    k2["ms_ratio_to_mxfp8"] = round(k2["ms"] / base["ms"], 3)
    res["mxfp4_k2_256x256pbx"] = k2
    _progress(k2)
    res["ratio_to_mxfp8"] = res["mxfp4"]["256x256pbx"]["ratio_to_mxfp8"]
    res["ms_ratio_k2_to_mxfp8"] = k2["ms_ratio_to_mxfp8"]
    res["tiles_checked"] = sum(r["tiles_checked"] for r in (base, k2, *res["mxfp4"].values()))
    res["tiles_total"] = sum(r["tiles"] for r in (base, k2, *res["mxfp4"].values()))
    emit(res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
