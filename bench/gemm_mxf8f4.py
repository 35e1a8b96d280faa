"""Mixed MXFP8 × MXFP4 GEMM tiles (8-bit A, 4-bit B) beside the MXFP8 and
MXFP4 production tiles, one GPU, one process.

Set-up and timing are bench/gemm_fp8.py's (its ``measure``: the balancer run
to its split, untimed computes until the clocks are up, W warm-up computes,
then K computes in enqueue mode on one queue between two device syncs; the
median of ROUNDS such rounds).  Order: GemmMxFp8 256x256pbx, GemmMxFp4
256x256pbx, then both mixed tiles, all at N³ (N = 8192).  The mixed
128x256pbx loop has, per K-tile, the staging bytes, fragment reads, matrix
instructions and FLOPs of the MXFP8 256x256pbx loop, so at equal M, N and K it
is expected to take that kernel's time per step; the MXFP8 baseline is measured
a second time at the end, and the difference between its two runs is the
run-to-run spread the ratio is read against.  The operands are the classes'
default data (block factors 2^-12 .. 2^12).  Every run's whole output is
checked against a float64 product of the dequantised operands
(``verify_full``) and must cover every tile.  Prints one JSON line with

    ms_ratio_to_mxfp8          ms(mixed 128x256pbx) over ms(MXFP8 256x256pbx)
    mxfp8_spread               ms(MXFP8, second run) over ms(MXFP8, first run)

both from the same run.

    python bench/gemm_mxf8f4.py [--steps K] [--warmup W] [--size N]
"""
import argparse
import sys

from common import emit
from gemm_fp8 import ROUNDS, measure


def _progress(r) -> None:
    """One line per finished measurement on stderr: the host-side quantisation
    of 8192² operands alone takes a while."""
    print("%s %s: %.4f ms, %.1f TFLOP/s" % (r["tile"], r["shape"], r["ms"], r["tflops"]), file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import MXF8F4_TILES, GemmMxFp4, GemmMxFp8, GemmMxFp8Fp4

    gpu = ck.ClPlatforms.all().gpus()[0]
    s = a.size
    res = {"bench": "gemm_mxf8f4", "device": gpu.device(0).name,
           "timing": "enqueue mode, one queue (one GEMM in flight), median of %d rounds of %d" % (ROUNDS, a.steps)}
    base = measure(GemmMxFp8, "256x256pbx", s, s, s, gpu, ("sgemm_mxfp8", "mx_quantize"), a.steps, a.warmup)
    res["mxfp8_256x256pbx"] = base
    _progress(base)
    f4 = measure(GemmMxFp4, "256x256pbx", s, s, s, gpu, ("sgemm_mxfp4",), a.steps, a.warmup)
    f4["ms_ratio_to_mxfp8"] = round(f4["ms"] / base["ms"], 3)
    res["mxfp4_256x256pbx"] = f4
    _progress(f4)
    res["mxf8f4"] = {}
    for tile in MXF8F4_TILES:
        r = measure(GemmMxFp8Fp4, tile, s, s, s, gpu, ("sgemm_mxf8f4",), a.steps, a.warmup)
        r["ms_ratio_to_mxfp8"] = round(r["ms"] / base["ms"], 3)
        res["mxf8f4"][tile] = r
        _progress(r)
    again = measure(GemmMxFp8, "256x256pbx", s, s, s, gpu, ("sgemm_mxfp8", "mx_quantize"), a.steps, a.warmup)
    res["mxfp8_256x256pbx_again"] = again
    _progress(again)
    res["ms_ratio_to_mxfp8"] = res["mxf8f4"]["128x256pbx"]["ms_ratio_to_mxfp8"]
    res["mxfp8_spread"] = round(again["ms"] / base["ms"], 3)
    runs = (base, f4, again, *res["mxf8f4"].values())
    res["tiles_checked"] = sum(r["tiles_checked"] for r in runs)
    res["tiles_total"] = sum(r["tiles"] for r in runs)
    emit(res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
