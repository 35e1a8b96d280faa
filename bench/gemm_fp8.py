"""fp8 e4m3 GEMM tiles beside the bf16 production tile, one GPU, one process.

Set-up and timing as bench.py times its headline: the balancer run to its
split, untimed computes until the clocks are up, W warm-up computes, then K
computes in enqueue mode on one queue (one GEMM in flight) between two device
syncs; the median of ROUNDS such rounds.  Order: GemmBf16 256x256pb at 8192³,
every fp8 tile at 8192³, every fp8 tile at 1024×8192×8192.  Every run's whole
output is checked against a float64 product (``verify_full``) and must cover
every tile.  Prints one JSON line; ``ratio_to_bf16`` is the fp8 tile's
throughput over the bf16 kernel's of the same run (8192³).

    python bench/gemm_fp8.py [--steps K] [--warmup W] [--size N]
"""
import argparse
import time

from common import emit, sync

SETTLE_COMPUTES = 100
ROUNDS = 5


def measure(cls, tile, m, n, k, gpu, libs, steps, warmup):
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.library import library

    cr = ck.ClNumberCruncher(gpu, "", prebuilt=library(*libs))
    g = cls(m, n, k, cruncher=cr, tile=tile)
    step = lambda: g.run(compute_id=1, resident=True)  # noqa: E731
    sync()
    for _ in range(SETTLE_COMPUTES + warmup):
        step()
    rounds = []
    for _ in range(ROUNDS):
        sync()
        t0 = time.perf_counter()
        cr.enqueue_mode = True
        for _ in range(steps):
            step()
        cr.enqueue_mode = False
        sync()
        rounds.append((time.perf_counter() - t0) * 1e3 / steps)
    ms = sorted(rounds)[len(rounds) // 2]
    err, checked = g.verify_full(compute_id=1)
    if checked != g.tiles:
        raise SystemExit(f"{cls.__name__} {tile} {m}x{n}x{k}: verify_full checked {checked} of {g.tiles} tiles")
    out = {"tile": tile, "shape": [m, n, k], "ms": round(ms, 4), "tflops": round(g.flops / ms / 1e9, 1),
           "rounds_tflops": [round(g.flops / r / 1e9, 1) for r in rounds], "max_rel_err": err,
           "tiles_checked": checked, "tiles": g.tiles}
    cr.dispose()
    for a in (g.A, g.B, g.C, g.dims):
        a.dispose()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import FP8_TILES, GemmBf16, GemmFp8

    gpu = ck.ClPlatforms.all().gpus()[0]
    s = a.size
    res = {"bench": "gemm_fp8", "device": gpu.device(0).name,
           "timing": "enqueue mode, one queue (one GEMM in flight), median of %d rounds of %d" % (ROUNDS, a.steps)}
    res["bf16_256x256pb"] = measure(GemmBf16, "256x256pb", s, s, s, gpu, ("sgemm_bf16",), a.steps, a.warmup)
    base = res["bf16_256x256pb"]["tflops"]
    res["fp8"], res["fp8_1024_rows"] = {}, {}
    for tile in FP8_TILES:
        r = measure(GemmFp8, tile, s, s, s, gpu, ("sgemm_fp8",), a.steps, a.warmup)
        r["ratio_to_bf16"] = round(r["tflops"] / base, 3)
        res["fp8"][tile] = r
    for tile in FP8_TILES:
        res["fp8_1024_rows"][tile] = measure(GemmFp8, tile, 1024, s, s, gpu, ("sgemm_fp8",), a.steps, a.warmup)
    res["fastest_fp8_tile"] = max(res["fp8"], key=lambda t: res["fp8"][t]["tflops"])
    emit(res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
