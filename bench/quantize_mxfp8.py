"""Device-side MXFP8 quantisation (kernels/mx_quantize.hip) on one GPU, one process.

Kernel rates: N×N fp32 and bf16 inputs resident in device memory, outputs left
there.  Each kernel's own execution time comes from the launches' start / stop
stamps (``record_kernel_times``): after SETTLE untimed computes, ROUNDS rounds
of K computes each, the median over all timed launches.  Bytes moved per
element: fp32 4 + 1 + 1/32, bf16 2 + 1 + 1/32; the pack pass reads and writes
the scales once (2 · N²/32 bytes).  ``cek_copy_u8`` moves the fp32 quantiser's
byte count (half read, half written) in the same process and is the
yardstick: ``fraction_of_copy`` is a kernel's bytes/s over the copy kernel's.
The quantised outputs of both sources are compared with the host codec on the
first 64 rows, the pack pass on everything.

End to end, N×N×N: ``quantize("A") + quantize("B") + run()`` from fp32 numpy
arrays (upload included) and from fp32 ClArrays already resident, against the
host route ``to_mxfp8`` twice + upload + ``run()``; wall clock around a device
sync, C compared bit for bit between the routes.

    python bench/quantize_mxfp8.py [--steps K] [--warmup W] [--size N] [--no-e2e]
"""
import argparse
import statistics
import time

import numpy as np
from common import emit, sync

SETTLE = 60
ROUNDS = 5


def kernel_ms(cr, step, steps, warmup):
    """Median execution time (ms) of the kernel launches ``step`` makes."""
    for _ in range(SETTLE + warmup):
        step()
    sync()
    cr.record_kernel_times = True
    cr.kernel_times(0)
    times, walls = [], []
    for _ in range(ROUNDS):
        sync()
        t0 = time.perf_counter()
        cr.enqueue_mode = True
        for _ in range(steps):
            step()
        cr.enqueue_mode = False
        sync()
        walls.append((time.perf_counter() - t0) * 1e3 / steps)
        times += [ms for _, ms in cr.kernel_times(0)]
    cr.record_kernel_times = False
    if len(times) != ROUNDS * steps:
        raise SystemExit(f"expected {ROUNDS * steps} kernel times, got {len(times)}")
    return statistics.median(times), min(times), statistics.median(walls)


def rate(nbytes, ms, best, wall):
    return {"bytes": int(nbytes), "kernel_ms": round(ms, 5), "tb_per_s": round(nbytes / ms / 1e9, 3),
            "best_tb_per_s": round(nbytes / best / 1e9, 3), "wall_ms_per_call": round(wall, 5)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import GemmMxFp8, pack_mx_scales, to_bf16_bits, to_mxfp8
    from cekirdekler_amd.ops.library import library
    from cekirdekler_amd.ops.quantize import MxFp8Quantizer, mxfp8_reference

    gpus = ck.ClPlatforms.all().gpus()
    if len(gpus) == 0:
        raise SystemExit("quantize_mxfp8: no GPU")
    gpu = gpus[0]
    N = a.size
    n = N * N
    cr = ck.ClNumberCruncher(gpu, "", prebuilt=library("sgemm_mxfp8", "mx_quantize", "stream"))
    res = {"bench": "quantize_mxfp8", "device": gpu.device(0).name, "shape": [N, N],
           "timing": f"kernel start/stop stamps, median of {ROUNDS} rounds of {a.steps} launches in enqueue mode"}

    rng = np.random.default_rng(0)
    x = np.ldexp(rng.uniform(-1, 1, (N, N // 32, 32)), rng.integers(-12, 13, (N, N // 32, 1)))
    x = x.astype(np.float32).reshape(N, N)
    head = 64  # rows checked against the host codec (the GPU tests check every case)

    # ---- the copy yardstick: the fp32 quantiser's bytes, half read, half written
    q_bytes = {"float32": n * 4 + n + n // 32, "bfloat16": n * 2 + n + n // 32}
    half = q_bytes["float32"] // 2 // (16 * 64) * (16 * 64)
    src = ck.ClArray(np.arange(half, dtype=np.uint8))
    dst = ck.ClArray(np.zeros(half, np.uint8))
    src.elements_per_work_item = dst.elements_per_work_item = 16
    src.write = dst.read = False
    src.next_param(dst).compute(cr, 20, "cek_copy_u8", half // 16, 64)
    src.read = dst.write = False
    copy = kernel_ms(cr, lambda: src.next_param(dst).compute(cr, 20, "cek_copy_u8", half // 16, 64), a.steps, a.warmup)
    cr.download(dst, 0)
    if not np.array_equal(dst.array, src.array):
        raise SystemExit("copy kernel: wrong output")
    res["copy_u8"] = rate(2 * half, *copy)
    copy_rate = 2 * half / copy[0]

    # ---- the quantise kernels and the pack pass
    quantizers = {}
    for name in ("float32", "bfloat16"):
        q = MxFp8Quantizer(N, N, src=name, cruncher=cr)
        quantizers[name] = q
        q.X.array[:] = (x if name == "float32" else to_bf16_bits(x)).ravel()
        q.run(compute_id=30, upload=True, download=True)
        codes, scales = mxfp8_reference(q.X.array[:head * N].reshape(head, N))
        if not (np.array_equal(q.codes.array[:head * N], codes.ravel())
                and np.array_equal(q.scales.array[:head * N // 32], scales.ravel())
                and np.array_equal(q.packed.array, pack_mx_scales(q.scales.array.reshape(N, N // 32)).ravel())):
            raise SystemExit(f"quantize {name}: output differs from the host codec")
        t = kernel_ms(cr, lambda: q.run(compute_id=30, upload=False, download=False, pack=False), a.steps, a.warmup)
        r = rate(q_bytes[name], *t)
        r["fraction_of_copy"] = round(q_bytes[name] / t[0] / copy_rate, 3)
        r["gelem_per_s"] = round(n / t[0] / 1e6, 1)
        res["quantize_" + name] = r
    q = quantizers["float32"]
    for arr in (q.dims, q.scales, q.packed):
        arr.read = arr.write = False
    q.packed.elements_per_work_item = 1
    pack = kernel_ms(cr, lambda: q.dims.next_param(q.scales, q.packed).compute(cr, 31, "cek_mx_pack_scales",
                                                                                q.packed.N, 64), a.steps, a.warmup)
    res["pack_scales"] = rate(2 * (n // 32), *pack)
    res["pack_scales"]["fraction_of_copy"] = round(2 * (n // 32) / pack[0] / copy_rate, 3)
    res["pack_ms_over_quantize_f32_ms"] = round(pack[0] / res["quantize_float32"]["kernel_ms"], 3)
    for q in quantizers.values():
        for arr in (q.X, q.codes, q.scales, q.packed):
            arr.dispose()
    src.dispose()
    dst.dispose()

    # ---- end to end: fp32 operands -> C
    if not a.no_e2e:
        b = np.ascontiguousarray(x[::-1])
        g1 = GemmMxFp8(N, N, N, cruncher=cr, fill="none")

        def device_route(xa, xb):
            sync()
            t0 = time.perf_counter()
            g1.quantize("A", xa)
            g1.quantize("B", xb)
            g1.run()
            sync()
            return (time.perf_counter() - t0) * 1e3

        device_route(x, b)  # buffers, pinning, code objects
        up = [device_route(x, b) for _ in range(5)]
        xa, xb = ck.ClArray(x.reshape(-1)), ck.ClArray(b.reshape(-1))
        device_route(xa, xb)  # uploads them
        xa.read = xb.read = False
        rs = [device_route(xa, xb) for _ in range(20)]
        c1 = g1.result()

        g2 = GemmMxFp8(N, N, N, cruncher=cr, fill="none")
        g2.run()  # buffers and code objects; the timed call uploads again
        sync()
        t0 = time.perf_counter()
        (ca, sa), (cb, sb) = to_mxfp8(x), to_mxfp8(b)
        t_codec = (time.perf_counter() - t0) * 1e3
        g2.A.array[:], g2.SA.array[:], g2.B.array[:], g2.SB.array[:] = ca.ravel(), sa.ravel(), cb.ravel(), sb.ravel()
        g2._uploaded = False  # as a first call: operands and packed scales go up
        g2.run()
        sync()
        t_host = (time.perf_counter() - t0) * 1e3
        c2 = g2.result()
        if not np.array_equal(c1.view(np.uint32), c2.view(np.uint32)):
            raise SystemExit("end to end: C of the device route differs from the host route's")
        res["end_to_end"] = {
            "shape": [N, N, N],
            "device_route_from_host_fp32_ms": round(statistics.median(up), 3),
            "device_route_resident_fp32_ms": round(statistics.median(rs), 3),
            "host_route_ms": round(t_host, 1), "host_route_to_mxfp8_ms": round(t_codec, 1),
            "c_bit_identical": True,
            "speedup_from_host_fp32": round(t_host / statistics.median(up), 1),
            "speedup_resident_fp32": round(t_host / statistics.median(rs), 1)}
    emit(res)
    cr.dispose()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
