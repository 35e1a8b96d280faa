"""Device-side MXFP4 quantisation (kernels/mx4_quantize.hip) on one GPU, one process.

Kernel rates: N×N fp32 and bf16 inputs resident in device memory, outputs left
there, timed as bench/quantize_mxfp8.py times its kernels (the launches' start
/ stop stamps, the median over ROUNDS rounds of K computes after SETTLE
untimed ones).  Bytes moved per element: fp32 4 + 1/2 + 1/32, bf16 2 + 1/2 +
1/32.  ``cek_copy_u8`` moves the fp32 quantiser's byte count (half read, half
written) in the same process and is the yardstick: ``fraction_of_copy`` is a
kernel's bytes/s over the copy kernel's.  The quantised outputs of both
sources are compared with the host codec on the first 64 rows, the packed
scales on everything.  (The pack pass is the MXFP8 one; quantize_mxfp8.py
times it.)

End to end, N×N×N: ``quantize_operand("A") + quantize_operand("B") + run()``
from fp32 numpy arrays (upload included) and from fp32 ClArrays already
resident, against the host route ``to_mxfp4`` twice + upload + ``run()``; wall
clock around a device sync, C compared bit for bit between the routes.

    python bench/quantize_mxfp4.py [--steps K] [--warmup W] [--size N] [--no-e2e]
"""
import argparse
import statistics
import time

import numpy as np
from common import emit, sync
from quantize_mxfp8 import ROUNDS, kernel_ms, rate


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import GemmMxFp4, pack_mx_scales, to_bf16_bits, to_mxfp4
    from cekirdekler_amd.ops.library import library
    from cekirdekler_amd.ops.quantize import MxFp4Quantizer, mxfp4_reference

    gpus = ck.ClPlatforms.all().gpus()
    if len(gpus) == 0:
        raise SystemExit("quantize_mxfp4: no GPU")
    gpu = gpus[0]
    N = a.size
    n = N * N
    cr = ck.ClNumberCruncher(gpu, "", prebuilt=library("sgemm_mxfp4", "mx4_quantize", "mx_quantize", "stream"))
    res = {"bench": "quantize_mxfp4", "device": gpu.device(0).name, "shape": [N, N],
           "timing": f"kernel start/stop stamps, median of {ROUNDS} rounds of {a.steps} launches in enqueue mode"}

    rng = np.random.default_rng(0)
    x = np.ldexp(rng.uniform(-1, 1, (N, N // 32, 32)), rng.integers(-12, 13, (N, N // 32, 1)))
    x = x.astype(np.float32).reshape(N, N)
    head = 64  # rows checked against the host codec (the GPU tests check every case)

    # ---- the copy yardstick: the fp32 quantiser's bytes, half read, half written
    q_bytes = {"float32": n * 4 + n // 2 + n // 32, "bfloat16": n * 2 + n // 2 + n // 32}
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

    # ---- the quantise kernels
    quantizers = {}
    for name in ("float32", "bfloat16"):
        q = MxFp4Quantizer(N, N, src=name, cruncher=cr)
        quantizers[name] = q
        q.X.array[:] = (x if name == "float32" else to_bf16_bits(x)).ravel()
        q.run(compute_id=30, upload=True, download=True)
        codes, scales = mxfp4_reference(q.X.array[:head * N].reshape(head, N))
        if not (np.array_equal(q.codes.array[:head * N // 2], codes.ravel())
                and np.array_equal(q.scales.array[:head * N // 32], scales.ravel())
                and np.array_equal(q.packed.array, pack_mx_scales(q.scales.array.reshape(N, N // 32)).ravel())):
            raise SystemExit(f"quantize {name}: output differs from the host codec")
        t = kernel_ms(cr, lambda: q.run(compute_id=30, upload=False, download=False, pack=False), a.steps, a.warmup)
        r = rate(q_bytes[name], *t)
        r["fraction_of_copy"] = round(q_bytes[name] / t[0] / copy_rate, 3)
        r["gelem_per_s"] = round(n / t[0] / 1e6, 1)
        res["quantize_" + name] = r
    for q in quantizers.values():
        for arr in (q.X, q.codes, q.scales, q.packed):
            arr.dispose()
    src.dispose()
    dst.dispose()

    # ---- end to end: fp32 operands -> C
    if not a.no_e2e:
        b = np.ascontiguousarray(x[::-1])
        g1 = GemmMxFp4(N, N, N, cruncher=cr, fill="none")

        def device_route(xa, xb):
            sync()
            t0 = time.perf_counter()
            g1.quantize_operand("A", xa)
            g1.quantize_operand("B", xb)
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

        g2 = GemmMxFp4(N, N, N, cruncher=cr, fill="none")
        g2.run()  # buffers and code objects; the timed call uploads again
        sync()
        t0 = time.perf_counter()
        (ca, sa), (cb, sb) = to_mxfp4(x), to_mxfp4(b)
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
            "host_route_ms": round(t_host, 1), "host_route_to_mxfp4_ms": round(t_codec, 1),
            "c_bit_identical": True,
            "speedup_from_host_fp32": round(t_host / statistics.median(up), 1),
            "speedup_resident_fp32": round(t_host / statistics.median(rs), 1)}
    emit(res)
    cr.dispose()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
