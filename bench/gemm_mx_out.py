"""What the MX GEMMs' output modes cost and save, one GPU, one process, one run.

Per operand format (MXFP8, MXFP4), at N×N×N with the 256x256pbx tile:

* ``plain``: the fp32 C in fragment order, tile-major (what the kernel has
  always stored);
* ``out_bfloat16`` / ``out_mxfp8`` / ``out_mxfp4``: the same loop with the
  row-major output of kernels/sgemm_mx_out.hip; a step is ``run()``, which
  for the MX outputs includes the pack compute of the scales;
* ``chain_mxfp8`` / ``chain_mxfp4``: the unfused route an output mode
  replaces — the plain GEMM, then the device quantiser on a resident fp32
  row-major N×N array, then the pack.  The plain C is not row-major, so the
  quantiser reads an array of the same size in its place: this is what a
  row-major fp32 C would have to pay afterwards.

Timing as bench/gemm_fp8.py's ``measure``: untimed computes until the clocks
are up, W warm-up steps, then K steps in enqueue mode on one queue between two
device syncs; the median of ROUNDS such rounds.  Every object gets the same
operands.  After its timing every output-mode run is checked against the host
codec of the plain kernel's C on sampled row panels (first, last and seeded
ones; rows are independent under blocks along N), bit for bit, and its packed
scales whole against ``pack_mx_scales`` of its row-major scales.  Prints one
JSON line; ``ratio_to_plain`` is a step's time over the plain kernel's of the
same run and format (below 1: faster).

    python bench/gemm_mx_out.py [--steps K] [--warmup W] [--size N]
"""
import argparse
import time

import numpy as np
from common import emit, sync
from gemm_fp8 import ROUNDS, SETTLE_COMPUTES

TILE = "256x256pbx"
PANEL_ROWS, PANELS = 64, 8
LIBS = ("sgemm_mxfp8", "sgemm_mxfp4", "mx_quantize", "mx4_quantize", "sgemm_mx_out")


def timed(cr, step, steps, warmup):
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
    return sorted(rounds)[len(rounds) // 2], rounds


def entry(g, ms, rounds):
    return {"ms": round(ms, 4), "tflops": round(g.flops / ms / 1e9, 1),
            "rounds_ms": [round(r, 4) for r in rounds]}


def host_codec_rows(c, out):
    from cekirdekler_amd.ops.gemm import to_bf16_bits
    from cekirdekler_amd.ops.quantize import mxfp4_reference, mxfp8_reference

    if out == "bfloat16":
        return to_bf16_bits(c).reshape(c.shape), None
    return (mxfp8_reference if out == "mxfp8" else mxfp4_reference)(c)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    a = ap.parse_args()
    import cekirdekler_amd as ck
    from cekirdekler_amd.ops.gemm import MX_OUTPUTS, GemmMxFp4, GemmMxFp8, pack_mx_scales
    from cekirdekler_amd.ops.library import library
    from cekirdekler_amd.ops.quantize import MxFp4Quantizer, MxFp8Quantizer

    gpus = ck.ClPlatforms.all().gpus()
    if len(gpus) == 0:
        raise SystemExit("gemm_mx_out: no GPU")
    gpu, N = gpus[0], a.size
    res = {"bench": "gemm_mx_out", "device": gpu.device(0).name, "shape": [N, N, N], "tile": TILE,
           "timing": "enqueue mode, one queue, median of %d rounds of %d steps" % (ROUNDS, a.steps),
           "check": "%d panels of %d rows against the host codec of the plain C, packed scales whole"
                    % (PANELS, PANEL_ROWS)}
    rng = np.random.default_rng(1)
    panels = sorted({0, N // PANEL_ROWS - 1, *rng.integers(0, N // PANEL_ROWS, PANELS - 2).tolist()})
    rows = np.concatenate([np.arange(p * PANEL_ROWS, (p + 1) * PANEL_ROWS) for p in panels])

    for fmt, cls in (("mxfp8", GemmMxFp8), ("mxfp4", GemmMxFp4)):
        cr = ck.ClNumberCruncher(gpu, "", prebuilt=library(*LIBS))
        seedling = cls(N, N, N, cruncher=cr, tile=TILE)  # the operands every object of this format gets
        operands = [x.array.copy() for x in (seedling.A, seedling.SA, seedling.B, seedling.SB)]

        def make(**kw):
            g = cls(N, N, N, cruncher=cr, tile=TILE, fill="none", **kw)
            for dst, src in zip((g.A, g.SA, g.B, g.SB), operands):
                dst.array[:] = src
            return g

        def drop(g):
            for x in (g.A, g.B, g.SA, g.SB, g._SAp, g._SBp, g.C, getattr(g, "Y", None), getattr(g, "SY", None),
                      getattr(g, "Yp", None)):
                if x is not None:
                    x.dispose()

        drop(seedling)
        out = res[fmt] = {}
        g = make()
        ms, rounds = timed(cr, lambda: g.run(compute_id=1), a.steps, a.warmup)
        out["plain"] = entry(g, ms, rounds)
        plain_ms = ms
        c = g.result()
        c_rows = c[rows]
        # the unfused route: plain GEMM, quantiser on a resident fp32 row-major array, pack
        x = ck.ClArray(np.ascontiguousarray(c.reshape(-1)))
        del c
        for qname, qcls in (("mxfp8", MxFp8Quantizer), ("mxfp4", MxFp4Quantizer)):
            q = qcls(N, N, "float32", cruncher=cr, x=x)
            q.run(compute_id=40, upload=True, download=False)  # X goes up once
            step = lambda: (g.run(compute_id=1), q.run(compute_id=40, upload=False, download=False))  # noqa: E731
            ms, rounds = timed(cr, step, a.steps, a.warmup)
            e = entry(g, ms, rounds)
            e["ratio_to_plain"] = round(ms / plain_ms, 3)
            out["chain_" + qname] = e
            for arr in (q.codes, q.scales, q.packed):
                arr.dispose()
        x.dispose()
        drop(g)
        for mode in MX_OUTPUTS:
            g = make(out=mode)
            ms, rounds = timed(cr, lambda: g.run(compute_id=1), a.steps, a.warmup)
            e = entry(g, ms, rounds)
            e["ratio_to_plain"] = round(ms / plain_ms, 3)
            arrays = [g.Y] + ([g.SY, g.Yp] if g.SY is not None else [])
            for arr in arrays:
                cr.download(arr, 0)
            want_y, want_s = host_codec_rows(c_rows, mode)
            y = g.Y.array.reshape(N, -1)[rows]
            if mode == "bfloat16":
                nan = (want_y & 0x7FFF) > 0x7F80
                ok = bool((((y & 0x7FFF) > 0x7F80) == nan).all() and (y[~nan] == want_y[~nan]).all())
            else:
                ok = bool(np.array_equal(y, want_y) and np.array_equal(g.SY.array.reshape(N, -1)[rows], want_s)
                          and np.array_equal(g.Yp.array, pack_mx_scales(g.SY.array.reshape(N, -1)).ravel()))
            if not ok:
                raise SystemExit(f"{fmt} out={mode}: the output differs from the host codec of the plain C")
            e["rows_checked"] = int(rows.size)
            out["out_" + mode] = e
            drop(g)
        cr.dispose()
    emit(res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
