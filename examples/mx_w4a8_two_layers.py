"""Two W4A8 layers with a ReLU between them: MXFP8 activations against MXFP4
weights, without a host round trip.

    X (fp32, on the device) → MXFP8 ─┐
    W1 (fp32) → MXFP4, once ─────────┴→ layer 1 (mixed GEMM, ReLU, MXFP8 output)
    W2 (fp32) → MXFP4, once ──────────→ layer 2 (mixed GEMM) → C (fp32)

The weights are quantised once with ``quantize("B")`` and stay resident at
half a byte per element; the activations go through ``quantize("A")`` every
step.  Layer 1 runs with ``out="mxfp8", act="relu"``: its kernel stores the
next layer's A operand, and ``take_operand("A", layer1)`` makes those resident
arrays layer 2's A.  The result is checked against the host model: the host
codecs of the same fp32 inputs, the float64 product, ReLU and the host MXFP8
codec between the layers.

    python examples/mx_w4a8_two_layers.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cekirdekler_amd as ck  # noqa: E402
from cekirdekler_amd.ops.gemm import GemmMxFp8Fp4, from_mxfp4, from_mxfp8, to_mxfp4, to_mxfp8  # noqa: E402
from cekirdekler_amd.ops.library import library  # noqa: E402

gpus = ck.ClPlatforms.all().gpus()
if len(gpus) == 0:
    raise SystemExit("mx_w4a8_two_layers: no GPU")
cr = ck.ClNumberCruncher(gpus[0], "", prebuilt=library("sgemm_mxf8f4", "sgemm_mxf8f4_out", "mx_quantize",
                                                      "mx4_quantize"))
batch, d_in, d_hidden, d_out = 512, 1024, 1024, 512
rng = np.random.default_rng(2)
x = rng.standard_normal((batch, d_in)).astype(np.float32)
w1 = (rng.standard_normal((d_hidden, d_in)) / np.sqrt(d_in)).astype(np.float32)
w2 = (rng.standard_normal((d_out, d_hidden)) / np.sqrt(d_hidden)).astype(np.float32)

layer1 = GemmMxFp8Fp4(batch, d_hidden, d_in, cruncher=cr, fill="none", out="mxfp8", act="relu")
layer2 = GemmMxFp8Fp4(batch, d_out, d_hidden, cruncher=cr, fill="none")
layer1.quantize("B", w1)  # fp32 → MXFP4 on the device, once
layer2.quantize("B", w2)
layer2.take_operand("A", layer1)

xd = ck.ClArray(x.ravel().copy())
for step in range(3):
    layer1.quantize("A", xd)  # fp32 → MXFP8 on the device (uploads x while xd.read is set)
    xd.read = False           # resident from now on
    layer1.run(compute_id=1)
    h2d = [r["h2d_bytes"] for r in layer1.records]
    layer2.run(compute_id=2)  # its own balancer state
    print(f"step {step}: layer 1 uploaded {sum(h2d)} B, layer 2 {cr.last_record()['h2d_bytes']} B")
c = layer2.result()

# the host model of the same two layers
a1 = from_mxfp8(*to_mxfp8(x)).astype(np.float64)
h = a1 @ from_mxfp4(*to_mxfp4(w1)).astype(np.float64).T
h = np.where(h > 0, h, 0.0).astype(np.float32)
a2 = from_mxfp8(*to_mxfp8(h)).astype(np.float64)
ref = a2 @ from_mxfp4(*to_mxfp4(w2)).astype(np.float64).T
err = float(np.abs(c - ref).max() / np.abs(ref).max())
print("C", c.shape, c.dtype, "| weights:", layer1.B.nbytes + layer2.B.nbytes, "bytes of e2m1 |",
      f"max |C - host model| / max |host model| = {err:.3e}")
# the hidden activations are rounded to e4m3 from fp32 sums that differ from the float64 ones in their last
# bits, so a few codes may fall to the other side of a rounding boundary: 2^-4 of a block's largest value each
if not err < 2e-2:
    raise SystemExit(f"mx_w4a8_two_layers: result differs from the host model ({err:.3e})")
print(f"layer 2 against the operands it multiplied: max rel err {layer2.verify(compute_id=2):.3e}")
cr.dispose()
