"""Two MX layers with a ReLU between them, without a host round trip.

    X (fp32, on the device) → MXFP4 → layer 1 (MXFP4 GEMM, ReLU, MXFP8 output)
                                     → layer 2 (MXFP8 GEMM) → C (fp32)

Layer 1 runs with ``out="mxfp8", act="relu"``: its kernel stores the next
layer's operand — row-major e4m3fn codes with E8M0 scales along N — instead of
the fp32 C, and ``take_operand`` makes those resident arrays layer 2's A.  After
the first call only the ``dims`` words cross PCIe.

    python examples/mx_two_layers.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cekirdekler_amd as ck  # noqa: E402
from cekirdekler_amd.ops.gemm import GemmMxFp4, GemmMxFp8  # noqa: E402
from cekirdekler_amd.ops.library import library  # noqa: E402

gpus = ck.ClPlatforms.all().gpus()
if len(gpus) == 0:
    raise SystemExit("mx_two_layers: no GPU")
cr = ck.ClNumberCruncher(gpus[0], "", prebuilt=library("sgemm_mxfp4", "mx4_quantize", "mx_quantize", "sgemm_mx_out",
                                                      "sgemm_mxfp8"))
batch, d_in, d_hidden, d_out = 1024, 1024, 2048, 512

# B of each layer: random weights, W1 [d_hidden][d_in] and W2 [d_out][d_hidden]
layer1 = GemmMxFp4(batch, d_hidden, d_in, cruncher=cr, out="mxfp8", act="relu")
layer2 = GemmMxFp8(batch, d_out, d_hidden, cruncher=cr, seed=1)
layer2.take_operand("A", layer1)

x = ck.ClArray(np.random.default_rng(2).standard_normal(batch * d_in).astype(np.float32))
for step in range(3):
    layer1.quantize_operand("A", x)  # fp32 → MXFP4 on the device (uploads x while x.read is set)
    x.read = False                   # resident from now on
    layer1.run(compute_id=1)
    h2d = [r["h2d_bytes"] for r in layer1.records]
    layer2.run(compute_id=2)  # its own balancer state
    print(f"step {step}: layer 1 uploaded {sum(h2d)} B, layer 2 {cr.last_record()['h2d_bytes']} B")

c = layer2.result()
print("C", c.shape, c.dtype, "| hidden activations:", layer1.out, layer1.Y.N, "bytes +", layer1.SY.N, "scale bytes")
# each layer against the float64 product of the operands it multiplied (layer
# 1's figure includes the e4m3 rounding of its output)
print(f"layer 1 max rel err {layer1.verify():.3e}, layer 2 max rel err {layer2.verify(compute_id=2):.3e}")
cr.dispose()
