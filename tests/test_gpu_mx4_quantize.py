"""GPU tier of the device-side MXFP4 quantiser (kernels/mx4_quantize.hip,
ops/quantize.py, GemmMxFp4.quantize_operand): every equality is exact.  The
smallest launch, every rounding case of the designed patterns, the packed
scales with 0xFF bytes, two and three logical devices with every replica
whole, then the GEMM fed from the device against the GEMM fed by the host
codec, mixed feeding and the stale-operand guards, a NaN block, and a bf16
source."""
import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import (GemmMxFp4, from_bf16_bits, from_mxfp4, pack_mx_scales, to_bf16_bits,
                                      to_mxfp4)
from cekirdekler_amd.ops.library import library
from cekirdekler_amd.ops.quantize import MxFp4Quantizer, mxfp4_reference
from test_mx4_quantize_host import designed_reference4
from test_mx_quantize_host import first_mismatches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "",
                            prebuilt=library("sgemm_mxfp4", "mx4_quantize", "mx_quantize"))
    yield c
    c.dispose()


def _wide(rows, K, seed, spread=12):
    """Seeded uniform [-1, 1) values times 2^u per block of 32, u in [-spread, spread]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, K // 32, 32))
    return np.ldexp(x, rng.integers(-spread, spread + 1, (rows, K // 32, 1))).astype(np.float32).reshape(rows, K)


def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_quantised(q, x):
    """q's host codes and scales equal the host codec's of x ([rows][K])."""
    codes, scales = mxfp4_reference(x)
    assert np.array_equal(q.scales.array, scales.ravel()), first_mismatches(_bits(x), q.scales.array, scales, 32)
    assert np.array_equal(q.codes.array, codes.ravel()), first_mismatches(_bits(x), q.codes.array, codes, 2)


# ------------------------------------------------------------ 1: one work-group


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
@pytest.mark.parametrize("rows,K", [(1, 2048), (64, 32)])
def test_smallest_launch(cr, rows, K, src):
    x = _wide(rows, K, seed=rows + K, spread=20)
    if src == "bfloat16":
        x = to_bf16_bits(x).reshape(rows, K)
    q = MxFp4Quantizer(rows, K, src=src, cruncher=cr)
    assert q.packed is None and q.blocks == 64 and q.codes.is_fp4 and q.codes.N == 1024
    q.X.array[:] = x.ravel()
    q.codes.array[:] = 0xAA
    q.scales.array[:] = 0xAA
    q.run()
    _assert_quantised(q, x)


# -------------------------------------------------------- 2: every rounding case


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
def test_every_rounding_case(cr, src):
    """designed_patterns() as a flat (n/32) x 32 input (bfloat16: its high
    halves): packed codes and scales bit for bit the host codec's.  A mismatch
    is reported with the bit patterns of the two inputs of its byte."""
    x, codes, scales = designed_reference4(src)
    q = MxFp4Quantizer(x.shape[0], 32, src=src, cruncher=cr)
    q.X.array[:] = x.ravel()
    q.codes.array[:] = 0xAA
    q.scales.array[:] = 0xAA
    q.run()
    bad_s = first_mismatches(_bits(x), q.scales.array, scales, 32)
    bad_c = first_mismatches(_bits(x), q.codes.array, codes, 2)
    assert not bad_s and not bad_c, (int((q.scales.array != scales.ravel()).sum()), bad_s,
                                     int((q.codes.array != codes.ravel()).sum()), bad_c)


# ------------------------------------------------------------- 3: packed scales


def test_packed_scales_with_nan_blocks(cr):
    rows, K = 128, 384
    x = _wide(rows, K, seed=3)
    for r, k in ((0, 0), (5, 33), (63, 383), (64, 128), (127, 352)):
        x[r, k] = np.nan
    q = MxFp4Quantizer(rows, K, cruncher=cr)
    q.X.array[:] = x.ravel()
    q.packed.array[:] = 0xAAAAAAAA
    q.run()
    _assert_quantised(q, x)
    s = q.scales.array.reshape(rows, K // 32)
    assert int((s == 0xFF).sum()) == 5 and s[5, 1] == 0xFF and s[127, 11] == 0xFF
    np.testing.assert_array_equal(q.packed.array, pack_mx_scales(s).ravel())
    assert int((q.packed.array.view(np.uint8) == 0xFF).sum()) == 5


# ------------------------------------------------------ 4: several logical devices


@pytest.mark.parametrize("ndev", [2, 3])
def test_logical_devices_hold_whole_outputs(ndev):
    g0 = ck.ClPlatforms.all().gpus()[0]
    devs = g0
    for _ in range(ndev - 1):
        devs = devs + g0
    c = ck.ClNumberCruncher(devs, "", prebuilt=library("mx4_quantize", "mx_quantize"))
    c.set_time_scale(ndev - 1, 1.7)  # uneven split after the first call
    rows, K = 512, 1024
    n = rows * K
    q = MxFp4Quantizer(rows, K, cruncher=c)
    for it in range(4):
        x = _wide(rows, K, seed=40 + it)
        codes, scales = to_mxfp4(x)
        q.X.array[:] = x.ravel()
        q.run(compute_id=5, download=False)
        assert len(q.records) == 2
        for rec, out_bytes, total in ((q.records[0], n // 2 + n // 32, q.blocks), (q.records[1], n // 32, n // 128)):
            assert rec["d2h_bytes"] == 0, rec
            assert rec["gather_bytes"] == (ndev - 1) * out_bytes, rec
            r = rec["ranges"]
            assert len(r) == ndev and sum(r) == total and all(v % 64 == 0 for v in r), r
        for d in range(ndev):  # every replica is whole
            for arr, want in ((q.codes, codes), (q.scales, scales), (q.packed, pack_mx_scales(scales))):
                arr.array[:] = 0
                c.download(arr, d)
                np.testing.assert_array_equal(arr.array, want.ravel(), err_msg=f"call {it}, device {d}")
    assert len(set(c.ranges(5))) > 1  # the split moved while resident
    # X left resident: no upload, the same outputs
    q.run(compute_id=5, upload=False, download=True)
    assert q.records[0]["h2d_bytes"] == 0
    _assert_quantised(q, x)
    np.testing.assert_array_equal(q.packed.array, pack_mx_scales(scales).ravel())
    c.dispose()


# ------------------------------------------------------------ 5: GEMM end to end

GEMM_CASES = [("128x128", (128, 128, 256)), ("256x256pbx", (256, 256, 256)), ("256x256pbx", (1024, 768, 768))]
_HOST = {}


def _feed(g, ca, sa, cb, sb):
    g.A.array[:], g.SA.array[:], g.B.array[:], g.SB.array[:] = ca.ravel(), sa.ravel(), cb.ravel(), sb.ravel()


def _host_route(cr, tile, shape, seed=0, nan_at=None):
    """Seeded fp32 a, b (``nan_at``: an element of a made NaN), their
    host-codec MXFP4 forms and the C of a GEMM fed with those by upload, once
    per case."""
    key = (tile, shape, seed, nan_at)
    if key not in _HOST:
        M, N, K = shape
        a, b = _wide(M, K, 100 + seed + sum(shape)), _wide(N, K, 200 + seed + sum(shape))
        if nan_at is not None:
            a[nan_at] = np.nan
        (ca, sa), (cb, sb) = to_mxfp4(a), to_mxfp4(b)
        g2 = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
        _feed(g2, ca, sa, cb, sb)
        g2.C.array[:] = np.nan if nan_at is None else 0.0
        g2.run()
        case = dict(a=a, b=b, ca=ca, sa=sa, cb=cb, sb=sb, c=g2.result())
        for v in case.values():
            v.setflags(write=False)
        _HOST[key] = case
    return _HOST[key]


def _assert_same_c(got, want):
    assert got.dtype == np.float32 and not np.isnan(want).any()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("tile,shape", GEMM_CASES)
def test_gemm_fed_from_the_device(cr, tile, shape):
    M, N, K = shape
    h = _host_route(cr, tile, shape)
    g1 = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    g1.quantize_operand("A", h["a"])
    g1.quantize_operand("B", h["b"])
    assert g1._stale == {"A", "B"}
    g1.C.array[:] = np.nan
    g1.run()
    # neither operand nor scales go up: at most the dims array
    assert cr.last_record()["h2d_bytes"] <= g1.dims.nbytes, cr.last_record()
    _assert_same_c(g1.result(), h["c"])
    g1.sync_operands()
    assert not g1._stale
    for arr, want in ((g1.A, h["ca"]), (g1.SA, h["sa"]), (g1.B, h["cb"]), (g1.SB, h["sb"])):
        np.testing.assert_array_equal(arr.array, want.ravel())
    # |C - ref| <= K · 2^-23 · Σ_k |a_k·b_k| per element, a and b the dequantised
    # operands: the products are exact (e2m1 values times powers of two) and
    # each of the K fp32 additions is off by at most one unit in the last place
    # of a partial sum <= Σ|a·b|.  Nothing leaves fp32's normal range: nonzero
    # elements are at least 2^-1 under block scales of at least 2^-21
    # (asserted), so nonzero products are above 2^-44.  verify_full reports
    # max |C - ref| / max |ref| per tile: the same bound, taken per tile.
    assert int(g1.SA.array.min()) >= 127 - 21 and int(g1.SB.array.min()) >= 127 - 21
    a = from_mxfp4(h["ca"], h["sa"]).astype(np.float64)
    b = from_mxfp4(h["cb"], h["sb"]).astype(np.float64)
    ref = a @ b.T
    bound = K * 2.0 ** -23 * (np.abs(a) @ np.abs(b).T)
    per_tile = lambda x: x.reshape(M // g1.BM, g1.BM, N // g1.BN, g1.BN).max(axis=(1, 3))  # noqa: E731
    limit = float((per_tile(bound) / per_tile(np.abs(ref))).max())
    err, checked = g1.verify_full(1)
    print(f"mxfp4 quantize+gemm {tile} {shape}: verify_full = {err:.3e}, limit = {limit:.3e}")
    assert checked == g1.tiles and err <= limit, (err, limit, checked)


# ----------------------------------------------------- 6: mixed feeding and guards


def test_mixed_feeding_and_guards(cr):
    tile, shape = "256x256pbx", (256, 256, 256)
    M, N, K = shape
    h = _host_route(cr, tile, shape)
    g = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    g.B.array[:], g.SB.array[:] = h["cb"].ravel(), h["sb"].ravel()
    g.quantize_operand("A", h["a"])  # A on the device, B and SB from the host
    g.C.array[:] = np.nan
    g.run()
    _assert_same_c(g.result(), h["c"])
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g.run(resident=False)
    g.sync_operands()
    np.testing.assert_array_equal(g.SA.array, h["sa"].ravel())
    g.C.array[:] = np.nan
    g.run(resident=False)
    _assert_same_c(g.result(download=False), h["c"])
    # a second quantisation with other data (and other scales) gives its C
    h2 = _host_route(cr, tile, shape, seed=7)
    assert (h2["sa"] != h["sa"]).mean() > 0.5
    g.quantize_operand("A", ck.ClArray(h2["a"].ravel().copy()))  # an fp32 ClArray this time
    g.quantize_operand("B", h2["b"])
    g.C.array[:] = np.nan
    g.run()
    _assert_same_c(g.result(), h2["c"])
    # download=True brings codes and scales along: nothing is stale
    g.quantize_operand("A", h["a"], download=True)
    assert g._stale == {"B"}
    np.testing.assert_array_equal(g.A.array, h["ca"].ravel())
    np.testing.assert_array_equal(g.SA.array, h["sa"].ravel())
    with pytest.raises(NotImplementedError, match="separate, later change"):
        g.quantize("A", h["a"])


# ------------------------------------------------------------------ 7: a NaN block


def test_nan_block_through_quantize_operand(cr):
    """One NaN in A: its block's scale byte is 0xFF on both routes, so row 37
    of C is NaN and everything else is bit for bit the host-fed GEMM's."""
    tile, shape = "256x256pbx", (256, 256, 256)
    M, N, K = shape
    h = _host_route(cr, tile, shape, nan_at=(37, 70))
    assert h["sa"][37, 2] == 0xFF and int((h["sa"] == 0xFF).sum()) == 1
    g = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    g.quantize_operand("A", h["a"])
    g.quantize_operand("B", h["b"])
    g.C.array[:] = 0.0
    g.run()
    got, want = g.result(), h["c"]
    assert np.isnan(want[37]).all() and int(np.isnan(want).sum()) == N
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])
    g.sync_operands()
    np.testing.assert_array_equal(g.SA.array, h["sa"].ravel())
    np.testing.assert_array_equal(g.A.array, h["ca"].ravel())


# --------------------------------------------------------------- 8: bf16 source


def test_bf16_source_end_to_end(cr):
    tile, shape = "256x256pbx", (256, 256, 256)
    M, N, K = shape
    abits, bbits = to_bf16_bits(_wide(M, K, 71)), to_bf16_bits(_wide(N, K, 72))
    (ca, sa), (cb, sb) = to_mxfp4(from_bf16_bits(abits)), to_mxfp4(from_bf16_bits(bbits))
    g2 = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    _feed(g2, ca, sa, cb, sb)
    g2.run()
    want = g2.result()
    g1 = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    xa = ck.ClArray(abits.ravel().copy(), "bfloat16")
    g1.quantize_operand("A", xa)                      # a bf16 ClArray, uploaded (read is set)
    g1.quantize_operand("B", bbits, src="bfloat16")   # bit patterns in a numpy array
    g1.C.array[:] = np.nan
    g1.run()
    _assert_same_c(g1.result(), want)
    xa.read = False                                   # resident now: quantised again where it lies
    xa.array[:] = 0
    g1.quantize_operand("A", xa)
    g1.run()
    _assert_same_c(g1.result(), want)
    g1.sync_operands()
    for arr, ref in ((g1.A, ca), (g1.SA, sa), (g1.B, cb), (g1.SB, sb)):
        np.testing.assert_array_equal(arr.array, ref.ravel())
