"""Device-side MXFP4 quantisation on the host (no GPU): what the designed
input patterns of test_mx_quantize_host.py cover of the codec to_mxfp4 (the
GPU tier, test_gpu_mx4_quantize.py, runs them), the kernels' algorithm as
integer / float32 numpy (ops/quantize.py mxfp4_kernel_model) against the
float64 codec bit for bit, argument errors, the stale-operand bookkeeping of
GemmMxFp4.quantize_operand, the library entry and its code object."""
import functools

import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import GemmMxFp4, to_mxfp4, unpack_fp4
from cekirdekler_amd.ops.quantize import (MxFp4Quantizer, MxFp8Quantizer, e2m1_convert_model, mxfp4_kernel_model,
                                          mxfp4_reference)
from test_mx_quantize_host import DESIGNED_BODY, designed_patterns, first_mismatches

TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


@functools.lru_cache(maxsize=2)
def designed_reference4(src: str = "float32"):
    """to_mxfp4 of designed_patterns() as (n/32) x 32 (bfloat16: of the high
    halves as bf16 bit patterns): (input, packed codes, scales), computed once."""
    p = designed_patterns().reshape(-1, 32)
    x = p.view(np.float32) if src == "float32" else (p >> np.uint32(16)).astype(np.uint16)
    with np.errstate(invalid="ignore"):  # signalling NaN patterns in a float64 cast
        codes, scales = mxfp4_reference(x)
    for a in (x, codes, scales):
        a.setflags(write=False)
    return x, codes, scales


def _scaled(bits, scales):
    """|value| of fp32 bit patterns [blocks][32] over their block's scale [blocks], float64 (exact)."""
    v = (bits & np.uint32(0x7FFFFFFF)).view(np.float32).astype(np.float64)
    return np.ldexp(v, (127 - scales.astype(np.int64))[:, None])


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
def test_designed_patterns_cover_the_codec(src):
    x, packed, scales = designed_reference4(src)
    nb = DESIGNED_BODY // 32
    bits = x.view(np.uint32) if src == "float32" else x.astype(np.uint32) << np.uint32(16)
    codes = unpack_fp4(packed)
    body_b, body_c, body_s = bits[:nb], codes[:nb], scales.ravel()[:nb]
    assert sorted(np.unique(body_c).tolist()) == list(range(16))
    plain = body_s != 0xFF
    assert int(body_s[plain].min()) == 0 and int(body_s[plain].max()) == 252
    # blocks with a NaN: enough to exercise the 0xFF rule, too few to swamp the codes
    nan_blocks = int((~plain).sum())
    assert nan_blocks == (741 if src == "float32" else 737) and nb == 174_088  # as designed
    assert 500 <= nan_blocks < 0.01 * nb
    with np.errstate(invalid="ignore", over="ignore"):
        v = _scaled(body_b[plain], body_s[plain])
        for tie in TIES:
            assert int((v == tie).sum()) >= 1000, tie
        if src == "float32":  # one fp32 ulp to either side of each tie
            a = body_b[plain] & np.uint32(0x7FFFFFFF)
            below, above = _scaled(a + np.uint32(1), body_s[plain]), _scaled(a - np.uint32(1), body_s[plain])
            for tie in TIES:
                assert int((below == tie).sum()) >= 1000 and int((above == tie).sum()) >= 1000, tie
        saturated = np.isfinite(v) & (v > 6.0)
    assert int(saturated.sum()) > 100_000 and ((body_c[plain][saturated] & 7) == 7).all()
    # the special blocks
    sc, cc = scales.ravel()[nb:][:8], codes[nb:][:8]
    assert sc[:2].tolist() == [127, 127] and (cc[0] == 0).all() and (cc[1] == 8).all()  # zeros keep their sign
    assert sc[2] == 0xFF and (cc[2] == 0).all()                 # all NaN
    assert sc[3] == 127 and (cc[3] == 7).all()                  # all +inf: no say in the scale, saturated
    assert sc[4] == 0xFF and cc[4, :4].tolist() == [0, 15, 0, 8]  # NaN, -inf, 1.0 / 64, -1.75 / 64 under amax 448
    assert sc[5] == 0 and (cc[5] & 7).max() > 0                 # subnormals times 2^127 have nonzero codes
    assert sc[6] == 252                                         # FLT_MAX leader (bf16: 0x7F7F)


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
def test_kernel_model_equals_the_float64_codec(src):
    """The kernels' route (exponent field, one fp32 multiply, e2m1 bit
    rounding, NaN mask) is to_mxfp4's (frexp, float64 ldexp, midpoint
    comparisons) bit for bit."""
    x, codes, scales = designed_reference4(src)
    got_c, got_s = mxfp4_kernel_model(x, src)
    assert got_c.dtype == np.uint8 and got_s.dtype == np.uint8 and got_c.shape == codes.shape
    xb = x.view(x.dtype.str.replace("f", "u"))
    assert np.array_equal(got_s, scales), first_mismatches(xb, got_s, scales, 32)
    assert np.array_equal(got_c, codes), first_mismatches(xb, got_c, codes, 2)


def test_convert_model_on_the_grid():
    y = np.array([0.0, 0.25, 0.2500001, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0, 3.5, 4.0, 5.0, 5.0000005, 6.0,
                  7.9, 1e30, np.inf, -0.0, -0.25, -0.75, -6.5, -np.inf], np.float32)
    want = [0, 0, 1, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6, 6, 6, 7, 7, 7, 7, 7, 8, 8, 10, 15, 15]
    assert e2m1_convert_model(y).tolist() == want


def test_reference_of_bf16_is_the_codec_of_the_decoded_values():
    bits = np.array([[0x3F80, 0xBF80, 0x7F80, 0x7FC0, 0x0001, 0x8000] + [0x4000] * 26,
                     [0x3F80, 0xBF80, 0xFF80, 0x4040, 0x0001, 0x8000] + [0x4000] * 26], np.uint16)
    want = to_mxfp4((bits.astype(np.uint32) << 16).view(np.float32))
    got = mxfp4_reference(bits)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].ravel().tolist() == [0xFF, 126] and got[0].shape == (2, 16)  # a NaN; amax 3 = 1.5 · 2^1
    arr = ck.ClArray(bits.ravel().copy(), "bfloat16")
    assert arr.is_bf16 and np.array_equal(mxfp4_reference(arr)[0], want[0].ravel())


# ---------------------------------------------------------------- arguments


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


def test_quantizer_argument_errors(cpu_cr):
    with pytest.raises(ValueError, match="K %"):
        MxFp4Quantizer(64, 48, cruncher=cpu_cr)
    with pytest.raises(ValueError, match="multiple of 64"):
        MxFp4Quantizer(3, 32 * 7, cruncher=cpu_cr)
    with pytest.raises(ValueError, match="src"):
        MxFp4Quantizer(64, 128, src="float16", cruncher=cpu_cr)
    with pytest.raises(ValueError, match=f"codes must be a ClArray of {64 * 128 // 2} uint8"):
        MxFp4Quantizer(64, 128, cruncher=cpu_cr, codes=ck.ClArray(64 * 128, "float4_e2m1fn_x2"))  # one per element
    with pytest.raises(ValueError, match="scales"):
        MxFp4Quantizer(64, 128, cruncher=cpu_cr, scales=ck.ClArray(64 * 128 // 32, np.int32))
    with pytest.raises(ValueError, match="packed"):
        MxFp4Quantizer(32, 64, cruncher=cpu_cr, packed=ck.ClArray(16, np.uint32))
    with pytest.raises(ValueError):
        mxfp4_kernel_model(np.zeros((2, 48), np.float32))
    with pytest.raises(ValueError, match="uint16"):
        mxfp4_kernel_model(np.zeros((2, 64), np.float32), "bfloat16")


def test_quantizer_refuses_a_cruncher_without_its_kernels(cpu_cr):
    """Never a launch: the constructor names the missing kernel and its library."""
    with pytest.raises(ck.ClComputeError, match="cek_mx4_quantize_f32.*'mx4_quantize'"):
        MxFp4Quantizer(64, 128, cruncher=cpu_cr)
    with pytest.raises(ck.ClComputeError, match=r"cek_mx_quantize_f32.*library\('mx_quantize'\)"):
        MxFp8Quantizer(64, 128, cruncher=cpu_cr)  # as it was
    g = GemmMxFp4(256, 256, 256, cruncher=cpu_cr, tile="128x128", fill="none")
    with pytest.raises(ValueError, match="cek_mx4_quantize_f32.*mx4_quantize"):
        g.quantize_operand("A", np.zeros((256, 256), np.float32))
    assert not g._stale


def test_quantize_operand_argument_errors(cpu_cr):
    g = GemmMxFp4(256, 128, 256, cruncher=cpu_cr, tile="128x128", fill="none")
    ok = np.zeros((256, 256), np.float32)
    with pytest.raises(ValueError, match="'A' or 'B'"):
        g.quantize_operand("C", ok)
    with pytest.raises(ValueError, match="elements"):
        g.quantize_operand("B", ok)  # B is 128 x 256
    with pytest.raises(ValueError, match="elements"):
        g.quantize_operand("A", ok[:, :96])
    with pytest.raises(ValueError, match="src"):
        g.quantize_operand("A", ok, src="float16")
    with pytest.raises(ValueError, match="float32"):
        g.quantize_operand("A", ok.astype(np.float64))
    with pytest.raises(ValueError, match="uint16"):
        g.quantize_operand("A", ok, src="bfloat16")
    with pytest.raises(ValueError, match="ClArray"):
        g.quantize_operand("A", ck.ClArray(np.zeros(256 * 256, np.int32)))
    with pytest.raises(ValueError, match="ClArray"):
        g.quantize_operand("A", ck.ClArray(256 * 256, "bfloat16"), src="float32")
    assert not g._stale and not g._quantizers


def test_stale_operand_state(cpu_cr):
    """What run() uploads follows the stale marks, as in GemmMxFp8; quantize
    itself still refuses as before and leaves the marks alone."""
    g = GemmMxFp4(256, 256, 256, cruncher=cpu_cr, tile="128x128")
    assert [a is b for a, b in zip(g._inputs(False), (g.dims, g.A, g.B, g._SAp, g._SBp))] == [True] * 5
    g._SAp.array[:] = 0xDEADBEEF
    g._stale.add("A")
    ins = g._inputs(True)
    assert len(ins) == 3 and ins[0] is g.dims and ins[1] is g.B and ins[2] is g._SBp
    assert (g._SAp.array == 0xDEADBEEF).all()
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g.run(resident=False)
    with pytest.raises(NotImplementedError, match="separate, later change"):
        g.quantize("A", np.zeros((256, 256), np.float32))
    assert g._stale == {"A"}


# ------------------------------------------------------------------ library


def test_mx4_quantize_library_entry():
    from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object

    names = ["cek_mx4_quantize_bf16", "cek_mx4_quantize_f32"]
    assert sorted(LIBRARY["mx4_quantize"]) == names
    assert all(ARITY[k] == 3 for k in names)
    with open(code_object("mx4_quantize"), "rb") as f:
        blob = f.read()
    for k in names:
        assert b"\0" + k.encode() + b".kd\0" in blob, k
    # the older MX entries are as they were
    assert LIBRARY["mx_quantize"] == ["cek_mx_quantize_f32", "cek_mx_quantize_bf16", "cek_mx_pack_scales"]
    assert LIBRARY["sgemm_mxfp8"] == ["cek_sgemm_mxfp8_128x128", "cek_sgemm_mxfp8_256x256pbx"]
    assert LIBRARY["sgemm_mxfp4"] == ["cek_sgemm_mxfp4_128x128", "cek_sgemm_mxfp4_256x256pbx"]
