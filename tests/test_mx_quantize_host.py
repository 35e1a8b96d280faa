"""Device-side MXFP8 quantisation on the host (no GPU): the designed input
patterns the GPU tier runs (test_gpu_mx_quantize.py imports them), the
kernels' algorithm as integer / float32 numpy (ops/quantize.py
mxfp8_kernel_model) against the float64 codec to_mxfp8 bit for bit, argument
errors, the library entry and its code object."""
import functools

import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import GemmMxFp8, to_mxfp8
from cekirdekler_amd.ops.quantize import MxFp8Quantizer, mxfp8_kernel_model, mxfp8_reference

DESIGNED_BODY = 5_570_816  # items 1-3 of designed_patterns()


def _special_blocks() -> np.ndarray:
    f = lambda *v: np.array(v, np.float32).view(np.uint32)  # noqa: E731
    nan, inf = np.uint32(0x7FC00000), np.uint32(0x7F800000)
    b = np.zeros((8, 32), np.uint32)
    b[1] = 0x80000000                                   # all -0
    b[2] = nan                                          # all NaN
    b[2, 1::2] = 0xFFC00001                             # (signed, with a payload)
    b[3] = inf                                          # all +inf
    b[4] = np.resize(f(448.0, -0.5, 3.0e-3, -1.75, 1.0), 32)
    b[4, :3] = nan, inf | np.uint32(0x80000000), f(1.0)[0]  # NaN, -inf, 1.0, ...
    b[5] = np.arange(1, 33, dtype=np.uint32) * 0x3FFFF  # fp32 subnormals only, up to 0x7FFFE0
    b[5, 1::2] |= 0x80000000
    b[6] = np.resize(f(1.0, -2.0 ** 100, 2.0 ** 119, 2.0 ** 127 * 1.75, -2.0 ** 118 * 1.0625), 32)
    b[6, 0] = 0x7F7FFFFF                                # FLT_MAX leader
    b[7] = np.resize(np.array([0x00000001, 0x807FFFFF, 0x00400000, 0x80200000, 0x00080000, 0x00040000], np.uint32), 32)
    b[7, 0] = 0x00800000                                # smallest normal leader
    return b.ravel()


@functools.lru_cache(maxsize=1)
def designed_patterns() -> np.ndarray:
    """fp32 bit patterns (uint32, read-only), blocks of 32, a multiple of 2048:

    1. P: every pattern whose low half is 0x0000, 0x0001 or 0xFFFF, ascending.
    2. a seeded permutation of P (huge beside tiny: underflow to signed zero).
    3. leader blocks: element 0 has mantissa 0 or 0x7FFFFF and exponent field
       E in 1..254; the other 31 have exponent field E - d (d in 0..12), both
       signs, all 128 top-7 mantissa values and low halves 0, 1, 0xFFFF (768
       followers per leader, repeated to fill 25 blocks): every e4m3 rounding
       tie and one fp32 ulp to either side of it, at every kept-bit count down
       to the round-to-zero boundary.
    4. named special blocks (_special_blocks), then zeros."""
    low = np.array([0x0000, 0x0001, 0xFFFF], np.uint32)
    P = ((np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)) | low[None, :]).ravel()
    perm = np.random.default_rng(20260).permutation(P)
    sign = np.array([0, 0x80000000], np.uint32)
    top7 = np.arange(128, dtype=np.uint32) << np.uint32(16)
    F = (sign[:, None, None] | top7[None, :, None] | low[None, None, :]).ravel()  # 768
    F = np.resize(F, 25 * 31).reshape(25, 31)
    lead, fexp = [], []
    for mant in (0, 0x7FFFFF):
        for E in range(1, 255):
            for d in range(0, min(12, E) + 1):
                lead.append((E << 23) | mant)
                fexp.append((E - d) << 23)
    lead, fexp = np.array(lead, np.uint32), np.array(fexp, np.uint32)
    blocks = np.empty((len(lead), 25, 32), np.uint32)
    blocks[:, :, 0] = lead[:, None]
    blocks[:, :, 1:] = F[None] | fexp[:, None, None]
    body = np.concatenate([P, perm, blocks.ravel()])
    assert body.size == DESIGNED_BODY
    out = np.concatenate([body, _special_blocks()])
    out = np.concatenate([out, np.zeros(-out.size % 2048, np.uint32)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def designed_reference(src: str = "float32"):
    """to_mxfp8 of designed_patterns() as (n/32) x 32 (bfloat16: of the high
    halves as bf16 bit patterns): (input, codes, scales), computed once."""
    p = designed_patterns().reshape(-1, 32)
    x = p.view(np.float32) if src == "float32" else (p >> np.uint32(16)).astype(np.uint16)
    with np.errstate(invalid="ignore"):  # signalling NaN patterns in a float64 cast
        codes, scales = mxfp8_reference(x)
    for a in (x, codes, scales):
        a.setflags(write=False)
    return x, codes, scales


def first_mismatches(x, got, want, per: int = 1, limit: int = 6) -> list:
    """The first few (index, input pattern(s), got, want) of two flat arrays
    (``per`` inputs per output element)."""
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())[:limit]
    xs = np.asarray(x).ravel()
    return [(int(i), [hex(int(v)) for v in xs[i * per:(i + 1) * per][:4]], hex(int(np.asarray(got).ravel()[i])),
             hex(int(np.asarray(want).ravel()[i]))) for i in bad]


def test_designed_patterns_cover_the_codec():
    p = designed_patterns()
    assert p.dtype == np.uint32 and p.size % 2048 == 0 and p.size - DESIGNED_BODY < 2 * 2048
    _, codes, scales = designed_reference("float32")
    body_c, body_s = codes.ravel()[:DESIGNED_BODY], scales.ravel()[:DESIGNED_BODY // 32]
    assert len(np.unique(body_c)) >= 250 and len(np.unique(body_s)) >= 240
    assert len(np.unique(body_c)) == 255 and len(np.unique(body_s)) == 247  # as designed
    assert not (scales == 0xFF).any()
    assert int(((body_c & 0x7F) == 0x7E).sum()) >= 100_000  # saturated
    assert int(((body_c & 0x7F) == 0x7F).sum()) >= 1000     # NaN
    assert not (body_c == 0xFF).any()                       # NaN carries no sign
    # the special blocks: zeros keep their sign under byte 127, NaN and inf have no say in the scale
    sc, cc = scales.ravel()[DESIGNED_BODY // 32:][:8], codes.ravel()[DESIGNED_BODY:].reshape(-1, 32)[:8]
    assert sc[:4].tolist() == [127, 127, 127, 127]
    assert (cc[0] == 0).all() and (cc[1] == 0x80).all() and (cc[2] == 0x7F).all() and (cc[3] == 0x7E).all()
    assert sc[4] == 127 and cc[4, :4].tolist() == [0x7F, 0xFE, 0x38, 0xBE]  # amax 448: e = 0; 1.0, -1.75
    assert sc[5] == 0 and (cc[5] & 0x7F).max() > 0  # subnormals times 2^127 have nonzero codes
    assert sc[6] == 127 + 119 and sc[7] == 0


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
def test_kernel_model_equals_the_float64_codec(src):
    """The kernels' route (exponent field, one fp32 multiply, e4m3 bit
    rounding) is to_mxfp8's (frexp, float64 ldexp, float32 cast) bit for bit."""
    x, codes, scales = designed_reference(src)
    got_c, got_s = mxfp8_kernel_model(x, src)
    assert got_c.dtype == np.uint8 and got_s.dtype == np.uint8 and got_c.shape == codes.shape
    assert np.array_equal(got_s, scales), first_mismatches(x.view(x.dtype.str.replace("f", "u")), got_s, scales, 32)
    assert np.array_equal(got_c, codes), first_mismatches(x.view(x.dtype.str.replace("f", "u")), got_c, codes)


def test_reference_of_bf16_is_the_codec_of_the_decoded_values():
    bits = np.array([[0x3F80, 0xBF80, 0x7F80, 0x7FC0, 0x0001, 0x8000] + [0x4000] * 26], np.uint16)
    want = to_mxfp8((bits.astype(np.uint32) << 16).view(np.float32))
    got = mxfp8_reference(bits)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    arr = ck.ClArray(bits.ravel().copy(), "bfloat16")
    assert arr.is_bf16 and np.array_equal(mxfp8_reference(arr)[0], want[0].ravel())


# ---------------------------------------------------------------- arguments


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


def test_quantizer_argument_errors(cpu_cr):
    with pytest.raises(ValueError, match="K %"):
        MxFp8Quantizer(64, 48, cruncher=cpu_cr)
    with pytest.raises(ValueError, match="multiple of 64"):
        MxFp8Quantizer(3, 32 * 7, cruncher=cpu_cr)
    with pytest.raises(ValueError, match="src"):
        MxFp8Quantizer(64, 128, src="float16", cruncher=cpu_cr)
    with pytest.raises(ValueError, match="codes"):
        MxFp8Quantizer(64, 128, cruncher=cpu_cr, codes=ck.ClArray(64 * 128 - 32, "float8_e4m3fn"))
    with pytest.raises(ValueError, match="packed"):
        MxFp8Quantizer(32, 64, cruncher=cpu_cr, packed=ck.ClArray(16, np.uint32))
    with pytest.raises(ValueError):
        mxfp8_kernel_model(np.zeros((2, 48), np.float32))


def test_quantizer_refuses_a_cruncher_without_its_kernels(cpu_cr):
    """Never a launch: the constructor names the missing kernel."""
    with pytest.raises(ck.ClComputeError, match="cek_mx_quantize_f32.*mx_quantize"):
        MxFp8Quantizer(64, 128, cruncher=cpu_cr)
    g = GemmMxFp8(256, 256, 128, cruncher=cpu_cr, tile="128x128", fill="none")
    with pytest.raises(ValueError, match="cek_mx_quantize_f32.*mx_quantize"):
        g.quantize("A", np.zeros((256, 128), np.float32))
    assert not g._stale


def test_gemm_quantize_argument_errors(cpu_cr):
    g = GemmMxFp8(256, 128, 128, cruncher=cpu_cr, tile="128x128", fill="none")
    ok = np.zeros((256, 128), np.float32)
    with pytest.raises(ValueError, match="'A' or 'B'"):
        g.quantize("C", ok)
    with pytest.raises(ValueError, match="elements"):
        g.quantize("B", ok)  # B is 128 x 128
    with pytest.raises(ValueError, match="elements"):
        g.quantize("A", ok[:, :96])
    with pytest.raises(ValueError, match="src"):
        g.quantize("A", ok, src="float16")
    with pytest.raises(ValueError, match="float32"):
        g.quantize("A", ok.astype(np.float64))
    with pytest.raises(ValueError, match="uint16"):
        g.quantize("A", ok, src="bfloat16")
    with pytest.raises(ValueError, match="ClArray"):
        g.quantize("A", ck.ClArray(np.zeros(256 * 128, np.int32)))
    with pytest.raises(ValueError, match="ClArray"):
        g.quantize("A", ck.ClArray(256 * 128, "bfloat16"), src="float32")
    assert not g._stale and not g._quantizers


def test_stale_operand_state(cpu_cr):
    """What run() uploads follows the stale marks: a device-quantised operand
    leaves the upload list with its packed scales, which are not re-packed
    from the host scales; a host-resident run is refused until sync."""
    g = GemmMxFp8(256, 256, 128, cruncher=cpu_cr, tile="128x128")
    assert [a is b for a, b in zip(g._inputs(False), (g.dims, g.A, g.B, g._SAp, g._SBp))] == [True] * 5
    g._SAp.array[:] = 0xDEADBEEF
    g._stale.add("A")
    ins = g._inputs(True)
    assert len(ins) == 3 and ins[0] is g.dims and ins[1] is g.B and ins[2] is g._SBp
    assert (g._SAp.array == 0xDEADBEEF).all()
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g.run(resident=False)


# ------------------------------------------------------------------ library


def test_mx_quantize_library_entry():
    from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object

    names = ["cek_mx_pack_scales", "cek_mx_quantize_bf16", "cek_mx_quantize_f32"]
    assert sorted(LIBRARY["mx_quantize"]) == names
    assert all(ARITY[k] == 3 for k in names)
    assert LIBRARY["sgemm_mxfp8"] == ["cek_sgemm_mxfp8_128x128", "cek_sgemm_mxfp8_256x256pbx"]
    with open(code_object("mx_quantize"), "rb") as f:
        blob = f.read()
    for k in names:
        assert b"\0" + k.encode() + b".kd\0" in blob, k
