"""Cases for the MXFP4 GEMM (kernels/sgemm_mxfp4.hip, gemm8_tile.h with e2m1
operands, ops.gemm.GemmMxFp4), in the manner of gemm8_oracles.py: the shapes, the exact
data, the scale-mapping probe with its wrong maps, and the single-instruction
probe of v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1 operands.

No GPU use here.  The CPU tier (test_mxfp4_host.py) checks the builders and
shows that every wrong map changes more than half of C; the GPU tier
(test_gpu_gemm_mxfp4.py) applies the same builders and comparisons to what
the kernels and the instruction return.

Element values are given as numbers (checked to be e2m1 values) and scales as
exponents or bytes; every expectation is exact float64 arithmetic on them,
rounded once to fp32 where it says so.
"""
from __future__ import annotations

import functools

import numpy as np

from cekirdekler_amd.ops import gemm
from gemm_oracles import FINITE, NAN, NEG_INF, POS_INF

E8M0_NAN = 0xFF
# every e2m1 value but -0
VALUES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.5, -1, -1.5, -2, -3, -4, -6], np.float32)
NONZERO = VALUES[1:]

# --------------------------------------------------------------------------- shapes
# K/256 = 1, 2, 3, 5: the ping-pong prologue stages two K-tiles ahead, the Bt
# ring has three buffers and the scales are prefetched one K-tile ahead
# (clamped at the end), so these are the counts at which the loop ends can go wrong
K_TAIL_SHAPES = [(256, 256, 256), (512, 256, 512), (256, 512, 768), (1024, 768, 1280)]
SHAPES = {"256x256pbx": K_TAIL_SHAPES, "128x128": K_TAIL_SHAPES + [(128, 128, 256), (384, 128, 512)]}
RANDOM_SHAPE = (1024, 512, 512)
HOST_SHAPE = (1024, 512, 512)      # host-resident, streamed and re-upload paths: 8 tiles of 256²
TWO_DEVICE_SHAPE = (1024, 1024, 512)

# --------------------------------------------------------------------------- helpers

def pack_values(x):
    """Exactly representable values ``[rows][K]`` → packed fp4x2 bytes ``[rows][K/2]`` (checked)."""
    x = np.asarray(x, np.float32)
    c = gemm.to_fp4_e2m1_codes(x)
    assert np.array_equal(gemm.from_fp4_e2m1_codes(c), x), "value not exact in e2m1"
    return gemm.pack_fp4(c)


def scaled(x, e):
    """float64 [rows][K] elements times 2^e per block of 32 (exact)."""
    rows, K = x.shape
    e = np.broadcast_to(np.asarray(e), (rows, K // 32))
    return (np.asarray(x, np.float64).reshape(rows, K // 32, 32) * np.ldexp(1.0, e)[..., None]).reshape(rows, K)


def set_operands(g, a, b, ea, eb):
    """Fill a GemmMxFp4 from element values and scale exponents (one per row
    and block of 32, or one for all)."""
    g.A.array[:] = pack_values(a).ravel()
    g.B.array[:] = pack_values(b).ravel()
    g.SA.array[:] = np.broadcast_to(127 + np.asarray(ea), (g.M, g.K // 32)).ravel()
    g.SB.array[:] = np.broadcast_to(127 + np.asarray(eb), (g.N, g.K // 32)).ravel()


@functools.lru_cache(maxsize=None)
def int_case(shape):
    """All 15 e2m1 values, scale exponents in {-1, 0, 1} per row and block,
    independently for A and B, and the float64 product, once per shape.

    In units of 2^-4 (elements are multiples of 2^-1, scales at least 2^-1
    each) every product is an integer of at most 6·6·2·2·2^4 = 2304 and every
    partial sum an integer below K·2304 < 2^24: exact in fp32 in any summation
    order.  The products inside a group of 8 neighbouring k share one block,
    so one pair of scales, and differ by at most 36 / 0.25 = 144 < 2^8, with 6
    significant bits at the most: far inside the bits the instruction keeps
    (profiles/gemm_mxfp4.md)."""
    M, N, K = shape
    rng = np.random.default_rng(sum(shape))
    a = VALUES[rng.integers(0, 15, (M, K))]
    b = VALUES[rng.integers(0, 15, (N, K))]
    ea = rng.integers(-1, 2, (M, K // 32))
    eb = rng.integers(-1, 2, (N, K // 32))
    assert K * 2304 < 2 ** 24
    assert float(np.abs(a).max()) == 6 and float(np.abs(b).max()) == 6 and len(np.unique(a)) == 15
    ref = scaled(a, ea) @ scaled(b, eb).T
    assert np.array_equal(np.rint(ref * 16), ref * 16) and np.abs(ref * 16).max() < 2 ** 24
    assert (np.abs(scaled(a, ea)) @ np.abs(scaled(b, eb)).T * 16).max() < 2 ** 24
    for x in (a, b, ea, eb, ref):
        x.setflags(write=False)
    return a, b, ea, eb, ref


# --------------------------------------------------------------------------- the scale-mapping probe
# The MXFP8 probe's construction at K = 768 (three K-tiles of 256 k, six
# 128-k steps, 24 blocks).  SA[m][b] = 127 + ((3m + c·b) % 5 - 2): c = 5 is a
# blind spot there (5b % 5 = 0: SA does not vary with the block).  Here a
# coefficient must also tell blocks 4 apart (the two 128-k steps of a K-tile):
# SB's 2b moves by 8 % 5 = 3 there, SA's c·b by 4c % 5, and when both scales'
# steps are exchanged together the two shifts must not cancel mod 5, which
# c = 3 does (12 % 5 = 2, 2 + 3 = 5: under half of C changes).  c = 2 (3 + 3)
# and c = 4 (1 + 3) leave no blind spot; test_mxfp4_host.py shows all of it.
PROBE_SA_BLOCK_COEFF = [2, 4]
PROBE_BLIND_COEFF = {5: ("A block + 1", "SA steps exchanged"), 3: ("both scales' steps exchanged",)}
PROBE_SHAPE = (256, 512, 768)


def probe_case(c):
    """A picks one k per row (value 1), SA and SB vary with row and block, Bt
    holds the 14 nonzero e2m1 values, asymmetric in n and k and different at k
    and k ^ 1 (5 % 14 != 0) and at k and k ^ 128 (640 % 14 != 0)."""
    M, N, K = PROBE_SHAPE
    m, n, k, blk = np.arange(M), np.arange(N), np.arange(K), np.arange(K // 32)
    pick = (37 * m + 11) % K
    a = np.zeros((M, K), np.float32)
    a[m, pick] = 1
    b = NONZERO[(3 * n[:, None] + 5 * k[None, :]) % 14]
    ea = (3 * m[:, None] + c * blk[None, :]) % 5 - 2
    eb = (7 * n[:, None] + 2 * blk[None, :]) % 5 - 2
    return PROBE_SHAPE, pick, a, b, ea, eb


def probe_expected_and_wrong(c):
    """(want, {name: C a wrong map would give}) for probe_case(c): the wrong
    maps of the MXFP8 probe (unit scales, the k block of either scale shifted
    by one, the scale row shifted by one fragment, SA and SB swapped in role)
    and those particular to fp4: the two nibbles of A's bytes swapped (k ^ 1),
    the two 128-k steps of a K-tile exchanged in A alone (k ^ 128: data and
    scales move together, against Bt in place), and the steps exchanged in the
    scales alone (block ^ 4), for A, for Bt and for both."""
    (M, N, K), pick, a, b, ea, eb = probe_case(c)
    nb = K // 32
    pb = pick // 32
    m, n = np.arange(M), np.arange(N)

    def c_of(k_at, ea_at, eb_at):  # k [M], exponents [M] and [M][N]
        return b[:, k_at].T.astype(np.float64) * np.ldexp(1.0, ea_at[:, None] + eb_at)

    want = c_of(pick, ea[m, pb], eb[:, pb].T)
    np.testing.assert_array_equal(want, scaled(a, ea) @ scaled(b, eb).T)
    wrong = {
        "unit scales": b[:, pick].T.astype(np.float64),
        "A block + 1": c_of(pick, ea[m, (pb + 1) % nb], eb[:, pb].T),
        "B block + 1": c_of(pick, ea[m, pb], eb[:, (pb + 1) % nb].T),
        "A row + 16": c_of(pick, ea[(m + 16) % M, pb], eb[:, pb].T),
        "B row + 16": c_of(pick, ea[m, pb], eb[(n + 16) % N][:, pb].T),
        "SA <-> SB": c_of(pick, eb[m % N, pb], ea[n % M][:, pb].T),
        "A nibbles swapped": c_of(pick ^ 1, ea[m, pb], eb[:, pb].T),
        "A steps exchanged": c_of(pick ^ 128, ea[m, pb], eb[:, (pick ^ 128) // 32].T),
        "SA steps exchanged": c_of(pick, ea[m, pb ^ 4], eb[:, pb].T),
        "SB steps exchanged": c_of(pick, ea[m, pb], eb[:, pb ^ 4].T),
        "both scales' steps exchanged": c_of(pick, ea[m, pb ^ 4], eb[:, pb ^ 4].T),
    }
    return want, wrong


# --------------------------------------------------------------------------- the single-instruction probe
# One wave per problem does one v_mfma_scale_f32_16x16x128_f8f6f4 with
# cbsz = blgp = 4 (e2m1) on a 16×128 A, a 16×128 Bt (64 B per row) and one
# scale dword per lane and operand.  The loader is the natural one: lane l
# (row r = l % 16, q = l / 16) takes bytes [16q, 16q + 16) of its row into
# registers 0–3; registers 4–7 are filled with 0x77 (two 6.0 per byte) to show
# that the instruction ignores them.  Its scale dword comes as it is from the
# buffer, and SEL[p] = 4·op_sel(A) + op_sel(B) picks the bytes.  Its four
# results are C[4q + v][l % 16].  What the hardware does with that is the
# question; the answers are in profiles/gemm_mxfp4.md.
PROBE_SRC = r"""
typedef int p4_i32x8 __attribute__((ext_vector_type(8)));
typedef float p4_f32x4 __attribute__((ext_vector_type(4)));
#define P4_CASE(OA, OB)                                                                             \
  case OA * 4 + OB:                                                                                 \
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb, acc, 4, 4, OA, sa, OB, sb);     \
    break;
#define P4_ROW(OA) P4_CASE(OA, 0) P4_CASE(OA, 1) P4_CASE(OA, 2) P4_CASE(OA, 3)
__global__ void mx4_probe(const unsigned char* A, const unsigned char* Bt, const unsigned char* SA,
                          const unsigned char* SB, const int* SEL, float* C) {
  long long gid = get_global_id(0);
  long long p = gid >> 6;
  int l = (int)(gid & 63), r = l & 15, q = l >> 4;
  const int* a = (const int*)(A + p * 1024 + r * 64);
  const int* b = (const int*)(Bt + p * 1024 + r * 64);
  p4_i32x8 fa, fb;
  for (int w = 0; w < 4; ++w) {
    fa[w] = a[4 * q + w];
    fb[w] = b[4 * q + w];
    fa[4 + w] = 0x77777777;
    fb[4 + w] = 0x77777777;
  }
  int sa = ((const int*)SA)[p * 64 + l], sb = ((const int*)SB)[p * 64 + l];
  p4_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  switch (SEL[p]) {
    P4_ROW(0) P4_ROW(1) P4_ROW(2) P4_ROW(3)
  }
  for (int v = 0; v < 4; ++v) C[p * 256 + (4 * q + v) * 16 + r] = acc[v];
}
"""
PROBE_KERNEL = "mx4_probe"
DECOY = 127 + 40  # exponent of the scale bytes op_sel must NOT pick, plus the byte index: 40 … 43


def _b_asym():
    """Bt [16][128] of nonzero e2m1 values whose 128 columns (over n) are all
    different (rows 0 and 1 are the two base-14 digits of k, the others mix
    them): a column of C names its k."""
    n, k = np.arange(16)[:, None], np.arange(128)[None, :]
    idx = (k * (2 * n + 1) + (k // 14) * n + 3 * n) % 14
    idx[0], idx[1] = k[0] % 14, k[0] // 14
    b = NONZERO[idx]
    cols = {tuple(b[:, i]) for i in range(128)}
    assert len(cols) == 128
    return b


def _lane_scales(s, sel, decoy):
    """Scale bytes [16 rows][4 blocks] → one dword per lane (l = 16·block +
    row under the expected map): byte `sel` is the lane's scale, the others
    DECOY + byte index (decoy) or 127."""
    s = np.asarray(s, np.uint8).reshape(16, 4)
    d = np.empty((64, 4), np.uint8)
    d[:] = (DECOY + np.arange(4)) if decoy else 127
    d[:, sel] = s.T.reshape(64)  # lane 16q + r ← s[r][q]
    return d.reshape(-1)


def _emu(a, b, sa, sb):
    """Exact float64 C of a 16×16×128 problem from element values and scale
    bytes (0xFF: the block is NaN), then (cls, expected) after one rounding to fp32."""
    def deq(x, s):
        return (np.asarray(x, np.float64).reshape(16, 4, 32) * gemm.e8m0_to_f64(s).reshape(16, 4)[..., None]).reshape(16, 128)

    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x, y = deq(a, sa), deq(b, sb)
        c = (x[:, None, :] * y[None, :, :]).sum(axis=2).astype(np.float32)
    cls = np.where(np.isnan(c), NAN, np.where(c == np.inf, POS_INF, np.where(c == -np.inf, NEG_INF, FINITE)))
    cls = cls.astype(np.int8)
    return cls, np.where(cls == FINITE, c, 0).astype(np.float64)


K_MAP_PROBLEMS = 8  # one-hot rows at k = 16j + r, j < 8: every k of the instruction once per operand


@functools.lru_cache(maxsize=None)
def probe_problems():
    """name → dict(a, b: element values [16][128]; sa, sb: scale bytes
    [16][4]; sel: (op_sel A, op_sel B); decoy; want: (cls, expected) under
    the expected maps; show: (row, col) sites the record keeps)."""
    rng = np.random.default_rng(41)
    out = {}
    one = np.full((16, 4), 127)

    def ints(lo=-4, hi=4):  # e2m1 holds the integers 0 … 4 (and 6)
        return rng.integers(lo, hi + 1, (16, 128)).astype(np.float32)

    def add(name, a, b, sa, sb, show, sel=(0, 0), decoy=False):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        sa, sb = np.asarray(sa, np.uint8).reshape(16, 4).copy(), np.asarray(sb, np.uint8).reshape(16, 4).copy()
        p = dict(a=a, b=b, sa=sa, sb=sb, sel=sel, decoy=decoy, want=_emu(a, b, sa, sb), show=tuple(show))
        for v in (a, b, sa, sb) + p["want"]:
            v.setflags(write=False)
        out[name] = p

    r = np.arange(16)
    asym = _b_asym()
    # question 1: which k each (lane, byte, nibble) supplies — A one-hot
    # against the asymmetric Bt, then Bt one-hot against the asymmetric A
    for j in range(K_MAP_PROBLEMS):
        hot = np.zeros((16, 128), np.float32)
        hot[r, 16 * j + r] = 1
        add(f"k_map_a{j}", hot, asym, one, one, [(0, 0), (5, 9), (15, 15)])
        add(f"k_map_b{j}", asym, hot, one, one, [(0, 0), (5, 9), (15, 15)])
    # question 2: which (row, block) a lane's scale byte applies to and which
    # byte op_sel picks — one-hot rows at k = (37r + 11) % 128 (blocks 0 … 3),
    # every (row, block) its own exponent 4·row + block − 32, the bytes op_sel
    # must not pick at exponents 40 … 43
    hot = np.zeros((16, 128), np.float32)
    hot[r, (37 * r + 11) % 128] = 1
    distinct = 127 + 4 * r[:, None] + np.arange(4)[None, :] - 32
    for o in range(4):
        add(f"scale_map_a{o}", hot, asym, distinct, one, [(0, 0), (5, 9), (15, 15)], sel=(o, (o + 1) % 4), decoy=True)
        add(f"scale_map_b{o}", asym, hot, one, distinct, [(0, 0), (9, 5), (15, 15)], sel=((o + 2) % 4, o), decoy=True)
    # the probe's own maps on dense data: mixed block scales, exact
    add("baseline", ints(), ints(), 127 + rng.integers(-2, 3, (16, 4)), 127 + rng.integers(-2, 3, (16, 4)),
        [(0, 0), (5, 9), (15, 15)])
    # question 3: scale byte 0xFF on one block of A, of Bt, and on a block of A that is all zeros
    ai, bi = ints(), ints()
    ai[12, 96:] = 0
    sa, sb = one.copy(), one.copy()
    sa[4, 1] = sa[12, 3] = sb[7, 2] = E8M0_NAN
    add("scale_nan", ai, bi, sa, sb, [(4, 0), (4, 1), (12, 0), (0, 7), (1, 7), (0, 0)], sel=(1, 2))
    # question 4: exponent sums +254, 0 (254 with 0) and -254: positive A, every row of Bt of one sign
    ai = rng.integers(1, 5, (16, 128)).astype(np.float32)
    sign = np.where(r % 3 == 0, -1, 1)[:, None]
    bi = rng.integers(0, 5, (16, 128)).astype(np.float32) * sign
    bi[:, 1] = sign[:, 0]
    ends = np.repeat(np.where(r < 8, 254, 0), 4)
    add("scale_sums", ai, bi, ends, ends, [(0, 0), (0, 1), (0, 8), (8, 0), (8, 8), (8, 9)], sel=(2, 3))
    # question 5: results in fp32's subnormal range: ea + eb = -140 (rows 0 … 11) and -149 (rows 12 … 15), integers
    sa = np.repeat(np.where(r < 12, 127 - 70, 127 - 79), 4)
    add("subnormal", ints(), ints(), sa, np.full(64, 127 - 70), [(0, 0), (1, 2), (12, 0), (13, 5)], sel=(3, 1))
    # question 6: two products of very different magnitude at neighbouring k.
    # Inside a block e2m1 cannot make them differ by more than 36 / 0.25 = 144:
    # "adjacent_k" has 6·6 at k = 0 against the values · 0.5 at k = 1 …
    ai, bi = np.zeros((16, 128), np.float32), np.zeros((16, 128), np.float32)
    ai[:, 0] = bi[:, 0] = 6
    ai[:, 1] = NONZERO[r % 14]
    bi[:, 1] = 0.5
    add("adjacent_k", ai, bi, one, one, [(0, 0), (5, 6), (13, 2)])
    # … and across a block boundary the scales do what the elements cannot:
    # 2^16 at k = 31 (4·2^6 each) against 2^(14-i-j) at k = 32 (1·2^(7-i), 1·2^(7-j)),
    # gemm8_oracles' adjacent_k moved onto the boundary of blocks 0 and 1
    ai, bi = np.zeros((16, 128), np.float32), np.zeros((16, 128), np.float32)
    ai[:, 31] = bi[:, 31] = 4
    ai[:, 32] = bi[:, 32] = 1
    sa = one.copy()
    sa[:, 0] = 127 + 6
    sa[:, 1] = 127 + 7 - r
    add("adjacent_blocks", ai, bi, sa, sa, [(0, 0), (5, 6), (6, 6), (11, 10), (11, 11), (15, 15)])
    sub = out["subnormal"]["want"][1]
    assert (np.abs(sub) < 2.0 ** -126).all() and (sub != 0).mean() > 0.9
    ss = out["scale_sums"]["want"]
    assert (ss[0][:8, :8] != FINITE).all() and (ss[0][8:] == FINITE).all() and (ss[1][8:, 8:] == 0).all()
    assert (ss[1][:8, 8:] != 0).mean() > 0.9
    assert (out["scale_nan"]["want"][0] == NAN).sum() == 2 * 16 + 14
    return out


# the questions whose IEEE / OCP answer the instruction must give
PROBE_IEEE = ("baseline", "scale_nan", "scale_sums", "subnormal")


def probe_buffers():
    """The problems concatenated for one launch: (names, A, Bt, SA, SB, SEL);
    A / Bt packed bytes, SA / SB one dword per lane as bytes, SEL int32."""
    pr = probe_problems()
    names = list(pr)
    a = np.concatenate([pack_values(pr[n]["a"]).ravel() for n in names])
    b = np.concatenate([pack_values(pr[n]["b"]).ravel() for n in names])
    sa = np.concatenate([_lane_scales(pr[n]["sa"], pr[n]["sel"][0], pr[n]["decoy"]) for n in names])
    sb = np.concatenate([_lane_scales(pr[n]["sb"], pr[n]["sel"][1], pr[n]["decoy"]) for n in names])
    sel = np.array([4 * pr[n]["sel"][0] + pr[n]["sel"][1] for n in names], np.int32)
    return names, a, b, sa, sb, sel


def probe_report(name, c):
    """One line of raw answers for a problem: class counts got / expected,
    finite mismatches and the values at the problem's `show` sites."""
    import gemm_oracles as go

    p = probe_problems()[name]
    cls, expected = p["want"]
    got = go.classify(c)
    fin = (cls == FINITE) & (got == FINITE)
    wrong = int((fin & (np.where(fin, c, 0).astype(np.float64) != expected)).sum())
    counts = lambda x: [int((x == k).sum()) for k in (FINITE, POS_INF, NEG_INF, NAN)]  # noqa: E731
    vals = ", ".join(f"C[{i}][{j}] = {float(c[i, j])!r} (0x{int(c.view(np.uint32)[i, j]):08X})" for i, j in p["show"])
    return (f"probe4 {name}: finite/+inf/-inf/nan got {counts(got)} expected {counts(cls)}, "
            f"{wrong} finite values differ; {vals}")


def measured_k_map(answers, operand):
    """Question 1 read back: for operand "a" (or "b"), the k of the OTHER
    operand that each k position of this one met, as an int array [128]
    (-1: no column of the asymmetric operand matches).  Position k is (lane
    16·(k/32) + row, byte (k % 32)/2, nibble k % 2) under the natural loader."""
    asym = _b_asym().astype(np.float64)
    out = np.full(128, -1)
    for j in range(K_MAP_PROBLEMS):
        c = answers[f"k_map_{operand}{j}"].astype(np.float64)
        for r in range(16):
            vec = c[r, :] if operand == "a" else c[:, r]
            hit = np.flatnonzero((asym == vec[:, None]).all(axis=0))
            if len(hit) == 1:
                out[16 * j + r] = hit[0]
    return out


def measured_scale_map(answers, operand, o):
    """Question 2 read back: the exponent that met each one-hot row's product,
    as (row, block) of the scale byte it names — int arrays [16] each; row -1:
    the exponent is none of the 64 (40 + b: the byte op_sel = b would pick)."""
    p = probe_problems()[f"scale_map_{operand}{o}"]
    c = answers[f"scale_map_{operand}{o}"].astype(np.float64)
    asym = _b_asym().astype(np.float64)
    k = (37 * np.arange(16) + 11) % 128
    unit = asym[:, k].T if operand == "a" else asym[:, k]  # the unit-scale C
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.log2(c / unit)
    e = e if operand == "a" else e.T  # [one-hot row][other]
    assert (e == e[:, :1]).all(), "one exponent per one-hot row"
    e = e[:, 0].astype(np.int64) + 32
    ok = (e >= 0) & (e < 64)
    return np.where(ok, e // 4, -1), np.where(ok, e % 4, e - 32), k // 32
