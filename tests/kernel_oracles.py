"""float64 numpy oracles for the non-GEMM kernel library (mandelbrot, nbody,
reduce, stream), with error bounds derived from the kernels' own arithmetic.

No GPU use: the CPU tier (test_kernel_oracles.py) shows that the comparisons
reject wrong kernels, the GPU tier (test_gpu_kernel_oracles.py) applies the
same comparison functions to what the kernels return.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # float32 unit roundoff

# --------------------------------------------------------------------------- cases
# (shared by both tiers, so the CPU tier validates exactly what the GPU tier runs)

MANDEL_BAND_SHAPES = [(64, 8), (16, 32), (48, 32), (48, 96), (256, 128), (768, 128)]  # (W, H)
MANDEL_QUAD_EXTRA_SHAPES = [(48, 64)]
MANDEL_MAX_ITERS = [1, 5, 8, 9, 12, 16, 17, 31, 32, 33, 40, 63, 64, 65, 100]
MANDEL_VIEWS = [(-2.0, -1.5, 3.0, 3.0), (-0.8, -0.2, 0.4, 0.4), (-0.75, 0.05, 0.1, 0.1)]  # (x0, y0, w, h)
MANDEL_MAX_UNDECIDABLE = 0.04


def mandel_quad_shapes():
    """The shapes the 4-pixel kernel's size rule (W·H a multiple of 1024) admits."""
    return [s for s in MANDEL_BAND_SHAPES + MANDEL_QUAD_EXTRA_SHAPES if (s[0] * s[1]) % 1024 == 0]


def mandel_view_f32(view, W, H) -> np.ndarray:
    """{x0, y0, dx, dy} in float32, as MandelbrotRenderer stores it."""
    x0, y0, w, h = view
    return np.array([x0, y0, w / W, h / H], np.float32)


# --------------------------------------------------------------------------- mandelbrot

def mandelbrot_orbits(view_f32, W, H, max_iter):
    """float64 orbits of every pixel with the float32 error radius carried
    along.  Returns (esc, und): esc[p] is the first k < max_iter with
    |z_k|² > 4 (max_iter if none), und[p] the first k <= esc[p] at which the
    escape test of a float32 kernel is not determined (max_iter if none).

    e_k bounds |z_k(float32) − z_k(float64)| to first order:
        e_{k+1} = 2|z_k|·e_k + e_k² + 8u·(|z_k|² + |c|) + 2^-20
    (8u: at most 3 roundings per component of z² + c, fused or not; 2^-20: c
    built as x0 + col·dx (+ dx) in float32, |c| < 4).  The test at k is
    undetermined when
        | |z_k|² − 4 | <= 2|z_k|·e_k + e_k² + 4u·|z_k|² + 2^-19
    (4u: the roundings of |z|² itself; 2^-19: the packed clamp count's 2^-20
    band below 4) or when e_k is no longer finite.
    """
    x0, y0, dx, dy = (float(np.float32(v)) for v in view_f32)
    cr = np.broadcast_to(x0 + np.arange(W, dtype=np.float64) * dx, (H, W)).copy()
    ci = np.broadcast_to((y0 + np.arange(H, dtype=np.float64) * dy)[:, None], (H, W)).copy()
    cabs = np.hypot(cr, ci)
    zr = np.zeros((H, W))
    zi = np.zeros((H, W))
    e = np.zeros((H, W))
    esc = np.full((H, W), max_iter, np.int64)
    und = np.full((H, W), max_iter, np.int64)
    active = np.ones((H, W), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(max_iter):
            m = zr * zr + zi * zi
            za = np.sqrt(m)
            rad = 2 * za * e + e * e + 4 * U * m + 2.0 ** -19
            doubt = active & (und == max_iter) & ~(np.abs(m - 4) > rad)  # NaN/inf radius: in doubt
            und[doubt] = k
            out = active & (m > 4)
            esc[out] = k
            active &= ~out
            if not active.any():
                break
            e_next = 2 * za * e + e * e + 8 * U * (m + cabs) + 2.0 ** -20
            zr_next = zr * zr - zi * zi + cr
            zi_next = 2 * zr * zi + ci
            zr = np.where(active, zr_next, zr)
            zi = np.where(active, zi_next, zi)
            e = np.where(active, e_next, e)
    return esc, und


def mandelbrot_from_orbits(esc, und, max_iter):
    """(n, decidable) for `max_iter` from orbits run at least that far.  A
    kernel tests |z_k|² for k < max_iter only, and a pixel's count is settled
    at its escape."""
    n = np.minimum(esc, max_iter).astype(np.int32)
    decidable = und > np.minimum(esc, max_iter - 1)
    return n, decidable


def mandelbrot_oracle(view_f32, W, H, max_iter):
    """(n, decidable): the escape count of every pixel and whether any correct
    float32 kernel must return exactly that count."""
    esc, und = mandelbrot_orbits(view_f32, W, H, max_iter)
    return mandelbrot_from_orbits(esc, und, max_iter)


def check_mandelbrot(img, n, decidable, max_iter, max_undecidable=MANDEL_MAX_UNDECIDABLE) -> None:
    """The comparison both tiers use: every count within [0, max_iter], the
    undecidable share small enough for the comparison to mean something, and
    exact equality on every decidable pixel."""
    img = np.asarray(img)
    assert img.shape == n.shape, (img.shape, n.shape)
    lo, hi = int(img.min()), int(img.max())
    assert 0 <= lo and hi <= max_iter, f"counts outside [0, {max_iter}]: min {lo}, max {hi}"
    share = 1.0 - float(decidable.mean())
    assert share <= max_undecidable, f"undecidable share {share:.4f} > {max_undecidable}"
    bad = decidable & (img != n)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{int(bad.sum())} decidable pixels differ (max_iter {max_iter}); first at row {r}, "
                             f"col {c}: got {int(img[r, c])}, oracle {int(n[r, c])}")


def mandelbrot_f32_fused(view_f32, W, H, max_iter) -> np.ndarray:
    """A second float32 emulation, with the fused forms the block kernels use:
    every a·b + c goes through float64 and is rounded once."""
    f32, f64 = np.float32, np.float64
    x0, y0, dx, dy = (f64(np.float32(v)) for v in view_f32)
    cr = np.broadcast_to((x0 + np.arange(W, dtype=f64) * dx).astype(f32), (H, W)).astype(f64)
    ci = np.broadcast_to((y0 + np.arange(H, dtype=f64) * dy).astype(f32)[:, None], (H, W)).astype(f64)
    zr = np.zeros((H, W))  # float32 values held in float64
    zi = np.zeros((H, W))
    n = np.full((H, W), max_iter, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(max_iter):
            zi2 = (zi * zi).astype(f32).astype(f64)
            m = (zr * zr + zi2).astype(f32)
            n[(m > 4) & (n == max_iter)] = k
            t = (zr * zi).astype(f32).astype(f64)
            a = (zr * zr + cr).astype(f32).astype(f64)
            zr_next = (a - zi * zi).astype(f32).astype(f64)
            zi = (2 * t + ci).astype(f32).astype(f64)
            zr = zr_next
    return n


# --------------------------------------------------------------------------- n-body

NBODY_G = 6.5
NBODY_EPS = 0.01
NBODY_DT = 1e-3
NBODY_SIZES = [(2, 512), (2, 768), (2, 1024), (4, 1024), (4, 2048)]  # (bodies per work item, n)
NBODY_TERM_ROUNDINGS = 32  # per-term roundings (about 18), rounded up


def nbody_bodies(n, kind="normal", seed=0) -> np.ndarray:
    """(n, 4) float32 {x, y, z, m}: standard normal positions, masses
    log-uniform over three decades with a few exactly 0.  kind "shifted":
    +100 in x (cancellation in d); "coincident": two bodies at one place."""
    rng = np.random.default_rng(seed)
    pos = np.empty((n, 4), np.float32)
    pos[:, :3] = rng.standard_normal((n, 3)).astype(np.float32)
    pos[:, 3] = (10.0 ** rng.uniform(-3, 0, n)).astype(np.float32)
    pos[rng.choice(n, 5, replace=False), 3] = 0.0
    if kind == "shifted":
        pos[:, 0] += np.float32(100.0)
    elif kind == "coincident":
        pos[n - 3, :3] = pos[7, :3]
        pos[n - 3, 3] = pos[7, 3] = 1.0
    elif kind != "normal":
        raise ValueError(kind)
    return pos


def nbody_accel_oracle(pos, eps2, G, chunk=256):
    """(a, S): the float64 all-pairs acceleration a_i = G Σ_j m_j d_ij r^-3,
    d_ij = x_j − x_i, r² = |d_ij|² + eps2, and S, the per-body per-component
    sum of the terms' magnitudes G Σ_j m_j |d_ij| r^-3."""
    p = np.asarray(pos).reshape(-1, 4).astype(np.float64)
    a = np.zeros((len(p), 3))
    S = np.zeros((len(p), 3))
    for s in range(0, len(p), chunk):
        d = p[None, :, :3] - p[s:s + chunk, None, :3]
        r2 = (d * d).sum(-1) + float(eps2)
        t = d * (p[None, :, 3] * r2 ** -1.5)[..., None]
        a[s:s + chunk] = float(G) * t.sum(1)
        S[s:s + chunk] = abs(float(G)) * np.abs(t).sum(1)
    return a, S


def nbody_accel_bound(S, n):
    """|a_kernel − a| per body and component, first order: sequential float32
    accumulation of n terms gives (n − 1)u, each term carries at most about
    18u (one rounding in d, three fmas in r², a 1-ulp reciprocal square root
    cubed, three multiplies), rounded up to 32."""
    return (n + NBODY_TERM_ROUNDINGS) * U * S


def ulp32(x):
    """float32 spacing at |x|."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def leapfrog_oracle(pos, vel, acc, dt, v_kernel=None):
    """(x', v') in float64: v' = a·dt + v, x' = v'·dt + x.  With `v_kernel`
    (the kernel's own float32 v') x' is evaluated on that, which is what a
    kernel that uses fmaf must match to 1 ulp."""
    p = np.asarray(pos).reshape(-1, 4).astype(np.float64)
    v = np.asarray(vel).reshape(-1, 4).astype(np.float64)
    a = np.asarray(acc).reshape(-1, 4).astype(np.float64)
    v1 = a[:, :3] * float(dt) + v[:, :3]
    vk = v1 if v_kernel is None else np.asarray(v_kernel).reshape(-1, 4).astype(np.float64)[:, :3]
    x1 = vk * float(dt) + p[:, :3]
    return x1, v1


def kinetic_terms(pos, vel) -> np.ndarray:
    """½·m·|v|² per body, float64."""
    p = np.asarray(pos).reshape(-1, 4).astype(np.float64)
    v = np.asarray(vel).reshape(-1, 4).astype(np.float64)
    return 0.5 * p[:, 3] * (v[:, :3] ** 2).sum(1)


# --------------------------------------------------------------------------- reduce

# the longest chain of float32 additions an element passes through
REDUCE_DEPTH = {"cek_reduce_sum_f32": 14,       # 4 in the lane, 6 shuffle levels, 4 across waves
                "cek_reduce_sum_f32_x32": 20}


def reduce_final_depth(n) -> int:
    return -(-n // 256) + 10


def energy_depth(bodies_per_item) -> int:
    return bodies_per_item + 4 + 6 + 3


def block_sums_oracle(x, block):
    """(sums, abs_sums) per block of `block` elements, float64."""
    b = np.asarray(x).astype(np.float64).reshape(-1, block)
    return b.sum(1), np.abs(b).sum(1)


def block_sum_bound(abs_sums, depth):
    return depth * U * abs_sums


def check_bound(got, ref, bound, what=""):
    """Asserts |got − ref| <= bound element by element; returns the largest
    err / bound over the elements with a non-zero bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(ref), (got.shape, np.shape(ref))
    assert np.isfinite(got).all(), f"{what}: non-finite values at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - ref)
    bad = err > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound; first at {i}: "
                             f"got {got[i]!r}, oracle {np.asarray(ref)[i]!r}, err {err[i]:.3e}, bound "
                             f"{np.asarray(bound)[i]:.3e}")
    nz = np.asarray(bound) > 0
    return float((err[nz] / np.asarray(bound)[nz]).max()) if nz.any() else 0.0


def reduce_data(groups, block, seed=0) -> np.ndarray:
    """Signed float32 data over six decades plus a per-block offset, so every
    block sum is distinct."""
    rng = np.random.default_rng(seed)
    x = rng.choice([-1.0, 1.0], groups * block) * 10.0 ** rng.uniform(-3, 3, groups * block)
    x = x.reshape(groups, block) + (np.arange(groups)[:, None] + 1) * 7.0
    return x.astype(np.float32).reshape(-1)
