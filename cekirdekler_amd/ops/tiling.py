"""The layouts the GEMM kernels write and read, as numpy index arithmetic: C
tiles in fragment order, the tile orders (grouped rows, square shells) and
the packed E8M0 scale dwords of the MX kernels."""
from __future__ import annotations

import numpy as np


def tile_to_rows(t: np.ndarray, geom) -> np.ndarray:
    """Fragment-ordered C tiles (``[..., BM·BN]``) → row-major ``[..., BM, BN]``.
    In-tile offset of (row, col) = ((((wr·WN + wc)·FM + i)·FN + j)·64 + fq·16 + fr)·4 + r
    with row = wr·16FM + i·16 + fq·4 + r and col = wc·16FN + j·16 + fr."""
    WM, WN, FM, FN = geom
    lead = t.shape[:-1]
    x = t.reshape(lead + (WM, WN, FM, FN, 4, 16, 4))
    n = len(lead)
    perm = list(range(n)) + [n + 0, n + 2, n + 4, n + 6, n + 1, n + 3, n + 5]
    return x.transpose(perm).reshape(lead + (WM * FM * 16, WN * FN * 16))


def rows_to_tile(b: np.ndarray, geom) -> np.ndarray:
    """Inverse of :func:`tile_to_rows`: row-major ``[..., BM, BN]`` → fragment order."""
    WM, WN, FM, FN = geom
    lead = b.shape[:-2]
    x = b.reshape(lead + (WM, FM, 4, 4, WN, FN, 16))  # wr i fq r wc j fr
    n = len(lead)
    perm = list(range(n)) + [n + 0, n + 4, n + 1, n + 5, n + 2, n + 6, n + 3]
    return np.ascontiguousarray(x.transpose(perm)).reshape(lead + (-1,))


def tile_coords(t: np.ndarray, M: int, N: int, BM: int, BN: int, group_m: int, panels: int = 0):
    """Tile index → (tile row, tile col) under the kernel's order
    (``cek_tile_coords`` in kernels/cek_kernel.h): grouped rows, or square
    shells of ``panels`` row panels (shell s = R_s then C_s)."""
    t = np.asarray(t)
    ntm, ntn = M // BM, N // BN

    def grouped(r, rows, cols):
        gm = max(1, group_m)
        per = gm * cols
        first = (r // per) * gm
        gsz = np.minimum(rows - first, gm)
        in_g = r % per
        return first + in_g % gsz, in_g // gsz

    if panels <= 0:
        return grouped(t, ntm, ntn)
    pm, pn = ntm // panels, ntn // panels
    tm = np.empty_like(t)
    tn = np.empty_like(t)
    s = np.floor(np.sqrt(t // (pm * pn))).astype(np.int64)
    s = np.where((s + 1) ** 2 * pm * pn <= t, s + 1, s)
    s = np.where(s * s * pm * pn > t, s - 1, s)
    r = t - s * s * pm * pn
    r_tiles = pm * (s + 1) * pn
    for sh in np.unique(s):
        sel = s == sh
        rr = r[sel]
        isr = rr < r_tiles[sel]
        a, b = grouped(rr[isr], pm, (sh + 1) * pn)
        c, d = grouped(rr[~isr] - pm * (sh + 1) * pn, max(sh * pm, 1), pn)
        out_m = np.empty(rr.shape, t.dtype)
        out_n = np.empty(rr.shape, t.dtype)
        out_m[isr], out_n[isr] = a + sh * pm, b
        out_m[~isr], out_n[~isr] = c, d + sh * pn
        tm[sel], tn[sel] = out_m, out_n
    return tm, tn


def untile(c: np.ndarray, M: int, N: int, BM: int, BN: int, group_m: int = 1, geom=None,
           panels: int = 0) -> np.ndarray:
    """Tile-major C (the kernel's tile order) → row-major [M][N]; ``geom``:
    the tile's wave geometry when its elements are in fragment order (bf16
    kernels), None for row-major tiles; ``panels``: shell order."""
    ntm, ntn = M // BM, N // BN
    tiles = c.reshape(ntm * ntn, BM, BN) if geom is None else tile_to_rows(c.reshape(ntm * ntn, BM * BN), geom)
    tm, tn = tile_coords(np.arange(ntm * ntn), M, N, BM, BN, group_m, panels)
    out = np.empty((ntm, ntn, BM, BN), c.dtype)
    out[tm, tn] = tiles
    return out.transpose(0, 2, 1, 3).reshape(M, N)


def pack_mx_scales(s: np.ndarray) -> np.ndarray:
    """Row-major scale bytes ``[R][K/32]`` → the kernels' packed dwords
    (kernels/sgemm_mxfp8.hip): uint32 ``[K/128][R/64][64]``, byte ``i`` of
    dword ``(kt·R/64 + g)·64 + l`` = ``s[g·64 + i·16 + l % 16][kt·4 + l // 16]``.
    R % 64 = 0 and (K/32) % 4 = 0."""
    s = np.asarray(s, np.uint8)
    R, nb = s.shape
    if R % 64 or nb % 4:
        raise ValueError(f"rows % 64 and blocks % 4 must be 0 (got {R}, {nb})")
    x = s.reshape(R // 64, 4, 16, nb // 4, 4)  # g i fr kt fq
    return np.ascontiguousarray(x.transpose(3, 0, 4, 2, 1)).view("<u4").reshape(nb // 4, R // 64, 64)  # kt g fq fr [i]


def unpack_mx_scales(p: np.ndarray) -> np.ndarray:
    """Inverse of :func:`pack_mx_scales`: uint32 ``[K/128][R/64][64]`` → uint8 ``[R][K/32]``."""
    p = np.ascontiguousarray(p, dtype="<u4")
    KT, G, _ = p.shape
    x = p.view(np.uint8).reshape(KT, G, 4, 16, 4)  # kt g fq fr i
    return np.ascontiguousarray(x.transpose(1, 4, 3, 0, 2)).reshape(G * 64, KT * 4)  # g i fr kt fq
