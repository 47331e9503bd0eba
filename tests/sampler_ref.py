"""The bilinear sampler of csrc/sampler.hip (bilinear_fwd_k, bilinear_bwd_det_k, bilinear_bwd_k) restated in fp64 numpy, with the
magnitude sums the per-element rounding bounds of tests/test_gpu_sampler_edges.py need, and its host dispatch (sampler_forward /
sampler_backward) restated as sampler_plan().  A plain module, imported as tests/locnet_ref.py is.

Taps.  The cell (y0, x0) and the weights (wy0, wx0) of a sample are computed AS THE KERNEL DOES, in fp32 (bilin_taps):
    xc = (xf + 1) * (Wi - 1) * 0.5,  x0 = floor(xc),  wx0 = 1 - (xc - x0)
No product here feeds a sum, so nothing can be contracted into an fma and numpy's fp32 reproduces the device's cell: ggrid is
discontinuous across cells, and a reference that picked the neighbouring cell for a coordinate within an ulp of a boundary would be
compared with the wrong branch.  Everything after the taps - the four weights' products, the sums - is fp64 on those fp32 values.
taps="f64" does the tap arithmetic in fp64 too (tests/test_sampler_ref_host.py compares that form with torch's grid_sample).

Layout: img [Nimg][Hi][Wi][C], grid [N][Ho][Wo][2] as (y, x) in [-1, 1] (align_corners), out / gout [N][Ho][Wo][C],
gimg [N][Hi][Wi][C], ggrid like grid.  Sample n reads image n % Nimg (the shared form); gimg stays per sample."""
import numpy as np

f32, f64 = np.float32, np.float64

# the constants of the host dispatch; tests/test_sampler_ref_host.py reads every one of them out of common.h / sampler.hip
NUM_CU = 256                 # common.h kNumCU
EW_WGS_PER_CU = 4            # common.h kEwWgsPerCU (cg::ew_grid's cap)
DET_LDS_LIMIT = 140 * 1024   # sampler_backward: `shb <= 140 * 1024`
DET_MAX_C = 256              # sampler_backward: `C <= 256`
HEAVY = 64                   # bilinear_bwd_det_k: kHeavy
ATOMIC_BLOCKS_PER_CU = 8     # sampler_backward: `blocks > cg::kNumCU * 8`


def bilin_taps(grid, Hi, Wi, taps="f32"):
    """-> y0, x0 (int64, clipped to [-2, size]: every clipped value is as far outside as the original), wy0, wx0 (fp64 holding the
    fp32 values unless taps == "f64"), and the four in-image flags in the kernel's order 00, 01, 10, 11 (y, then x)."""
    ft = f32 if taps == "f32" else f64
    g = np.asarray(grid).astype(ft)
    yf, xf = g[..., 0], g[..., 1]
    xc = (xf + ft(1)) * ft(Wi - 1) * ft(0.5)
    yc = (yf + ft(1)) * ft(Hi - 1) * ft(0.5)
    x0f, y0f = np.floor(xc), np.floor(yc)
    wx0 = ft(1) - (xc - x0f)
    wy0 = ft(1) - (yc - y0f)
    assert wx0.dtype == ft and wy0.dtype == ft
    x0 = np.clip(x0f, -2, Wi).astype(np.int64)          # numpy's cast of 1e30 is undefined; the device's saturates: outside either way
    y0 = np.clip(y0f, -2, Hi).astype(np.int64)
    xin0, xin1 = (x0 >= 0) & (x0 <= Wi - 1), (x0 + 1 >= 0) & (x0 + 1 <= Wi - 1)
    yin0, yin1 = (y0 >= 0) & (y0 <= Hi - 1), (y0 + 1 >= 0) & (y0 + 1 <= Hi - 1)
    return y0, x0, wy0.astype(f64), wx0.astype(f64), (yin0 & xin0, yin0 & xin1, yin1 & xin0, yin1 & xin1)


def _tap_list(grid, Hi, Wi, taps):
    """The four taps of every output pixel: (dy, dx, in flag, weight) with the weight's factors ordered as the kernels write them."""
    y0, x0, wy0, wx0, ins = bilin_taps(grid, Hi, Wi, taps)
    w = (wx0 * wy0, (1.0 - wx0) * wy0, wx0 * (1.0 - wy0), (1.0 - wx0) * (1.0 - wy0))
    return y0, x0, wy0, wx0, [(dy, dx, ins[2 * dy + dx], w[2 * dy + dx]) for dy in (0, 1) for dx in (0, 1)]


def _gather(img, n_img, yy, xx, ok):
    """img[n_img, yy, xx, :] where ok, zeros elsewhere (the indices are made valid first: no address from an outside cell)."""
    v = img[n_img, np.where(ok, yy, 0), np.where(ok, xx, 0)]
    return np.where(ok[..., None], v, 0.0)


def forward(img, grid, taps="f32"):
    """-> out, terms = sum over the taps of |w img| per element."""
    img = np.asarray(img, f64)
    Nimg, Hi, Wi, C = img.shape
    N = grid.shape[0]
    y0, x0, _, _, tl = _tap_list(grid, Hi, Wi, taps)
    n_img = (np.arange(N) % Nimg)[:, None, None]
    out = np.zeros(grid.shape[:3] + (C,), f64)
    terms = np.zeros_like(out)
    for dy, dx, ok, w in tl:
        v = _gather(img, n_img, y0 + dy, x0 + dx, ok) * w[..., None]
        out += v
        terms += np.abs(v)
    return out, terms


def backward(img, grid, gout, taps="f32"):
    """-> dict(gimg, gimg_terms = sum |w gout| per element, taps = the number of taps that land on each source pixel [N][Hi][Wi],
    ggrid, ggrid_terms = per pixel and component the sum of |coefficient| sum_c |img gout| over the four taps, scaled as ggrid is)."""
    img, gout = np.asarray(img, f64), np.asarray(gout, f64)
    Nimg, Hi, Wi, C = img.shape
    N, Ho, Wo, _ = grid.shape
    assert gout.shape == (N, Ho, Wo, C)
    y0, x0, wy0, wx0, tl = _tap_list(grid, Hi, Wi, taps)
    n_img = (np.arange(N) % Nimg)[:, None, None]
    n_own = np.broadcast_to(np.arange(N)[:, None, None], y0.shape)
    gimg = np.zeros((N * Hi * Wi, C), f64)
    gterms = np.zeros_like(gimg)
    count = np.zeros(N * Hi * Wi, np.int64)
    d, da = {}, {}
    for dy, dx, ok, w in tl:
        q = ((n_own * Hi + np.where(ok, y0 + dy, 0)) * Wi + np.where(ok, x0 + dx, 0))[ok]
        v = (w[..., None] * gout)[ok]
        np.add.at(gimg, q, v)
        np.add.at(gterms, q, np.abs(v))
        np.add.at(count, q, 1)
        prod = _gather(img, n_img, y0 + dy, x0 + dx, ok) * gout
        d[dy, dx], da[dy, dx] = prod.sum(-1), np.abs(prod).sum(-1)
    # bilinear_bwd_det_k / bilinear_bwd_k:  gy = -wx0 d00 + wx0 d10 - (1 - wx0) d01 + (1 - wx0) d11, times (Hi - 1) / 2
    #                                       gx = -wy0 d00 + wy0 d01 - (1 - wy0) d10 + (1 - wy0) d11, times (Wi - 1) / 2
    gy = -wx0 * d[0, 0] + wx0 * d[1, 0] - (1.0 - wx0) * d[0, 1] + (1.0 - wx0) * d[1, 1]
    gx = -wy0 * d[0, 0] + wy0 * d[0, 1] - (1.0 - wy0) * d[1, 0] + (1.0 - wy0) * d[1, 1]
    ty = np.abs(wx0) * (da[0, 0] + da[1, 0]) + np.abs(1.0 - wx0) * (da[0, 1] + da[1, 1])
    tx = np.abs(wy0) * (da[0, 0] + da[0, 1]) + np.abs(1.0 - wy0) * (da[1, 0] + da[1, 1])
    sy, sx = (Hi - 1) * 0.5, (Wi - 1) * 0.5
    return dict(gimg=gimg.reshape(N, Hi, Wi, C), gimg_terms=gterms.reshape(N, Hi, Wi, C), taps=count.reshape(N, Hi, Wi),
                ggrid=np.stack([gy * sy, gx * sx], -1), ggrid_terms=np.stack([ty * sy, tx * sx], -1))


def heavy_pixels(grid, Hi, Wi):
    """The tap total of every source pixel as bilinear_bwd_det_k counts it: the sizes of the four buckets (y0, x0) = (y - 1, x - 1),
    (y - 1, x), (y, x - 1), (y, x), from the fp32 taps -> [N][Hi][Wi].  More than HEAVY: the whole workgroup sums that pixel."""
    y0, x0, _, _, _ = bilin_taps(grid, Hi, Wi)
    N = grid.shape[0]
    CW = Wi + 1
    placed = (y0 >= -1) & (y0 <= Hi - 1) & (x0 >= -1) & (x0 <= Wi - 1)
    n = np.broadcast_to(np.arange(N)[:, None, None], y0.shape)
    cnt = np.zeros((N, Hi + 1, CW), np.int64)                 # bucket (y0 + 1, x0 + 1)
    np.add.at(cnt, (n[placed], y0[placed] + 1, x0[placed] + 1), 1)
    return cnt[:, :-1, :-1] + cnt[:, :-1, 1:] + cnt[:, 1:, :-1] + cnt[:, 1:, 1:]


def _cdiv(a, b):
    return -(-a // b)


def _ew(n):
    """cg::ew_grid and the regime of the launch: one workgroup, many without a wrap, or a grid-stride wrap behind the cap."""
    cap = NUM_CU * EW_WGS_PER_CU
    blocks = max(1, min(_cdiv(n, 256), cap))
    return blocks, ("wrap" if n > blocks * 256 else ("many" if blocks > 1 else "one"))


def sampler_plan(N, Nimg, Hi, Wi, C, Ho, Wo, aligned, grid_aligned=None):
    """sampler.hip sampler_forward / sampler_backward for N samples on Nimg images.  aligned: img, out, gout and gimg sit on 16-byte
    boundaries; grid_aligned: the grid on an 8-byte one (default: as the tensors).  -> dict(forward=..., backward=...)."""
    grid_aligned = aligned if grid_aligned is None else grid_aligned
    P, Q = Ho * Wo, Hi * Wi
    total = N * P * C
    v4f = C % 4 == 0 and aligned and grid_aligned
    blocks, regime = _ew(total // 4 if v4f else total)
    fwd = dict(kernel="bilinear_fwd_k<4>" if v4f else "bilinear_fwd_k<1>", blocks=blocks, ew=regime)
    shb = (6 * P + 2 * (Hi + 1) * (Wi + 1) + 1) * 4
    if shb <= DET_LDS_LIMIT and C <= DET_MAX_C:
        v4 = C % 4 == 0 and aligned
        units = C // 4 if v4 else C
        G = 4
        while G < 64 and G < units:
            G <<= 1
        want = max(1, min(16, NUM_CU * 4 // max(1, N)))
        S = max(max(32, 256 // G), _cdiv(max(P, Q), want))
        nchunks = _cdiv(max(P, Q), S)
        CACC = 1 if (v4 or C <= 64) else (2 if C <= 128 else 4)
        VW = 4 if v4 else 1
        assert G * CACC * VW >= C, "every channel has a lane"
        bwd = dict(path="det", v4=v4, G=G, CACC=CACC, want=want, S=S, nchunks=nchunks, ngrp=256 // G, blocks=N * nchunks,
                   lds=shb + 4 * (256 + 4 + 256 * CACC * VW),            # dynamic + part[256], wtot[4], coop[256 CACC VW]
                   idle_lanes=G * CACC * VW > C, ragged=nchunks * S != max(P, Q))
    else:
        G = 4
        while G < 64 and G < C:
            G <<= 1
        npix = N * P
        blocks = max(1, min(_cdiv(npix * G, 256), NUM_CU * ATOMIC_BLOCKS_PER_CU))
        bwd = dict(path="atomic", why="C" if C > DET_MAX_C else "lds", G=G, blocks=blocks, wraps=npix > blocks * 256 // G, lds=shb)
    return dict(forward=fwd, backward=bwd)


def describe(plan):
    """A plan as the one line a case table states: every number that names a regime of the kernels."""
    f, b = plan["forward"], plan["backward"]
    if b["path"] == "det":
        s = (f"det {'v4' if b['v4'] else 'scalar'} G={b['G']} CACC={b['CACC']}{' idle-lanes' if b['idle_lanes'] else ''} want={b['want']} "
             f"S={b['S']} chunks={b['nchunks']}{' ragged' if b['ragged'] else ''} ngrp={b['ngrp']} lds={b['lds']}")
    else:
        s = f"atomic({b['why']}) G={b['G']} blocks={b['blocks']}{' wraps' if b['wraps'] else ''}"
    return s + f" | {f['kernel']} {f['ew']}"
