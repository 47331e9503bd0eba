// What the two staging families of a GEMM in gemm.hip (register staging: igemm_nn_kernel / igemm_tn_kernel, LDS-direct loads:
// igemm_nng_kernel / igemm_tng_kernel) have in common in front of and inside the K loop, written once:
//   the tile order         nn_tile_order / tn_tile_order: (blockIdx, gridDim, xcd_swizzle) -> (row tile, column tile, split)
//   the NN gather state    NNGather: row decode, 64-bit tap-validity masks, the tap walk (start at a K offset, advance by one K tile; the
//                          position-major walk over the valid taps only is its compile-time variant), weight offsets, descriptors
//   the TN addressing      tn_col_decode, tn_lean_geom (the geometry rule, host and device), tn_lean_a / tn_lean_b (loop invariants),
//                          tn_tile_bases (the wave-uniform bases of one K tile)
//   the loop               k_loop2 (two K tiles per trip, compile-time LDS buffer index), mfma_k_major (K-major fragments, swizzled A or
//                          plain); the accumulators start as `f32x16 acc[MI][NI] = {}` - no zeroing loop anywhere
// Included by gemm.hip alone, inside its anonymous namespace, behind Geom, tap_decode, pix_decode and a_swizzle.  Per-lane arrays are
// handed over by reference to arrays of compile-time extent and never indexed at run time (that would put them in scratch); pointers and
// scalars of the kernel arguments come by value.  Two shapes here are the ones that kept every kernel's register allocation at or below
// the hand-inlined code's (profiles/gemm_prologue_resources.txt): decode_row takes ONE row and the kernels loop, and tn_lean_b adds the
// column as rel + n0 + 4 * b_nv, in that association.
#pragma once

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const float* base) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
}

// ---- tile order -------------------------------------------------------------------------------------------------------------------
struct TileIdx { int tm, tn, split; };

// contiguous ranges per XCD: workgroup b is dispatched to XCD b % 8 (each XCD has its own L2), so hand every XCD a CONTIGUOUS range of
// tiles - neighbours then share their A rows / B columns through one L2 instead of eight
__device__ __forceinline__ int xcd_ranges(int bid) { return (bid & 7) * ((int)gridDim.x >> 3) + (bid >> 3); }

// NN: row ranges per XCD (xcd_swizzle bit 1) or, STATIONARY kernels only, weights-stationary XCDs (bit 4).  NATURAL: neither - the
// position-major kernel, where consecutive tiles on consecutive XCDs spread the short border positions and the long centre ones evenly
// over the XCDs (contiguous ranges would give one XCD the top row of the image and another the middle).
template <bool STATIONARY, bool NATURAL>
__device__ __forceinline__ TileIdx nn_tile_order(int ntn, int xcd_swizzle) {
    int bid = blockIdx.x;
    int tn, tm;
    const int tiles_m = (int)gridDim.x / ntn, xg = ntn <= 8 ? 8 / ntn : 0;       // xg: XCDs per column tile
    if (STATIONARY && !NATURAL && (xcd_swizzle & 4) && (ntn == 2 || ntn == 4 || ntn == 8) && (gridDim.x & 7) == 0 && tiles_m % xg == 0) {
        // WEIGHTS-stationary XCDs (round 5): XCD k = bid % 8 owns column tile k % ntn and one of 8 / ntn row ranges, so its
        // L2 holds ONE [Ktot x BN] slice of the (phase) kernel - 1 MB for conv1's forward, where the row-range order below made all eight
        // XCDs fetch all four column slices: 8 x 16.8 MB of kernels per launch against 4 x 4.2 MB of input now (r x c XCD grid over
        // rows x columns: traffic = c * |x| + r * |w|)
        const int k = bid & 7, j = bid >> 3;
        tn = k % ntn;
        tm = (k / ntn) * (tiles_m / xg) + j;
    } else {
        if (!NATURAL && (xcd_swizzle & 1) && (gridDim.x & 7) == 0) bid = xcd_ranges(bid);
        tn = ntn == 1 ? 0 : bid % ntn; tm = ntn == 1 ? bid : bid / ntn;
    }
    return {tm, tn, (int)blockIdx.y};
}

// TN: pixel-chunk XCDs (bit 2), else row ranges (bit 1)
__device__ __forceinline__ TileIdx tn_tile_order(int ntn, int xcd_swizzle) {
    int bid = blockIdx.x, split = blockIdx.y;
    if ((xcd_swizzle & 2) && (gridDim.y & 7) == 0) {
        // XCD = pixel chunk: workgroup L of the dispatch order (x fastest, then y) runs on XCD L % 8; give every XCD the splits
        // congruent to its number, for all tiles - it then reads one eighth of x and dy (each pixel chunk is wanted by every
        // tile), instead of every XCD reading all of dy for its few tiles
        const int L = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x, s8 = (int)gridDim.y >> 3;
        split = (L & 7) + 8 * ((L >> 3) % s8);
        bid = (L >> 3) / s8;
    } else if ((xcd_swizzle & 1) && (gridDim.x & 7) == 0) {
        bid = xcd_ranges(bid);
    }
    return {ntn == 1 ? bid : bid / ntn, ntn == 1 ? 0 : bid % ntn, split};
}

// ---- NN gather state --------------------------------------------------------------------------------------------------------------
// The FAST gather of a BM x BKT tile of A and a BKT x BN tile of the weights: a thread owns quad position a_kv of rows a_r + ARPP p and
// quad b_nv of weight rows b_kr + BRPP q.  (tapi, ci0, toff) describe the NEXT K tile: tap index, first channel, element offset of the tap;
// all of it lives in SGPRs.  PM (position-major rows, Geom::pmn): every row of the tile has the same mask and the walk visits its valid
// taps only.
template <int BM, int BN, int BKT, bool PM>
struct NNGather {
    static constexpr int KV = BKT / 4;        // quads per A row
    static constexpr int ARPP = 256 / KV;     // A rows per pass of the workgroup
    static constexpr int AROWS = BM / ARPP;   // quads per thread per tile (A)
    static_assert(BM % ARPP == 0 && AROWS >= 1, "BM multiple of rows-per-pass");
    static constexpr int NVEC = BN / 4;
    static constexpr int BRPP = 256 / NVEC;   // B rows per pass
    static constexpr int BPASS = (BKT + BRPP - 1) / BRPP;

    unsigned long long cur[AROWS];     // tap-validity mask of each row, shifted so bit 0 = next tile's tap
    unsigned long long um;             // PM: the tile's tap-validity mask (unshifted, wave-uniform)
    unsigned rowbytes[AROWS];
    unsigned bvoff[BPASS];
    int tapi, ci0, toff, minoff;
    __amdgpu_buffer_rsrc_t rsx, rsw;

    // row m of the tile -> its pixel (oy, ox), validity and element offset in the source tensor (PM: pos_u = the tile's pixel position)
    static __device__ __forceinline__ void decode_row(const Geom& g, int m, int pos_u, int& rowb, int& r_oy, int& r_ox, bool& r_ok) {
        r_ok = m < g.M;
        int n;
        if (PM) {
            n = m & (g.pmn - 1);
            r_oy = g.lgW >= 0 ? pos_u >> g.lgW : pos_u / g.Wg;
            r_ox = pos_u - r_oy * g.Wg;
        } else pix_decode(g, r_ok ? m : 0, n, r_oy, r_ox);
        rowb = ((n * g.Hs + r_oy * g.td.ss) * g.Ws + r_ox * g.td.ss) * g.Cin;
    }

    // cur[p] bit t = tap t of this launch reads inside the image at row p
    __device__ __forceinline__ void tap_masks(const Geom& g, int pa, int pb, const int (&r_oy)[AROWS], const int (&r_ox)[AROWS],
                                              const bool (&r_ok)[AROWS]) {
        const TapDesc& d = g.td;
        const int kh = d.kk / d.kw;
#pragma unroll
        for (int p = 0; p < AROWS; ++p) cur[p] = 0ull;
        for (int grp = 0; grp < d.ngroups; ++grp) {
            int ga = pa, gb = pb;
            if (d.ngroups > 1) { ga = grp >> 1; gb = grp & 1; }
            unsigned xb[AROWS];
#pragma unroll
            for (int p = 0; p < AROWS; ++p) xb[p] = 0u;
            for (int rx = 0; rx < d.kw; ++rx) {
                const int tx = d.sgn * ((gb ? d.r0x1 : d.r0x0) + rx);
#pragma unroll
                for (int p = 0; p < AROWS; ++p)
                    xb[p] |= ((unsigned)(r_ox[p] + tx) < (unsigned)g.Wv ? 1u : 0u) << rx;
            }
            for (int ry = 0; ry < kh; ++ry) {
                const int ty = d.sgn * ((ga ? d.r0y1 : d.r0y0) + ry);
                const int sh = grp * d.kk + ry * d.kw;
#pragma unroll
                for (int p = 0; p < AROWS; ++p)
                    if (r_ok[p] && (unsigned)(r_oy[p] + ty) < (unsigned)g.Hv) cur[p] |= (unsigned long long)xb[p] << sh;
            }
        }
    }

    // The whole set-up: masks, the walk's start at K offset ks (PM: at unit `split` of the tile's valid taps, T = its K tiles), the
    // per-lane byte offsets (aq: the quad of its rows this lane loads) and the descriptors.  false: a position-major workgroup past its
    // tile's units has nothing to do.
    __device__ __forceinline__ bool start(const Geom& g, const ZTile z, const float* gx, const float* wph, int kchunk, int ks, int split, int& T,
                                          int aq, int n0, int b_nv, int b_kr, const int (&rowb)[AROWS], const int (&r_oy)[AROWS],
                                          const int (&r_ox)[AROWS], const bool (&r_ok)[AROWS]) {
        tap_masks(g, z.pa, z.pb, r_oy, r_ox, r_ok);
        um = 0ull;
        minoff = sel4(z.phase, g.minoff0, g.minoff1, g.minoff2, g.minoff3);   // host-computed (finish_geom)
        if (PM) {
            // every row of the tile has the mask of row 0; the tile's VALID taps (16 .. 49 of the 7x7 kernel at 8x8) are walked in tap
            // order, in as many equal K units as their length asks for (kchunk = the unit the host aims at), one workgroup each
            um = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(cur[0] >> 32)) << 32) |
                 (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cur[0]);   // (the builtin returns int: no sign extension)
            const int kv = __builtin_popcountll(um) * g.Cin;
            const int nunits = (kv + kchunk - 1) / kchunk;            // <= gridDim.y; a workgroup past them has nothing to do:
            if (split >= nunits) return false;                        // the reduce adds this tile's nunits partials only
            const int kch = ((kv / BKT + nunits - 1) / nunits) * BKT;
            const int ksv = split * kch, kev = min(kv, ksv + kch);
            T = kev > ksv ? (kev - ksv) / BKT : 0;
            const int vi = ksv / g.Cin;
            ci0 = ksv - vi * g.Cin;
            unsigned long long r = um;
            for (int c = 0; c < vi; ++c) r &= r - 1;
            tapi = r ? __builtin_ctzll(r) : g.ntaps;
        } else {
            tapi = ks == 0 ? 0 : ks / g.Cin;
            ci0 = ks - tapi * g.Cin;
        }
        { int ty, tx; tap_decode(g, tapi, z.pa, z.pb, ty, tx, toff); }
#pragma unroll
        for (int p = 0; p < AROWS; ++p) {
            cur[p] >>= tapi;
            rowbytes[p] = (unsigned)(rowb[p] + 4 * aq) * 4u;
        }
#pragma unroll
        for (int q = 0; q < BPASS; ++q) {
            const int kr = b_kr + q * BRPP;
            const int n = n0 + 4 * b_nv;
            bvoff[q] = (kr < BKT && n < g.Cout) ? (unsigned)(kr * g.Cout + n) * 4u : OOB;
        }
        // base shifted down by the most negative tap offset so that the SGPR offset stays non-negative
        rsx = buf_rsrc(gx + minoff);
        rsw = buf_rsrc(wph);
        return true;
    }

    // the next K tile: SGPR byte offset of its tap and channels, per-lane byte offset of row p (out of range: the padding, zeros)
    __device__ __forceinline__ int soff() const { return (toff - minoff + ci0) * 4; }
    __device__ __forceinline__ unsigned avoff(int p) const { return (PM || ((unsigned)cur[p] & 1u)) ? rowbytes[p] : OOB; }   // PM: only valid taps are visited

    // one K tile on; all SGPR arithmetic
    __device__ __forceinline__ void advance(const Geom& g, int pa, int pb) {
        ci0 += BKT;
        if (ci0 >= g.Cin) {
            ci0 = 0;
            if (PM) {
                const unsigned long long rest = um >> (tapi + 1);      // tapi + 1 <= 64 taps - 1 (finish_geom caps a launch at 64 taps ...)
                tapi = rest ? tapi + 1 + __builtin_ctzll(rest) : g.ntaps;
            } else {
                ++tapi;
#pragma unroll
                for (int p = 0; p < AROWS; ++p) cur[p] >>= 1;
            }
            if (tapi < g.ntaps) { int ty, tx; tap_decode(g, tapi, pa, pb, ty, tx, toff); }
        }
    }
};

// ---- TN addressing ----------------------------------------------------------------------------------------------------------------
// row mm of dW = (tap, ci): the tap's pixel displacement and the element offset of (tap, ci) from a pixel of the source tensor
__device__ __forceinline__ void tn_col_decode(const Geom& g, int mm, int pa, int pb, bool& ok, int& ty, int& tx, int& off) {
    ok = mm < g.Ktot;
    const int mc = ok ? mm : 0;
    const int tap = mc / g.Cin;
    int o;
    tap_decode(g, tap, pa, pb, ty, tx, o);
    off = o + (mc - tap * g.Cin);
}

// source base = pix * Cin: the grid and the source tensor have the same geometry (always true for "same"-padded layers);
// dy rows consecutive: no output stride, one phase
__host__ __device__ __forceinline__ bool tn_lin_src(const Geom& g) { return g.td.ss == 1 && g.Hs == g.Hg && g.Ws == g.Wg; }
__host__ __device__ __forceinline__ bool tn_lin_out(const Geom& g) { return g.so == 1 && g.nphase == 1; }
// Lean (image-major) tile addressing: power-of-two grids of at least one K tile per image (all layers of the models) - a K tile is 16
// consecutive grid pixels starting at a multiple of 16, so the image and the tile's first row / column are wave-uniform (SALU), while a
// thread's own row / column offset inside the tile, its tap and its byte offsets are loop invariants.  Per tile and operand row that
// leaves two adds, two compares and a select instead of ~25 VALU of pixel decoding.  The rule of igemm_tn_kernel's lean arm and of the
// host's choice of igemm_tng_kernel (tng_ok), which has no other arm.
__host__ __device__ __forceinline__ bool tn_lean_geom(const Geom& g) {
    return g.lgW >= 0 && g.lgHW >= 0 && g.Hg * g.Wg >= BK && tn_lin_src(g) && (tn_lin_out(g) || g.so == 2);
}

// Loop invariants of a thread's A rows (K tile rows a_kr + RPP q, its column's tap at (c_ty, c_tx) / c_off).  mode 0: image-major K tiles,
// 1: flat (1 x 1 kernel, consecutive rows), 2: position-major (rows an image apart, the position is the tile's) - 1, 2: igemm_tng_kernel only.
template <int PASS, int RPP>
__device__ __forceinline__ void tn_lean_a(const Geom& g, int mode, int a_kr, bool c_ok, int c_ty, int c_tx, int c_off, int minoff, int (&l_ay)[PASS],
                                          int (&l_ax)[PASS], unsigned (&l_avoff)[PASS]) {
    const bool flat = mode == 1, pm = mode == 2, wide = flat || g.Wg >= BK;
#pragma unroll
    for (int q = 0; q < PASS; ++q) {
        const int kr = a_kr + q * RPP;
        const int kyo = (wide || pm) ? 0 : (kr >> g.lgW), kxo = (flat || pm) ? 0 : (wide ? kr : (kr & (g.Wg - 1)));
        l_ay[q] = kyo + c_ty;
        l_ax[q] = kxo + c_tx;
        l_avoff[q] = (c_ok && (PASS * RPP == BK || kr < BK)) ? (unsigned)(kr * (pm ? g.Hs * g.Ws : 1) * g.Cin + c_off - minoff) * 4u : OOB;
    }
}
// ... and of its dy rows b_kr + RPP q at columns ncol .. ncol + 3 (b_nok: inside Cout)
template <int PASS, int RPP>
__device__ __forceinline__ void tn_lean_b(const Geom& g, int mode, int b_kr, bool b_nok, int n0, int b_nv, unsigned (&l_bvoff)[PASS]) {
    const bool flat = mode == 1, pm = mode == 2, wide = flat || g.Wg >= BK, lin_out = tn_lin_out(g);
#pragma unroll
    for (int q = 0; q < PASS; ++q) {
        const int kr = b_kr + q * RPP;
        const int byo = wide ? 0 : (kr >> g.lgW), bxo = wide ? kr : (kr & (g.Wg - 1));
        const int rel = pm ? kr * g.Hout * g.Wout * g.Cout : (lin_out ? kr * g.Cout : (byo * g.so * g.Wout + bxo * g.so) * g.Cout);
        l_bvoff[q] = (b_nok && (PASS * RPP == BK || kr < BK)) ? (unsigned)(rel + n0 + 4 * b_nv) * 4u : OOB;
    }
}

// wave-uniform bases of the K tile at grid pixel p0 (image-major or flat): first row / column, SGPR byte offsets of x and dy
__device__ __forceinline__ void tn_tile_bases(const Geom& g, bool flat, int p0, int pa, int pb, int& oyb, int& oxb, int& soa, int& sob) {
    const int r0 = flat ? 0 : (p0 & (g.Hg * g.Wg - 1));
    oyb = flat ? 0 : (r0 >> g.lgW); oxb = flat ? 0 : (r0 & (g.Wg - 1));
    soa = p0 * g.Cin * 4;
    if (tn_lin_out(g)) sob = p0 * g.Cout * 4;
    else {
        const int nimg = p0 >> g.lgHW;
        sob = (((nimg * g.Hout + oyb * g.so + pa) * g.Wout + oxb * g.so + pb) * g.Cout) * 4;
    }
}
__device__ __forceinline__ bool tn_row_ok(const Geom& g, int oy, int ox) { return (unsigned)oy < (unsigned)g.Hv && (unsigned)ox < (unsigned)g.Wv; }

// ---- the loop ---------------------------------------------------------------------------------------------------------------------
// The K loop, unrolled by two: k_tile(buffer, t) gets the LDS double-buffer index as a compile-time constant, so that every ds_read /
// ds_write address is a loop-invariant register plus an immediate offset - no address VALU in the loop
template <class KTile>
__device__ __forceinline__ void k_loop2(int T, KTile&& k_tile) {
    for (int t = 0; t < T; t += 2) {
        k_tile(std::integral_constant<int, 0>{}, t);
        if (t + 1 < T) k_tile(std::integral_constant<int, 1>{}, t + 1);
    }
}

// One K tile of K-major operands (A[k][m], B[k][n]): per MFMA step one ds_read_b32 per operand, half-wave h takes row kk + h.
// SWZ: the A columns are XOR-swizzled (a_swizzle, the transposed stores of igemm_nn_kernel) - A points at the wave's first column and
// l31 picks the lane's; plain: A and B point at the lane's own column.
template <int MI, int NI, int LDA, int LDB, int BKT, bool SWZ>
__device__ __forceinline__ void mfma_k_major(f32x16 (&acc)[MI][NI], const float* A, const float* B, int h, int l31) {
#pragma unroll
    for (int kk = 0; kk < BKT; kk += 2) {
        float av[MI], bv[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) av[i] = SWZ ? A[(kk + h) * LDA + i * 32 + (l31 ^ a_swizzle<BKT>(kk >> 2))] : A[(kk + h) * LDA + i * 32];
#pragma unroll
        for (int j = 0; j < NI; ++j) bv[j] = B[(kk + h) * LDB + j * 32];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
}
