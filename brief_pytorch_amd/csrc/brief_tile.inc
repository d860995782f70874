// brief_tile.inc — the tile helpers of the family kernels (FFN, NeRF, MFN, tapered SIREN, the Jacobian decode, the Hessian decode): ONE
// text, compiled once per family.  A family file sets its prefix and includes this file where its helpers stand:
//     #define TILE_(name) nerf_##name
//     #include "brief_tile.inc"
// and gets nerf_box_coords, nerf_chain, nerf_bias, nerf_bias_col, nerf_fetch, nerf_write_image, nerf_stash and nerf_frag, functions of
// its own.  They are NOT one set of functions called by every family: with the NeRF, MFN and taper kernels calling the ffn_* helpers, 88
// of the 330 kernels compiled to other code, k_ffn_fwd instantiations whose source had not changed among them
// (profiles/r12_family_driver.md, third row).  Included under a prefix, every family's kernels see the tokens they saw when each file
// carried a copy, and compile to the same code (profiles/r18_tile_helpers.md, profiles/r21_derivative_decode.md).  Nothing here is
// instantiated or emitted for a family that does not call it: bias_col and fetch are called by the two derivative decodes (brief_jac.inc,
// brief_hess.inc) only, bias, stash and frag by the four network families only.
//
// TILE_CHAIN_PACKED (set by brief_taper.inc, brief_jac.inc and brief_hess.inc, whose fragment rows are exactly ksteps steps long): the
// chain takes no row stride KS and uses ksteps for both.  It is a second text, not a forwarder to the KS form: a forwarder, and equally
// the count passed twice, compiled k_taper_fwd and k_jac_fwd to other code.
// Both macros are undefined again at the end of this file.

#ifndef TILE_
#error "define TILE_(name) as the family's prefix before including brief_tile.inc"
#endif

// box-linear index b -> coordinates (the arithmetic of box_coords, on the box of the family's args): bit-identical to the whole-grid decode
__device__ __forceinline__ void TILE_(box_coords)(const GridArgs &g, const BoxArgs &bx, int cin, int64_t b, float &x0, float &x1, float &x2)
{
    uint32_t i0, i1, i2 = 0u;
    if (cin == 3) {
        const uint32_t e2 = (uint32_t)bx.extent[2], e1 = (uint32_t)bx.extent[1];
        if (bx.fast) {
            const uint32_t bu = (uint32_t)b;
            const uint32_t t2 = fast_div(bu, bx.magic[2], e2);
            const uint32_t t1 = fast_div(t2, bx.magic[1], e1);
            i0 = t1; i1 = t2 - t1 * e1; i2 = bu - t2 * e2;
        } else {
            const int64_t t2 = b / (int64_t)e2, t1 = t2 / (int64_t)e1;
            i0 = (uint32_t)t1; i1 = (uint32_t)(t2 - t1 * e1); i2 = (uint32_t)(b - t2 * e2);
        }
    } else {
        const uint32_t e1 = (uint32_t)bx.extent[1];
        if (bx.fast) {
            const uint32_t bu = (uint32_t)b;
            const uint32_t t1 = fast_div(bu, bx.magic[1], e1);
            i0 = t1; i1 = bu - t1 * e1;
        } else {
            const int64_t t1 = b / (int64_t)e1;
            i0 = (uint32_t)t1; i1 = (uint32_t)(b - t1 * e1);
        }
    }
    x0 = lin_coord32(g, 0, (uint32_t)bx.start[0] + (uint32_t)bx.step[0] * i0);
    x1 = lin_coord32(g, 1, (uint32_t)bx.start[1] + (uint32_t)bx.step[1] * i1);
    if (cin == 3) x2 = lin_coord32(g, 2, (uint32_t)bx.start[2] + (uint32_t)bx.step[2] * i2);
}

#ifndef TILE_CHAIN_PACKED
// acc[t] += A(mt = wv + 4 t, steps [0, ksteps)) * image, for the tiles mt < mts; A block (mt, step) at A + ((mt * KS + step) * 64 + lane) * 4
template <int MTW>
__device__ __forceinline__ void TILE_(chain)(f32x16 (&acc)[MTW], const float *__restrict__ A, int KS, int ksteps, int mts,
                                             const float4 *Xs, int wv, int lane)
{
    float4 an[MTW];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
        if (wv + 4 * t < mts) an[t] = *reinterpret_cast<const float4 *>(A + ((int64_t)(wv + 4 * t) * KS * 64 + lane) * 4);
    for (int it = 0; it < ksteps; ++it) {
        float4 ac[MTW];
#pragma unroll
        for (int t = 0; t < MTW; ++t) ac[t] = an[t];
        if (it + 1 < ksteps) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
                if (wv + 4 * t < mts) an[t] = *reinterpret_cast<const float4 *>(A + (((int64_t)(wv + 4 * t) * KS + it + 1) * 64 + lane) * 4);
        }
        const float4 b = Xs[it * 64 + lane];
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
            if (wv + 4 * t < mts) {
                acc[t] = MFMA(ac[t].x, b.x, acc[t]);
                acc[t] = MFMA(ac[t].y, b.y, acc[t]);
                acc[t] = MFMA(ac[t].z, b.z, acc[t]);
                acc[t] = MFMA(ac[t].w, b.w, acc[t]);
            }
        }
    }
}
#else
// acc[t] += A(mt = wv + 4 t, steps [0, ksteps)) * image, for the tiles mt < mts; A block (mt, step) at A + ((mt * ksteps + step) * 64 + lane) * 4
template <int MTW>
__device__ __forceinline__ void TILE_(chain)(f32x16 (&acc)[MTW], const float *__restrict__ A, int ksteps, int mts,
                                             const float4 *Xs, int wv, int lane)
{
    float4 an[MTW];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
        if (wv + 4 * t < mts) an[t] = *reinterpret_cast<const float4 *>(A + ((int64_t)(wv + 4 * t) * ksteps * 64 + lane) * 4);
    for (int it = 0; it < ksteps; ++it) {
        float4 ac[MTW];
#pragma unroll
        for (int t = 0; t < MTW; ++t) ac[t] = an[t];
        if (it + 1 < ksteps) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
                if (wv + 4 * t < mts) an[t] = *reinterpret_cast<const float4 *>(A + (((int64_t)(wv + 4 * t) * ksteps + it + 1) * 64 + lane) * 4);
        }
        const float4 b = Xs[it * 64 + lane];
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
            if (wv + 4 * t < mts) {
                acc[t] = MFMA(ac[t].x, b.x, acc[t]);
                acc[t] = MFMA(ac[t].y, b.y, acc[t]);
                acc[t] = MFMA(ac[t].z, b.z, acc[t]);
                acc[t] = MFMA(ac[t].w, b.w, acc[t]);
            }
        }
    }
}
#endif

template <int MTW>
__device__ __forceinline__ void TILE_(bias)(f32x16 (&acc)[MTW], const float *__restrict__ b, int nt, int wv, int hi)
{
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int mt = wv + 4 * t;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = mt < nt ? b[32 * mt + ROWMAP(r, hi)] : 0.f;
    }
}

// the bias in the value column of a derivative decode (value_col), zero in the tangent and second-derivative columns
template <int MTW>
__device__ __forceinline__ void TILE_(bias_col)(f32x16 (&acc)[MTW], const float *__restrict__ b, int nt, int wv, int hi, bool value_col)
{
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int mt = wv + 4 * t;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = mt < nt && value_col ? b[32 * mt + ROWMAP(r, hi)] : 0.f;
    }
}

// sample n of a decode batch -> its coordinates (x0, x1, x2, 0), zeros past the end of the batch: the sources of the family decode
// kernels (coords, else idx or n + offset into the box or the grid); Args: JacArgs or a struct derived from it
template <bool BOX, class Args>
__device__ __forceinline__ float4 TILE_(fetch)(const Args &a, int cin, int64_t n)
{
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (n < a.n) {
        const int64_t j = a.idx ? a.idx[n] : n + a.offset;
        if (a.coords) {
            x0 = a.coords[j * cin];
            x1 = a.coords[j * cin + 1];
            if (cin == 3) x2 = a.coords[j * cin + 2];
        } else if (BOX) {
            TILE_(box_coords)(a.grid, a.box, cin, j, x0, x1, x2);
        } else {
            grid_coords(a.grid, cin, j, x0, x1, x2);
        }
    }
    return make_float4(x0, x1, x2, 0.f);
}

template <int MTW>
__device__ __forceinline__ void TILE_(write_image)(float4 *Xs, const f32x16 (&h)[MTW], int nt, int wv, int lane)
{
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int mt = wv + 4 * t;
        if (mt < nt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Xs[(mt * 4 + q) * 64 + lane] = make_float4(h[t][4 * q], h[t][4 * q + 1], h[t][4 * q + 2], h[t][4 * q + 3]);
        }
    }
}

// plane[row][col0 + s] for every accumulator element this lane holds
template <int MTW>
__device__ __forceinline__ void TILE_(stash)(float *__restrict__ plane, int64_t npad, int64_t col0, const f32x16 (&h)[MTW], int nt, int wv, int hi, int s)
{
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int mt = wv + 4 * t;
        if (mt < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) plane[(int64_t)(32 * mt + ROWMAP(r, hi)) * npad + col0 + s] = h[t][r];
        }
    }
}

// fragment element q of a block sequence with KS steps per row tile: (row, k)   (the k_*_repack kernels)
__device__ __forceinline__ void TILE_(frag)(int64_t q, int KS, int &row, int &k)
{
    const int j = (int)(q & 3), lanei = (int)((q >> 2) & 63);
    const int64_t blk = q >> 8;
    const int step = (int)(blk % KS), mt = (int)(blk / KS);
    row = 32 * mt + (lanei & 31);
    k = 8 * step + 4 * (lanei >> 5) + j;
}

#undef TILE_CHAIN_PACKED
#undef TILE_
