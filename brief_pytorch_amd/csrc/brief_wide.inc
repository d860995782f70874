// brief_wide.inc — k_wide<MTW, TRAIN>: the exact-f32 fused forward / loss / dgrad walk for widths ABOVE 1024 features (33 .. 128 feature tiles;
// included by brief_hip.hip after brief_lean.inc: it runs k_lean's rolled chain, lean_chain_rt, on K-slabs).
//
// SIREN.calc_features (utils/Networks.py:299-314, main.py:248-264) has no upper bound: the shipped opt/SingleTask/default.yaml (ratio 80) on a
// 1024^3 uint16 volume solves to F = 1494.  k_lean stops at 32 tiles because it keeps (i) a whole layer's activation image in LDS (128 KB at 1024
// features) and (ii) all of a wave's feature tiles in ONE register array (8 tiles x 16 registers).  Above that neither fits, so here
//   * a layer's OUTPUT tiles are walked in P = ceil(nt / 4 MTW) passes of 4 waves x MTW <= 8 tile slots (wide_mtw picks MTW; tile of slot t in pass p:
//     wave + 4 (p MTW + t), the mapping k_reduce's records assume), one register array per pass;
//   * a layer's INPUT (the previous layer's activations / the next layer's deltas: 4 KB per feature tile and 32-sample tile) is the LDS image
//     of the narrower kernels SPILLED to memory: every workgroup owns two ping-pong planes of FP x 32 floats in REGISTER-IMAGE order (float4
//     (k-tile, q, lane): exactly the bytes the LDS image holds; 512 KB per workgroup at 2048 features, L2 / Infinity Cache resident), which the
//     epilogues write with 16-byte stores and which come back one K-SLAB of <= 32 feature tiles (128 KB of LDS) at a time, for every pass,
//     through registers (eight 16-byte loads in flight per lane), between two barriers, no double buffer.  Measured on one box, interleaved
//     (tools/ab_wide.sh, k_wide at 4x1494 / 4x2048, 100 000 samples): this form 23.1 / 40.7 ms; the slab staged from the row-ordered stash
//     planes with one-dword loads (+ the sine while staging: the first version) 23.5 / 41.3 ms; the same image planes copied by LDS-DMA
//     (global_load_lds_dwordx4, -DBRIEF_WIDE_GLDS=1) 25.1 / 43.7 ms — the DMA form is the slowest by 6 %.  The TRAIN step's planes live in
//     its workspace, inference takes them from the caller (brief_siren_forward_ws);
//   * the TRAIN step still writes the stash planes k_wgrad reads (phases and deltas, [FP rows][32 samples] per tile);
//   * the state k_lean carries across phases in registers comes back from the planes instead: the LAST sine layer's phase is stashed too
//     (one more Z plane than narrower nets: L - 1), its sine (head gradients) and cosine (top delta) are taken from the reload;
//   * the skinny gradients (first layer, head) are accumulated straight into the wave's record in global memory (P x 4 slots x 8 floats per
//     lane would not fit beside 128 accumulator and 128 ring registers); head weights are read from the packed buffer, not staged in LDS.
// Everything a pass adds per tile (staging, reloads, record updates) is O(F) per sample against the chains' O(F^2).
// Cross-wave traffic through global memory inside one workgroup: the waves of a workgroup run on one CU and share its write-through vector
// L1, so `s_waitcnt vmcnt(0)` + `s_barrier` orders a wave's image stores before its mates' staging loads (wide_mem_barrier).
constexpr int WIDE_SLAB = 32;      // feature tiles per K-slab: 32 x 4 KB = 128 KB of LDS
// Tile slots per wave and pass (the kernel's template parameter; the pass count follows: P = ceil(nt / 4 MTW)).  k_lean's rate barely depends on the slot
// count (0.76 .. 0.80 of the peak from 3 to 8 slots per wave, profiles/r04_widths.md), empty slots cost their full share — so the host picks the pair
// that leaves the fewest slots empty, a pass more being priced at the ~1.5 % its re-staging of the slabs costs: 35 tiles run 3 passes x 3 slots (36 slots)
// instead of 2 x 5 (40), 57 tiles 3 x 5 (60) instead of 2 x 8 (64); 47 keep 2 x 6, 64 keep 2 x 8.
__host__ __device__ inline int wide_mtw(int nt)
{
    int best = 8;
    float best_cost = 1e30f;
    for (int m = 8; m >= 3; --m) {
        const int P = (nt + 4 * m - 1) / (4 * m);
        const float cost = (float)(4 * m * P) * (1.0f + 0.015f * (float)P);
        if (cost < best_cost - 1e-3f) { best_cost = cost; best = m; }
    }
    return best;
}
struct WideLds { int r, g_off, part_off, total; };      // floats
__host__ __device__ inline WideLds wide_lds(int MTW)
{
    WideLds l;
    const int slab = WIDE_SLAB * 1024, t = 4 * 32 * MTW * 33;      // K-slab image | per-wave transposed scratch (aliases it)
    l.r = (slab > t ? slab : t) + 256;                             // + one k-step: the chain's B prefetch reads one step past the slab
    l.g_off = l.r;
    l.part_off = l.g_off + 4 * 256;
    l.total = l.part_off + 4 * 32 * 4;
    return l;
}

__device__ __forceinline__ void wide_mem_barrier()
{
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// k-tiles [k0, k0 + kt_n) of an image-ordered plane -> the LDS slab: wave w copies the (k-tile, q) steps w, w + 4, ... (a step = 64 lanes x
// 16 bytes = 1 KB, the same bytes in the plane and in LDS)
#ifndef BRIEF_WIDE_GLDS
#define BRIEF_WIDE_GLDS 0      // 1 (A/B): by LDS-DMA, one global_load_lds_dwordx4 per step (LDS destination = wave-uniform base + lane x 16): 6 % slower
#endif
__device__ __forceinline__ void wide_stage(float4 *X, const float4 *plane, int k0, int kt_n, int wave, int lane)
{
    const int nkq = kt_n * 4;
    const float4 *src = plane + (int64_t)k0 * 256 + lane;
#if BRIEF_WIDE_GLDS
    for (int e = wave; e < nkq; e += 4)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + e * 64),
                                         (__attribute__((address_space(3))) void *)(X + e * 64), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    for (int e0 = wave; e0 < nkq; e0 += 32) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = e0 + 4 * u < nkq ? src[(e0 + 4 * u) * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e0 + 4 * u < nkq) X[(e0 + 4 * u) * 64 + lane] = v[u];
    }
#endif
}

// one feature tile's 16 x 64 values -> its four k-steps of an image-ordered plane (16-byte stores; the s_nop keeps a following VALU write
// of the data registers behind the store's read of them: hipcc 7.2 misses that hazard for > 64-bit stores)
__device__ __forceinline__ void wide_store_image(float4 *plane, int mt, int lane, const f32x16 &v)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) plane[(mt * 4 + q) * 64 + lane] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    asm volatile("s_nop 2" ::: "memory");
}

template <int MTW, bool TRAIN, bool BOX = false>      // BOX: inference over a box of the grid (box_coords)
__global__ __launch_bounds__(256, 1) void k_wide(const typename KArgsT<BOX>::type a)
{
    static_assert(!(TRAIN && BOX), "the box mapping is an inference instantiation");
    constexpr int TROWS = 32 * MTW;                    // local features of one wave in one pass
    constexpr int RS = (TROWS + 63) / 64;
    const brief_siren_desc &d = a.d;
    const int nt = brief_nt(d), FP = 32 * nt;
    const int P = (nt + 4 * MTW - 1) / (4 * MTW);      // passes over the output tiles (the host chose MTW for this width: wide_mtw)
    const int TR = brief_rec_tr(nt);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WideLds lds = wide_lds(MTW);
    float4 *X = reinterpret_cast<float4 *>(smem);
    float *T = smem;                                   // aliases the slab
    float *G = smem + lds.g_off;
    float4 *PART = reinterpret_cast<float4 *>(smem + lds.part_off);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int L = d.layers, cin = d.cin, cout = d.cout;
    const int kit = (d.features + 7) >> 3;             // chain steps that hold real (unpadded) features
    const int64_t npad = a.npad;
    const float *pk = a.pk;
    float *Gw = G + wave * 256;
    float *Tw = T + wave * (TROWS * 33);
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const float *headp = pk + brief_pk_head(d);        // Whp[4][FP], bhp[4]
    const int64_t hstride = brief_pk_hidden_stride(d);
    const int plane_bytes = FP * 128;                  // one 32-sample tile's block of a plane
    const int voff = ln * 4 + hi * 512;                // this lane's column and row half inside such a block
    float *rec = a.rec + (((int64_t)blockIdx.x + a.rec_base) * 4 + wave) * (8 * TR + 32);
    if (TRAIN) {
        for (int e = lane; e < 8 * TR + 32; e += 64) rec[e] = 0.f;      // the skinny gradients accumulate in the record itself
    }
    float accbh[4] = {0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    // (TRAIN: a launch may cover the tile range [n_begin / 32, ceil(n_end / 32)) only — the body / tail pair of the overlap plan — with its records behind rec_base)
    const int64_t Hn = ((a.n_end > 0 ? a.n_end : a.n) + 31) >> 5;
    for (int64_t tile = (a.n_begin >> 5) + blockIdx.x; tile < Hn; tile += gridDim.x) {
        // ---- sample inputs (kernarg scalars re-read per tile through an opaque pointer, as in k_fused)
        typedef const __attribute__((address_space(4))) FusedArgs *kargs_f;
        kargs_f ap = (kargs_f)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ap));
        const int64_t *k_idx = ap->idx;
        const float *k_tg = ap->targets, *k_wt = ap->weights, *k_co = ap->coords;
        const uint64_t k_pop = ap->rng_pop, k_seed = ap->rng_seed, k_step = ap->rng_step;
        const int64_t k_off = ap->offset;
        const int64_t n = tile * 32 + ln;
        const bool valid = n < a.n;
        int64_t j = 0;
        if (valid) j = k_idx ? k_idx[n] : (k_pop ? philox_index(n, k_pop, k_seed, k_step) : n + k_off);
        float x0 = 0.f, x1 = 0.f, x2 = 0.f;
        if (valid) {
            if (k_co) {
                x0 = k_co[j * cin];
                x1 = k_co[j * cin + 1];
                if (cin == 3) x2 = k_co[j * cin + 2];
            } else {
                GridArgs kg;
                kg.ndim = ap->grid.ndim; kg.lo = ap->grid.lo; kg.hi = ap->grid.hi; kg.fast = ap->grid.fast;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { kg.dims[ax] = ap->grid.dims[ax]; kg.step[ax] = ap->grid.step[ax]; kg.magic[ax] = ap->grid.magic[ax]; }
                sample_coords<BOX>(kg, cin, j, x0, x1, x2);
            }
        }
        // this tile's block of plane l: TRAIN — the stash planes (Z: phases of layers 0 .. L-2, D: deltas of layers 1 .. L-2);
        // inference — two ping-pong planes per workgroup in the caller's scratch (a.Z)
        auto zplane = [&](int l) -> float * { return a.Z + ((int64_t)l * FP * npad + tile * (int64_t)FP * 32); };      // (TRAIN only)
        auto dplane = [&](int l) -> float * { return a.D + ((int64_t)(l - 1) * FP * npad + tile * (int64_t)FP * 32); };
        // the two image-ordered ping-pong planes of this workgroup: layer l's activations (forward) / deltas (backward) go to plane l & 1
        auto iplane = [&](int l) -> float4 * {
            return reinterpret_cast<float4 *>((TRAIN ? a.slabs : a.Z) + ((int64_t)blockIdx.x * 2 + (l & 1)) * (int64_t)FP * 32);
        };
        f32x16 acc[1][MTW];      // one pass's state: accumulators -> phases -> deltas
        f32x16 px;               // (lean_chain_rt's second accumulator: unused without shared tiles)
        bool tv[MTW];
        float pph[4] = {0.f, 0.f, 0.f, 0.f};      // head partials of this wave over all passes
        // ---- sine layers 0 .. L-2
        for (int l = 0; l <= L - 2; ++l) {
            const bool last = (l == L - 2);
            const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void *)(TRAIN ? zplane(l) : a.Z), 0, plane_bytes, 0x00020000);
            const float *wl = pk + FP * 4 + (int64_t)(l > 0 ? l - 1 : 0) * hstride;      // this layer's block: Wf | Wb | bias
            const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void *)wl, 0, (int)((int64_t)FP * FP * 8), 0x00020000);
            if (l > 0) wide_mem_barrier();      // the previous layer's image plane is complete, the slab region is free
            for (int p = 0; p < P; ++p) {
                const int wv = wave + 4 * p * MTW;      // slot t of this pass holds feature tile wv + 4 t
#pragma unroll
                for (int t = 0; t < MTW; ++t) tv[t] = wv + 4 * t < nt;
                if (l == 0) {
                    const float b0 = hi ? x1 : x0;
                    const float b1 = hi ? 1.0f : x2;
#pragma unroll
                    for (int t = 0; t < MTW; ++t) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[0][t][r] = 0.f;
                        if (tv[t]) {
                            const float4 w = W0p[32 * (wv + 4 * t) + ln];
                            acc[0][t] = MFMA(hi ? w.y : w.x, b0, acc[0][t]);
                            acc[0][t] = MFMA(hi ? w.w : w.z, b1, acc[0][t]);
                        }
                    }
                } else {
                    const float *bp_ = wl + 2 * (int64_t)FP * FP;
#pragma unroll
                    for (int t = 0; t < MTW; ++t) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (tv[t]) b4 = *reinterpret_cast<const float4 *>(bp_ + 32 * (wv + 4 * t) + 8 * q + 4 * hi);
                            acc[0][t][4 * q] = b4.x; acc[0][t][4 * q + 1] = b4.y; acc[0][t][4 * q + 2] = b4.z; acc[0][t][4 * q + 3] = b4.w;
                        }
                    }
                    for (int k0 = 0; k0 < nt; k0 += WIDE_SLAB) {
                        const int kt_n = nt - k0 < WIDE_SLAB ? nt - k0 : WIDE_SLAB;
                        const int ksteps = kit - 4 * k0 < 4 * kt_n ? kit - 4 * k0 : 4 * kt_n;      // real steps of this slab (>= 1)
                        if (p > 0 || k0 > 0) lds_barrier();      // every wave is done with the previous slab
                        wide_stage(X, iplane(l - 1), k0, kt_n, wave, lane);
                        lds_barrier();
                        __builtin_amdgcn_s_setprio(3);
                        lean_chain_rt<1, MTW, 0, true>(acc, px, rsW, k0 * 4096, X, wv, lane, nt, ksteps, false);
                        __builtin_amdgcn_s_setprio(0);
                    }
                }
                // epilogue: the accumulator is the phase in revolutions (the weights carry om / 2 pi)
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wv + 4 * t;
                    f32x16 hv;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[0][t][r] = __builtin_amdgcn_fractf(acc[0][t][r]);
                    if (TRAIN) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) bstore1(acc[0][t][r], rz, voff, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) hv[r] = BRIEF_SIN_REV(acc[0][t][r]);
                    if (!last) wide_store_image(iplane(l), mt, lane, hv);
                    if (last) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (c < cout) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const float4 wv4 = *reinterpret_cast<const float4 *>(headp + (int64_t)c * FP + 32 * mt + 8 * q + 4 * hi);
                                    pph[c] = __fmaf_rn(wv4.x, hv[4 * q], pph[c]); pph[c] = __fmaf_rn(wv4.y, hv[4 * q + 1], pph[c]);
                                    pph[c] = __fmaf_rn(wv4.z, hv[4 * q + 2], pph[c]); pph[c] = __fmaf_rn(wv4.w, hv[4 * q + 3], pph[c]);
                                }
                            }
                        }
                    }
                }
            }
        }
        // ---- head: the waves' partial dot products, summed in wave order
#pragma unroll
        for (int c = 0; c < 4; ++c) pph[c] += __shfl_xor(pph[c], 32);
        if (hi == 0) PART[wave * 32 + ln] = make_float4(pph[0], pph[1], pph[2], pph[3]);
        lds_barrier();
        float zo[4], yh[4], g[4];
        {
            float4 tot = PART[ln];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 v = PART[w * 32 + ln];
                tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
            }
            const float tt[4] = {tot.x, tot.y, tot.z, tot.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                zo[c] = 0.f; yh[c] = 0.f; g[c] = 0.f;
                if (c < cout) {
                    zo[c] = tt[c] + headp[4 * (int64_t)FP + c];
                    yh[c] = d.output_act ? brief_fast_sinf(d.w0_hidden * zo[c]) : zo[c];
                }
                if (!TRAIN) {
                    if (c < cout && valid && wave == 0 && hi == 0) {
                        if (a.out_kind == BRIEF_OUT_F32) {
                            reinterpret_cast<float *>(a.out)[n * cout + c] = yh[c];
                        } else {
                            // utils/io.py:136-147: separate roundings, truncating cast
                            float t_ = __fsub_rn(yh[c], a.scale_min);
                            t_ = __fdiv_rn(t_, a.den);
                            t_ = fminf(fmaxf(t_, 0.f), 1.f);
                            const float u_ = __fadd_rn(__fmul_rn(t_, a.span), a.vmin);
                            if (a.out_kind == BRIEF_OUT_U16) reinterpret_cast<uint16_t *>(a.out)[n * cout + c] = (uint16_t)(int)u_;
                            else reinterpret_cast<uint8_t *>(a.out)[n * cout + c] = (uint8_t)(int)u_;
                        }
                    }
                    continue;
                }
                // ---- loss and dloss/dyhat (main.py:176-191)
                if (c < cout && valid) {
                    const float yvc = k_tg[j * cout + c];
                    float we = k_wt ? k_wt[j * cout + c] : 1.0f;
                    if (a.thr != 0.f && yh[c] <= a.thr) we = 1.0f;
                    const float df = yh[c] - yvc;
                    float li, gi;
                    if (a.loss_kind == BRIEF_LOSS_L2) { li = df * df; gi = 2.0f * df; }
                    else if (a.loss_kind == BRIEF_LOSS_SMOOTHL1) {
                        const float ad = fabsf(df);
                        if (ad < a.beta) { li = 0.5f * df * df / a.beta; gi = df / a.beta; }
                        else { li = ad - 0.5f * a.beta; gi = df < 0.f ? -1.0f : 1.0f; }
                    } else { li = 0.f; gi = 0.f; }
                    if (wave == 0 && hi == 0) lsum += li * we;
                    g[c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yvc : gi * we * a.inv_count;      // external: targets ARE dL/dyhat
                    if (d.output_act) g[c] *= d.w0_hidden * brief_fast_cosf(d.w0_hidden * zo[c]);
                    if (a.yhat_out && wave == 0 && hi == 0) a.yhat_out[n * cout + c] = yh[c];
                }
            }
        }
        if (!TRAIN) {
            lds_barrier();      // the head partials are rewritten by the next tile (with L = 2 nothing else separates the two)
            continue;
        }
        // ---- backward.  G: dL/dyhat of the 32 samples | their coordinates (this wave's own copies)
        if (hi == 0) *reinterpret_cast<float4 *>(Gw + ln * 4) = make_float4(g[0], g[1], g[2], g[3]);
        else *reinterpret_cast<float4 *>(Gw + 128 + ln * 4) = make_float4(x0, x1, x2, 1.0f);
        float gom[4];
        {
            const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;      // the om of the last sine layer rides on g
#pragma unroll
            for (int c = 0; c < 4; ++c) gom[c] = om_top * g[c];
        }
        // first-layer gradients from delta_0 held in acc (lane <-> local feature through this wave's transposed scratch)
        auto skinny0 = [&](int p) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) Tw[(32 * t + ROWMAP(r, hi)) * 33 + ln] = tv[t] ? acc[0][t][r] : 0.f;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // own-wave scratch: ordering only
#pragma unroll
            for (int rs = 0; rs < RS; ++rs) {
                float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
                const int row = lane + 64 * rs;
                const float *trow = Tw + (row < TROWS ? row : 0) * 33;
#pragma unroll 4
                for (int s = 0; s < 32; ++s) {
                    const float dv = trow[s];
                    const float4 xv = *reinterpret_cast<const float4 *>(Gw + 128 + s * 4);
                    s0.x = __fmaf_rn(dv, xv.x, s0.x); s0.y = __fmaf_rn(dv, xv.y, s0.y);
                    s0.z = __fmaf_rn(dv, xv.z, s0.z); s0.w = __fmaf_rn(dv, xv.w, s0.w);
                }
                if (row < TROWS && wave + 4 * (p * MTW + (row >> 5)) < nt) {
                    float *r0 = rec + ((int64_t)p * TROWS + row) * 4;      // dW0[f_local][x0, x1, x2, bias]
                    r0[0] += s0.x; r0[1] += s0.y; r0[2] += s0.z; r0[3] += s0.w;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        lds_barrier();      // the scratch aliases the slab: every wave is past the last forward chain (and past its head reads)
        // ---- top of the backward pass, pass by pass: the last sine layer's phases come back from the plane; sin -> head gradients,
        //      cos x (Wh^T g) -> delta_{L-2}
        {
            const __amdgpu_buffer_rsrc_t rzl = __builtin_amdgcn_make_buffer_rsrc((void *)zplane(L - 2), 0, plane_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void *)(L - 2 >= 1 ? dplane(L - 2) : zplane(0)), 0, plane_bytes, 0x00020000);
            for (int p = 0; p < P; ++p) {
                const int wv = wave + 4 * p * MTW;
#pragma unroll
                for (int t = 0; t < MTW; ++t) tv[t] = wv + 4 * t < nt;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        acc[0][t][r] = 0.f;
                        if (tv[t]) acc[0][t][r] = bload1(rzl, voff, (32 * (wv + 4 * t) + (r & 3) + 8 * (r >> 2)) * 128);
                    }
                }
#pragma unroll
                for (int t = 0; t < MTW; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        Tw[(32 * t + ROWMAP(r, hi)) * 33 + ln] = tv[t] ? BRIEF_SIN_REV(acc[0][t][r]) : 0.f;
                        acc[0][t][r] = BRIEF_COS_REV(acc[0][t][r]);
                    }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int rs = 0; rs < RS; ++rs) {
                    float4 sW = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
                    const int row = lane + 64 * rs;
                    const float *trow = Tw + (row < TROWS ? row : 0) * 33;
#pragma unroll 4
                    for (int s = 0; s < 32; ++s) {
                        const float hvs = trow[s];
                        const float4 gv = *reinterpret_cast<const float4 *>(Gw + s * 4);
                        sW.x = __fmaf_rn(hvs, gv.x, sW.x); sW.y = __fmaf_rn(hvs, gv.y, sW.y);
                        sW.z = __fmaf_rn(hvs, gv.z, sW.z); sW.w = __fmaf_rn(hvs, gv.w, sW.w);
                        sb.x += gv.x; sb.y += gv.y; sb.z += gv.z; sb.w += gv.w;
                    }
                    if (row < TROWS && wave + 4 * (p * MTW + (row >> 5)) < nt) {
                        float *rh = rec + 4 * TR + p * TROWS + row;      // dWh[c][f_local]
                        rh[0] += sW.x; rh[TR] += sW.y; rh[2 * TR] += sW.z; rh[3 * TR] += sW.w;
                    }
                    if (rs == 0 && p == 0) { accbh[0] += sb.x; accbh[1] += sb.y; accbh[2] += sb.z; accbh[3] += sb.w; }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wv + 4 * t;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (c < cout) {
                                const float4 wv4 = *reinterpret_cast<const float4 *>(headp + (int64_t)c * FP + 32 * mt + 8 * q + 4 * hi);
                                sacc.x = __fmaf_rn(wv4.x, gom[c], sacc.x); sacc.y = __fmaf_rn(wv4.y, gom[c], sacc.y);
                                sacc.z = __fmaf_rn(wv4.z, gom[c], sacc.z); sacc.w = __fmaf_rn(wv4.w, gom[c], sacc.w);
                            }
                        }
                        acc[0][t][4 * q] *= sacc.x; acc[0][t][4 * q + 1] *= sacc.y;
                        acc[0][t][4 * q + 2] *= sacc.z; acc[0][t][4 * q + 3] *= sacc.w;
                    }
                    if (L - 2 >= 1) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) bstore1(acc[0][t][r], rd, voff, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                        wide_store_image(iplane(L - 2), mt, lane, acc[0][t]);
                    }
                }
                if (L - 2 == 0) skinny0(p);      // no hidden layer: this is delta_0
            }
        }
        // ---- dgrad chain: layers L-2 .. 1.  delta_{l-1} = (om W_l^T delta_l) . cos(phase_{l-1})
        for (int l = L - 2; l >= 1; --l) {
            const __amdgpu_buffer_rsrc_t rzp = __builtin_amdgcn_make_buffer_rsrc((void *)zplane(l - 1), 0, plane_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rdout = __builtin_amdgcn_make_buffer_rsrc((void *)(l - 1 >= 1 ? dplane(l - 1) : zplane(0)), 0, plane_bytes, 0x00020000);
            const float *wl = pk + FP * 4 + (int64_t)(l - 1) * hstride;
            const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void *)wl, 0, (int)((int64_t)FP * FP * 8), 0x00020000);
            wide_mem_barrier();      // delta_l is complete in its image plane; the scratch is dead
            for (int p = 0; p < P; ++p) {
                const int wv = wave + 4 * p * MTW;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    tv[t] = wv + 4 * t < nt;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[0][t][r] = 0.f;
                }
                for (int k0 = 0; k0 < nt; k0 += WIDE_SLAB) {
                    const int kt_n = nt - k0 < WIDE_SLAB ? nt - k0 : WIDE_SLAB;
                    const int ksteps = kit - 4 * k0 < 4 * kt_n ? kit - 4 * k0 : 4 * kt_n;
                    if (p > 0 || k0 > 0) lds_barrier();
                    wide_stage(X, iplane(l), k0, kt_n, wave, lane);
                    lds_barrier();
                    __builtin_amdgcn_s_setprio(3);
                    lean_chain_rt<1, MTW, 0, true>(acc, px, rsW, FP * FP * 4 + k0 * 4096, X, wv, lane, nt, ksteps, false);
                    __builtin_amdgcn_s_setprio(0);
                }
                // the phases of layer l-1 come back from the plane, two feature tiles (32 requests) at a time
#pragma unroll
                for (int t2 = 0; t2 < MTW; t2 += 2) {
                    float zr[2][16];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int t = t2 + u < MTW ? t2 + u : MTW - 1;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            zr[u][r] = 0.f;
                            if (t2 + u < MTW && tv[t]) zr[u][r] = bload1s(rzp, voff, (32 * (wv + 4 * t) + (r & 3) + 8 * (r >> 2)) * 128);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int t = t2 + u < MTW ? t2 + u : MTW - 1;
                        if (t2 + u < MTW && tv[t]) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[0][t][r] *= BRIEF_COS_REV(zr[u][r]);
                        }
                    }
                }
                if (l - 1 >= 1) {
#pragma unroll
                    for (int t = 0; t < MTW; ++t) {
                        if (!tv[t]) continue;
#pragma unroll
                        for (int r = 0; r < 16; ++r) bstore1(acc[0][t][r], rdout, voff, (32 * (wv + 4 * t) + (r & 3) + 8 * (r >> 2)) * 128);
                        wide_store_image(iplane(l - 1), wv + 4 * t, lane, acc[0][t]);
                    }
                } else {
                    lds_barrier();      // the scratch aliases the slab: every wave is past this pass's last chain
                    skinny0(p);
                }
            }
        }
        lds_barrier();      // G and the scratch are rewritten by the next tile
    }
    if (!TRAIN) return;
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) rec[8 * TR + c] = accbh[c];
        rec[8 * TR + 4] = lsum;
    }
}
