// brief_fused.inc — k_fused<NT, TRAIN>: the exact-f32 fused forward / loss / dgrad walk with compile-time width (1, 2, 4 and 8 tiles TRAIN; 1 .. 4, 8, 12, 16 inference) (part of the single translation unit brief_hip.hip, which includes it in this order;
// it uses what the parts before it define).
template <int NT, bool INFER = false>
struct FusedLds {
    using K = KCfg<NT, INFER>;
    static constexpr int R_FLOATS = K::XS_FLOATS > K::T_FLOATS ? K::XS_FLOATS : K::T_FLOATS;
    static constexpr int G_OFF = R_FLOATS;
    static constexpr int HW_OFF = G_OFF + K::G_FLOATS;
    static constexpr int TOTAL = HW_OFF + 4 * K::FP + 4;
};

// resident TRAIN workgroups per CU: widths up to 4 tiles need <= 168 registers and run THREE (a third independent wave per SIMD
// fills what two leave idle: 5x128 0.325 -> 0.309 ms per step, 5x96 0.293 -> 0.267; tools/ab_wpe.py); 5-7 tiles need ~220-230
// registers: two (forced to 168 they spill ~40 registers and lose 1.6 %); above 8: one 512-register workgroup
// The 8-tile kernel (F = 225 ... 256, the headline) runs THREE workgroups per CU as well, in a lean form: it gives up the two
// register sets it parked across phases (the next layer's bias during an epilogue, the previous layer's phases during a dgrad
// chain: 64 registers; their latency is now covered by the two other waves of the SIMD) and fits 168 registers with one spilled
// dword: k_fused 0.680 -> 0.667 ms, 99.2 -> 100.1 M voxels/s (tools/ab_c2.sh).  5-7 tiles spill 36-46 registers in that form: two.
#ifndef BRIEF_LEAN
#define BRIEF_LEAN 1
#endif
#ifndef BRIEF_LEAN7
#define BRIEF_LEAN7 0      // 7: the 7-tile kernel in the lean three-workgroup form too (experiment: 168 VGPRs + 128 B of scratch)
#endif
constexpr bool fused_lean(int NT) { return BRIEF_LEAN && (NT == 8 || NT == BRIEF_LEAN7); }
constexpr int fused_train_wpe(int NT) { return NT > 8 ? 1 : (NT <= 4 || fused_lean(NT) ? (BRIEF_TRAIN_WPE > 3 ? BRIEF_TRAIN_WPE : 3) : BRIEF_TRAIN_WPE); }
template <int NT, bool TRAIN, bool BOX = false>      // BOX: inference over a box of the grid (box_coords)
__global__ __launch_bounds__(256, TRAIN ? fused_train_wpe(NT) : (NT > 8 ? 2 : 3)) void k_fused(const typename KArgsT<BOX>::type a)
{
    static_assert(!(TRAIN && BOX), "the box mapping is an inference instantiation");
#ifdef BRIEF_STAMPS
    float st_acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long st_last = clock64();
    const long long st_c0 = st_last, st_r0 = wall_clock64();      // shader cycles / 100 MHz reference: the clock the kernel ran at
#endif
    using K = KCfg<NT, !TRAIN>;
    using LD = FusedLds<NT, !TRAIN>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *X = reinterpret_cast<float4 *>(smem);
    float *T = smem;                       // aliases X
    float *G = smem + LD::G_OFF;
    float *HW = smem + LD::HW_OFF;         // Whp[4][FP], bhp[4]

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int wm = wave % K::WM, ws = wave / K::WM;
    const brief_siren_desc &d = a.d;
    const int L = d.layers, cin = d.cin, cout = d.cout;
    const int kit = (d.features + 7) >> 3;       // chain steps that hold real (unpadded) features
    const int64_t npad = a.npad;
    const float *pk = a.pk;
    float4 *Xs = X + ws * (NT * 256);
    float *Tw = T + wave * (K::TROWS * 33);
    float *Gw = G + wave * 256;
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const __amdgpu_buffer_rsrc_t rs_pk =
        __builtin_amdgcn_make_buffer_rsrc((void *)pk, 0, (int)(brief_pk_count(d) * 4), 0x00020000);
    const int stash_bytes = (a.diag & 1) ? 0 : (int)((int64_t)K::FP * npad * 4);   // one layer's plane (host checks < 2^31)

    // head weights -> LDS once per workgroup (every lane needs all of them in the head dot product)
    {
        const float *headp = pk + brief_pk_head(d);
        for (int e = threadIdx.x; e < 4 * K::FP + 4; e += 256) HW[e] = headp[e];
    }
    // de-phase the co-resident workgroups: started together they run their MFMA chains and their
    // epilogues in lockstep and the matrix pipe idles through every epilogue
    {
        const int slot = (int)blockIdx.x < a.pers_wgs ? blockIdx.x / a.stagger_cus : 0;
        for (int i = 0; i < slot * a.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    }
    lds_barrier();

    // persistent skinny-gradient accumulators (lane <-> local feature)
    float acc0[K::RS][4], accWh[K::RS][4];
#pragma unroll
    for (int rs = 0; rs < K::RS; ++rs)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc0[rs][c] = 0.f; accWh[rs][c] = 0.f; }
    float accbh[4] = {0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;

    // Body (+ optional tail) in ONE launch.  The first pers_wgs workgroups are persistent and own a fixed set of tiles each;
    // workgroups above them (BRIEF_TAIL_ROUNDS > 0, a diagnostic: off by default) own ONE tile each and are dealt by the
    // hardware dispatcher to whichever CU retires a workgroup first — a dynamic queue without an atomic ticket, every
    // workgroup still sums a FIXED set of tiles into its record.  Measured (profiles/r03_wg_timeline.md): a tile's
    // LATENCY is 80 us alone on a CU and 95-104 us beside a mate whatever the plan, so the ragged end of the kernel is
    // about half a tile long under any tile-granular scheduling; the single-tile workgroups pay ~6 us per round for their
    // prologues and end 14-18 us later than the static plan, whose slot imbalance (first-dispatched workgroup of a CU: 6
    // tiles in 570 us, its mate: 625 us) happens to cancel against the 53 first-slot workgroups that carry a 7th tile.
    const bool pers = (int)blockIdx.x < a.pers_wgs;
    const int64_t tile_end = pers ? a.pers_tiles : a.pers_tiles + ((int64_t)blockIdx.x - a.pers_wgs) + 1;
    const int64_t tile_step = pers ? a.pers_wgs : 1;
    for (int64_t tile = pers ? (int64_t)blockIdx.x : a.pers_tiles + ((int64_t)blockIdx.x - a.pers_wgs); tile < tile_end; tile += tile_step) {
        const int64_t n0 = (tile * K::WS + ws) * 32;
        const int64_t n = n0 + ln;
        const bool valid = n < a.n;
        // ---- sample inputs (every wave of the sample tile fetches them; they are tiny).  Targets and
        //      weights are fetched now although the loss needs them a whole forward pass later.
        // The ~40 scalars this section needs (pointers, rng, grid dims and magics) are re-read from the kernarg
        // segment every tile through an opaque pointer: kept live across the tile loop they are spilled to VGPR
        // lanes and come back one v_readlane (a VALU instruction) at a time, ~450 per tile.
#if BRIEF_KERNARG_RELOAD
        typedef const __attribute__((address_space(4))) FusedArgs *kargs_f;
        kargs_f ap = (kargs_f)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ap));
        const int64_t *k_idx = ap->idx;
        const float *k_tg = ap->targets, *k_wt = ap->weights, *k_co = ap->coords;
        const uint64_t k_pop = ap->rng_pop, k_seed = ap->rng_seed, k_step = ap->rng_step;
        const int64_t k_off = ap->offset;
        GridArgs kg;
        kg.ndim = ap->grid.ndim; kg.lo = ap->grid.lo; kg.hi = ap->grid.hi; kg.fast = ap->grid.fast;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { kg.dims[ax] = ap->grid.dims[ax]; kg.step[ax] = ap->grid.step[ax]; kg.magic[ax] = ap->grid.magic[ax]; }
#else
        const int64_t *k_idx = a.idx;
        const float *k_tg = a.targets, *k_wt = a.weights, *k_co = a.coords;
        const uint64_t k_pop = a.rng_pop, k_seed = a.rng_seed, k_step = a.rng_step;
        const int64_t k_off = a.offset;
        const GridArgs &kg = a.grid;
#endif
        int64_t j = 0;
        if (valid) j = k_idx ? k_idx[n] : (k_pop ? philox_index(n, k_pop, k_seed, k_step) : n + k_off);
        float x0 = 0.f, x1 = 0.f, x2 = 0.f;
        float yv[4] = {0.f, 0.f, 0.f, 0.f}, wv4[4] = {1.f, 1.f, 1.f, 1.f};
        if (valid) {
            if (TRAIN) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c < cout) {
                        yv[c] = k_tg[j * cout + c];
                        if (k_wt) wv4[c] = k_wt[j * cout + c];
                    }
                }
            }
            if (k_co) {
                x0 = k_co[j * cin];
                x1 = k_co[j * cin + 1];
                if (cin == 3) x2 = k_co[j * cin + 2];
            } else {
                sample_coords<BOX>(kg, cin, j, x0, x1, x2);
            }
        }
        f32x16 acc[K::MTW];
        f32x16 creg[K::MTW];   // w*cos(w z) of the last sine layer (TRAIN)
        f32x16 hreg[K::MTW];
        float4 bnext[K::MTW][4];   // next hidden layer's bias, fetched one epilogue ahead of its use
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { creg[t][r] = 0.f; hreg[t][r] = 0.f; }
#pragma unroll
            for (int q = 0; q < 4; ++q) bnext[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#define FUSED_LOAD_BIAS(layer)                                                                          \
    {                                                                                                   \
        const float *bp_ = pk + brief_pk_hidden(d, (layer)) + 2 * K::FP * K::FP;                        \
        _Pragma("unroll") for (int t = 0; t < K::MTW; ++t) {                                            \
            const int mt = wm + K::WM * t;                                                              \
            if (K::EXACT || mt < NT) {                                                                  \
                _Pragma("unroll") for (int q = 0; q < 4; ++q)                                           \
                    bnext[t][q] = *reinterpret_cast<const float4 *>(bp_ + 32 * mt + 8 * q + 4 * hi);    \
            }                                                                                           \
        }                                                                                               \
    }
        // ---- layer 0: z0 = W0 x + b0 as two K=2 MFMAs ([x0 x1 | x2 1] against W0p rows)
        {
            const float b0 = hi ? x1 : x0;
            const float b1 = hi ? 1.0f : x2;
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                const int mt = wm + K::WM * t;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
                if (K::EXACT || mt < NT) {
                    const float4 w = W0p[32 * mt + ln];
                    acc[t] = MFMA(hi ? w.y : w.x, b0, acc[t]);
                    acc[t] = MFMA(hi ? w.w : w.z, b1, acc[t]);
                }
            }
        }
        STAMP(0)
        // ---- sine layers 0 .. L-2
        for (int l = 0; l <= L - 2; ++l) {
            const bool last = (l == L - 2);
            if (l > 0) {
                if (TRAIN && fused_lean(NT)) FUSED_LOAD_BIAS(l)      // lean variant: no register set parked across the epilogue
#pragma unroll
                for (int t = 0; t < K::MTW; ++t) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[t][4 * q] = bnext[t][q].x; acc[t][4 * q + 1] = bnext[t][q].y;
                        acc[t][4 * q + 2] = bnext[t][q].z; acc[t][4 * q + 3] = bnext[t][q].w;
                    }
                }
                // matrix work first: the wave inside a chain outranks its SIMD mate's epilogue (-0.5 % step time; the opposite
                // order, epilogues first, costs +0.5 %: tools/ab_lib.sh, profiles/r02_issue_model.md)
                if (TRAIN) __builtin_amdgcn_s_setprio(3);
                chain<NT, !TRAIN>(acc, rs_pk, (int)(brief_pk_hidden(d, l) * 4), Xs, wm, lane, kit);
                if (TRAIN) __builtin_amdgcn_s_setprio(0);
                STAMP(1)
                lds_barrier();   // every wave is done reading the previous image
                STAMP(2)
            }
            if (!last && !(TRAIN && fused_lean(NT))) FUSED_LOAD_BIAS(l + 1)   // lands while this epilogue computes its sines
            // epilogue: stash z, h = sin(om z) (+ c = om cos(om z) on the last sine layer)
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                const int mt = wm + K::WM * t;
                if (K::EXACT || mt < NT) {
                    // the accumulator IS the phase om z in revolutions (the weights carry om / 2 pi: brief_layout.h); its fraction
                    // is what sin and cos are taken of, here and (TRAIN) again from the stash by the dgrad chain (cos) and by
                    // k_wgrad (sin).  One VALU instruction per element where the exact two-term reduction took five.
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = __builtin_amdgcn_fractf(acc[t][r]);
                    if (TRAIN && !last) {
                        const __amdgpu_buffer_rsrc_t rz =
                            __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)l * K::FP * npad), 0, stash_bytes, 0x00020000);
                        // stash planes are tile-blocked, [32-sample tile][FP rows][32 samples]: a tile's block is one contiguous
                        // 4 * 32 * FP bytes (rows 128 B apart), for this kernel's stores and reloads and for k_wgrad's panels
                        const int voff = (int)(n0 * (K::FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            bstore1(acc[t][r], rz, voff, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) hreg[t][r] = BRIEF_SIN_REV(acc[t][r]);
                }
            }
            if (TRAIN && last) {
                // a real (scalar) branch: if-converted, the 32 v_cos of every earlier layer were computed and thrown away
                asm volatile("" ::: "memory");
#pragma unroll
                for (int t = 0; t < K::MTW; ++t) {
                    if (K::EXACT || wm + K::WM * t < NT) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) creg[t][r] = BRIEF_COS_REV(acc[t][r]);      // its om rides on g (gom below)
                    }
                }
            }
            write_image<NT, !TRAIN>(Xs, hreg, wm, lane);
            STAMP(3)
            lds_barrier();
            STAMP(4)
        }
        // ---- head (every wave evaluates it for its sample tile; F MACs per sample)
        float zo[4], yh[4], g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            zo[c] = 0.f; yh[c] = 0.f; g[c] = 0.f;
            if (c < cout) {
                float p = 0.f;
                const float *wrow = HW + c * K::FP;
#pragma unroll
                for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 hv = Xs[(kt * 4 + q) * 64 + lane];
                        const float4 wv = *reinterpret_cast<const float4 *>(wrow + 32 * kt + 8 * q + 4 * hi);
                        p = __fmaf_rn(wv.x, hv.x, p); p = __fmaf_rn(wv.y, hv.y, p);
                        p = __fmaf_rn(wv.z, hv.z, p); p = __fmaf_rn(wv.w, hv.w, p);
                    }
                }
                p += __shfl_xor(p, 32);
                zo[c] = p + HW[4 * K::FP + c];
                yh[c] = d.output_act ? brief_fast_sinf(d.w0_hidden * zo[c]) : zo[c];
            }
        }
        if (!TRAIN) {
            if (wm == 0 && hi == 0 && valid) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= cout) break;
                    if (a.out_kind == BRIEF_OUT_F32) {
                        reinterpret_cast<float *>(a.out)[n * cout + c] = yh[c];
                    } else {
                        // utils/io.py:136-147: separate roundings, truncating cast
                        float t = __fsub_rn(yh[c], a.scale_min);
                        t = __fdiv_rn(t, a.den);
                        t = fminf(fmaxf(t, 0.f), 1.f);
                        const float u = __fadd_rn(__fmul_rn(t, a.span), a.vmin);
                        if (a.out_kind == BRIEF_OUT_U16) reinterpret_cast<uint16_t *>(a.out)[n * cout + c] = (uint16_t)(int)u;
                        else reinterpret_cast<uint8_t *>(a.out)[n * cout + c] = (uint8_t)(int)u;
                    }
                }
            }
            lds_barrier();   // image is re-used by the next tile
            continue;
        }
        // ---- loss and dloss/dyhat (main.py:176-191)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < cout && valid) {
                float we = wv4[c];
                if (a.thr != 0.f && yh[c] <= a.thr) we = 1.0f;
                const float df = yh[c] - yv[c];
                float li, gi;
                if (a.loss_kind == BRIEF_LOSS_L2) { li = df * df; gi = 2.0f * df; }
                else if (a.loss_kind == BRIEF_LOSS_SMOOTHL1) {
                    const float ad = fabsf(df);
                    if (ad < a.beta) { li = 0.5f * df * df / a.beta; gi = df / a.beta; }
                    else { li = ad - 0.5f * a.beta; gi = df < 0.f ? -1.0f : 1.0f; }
                } else { li = 0.f; gi = 0.f; }
                if (wm == 0 && hi == 0) lsum += li * we;
                g[c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yv[c] : gi * we * a.inv_count;      // external: targets ARE dL/dyhat
                if (d.output_act) g[c] *= d.w0_hidden * brief_fast_cosf(d.w0_hidden * zo[c]);
                if (a.yhat_out && wm == 0 && hi == 0) a.yhat_out[n * cout + c] = yh[c];
            }
        }
        STAMP(5)
        // ---- head gradients: transpose own h tiles through LDS (scratch aliases the image: every
        //      wave must be past its head reads first), lane <-> local feature
        lds_barrier();
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Tw[(32 * t + ROWMAP(r, hi)) * 33 + ln] = hreg[t][r];
        }
        if (hi == 0) *reinterpret_cast<float4 *>(Gw + ln * 4) = make_float4(g[0], g[1], g[2], g[3]);
        else *reinterpret_cast<float4 *>(Gw + 128 + ln * 4) = make_float4(x0, x1, x2, 1.0f);
        lds_barrier();
#pragma unroll
        for (int rs = 0; rs < K::RS; ++rs) {
            float4 sW = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
            const int row = lane + 64 * rs;
            const float *trow = Tw + (row < K::TROWS ? row : 0) * 33;
            if (cout == 1) {
                // one channel (every volume BRIEF compresses but RGB images): a quarter of the multiply-adds
#pragma unroll 8
                for (int s = 0; s < 32; ++s) {
                    const float gv = Gw[s * 4];
                    sW.x = __fmaf_rn(trow[s], gv, sW.x);
                    sb.x += gv;
                }
            } else {
#pragma unroll 4
                for (int s = 0; s < 32; ++s) {
                    const float hv = trow[s];
                    const float4 gv = *reinterpret_cast<const float4 *>(Gw + s * 4);
                    sW.x = __fmaf_rn(hv, gv.x, sW.x); sW.y = __fmaf_rn(hv, gv.y, sW.y);
                    sW.z = __fmaf_rn(hv, gv.z, sW.z); sW.w = __fmaf_rn(hv, gv.w, sW.w);
                    sb.x += gv.x; sb.y += gv.y; sb.z += gv.z; sb.w += gv.w;
                }
            }
            if (row < K::TROWS) { accWh[rs][0] += sW.x; accWh[rs][1] += sW.y; accWh[rs][2] += sW.z; accWh[rs][3] += sW.w; }
            if (rs == 0) { accbh[0] += sb.x; accbh[1] += sb.y; accbh[2] += sb.z; accbh[3] += sb.w; }
        }
        // ---- delta of the last sine layer: om cos(phase) * (Wh^T g); the om rides on g (4 multiplies per sample, not 16 MTW)
        f32x16 dl[K::MTW];
        float gom[4];
        {
            const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;
#pragma unroll
            for (int c = 0; c < 4; ++c) gom[c] = om_top * g[c];
        }
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
            const int mt = wm + K::WM * t;
#pragma unroll
            for (int r = 0; r < 16; ++r) dl[t][r] = 0.f;
            if (K::EXACT || mt < NT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c < cout) {
                            const float4 wv = *reinterpret_cast<const float4 *>(HW + c * K::FP + 32 * mt + 8 * q + 4 * hi);
                            sacc.x = __fmaf_rn(wv.x, gom[c], sacc.x); sacc.y = __fmaf_rn(wv.y, gom[c], sacc.y);
                            sacc.z = __fmaf_rn(wv.z, gom[c], sacc.z); sacc.w = __fmaf_rn(wv.w, gom[c], sacc.w);
                        }
                    }
                    dl[t][4 * q] = creg[t][4 * q] * sacc.x; dl[t][4 * q + 1] = creg[t][4 * q + 1] * sacc.y;
                    dl[t][4 * q + 2] = creg[t][4 * q + 2] * sacc.z; dl[t][4 * q + 3] = creg[t][4 * q + 3] * sacc.w;
                }
            }
        }
        STAMP(6)
        // ---- dgrad chain: layers L-2 .. 1
        for (int l = L - 2; l >= 1; --l) {
            // stash delta_l for the weight-gradient GEMM and publish it as the B image
            const __amdgpu_buffer_rsrc_t rd =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.D + (int64_t)(l - 1) * K::FP * npad), 0, stash_bytes, 0x00020000);
            const int voff_s = (int)(n0 * (K::FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                const int mt = wm + K::WM * t;
                if (K::EXACT || mt < NT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        bstore1(dl[t][r], rd, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                }
            }
            // z_{l-1} comes back from the stash while the chain runs (it is only needed after it)
            const __amdgpu_buffer_rsrc_t rzp =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)(l - 1) * K::FP * npad), 0, stash_bytes, 0x00020000);
            float zr[K::MTW][16];
            constexpr bool ZPRE = !fused_lean(NT);      // lean variant: the phases are fetched after the chain (two other waves cover the latency)
#define FUSED_LOAD_Z()                                                                                  \
    _Pragma("unroll") for (int t = 0; t < K::MTW; ++t) {                                                \
        const int mt = wm + K::WM * t;                                                                  \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                \
            zr[t][r] = 0.f;                                                                             \
            if (K::EXACT || mt < NT) zr[t][r] = bload1s(rzp, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128); \
        }                                                                                               \
    }
            if (ZPRE) FUSED_LOAD_Z()
            STAMP(7)
            lds_barrier();   // transpose scratch / previous chain finished with the image region
            write_image<NT, !TRAIN>(Xs, dl, wm, lane);
            lds_barrier();
            STAMP(8)
#pragma unroll
            for (int t = 0; t < K::MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            __builtin_amdgcn_s_setprio(3);
            chain<NT, !TRAIN>(acc, rs_pk, (int)((brief_pk_hidden(d, l) + K::FP * K::FP) * 4), Xs, wm, lane, kit);
            __builtin_amdgcn_s_setprio(0);
            STAMP(9)
            if (!ZPRE) FUSED_LOAD_Z()
#undef FUSED_LOAD_Z
            // delta_{l-1} = acc * cos(phase_{l-1}): the chain ran on w0_{l-1} W_l^T, the stash holds the phase in revolutions
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                const int mt = wm + K::WM * t;
                if (K::EXACT || mt < NT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        dl[t][r] = acc[t][r] * BRIEF_COS_REV(zr[t][r]);
                }
            }
        }
        STAMP(7)
        // ---- first-layer gradients from delta_0 (lane <-> local feature)
        lds_barrier();
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Tw[(32 * t + ROWMAP(r, hi)) * 33 + ln] = dl[t][r];
        }
        lds_barrier();
#pragma unroll
        for (int rs = 0; rs < K::RS; ++rs) {
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
            const int row = lane + 64 * rs;
            const float *trow = Tw + (row < K::TROWS ? row : 0) * 33;
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const float dv = trow[s];
                const float4 xv = *reinterpret_cast<const float4 *>(Gw + 128 + s * 4);
                s0.x = __fmaf_rn(dv, xv.x, s0.x); s0.y = __fmaf_rn(dv, xv.y, s0.y);
                s0.z = __fmaf_rn(dv, xv.z, s0.z); s0.w = __fmaf_rn(dv, xv.w, s0.w);
            }
            if (row < K::TROWS) { acc0[rs][0] += s0.x; acc0[rs][1] += s0.y; acc0[rs][2] += s0.z; acc0[rs][3] += s0.w; }
        }
        lds_barrier();
        STAMP(6)
    }
#undef FUSED_LOAD_BIAS
    if (TRAIN) {
        float *rec = a.rec + (((int64_t)blockIdx.x + a.rec_base) * 4 + wave) * BRIEF_REC_FLOATS;      // (rec_base: the tail launch of the tail plan)
#pragma unroll
        for (int rs = 0; rs < K::RS; ++rs) {
            const int row = lane + 64 * rs;
            if (row < 128) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    rec[row * 4 + c] = acc0[rs][c];                        // dW0[f_local][x0,x1,x2,bias]
                    rec[BRIEF_REC_DWH + c * 128 + row] = accWh[rs][c];     // dWh[c][f_local]
                }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) rec[BRIEF_REC_DBH + c] = accbh[c];
            rec[BRIEF_REC_LOSS] = lsum;
#ifdef BRIEF_STAMPS
            for (int i = 0; i < 10; ++i) rec[BRIEF_REC_STAMPS + i] = st_acc[i];
            rec[BRIEF_REC_STAMPS + 10] = (float)(clock64() - st_c0);
            rec[BRIEF_REC_STAMPS + 11] = (float)(wall_clock64() - st_r0);
            rec[BRIEF_REC_STAMPS + 12] = (float)(st_r0 & 0xFFFFFF);      // absolute start (100 MHz ticks, low 24 bits) and the XCC the workgroup ran on
            rec[BRIEF_REC_STAMPS + 13] = (float)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15);      // HW_REG_XCC_ID[3:0]
            rec[BRIEF_REC_STAMPS + 14] = (float)(__builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)) & 0xFFFF);  // HW_REG_HW_ID[15:0]: wave, simd, pipe, cu[11:8], sh[12], se[15:13]
#endif
        }
    }
}
