// brief_small.inc — k_small / k_small_group: narrow nets (F <= 64) without an HBM stash (part of the single translation unit brief_hip.hip, which includes it in this order;
// it uses what the parts before it define).
// ---------------------------------------------------------------------------------------------
// k_small<NT, HB>: the whole train step of a NARROW net (F <= 64: NT = 1, 2; at most HB hidden F x F layers)
// without any HBM stash.  For these widths (every net the reference's own YAMLs produce: F = 22 ... 56) the
// stash traffic of k_fused + k_wgrad, not the matrix pipe, sets the step time (1.8 KB per sample against
// 9 kFLOP), so here everything stays on chip:
//   * the pre-activations z_l of every sine layer stay in registers (16 per layer: a wave owns one 32x32 tile),
//     sin / cos are recomputed from them on the way back;
//   * the weight gradients accumulate in registers across all tiles a workgroup walks: delta_l and h_{l-1}
//     are transposed through LDS ([feature][sample] panels, stride 36 floats, conflict-free ds_read_b128) into
//     A / B operands whose k index is the sample, 16 MFMAs per (32x32 dW tile, 32 samples);
//   * NT = 1: the 4 waves are independent (own samples, own LDS regions, no barriers in the tile loop) and
//     fold their dW at the end;  NT = 2: wave (wm, ws) owns dW tile (wm, ws) over both sample tiles;
//   * one slab per workgroup and layer goes to k_reduce (same slab format as k_wgrad's).
// inputs of sample n for the train kernels: coordinates, targets, loss weights (defaults past the end of the batch)
// (The scalars it needs are re-read from the kernarg segment through an opaque pointer at every call: kept live across a
//  tile loop they get spilled to VGPR lanes and come back one v_readlane — a VALU instruction — at a time.)
typedef const __attribute__((address_space(4))) FusedArgs *kargs_t;
// AP: where the job's FusedArgs live — the kernarg segment (k_small: the kernel's only argument) or a table entry in global memory
// (k_small_group: one entry per co-trained job); k_idx / rng_step: this step's index set and Philox step (per-step values)
template <bool BOX = false, typename AP>      // BOX: k16's box instantiations (the kernarg segment holds the box)
__device__ __forceinline__ void small_inputs(AP ap, const int64_t *k_idx, uint64_t rng_step, int cin, int cout, int64_t n, float4 &xo, float4 &yo, float4 &wo)
{
    asm volatile("" : "+s"(ap));
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    float yv[4] = {0.f, 0.f, 0.f, 0.f}, wv4[4] = {1.f, 1.f, 1.f, 1.f};
    if (n < ap->n) {
        const float *k_tg = ap->targets, *k_wt = ap->weights, *k_co = ap->coords;
        const uint64_t k_pop = ap->rng_pop;
        const int64_t j = k_idx ? k_idx[n] : (k_pop ? philox_index(n, k_pop, ap->rng_seed, rng_step) : n + ap->offset);
        if (!k_tg) {
            // forward-only launch: no targets
        } else if (cout == 1) {
            yv[0] = k_tg[j];
            if (k_wt) wv4[0] = k_wt[j];
        } else {
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
            GridArgs kg;
            kg.ndim = ap->grid.ndim; kg.lo = ap->grid.lo; kg.hi = ap->grid.hi; kg.fast = ap->grid.fast;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { kg.dims[ax] = ap->grid.dims[ax]; kg.step[ax] = ap->grid.step[ax]; kg.magic[ax] = ap->grid.magic[ax]; }
            sample_coords<BOX>(kg, cin, j, x0, x1, x2);
        }
    }
    xo = make_float4(x0, x1, x2, 0.f);
    yo = make_float4(yv[0], yv[1], yv[2], yv[3]);
    wo = make_float4(wv4[0], wv4[1], wv4[2], wv4[3]);
}

template <int NT>
struct SmallLds {
    using K = KCfg<NT>;
    static constexpr int PANEL = 32 * 36;
    static constexpr int DT_OFF = K::XS_FLOATS;           // delta^T panels, one per wave
    static constexpr int HT_OFF = DT_OFF + 4 * PANEL;     // h^T panels, one per wave
    static constexpr int G_OFF = HT_OFF + 4 * PANEL;
    static constexpr int HW_OFF = G_OFF + 4 * 256;
    static constexpr int TOTAL = HW_OFF + 4 * K::FP + 4;
};
constexpr int small_wpe(int HB) { return HB <= 3 ? 2 : 1; }     // resident workgroups per CU (register budget; three for the one-hidden-layer bucket — 168 VGPRs, 56 B of
                                                                // scratch — measured slower: C1 0.128 against 0.102 ms per step)

// bid / gdim: this workgroup's number among, and the count of, the workgroups that serve THIS job (the whole grid for k_small; a
// contiguous range of it for k_small_group)
template <int NT, int HB, typename AP>
__device__ __forceinline__ void small_body(const FusedArgs &a, AP ap_in, const int64_t *step_idx, uint64_t step_rng, int bid, int gdim)
{
    static_assert(NT == 1 || NT == 2, "narrow nets only");
#ifdef BRIEF_STAMPS
    float st_acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long st_last = clock64();
#endif
    using K = KCfg<NT>;
    using LD = SmallLds<NT>;
    constexpr int PANEL = LD::PANEL;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *X = reinterpret_cast<float4 *>(smem);
    float *DT = smem + LD::DT_OFF, *HT = smem + LD::HT_OFF;
    float *G = smem + LD::G_OFF;
    float *HW = smem + LD::HW_OFF;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int wm = wave % K::WM, ws = wave / K::WM;
    const brief_siren_desc &d = a.d;
    const int L = d.layers, cin = d.cin, cout = d.cout;
    const int kit = (d.features + 7) >> 3;       // chain steps that hold real (unpadded) features
    const float *pk = a.pk;
    float4 *Xs = X + ws * (NT * 256);
    float *DTw = DT + wave * PANEL, *HTw = HT + wave * PANEL;
    float *Gw = G + wave * 256;
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const __amdgpu_buffer_rsrc_t rs_pk =
        __builtin_amdgcn_make_buffer_rsrc((void *)pk, 0, (int)(brief_pk_count(d) * 4), 0x00020000);
    // NT == 1: every LDS region is private to its wave and a wave's LDS operations complete in order
#define TILE_BARRIER() { if (NT > 1) lds_barrier(); else asm volatile("" ::: "memory"); }

    {
        const float *headp = pk + brief_pk_head(d);
        for (int e = threadIdx.x; e < 4 * K::FP + 4; e += 256) HW[e] = headp[e];
    }
    lds_barrier();

    f32x16 dW[HB];
    float dbv[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) {
        dbv[i] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) dW[i][r] = 0.f;
    }
    // skinny gradients: lane (ln, hi) <-> feature ln of the own tile, samples 16 hi .. 16 hi + 15
    float acc0[4] = {0.f, 0.f, 0.f, 0.f}, accWh[4] = {0.f, 0.f, 0.f, 0.f}, accbh[4] = {0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    const int prow = ln * 36 + 16 * hi;      // this lane's 16 samples of row ln in a panel

    const int64_t wg_samples = 32 * K::WS;
    const int64_t ntiles = (a.n + wg_samples - 1) / wg_samples;
    // (measured and not kept: fetching the next tile's inputs, or the next chain's first A fragments, one
    //  phase ahead costs more in registers -> scratch than the latency it hides)
    for (int64_t tile = bid; tile < ntiles; tile += gdim) {
        const int64_t n0 = (tile * K::WS + ws) * 32;
        const int64_t n = n0 + ln;
        const bool valid = n < a.n;
        float4 in_x, in_y, in_w;     // coords (x0,x1,x2,-) | targets | loss weights
        small_inputs(ap_in, step_idx, step_rng, cin, cout, n, in_x, in_y, in_w);
        const float x0 = in_x.x, x1 = in_x.y, x2 = in_x.z;
        const float yv[4] = {in_y.x, in_y.y, in_y.z, in_y.w}, wv4[4] = {in_w.x, in_w.y, in_w.z, in_w.w};
        f32x16 acc[1], hreg[1];
        f32x16 zst[HB + 1];
        float4 bnext[4];

#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) bnext[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        // ---- layer 0 (two K=2 MFMAs against [x0 x1 | x2 1], bias folded in)
        {
            const float4 w = W0p[32 * wm + ln];
            acc[0] = MFMA(hi ? w.y : w.x, hi ? x1 : x0, acc[0]);
            acc[0] = MFMA(hi ? w.w : w.z, hi ? 1.0f : x2, acc[0]);
        }
        STAMP(0)
        // ---- sine layers 0 .. L-2 (unrolled to the bucket size so that zst[] stays in registers)
#pragma unroll
        for (int l = 0; l <= HB; ++l) {
            if (l <= L - 2) {
                const bool last = (l == L - 2);
                if (l > 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[0][4 * q] = bnext[q].x; acc[0][4 * q + 1] = bnext[q].y;
                        acc[0][4 * q + 2] = bnext[q].z; acc[0][4 * q + 3] = bnext[q].w;
                    }
                    chain<NT>(acc, rs_pk, (int)(brief_pk_hidden(d, l) * 4), Xs, wm, lane, kit);
                    STAMP(1)
                    TILE_BARRIER()
                }
                if (!last) {
                    const float *bp_ = pk + brief_pk_hidden(d, l + 1) + 2 * K::FP * K::FP;
#pragma unroll
                    for (int q = 0; q < 4; ++q) bnext[q] = *reinterpret_cast<const float4 *>(bp_ + 32 * wm + 8 * q + 4 * hi);
                }
                // the accumulator is the phase om z in revolutions (the weights carry om / 2 pi); keep its fraction: the
                // backward pass takes sin and cos of it again
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][r] = __builtin_amdgcn_fractf(acc[0][r]);
                zst[l] = acc[0];
#pragma unroll
                for (int r = 0; r < 16; ++r) hreg[0][r] = BRIEF_SIN_REV(acc[0][r]);
                write_image<NT>(Xs, hreg, wm, lane);
                TILE_BARRIER()
                STAMP(2)
            }
        }
        // ---- head
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
        // ---- head gradients from the transposed last activation
#pragma unroll
        for (int r = 0; r < 16; ++r) HTw[ROWMAP(r, hi) * 36 + ln] = hreg[0][r];
        if (hi == 0) *reinterpret_cast<float4 *>(Gw + ln * 4) = make_float4(g[0], g[1], g[2], g[3]);
        else *reinterpret_cast<float4 *>(Gw + 128 + ln * 4) = make_float4(x0, x1, x2, 1.0f);
        TILE_BARRIER()      // also: every wave is past its head reads of the image
        if (cout == 1) {
            float sW = 0.f, sb = 0.f;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 hv = *reinterpret_cast<const float4 *>(HTw + prow + 4 * q4);
                const float hvv[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float gv = Gw[(16 * hi + 4 * q4 + jj) * 4];
                    sW = __fmaf_rn(hvv[jj], gv, sW);
                    sb += gv;
                }
            }
            accWh[0] += sW;
            accbh[0] += sb;
        } else {
            float4 sW = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 hv = *reinterpret_cast<const float4 *>(HTw + prow + 4 * q4);
                const float hvv[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float4 gv = *reinterpret_cast<const float4 *>(Gw + (16 * hi + 4 * q4 + jj) * 4);
                    sW.x = __fmaf_rn(hvv[jj], gv.x, sW.x); sW.y = __fmaf_rn(hvv[jj], gv.y, sW.y);
                    sW.z = __fmaf_rn(hvv[jj], gv.z, sW.z); sW.w = __fmaf_rn(hvv[jj], gv.w, sW.w);
                    sb.x += gv.x; sb.y += gv.y; sb.z += gv.z; sb.w += gv.w;
                }
            }
            accWh[0] += sW.x; accWh[1] += sW.y; accWh[2] += sW.z; accWh[3] += sW.w;
            accbh[0] += sb.x; accbh[1] += sb.y; accbh[2] += sb.z; accbh[3] += sb.w;
        }
        STAMP(3)
        // ---- Wh^T g: the last sine layer's delta is c_{L-2} times this (taken inside the unrolled loop below,
        //      where the layer index is a compile-time constant and z comes straight out of its registers)
        f32x16 dl[1];
        float gom[4];      // om of the last sine layer rides on g
        {
            const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;
#pragma unroll
            for (int c = 0; c < 4; ++c) gom[c] = om_top * g[c];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < cout) {
                    const float4 wv = *reinterpret_cast<const float4 *>(HW + c * K::FP + 32 * wm + 8 * q + 4 * hi);
                    sacc.x = __fmaf_rn(wv.x, gom[c], sacc.x); sacc.y = __fmaf_rn(wv.y, gom[c], sacc.y);
                    sacc.z = __fmaf_rn(wv.z, gom[c], sacc.z); sacc.w = __fmaf_rn(wv.w, gom[c], sacc.w);
                }
            }
            dl[0][4 * q] = sacc.x; dl[0][4 * q + 1] = sacc.y; dl[0][4 * q + 2] = sacc.z; dl[0][4 * q + 3] = sacc.w;
        }
#define SMALL_TOP_DELTA(layer)                                                                           \
    if ((layer) == L - 2) {                                                                              \
        _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                   \
            dl[0][r] *= BRIEF_COS_REV(zst[(layer)][r]);                                                  \
    }
        // ---- backward through the hidden layers L-2 .. 1: dW_l += delta_l h_{l-1}^T, delta_{l-1} = (W_l^T delta_l) . c_{l-1}
#pragma unroll
        for (int li = HB; li >= 1; --li) {
            SMALL_TOP_DELTA(li)
            if (li <= L - 2) {
                f32x16 cp;      // cos(phase_{li-1}): its om rides on the W^T copy the chain below runs on
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float fr = zst[li - 1][r];
                    HTw[ROWMAP(r, hi) * 36 + ln] = BRIEF_SIN_REV(fr);
                    cp[r] = BRIEF_COS_REV(fr);
                    DTw[ROWMAP(r, hi) * 36 + ln] = dl[0][r];
                }
                write_image<NT>(Xs, dl, wm, lane);
                TILE_BARRIER()
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
                STAMP(4)
                chain<NT>(acc, rs_pk, (int)((brief_pk_hidden(d, li) + K::FP * K::FP) * 4), Xs, wm, lane, kit);
                STAMP(5)
                // weight gradient: k = sample; lane (m, hi) feeds samples 16 hi + s at step s
#pragma unroll
                for (int st = 0; st < K::WS; ++st) {
                    if (NT == 1 && st != ws) continue;       // NT == 1: only the wave's own sample tile
                    const float *pa = (NT == 1 ? DTw : DT + (st * K::WM + wm) * PANEL) + prow;
                    const float *pb = (NT == 1 ? HTw : HT + (st * K::WM + ws) * PANEL) + prow;
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const float4 a4 = *reinterpret_cast<const float4 *>(pa + 4 * q4);
                        const float4 b4 = *reinterpret_cast<const float4 *>(pb + 4 * q4);
                        dW[li - 1] = MFMA(a4.x, b4.x, dW[li - 1]);
                        dW[li - 1] = MFMA(a4.y, b4.y, dW[li - 1]);
                        dW[li - 1] = MFMA(a4.z, b4.z, dW[li - 1]);
                        dW[li - 1] = MFMA(a4.w, b4.w, dW[li - 1]);
                        dbv[li - 1] += (a4.x + a4.y) + (a4.z + a4.w);
                    }
                }
                STAMP(6)
#pragma unroll
                for (int r = 0; r < 16; ++r) dl[0][r] = acc[0][r] * cp[r];
                TILE_BARRIER()      // panels and image are rewritten by the next layer
            }
        }
        SMALL_TOP_DELTA(0)
#undef SMALL_TOP_DELTA
        // ---- first-layer gradients from delta_0
#pragma unroll
        for (int r = 0; r < 16; ++r) DTw[ROWMAP(r, hi) * 36 + ln] = dl[0][r];
        TILE_BARRIER()
        {
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 dv = *reinterpret_cast<const float4 *>(DTw + prow + 4 * q4);
                const float dvv[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float4 xv = *reinterpret_cast<const float4 *>(Gw + 128 + (16 * hi + 4 * q4 + jj) * 4);
                    s0.x = __fmaf_rn(dvv[jj], xv.x, s0.x); s0.y = __fmaf_rn(dvv[jj], xv.y, s0.y);
                    s0.z = __fmaf_rn(dvv[jj], xv.z, s0.z); s0.w = __fmaf_rn(dvv[jj], xv.w, s0.w);
                }
            }
            acc0[0] += s0.x; acc0[1] += s0.y; acc0[2] += s0.z; acc0[3] += s0.w;
        }
        TILE_BARRIER()
        STAMP(7)
    }
#undef TILE_BARRIER
    // ---- per-wave record of the skinny gradients (format of k_fused: k_reduce reads both)
    {
        float *rec = a.rec + ((int64_t)bid * 4 + wave) * BRIEF_REC_FLOATS;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v0 = acc0[c] + __shfl_xor(acc0[c], 32);
            const float vh = accWh[c] + __shfl_xor(accWh[c], 32);
            const float vb = accbh[c] + __shfl_xor(accbh[c], 32);
            if (hi == 0) {
                rec[ln * 4 + c] = v0;
                rec[BRIEF_REC_DWH + c * 128 + ln] = vh;
            }
            if (lane == 0) rec[BRIEF_REC_DBH + c] = vb;
        }
        for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off);
        if (lane == 0) rec[BRIEF_REC_LOSS] = lsum;
#ifdef BRIEF_STAMPS
        if (lane == 0) for (int i = 0; i < 10; ++i) rec[BRIEF_REC_STAMPS + i] = st_acc[i];
#endif
    }
    // ---- hidden-layer partials: one slab per (layer, workgroup)
    const int64_t slab_sz = (int64_t)K::FP * K::FP + K::FP;
    if (NT == 2) {
#pragma unroll
        for (int i = 0; i < HB; ++i) {
            if (i < L - 2) {
                float *slab = a.slabs + ((int64_t)i * gdim + bid) * slab_sz;
#pragma unroll
                for (int r = 0; r < 16; ++r) slab[(32 * wm + ROWMAP(r, hi)) * K::FP + 32 * ws + ln] = dW[i][r];
                const float tot = dbv[i] + __shfl_xor(dbv[i], 32);
                if (ws == 0 && hi == 0) slab[K::FP * K::FP + 32 * wm + ln] = tot;
            }
        }
    } else {
        // fold the four waves' partial tiles in wave order (the tile loop's LDS regions are dead now)
        float *red = smem, *redb = smem + 3 * 1024;
        lds_barrier();
#pragma unroll
        for (int i = 0; i < HB; ++i) {
            if (i < L - 2) {
                if (wave > 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[(wave - 1) * 1024 + r * 64 + lane] = dW[i][r];
                    redb[(wave - 1) * 64 + lane] = dbv[i];
                }
                lds_barrier();
                if (wave == 0) {
                    f32x16 tsum = dW[i];
                    float bsum = dbv[i];
                    for (int w = 1; w < 4; ++w) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) tsum[r] += red[(w - 1) * 1024 + r * 64 + lane];
                        bsum += redb[(w - 1) * 64 + lane];
                    }
                    float *slab = a.slabs + ((int64_t)i * gdim + bid) * slab_sz;
#pragma unroll
                    for (int r = 0; r < 16; ++r) slab[ROWMAP(r, hi) * K::FP + ln] = tsum[r];
                    const float tot = bsum + __shfl_xor(bsum, 32);
                    if (hi == 0) slab[K::FP * K::FP + ln] = tot;
                }
                lds_barrier();
            }
        }
    }
}

template <int NT, int HB>
__global__ __launch_bounds__(256, small_wpe(HB)) void k_small(const FusedArgs a)
{
    kargs_t ap = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();      // FusedArgs is the kernel's only argument
    small_body<NT, HB>(a, ap, a.idx, a.rng_step, (int)blockIdx.x, (int)gridDim.x);
}

// Co-trained narrow nets in ONE launch (brief_multi_fit; the per-block loop of main.py:547-575 for the blocks one GPU owns): job j is
// served by workgroups [wg_begin[j], wg_begin[j + 1]) — exactly the grid, tile walk, records and slabs its own k_small launch would have,
// so every job's results are bit-identical to a fit on its own.  The static part of a job (pointers, net, grid, loss) sits in a device
// table uploaded once per brief_multi_fit call; what changes from step to step travels in the kernel arguments.
#define BRIEF_GROUP_MAX 64
struct SmallGroupArgs {
    const FusedArgs *table;
    int njobs;
    int wg_begin[BRIEF_GROUP_MAX + 1];
    uint64_t rng_step[BRIEF_GROUP_MAX];
    const int64_t *idx[BRIEF_GROUP_MAX];
};
// dst = *src, with src read through the constant address space (dword by dword: scalar loads, the copy dissolves into SGPRs)
template <typename T>
__device__ __forceinline__ void const_copy(T &dst, const T *src)
{
    static_assert(sizeof(T) % 4 == 0, "dword-sized arguments");
    const __attribute__((address_space(4))) uint32_t *s4 = (const __attribute__((address_space(4))) uint32_t *)src;
    uint32_t *d4 = reinterpret_cast<uint32_t *>(&dst);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) d4[i] = s4[i];
}
__device__ __forceinline__ int group_job(const int *begin, int njobs, int b)
{
    int j = 0;
    for (int k = 1; k < njobs; ++k) j += (b >= begin[k]);      // begin[] is ascending
    return j;
}
template <int NT, int HB>
__global__ __launch_bounds__(256, small_wpe(HB)) void k_small_group(const SmallGroupArgs g)
{
    const int b = (int)blockIdx.x;
    const int j = group_job(g.wg_begin, g.njobs, b);
    // the table entry is read through the CONSTANT address space (written by an earlier launch, never during this one): scalar loads
    // into SGPRs exactly like kernel arguments.  As plain global memory every use of an argument inside the tile loop was a vector
    // load + v_readfirstlane behind a wait (the kernel stores through pointers it loaded from the same table, so nothing could be
    // hoisted): 197 us per 64^3 job of a 4x35 net in a group of eight against 150 us on its own.
    kargs_t tp = (kargs_t)(g.table + j);
    FusedArgs a;
    const_copy(a, g.table + j);
    small_body<NT, HB>(a, tp, g.idx[j], g.rng_step[j], b - g.wg_begin[j], g.wg_begin[j + 1] - g.wg_begin[j]);
}
