// brief_x3.inc — BRIEF_PREC_BF16X3: split-precision helpers, k_fused_x3 and k_wgrad_x3 (part of the single translation unit brief_hip.hip, which includes it in this order;
// it uses what the parts before it define).
// ---------------------------------------------------------------------------------------------
// BRIEF_PREC_BF16X3: split-precision hidden GEMMs.  x = hi + lo with hi = bf16(x), lo = bf16(x - hi) keeps ~16 significant bits (fp16 halves, used by the forward chains: 22)
// of x; a product of two such operands is hi.hi + hi.lo + lo.hi (the dropped lo.lo term is 2^-16 of the product), three
// v_mfma_f32_32x32x16_bf16 with f32 accumulation where the exact path issues eight v_mfma_f32_32x32x2_f32: 96 instead of 512
// matrix-pipe cycles per 32 x 32 x 16 block.  tools/bf16x3_emulation.py: forward 7.9e-6 of max|y| and gradients 1.0e-5 of a
// tensor's max-abs against float64 on the 4x256 net (f32: 7e-7 / 4e-7; bands 2e-5 / 1e-4).  Same skeleton as the f32 path (32-sample
// tiles, f32 stashes, f32 head / loss / skinny gradients / optimizer); only the image and the weight fragments change.
typedef __bf16 x3_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 x3_f16x8 __attribute__((ext_vector_type(8)));
union X3Frag { uint4 u; x3_bf16x8 v; x3_f16x8 f; };
#define MFMA_X3(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define MFMA_X3F(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
// The FORWARD chains use fp16 halves (11 + 11 significant bits: the phase a deep net accumulates stays at f32's own accuracy,
// tools/fuzz_parity.py ... bf16x3): activations lie in [-1, 1] and the forward weight copies carry 2^6 on top of om / 2 pi so that
// their lo halves stay fp16-normal (|w om / 2 pi| ~ sqrt(6 / F) / 2 pi); the epilogue multiplies the accumulator by 2^-6, exactly.
// The BACKWARD chains and the weight-gradient GEMM keep bf16 halves: deltas span far more than fp16's 30 binades.
#define BRIEF_X3_FWD_SCALE 64.0f
#define BRIEF_X3_FWD_UNSCALE 0.015625f
__device__ __forceinline__ void x3_split_f16(float x, uint16_t &hi, uint16_t &lo)
{
    union { _Float16 h; uint16_t u; } a, b;
    a.h = (_Float16)x;
    b.h = (_Float16)(x - (float)a.h);
    hi = a.u; lo = b.u;
}
__device__ __forceinline__ void x3_split_bf16(float x, uint16_t &hi, uint16_t &lo)
{
    union { __bf16 h; uint16_t u; } a, b;
    a.h = (__bf16)x;
    b.h = (__bf16)(x - (float)a.h);
    hi = a.u; lo = b.u;
}

// registers 8s .. 8s+7 of an accumulator tile -> the hi and lo bf16 fragments of k-step s (the next layer's B operand)
template <bool F16>
__device__ __forceinline__ void x3_pack(const f32x16 &x, int s, uint4 &hi, uint4 &lo)
{
    X3Frag h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (F16) {
            const _Float16 b = (_Float16)x[8 * s + j];
            h.f[j] = b;
            l.f[j] = (_Float16)(x[8 * s + j] - (float)b);
        } else {
            const __bf16 b = (__bf16)x[8 * s + j];
            h.v[j] = b;
            l.v[j] = (__bf16)(x[8 * s + j] - (float)b);
        }
    }
    hi = h.u; lo = l.u;
}

// image layout: [hi | lo][kt][s][lane] x 16 B  (NT * 2 * 64 uint4 per half)
template <int NT, bool F16>
__device__ __forceinline__ void x3_write_image(uint4 *X16, const f32x16 (&h)[KCfg<NT>::MTW], int wm, int lane)
{
    using K = KCfg<NT>;
#pragma unroll
    for (int t = 0; t < K::MTW; ++t) {
        const int mt = wm + K::WM * t;
        if (K::EXACT || mt < NT) {
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                uint4 hi, lo;
                x3_pack<F16>(h[t], sx, hi, lo);
                X16[(mt * 2 + sx) * 64 + lane] = hi;
                X16[NT * 2 * 64 + (mt * 2 + sx) * 64 + lane] = lo;
            }
        }
    }
}

// one feature tile's 16 accumulator registers -> its two k-steps of hi | lo fragments in the image
template <bool F16>
__device__ __forceinline__ void x3_write_tile(uint4 *X16, const f32x16 &h, int mt, int lane)
{
#pragma unroll
    for (int sx = 0; sx < 2; ++sx) {
        uint4 hi, lo;
        x3_pack<F16>(h, sx, hi, lo);
        X16[(mt * 2 + sx) * 64 + lane] = hi;
        X16[8 * 2 * 64 + (mt * 2 + sx) * 64 + lane] = lo;
    }
}

#ifndef BRIEF_X3_PD
#define BRIEF_X3_PD 2
#endif
// the first PD k-steps of a chain's A fragments, requested AHEAD of the stash traffic that precedes the chain: vector-memory
// operations retire in order (stores count in vmcnt too), so fragments requested after an epilogue's 32 stash stores (or the
// dgrad's 32 stores + 32 phase loads) make the chain's first MFMA wait for all of those
template <int NT>
struct X3Pre { uint4 hi[BRIEF_X3_PD][KCfg<NT>::MTW], lo[BRIEF_X3_PD][KCfg<NT>::MTW]; };

#define X3_LOAD_INTO(dh_, dl_, it_)                                                                          \
    _Pragma("unroll") for (int t = 0; t < K::MTW; ++t) {                                                     \
        if (K::EXACT || wm + K::WM * t < NT) {                                                               \
            const u32x4 vh = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + (K::WM * t * NT * 2 + (it_)) * 1024, 0); \
            const u32x4 vl = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + soff_lo + (K::WM * t * NT * 2 + (it_)) * 1024, 0); \
            dh_[t] = make_uint4(vh.x, vh.y, vh.z, vh.w);                                                     \
            dl_[t] = make_uint4(vl.x, vl.y, vl.z, vl.w);                                                     \
        }                                                                                                    \
    }

template <int NT>
__device__ __forceinline__ void x3_preload(X3Pre<NT> &pre, __amdgpu_buffer_rsrc_t rs, int soff_layer, int lo_bytes, int wm, int lane)
{
    using K = KCfg<NT>;
    const int voff = lane * 16;
    int soff_w = soff_layer + wm * (NT * 2 * 1024);
    asm volatile("" : "+s"(soff_w));
    int soff_lo = lo_bytes;
    asm volatile("" : "+s"(soff_lo));
#pragma unroll
    for (int it = 0; it < BRIEF_X3_PD; ++it) X3_LOAD_INTO(pre.hi[it], pre.lo[it], it)
}

#undef X3_LOAD_INTO

// ---------------------------------------------------------------------------------------------
// BRIEF_PREC_BF16X3 train step and inference, 64-sample tiles: k_fused<8>'s job on split-precision MFMAs, every A (weight) fragment against TWO B
// fragments (two 32-sample halves of the tile).  A 32-sample tile pulls 256 KB of hi | lo fragments per layer through the CU's
// 64 B/clk vector-memory path — 4 096 cycles per tile-layer against 3 072 cycles of MFMA issue, the chains of the 32-sample
// kernel ran at 7.7 k cycles per layer; here a wave owns 2 feature tiles x 2 sample halves (64 accumulator registers) and the
// same bytes feed twice the MFMAs (a 32-sample form of this kernel lived inside k_fused until the end of round 3: git history,
// profiles/r03_bf16x3.md).  fp16 halves forward, bf16 halves
// backward, f32 stashes in the same tile-blocked planes, same records for k_reduce); only the order in which a workgroup's
// samples enter its skinny-gradient sums differs.  LDS: two hi | lo images (64 KB) + G + head weights + head partials = 76 KB,
// two workgroups per CU.
struct X3TLds {
    static constexpr int IMG_FLOATS = 2 * 4 * 64 * 33;          // two sample halves x (hi | lo) images = 64 KB, aliased by the transposed scratch [2 halves][4 waves][64 rows][33] = 66 KB
    static constexpr int G_OFF = IMG_FLOATS;
    static constexpr int HW_OFF = G_OFF + 4 * 256;
    static constexpr int PART_OFF = HW_OFF + 4 * 256 + 4;       // head partials [2 halves][4 waves][32] float4
    static constexpr int TOTAL = PART_OFF + 2 * 4 * 32 * 4;
};

template <bool F16, bool BPRE>      // BPRE: B fragments a step ahead (16 more registers: the inference kernel has them)
__device__ __forceinline__ void x3_chain2(f32x16 (&acc)[2][2], const X3Pre<8> &pre, __amdgpu_buffer_rsrc_t rs, int soff_layer, int lo_bytes,
                                          const uint4 *X16, int wm, int lane, int kit, bool two)
{
    constexpr int NT = 8, NIT = 16, PD = BRIEF_X3_PD, HALF = 2 * NT * 2 * 64;      // uint4 per sample half (hi + lo)
    using K = KCfg<8>;
    const int voff = lane * 16;
    int soff_w = soff_layer + wm * (NT * 2 * 1024);
    asm volatile("" : "+s"(soff_w));
    int soff_lo = lo_bytes;
    asm volatile("" : "+s"(soff_lo));
    uint4 ahi[NIT][2], alo[NIT][2];
    uint4 bhi[NIT][2], blo[NIT][2];
#pragma unroll
    for (int it = 0; it < PD; ++it)
#pragma unroll
        for (int t = 0; t < 2; ++t) { ahi[it][t] = pre.hi[it][t]; alo[it][t] = pre.lo[it][t]; }
#pragma unroll
    for (int h = 0; h < 2; ++h) { bhi[0][h] = X16[h * HALF + lane]; blo[0][h] = X16[h * HALF + NT * 2 * 64 + lane]; }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (it + PD < NIT) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const u32x4 vh = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + (K::WM * t * NT * 2 + it + PD) * 1024, 0);
                const u32x4 vl = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + soff_lo + (K::WM * t * NT * 2 + it + PD) * 1024, 0);
                ahi[it + PD][t] = make_uint4(vh.x, vh.y, vh.z, vh.w);
                alo[it + PD][t] = make_uint4(vl.x, vl.y, vl.z, vl.w);
            }
        }
        // (B fragments are read in the step that uses them: a step ahead they cost 16 more registers, and with those the persistent
        //  per-tile state no longer fits beside the chain — 25 spilled dwords, reloaded from scratch in every head / gradient phase)
        if (BPRE ? it + 1 < NIT : it > 0) {
            constexpr int ahead = BPRE ? 1 : 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bhi[it + ahead][h] = X16[h * HALF + (it + ahead) * 64 + lane];
                blo[it + ahead][h] = X16[h * HALF + NT * 2 * 64 + (it + ahead) * 64 + lane];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (it < kit) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                X3Frag fah, fal;
                fah.u = ahi[it][t]; fal.u = alo[it][t];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 1 && !two) continue;      // a single half-tile at the end of a workgroup's run (wave-uniform; no loads inside)
                    X3Frag fbh, fbl;
                    fbh.u = bhi[it][h]; fbl.u = blo[it][h];
                    if (F16) {
                        acc[h][t] = MFMA_X3F(fah.f, fbh.f, acc[h][t]);
                        acc[h][t] = MFMA_X3F(fah.f, fbl.f, acc[h][t]);
                        acc[h][t] = MFMA_X3F(fal.f, fbh.f, acc[h][t]);
                    } else {
                        acc[h][t] = MFMA_X3(fah.v, fbh.v, acc[h][t]);
                        acc[h][t] = MFMA_X3(fah.v, fbl.v, acc[h][t]);
                        acc[h][t] = MFMA_X3(fal.v, fbh.v, acc[h][t]);
                    }
                }
            }
        }
    }
}

template <bool TRAIN, bool BOX = false>      // false: inference (forward / decode_grid) — the forward half of the same walk, output written by the head;
                                             // BOX: inference over a box of the grid (box_coords)
__global__ __launch_bounds__(256, 2) void k_fused_x3(const typename KArgsT<BOX>::type a)
{
    static_assert(!(TRAIN && BOX), "the box mapping is an inference instantiation");
#ifdef BRIEF_STAMPS
    float st_acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long st_last = clock64();
    const long long st_c0 = st_last, st_r0 = wall_clock64();
#endif
    constexpr int NT = 8, FP = 256, HALF = 2 * NT * 2 * 64;
    using K = KCfg<8>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    uint4 *X16 = reinterpret_cast<uint4 *>(smem);
    float *T = smem;                       // aliases the images
    float *G = smem + X3TLds::G_OFF;
    float *HW = smem + X3TLds::HW_OFF;     // Whp[4][FP], bhp[4]
    float4 *PART = reinterpret_cast<float4 *>(smem + X3TLds::PART_OFF);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int wm = wave;
    const brief_siren_desc &d = a.d;
    const int L = d.layers, cin = d.cin, cout = d.cout;
    const int kit16 = (d.features + 15) >> 4;
    const int64_t npad = a.npad;
    const float *pk = a.pk;
    float *Tw = T + wave * 2 * (K::TROWS * 33);
    float *Gw = G + wave * 256;
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const __amdgpu_buffer_rsrc_t rs_x3 =
        __builtin_amdgcn_make_buffer_rsrc((void *)(a.pk + brief_pk16_off(a.d, 1)), 0, (int)(2 * brief_pk16_region(a.d) * 4), 0x00020000);
    const int x3_lo_bytes = (int)(brief_pk16_region(a.d) * 4);
    const int stash_bytes = (a.diag & 1) ? 0 : (int)((int64_t)FP * npad * 4);
    {
        const float *headp = pk + brief_pk_head(d);
        for (int e = threadIdx.x; e < 4 * FP + 4; e += 256) HW[e] = headp[e];
    }
    lds_barrier();
    float acc0[4] = {0.f, 0.f, 0.f, 0.f}, accWh[4] = {0.f, 0.f, 0.f, 0.f}, accbh[4] = {0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    // Work is dealt in 32-sample half-tiles walked two at a time.  With whole 64-sample tiles, 100 000 samples are 1 563 tiles for 512
    // resident workgroups — 3.05 rounds, a fourth round at 5 % occupancy.  Instead: R = Hn / (2 G) full rounds of pairs, strided
    // (round r: workgroup w takes half-tiles 2 (r G + w), +1 — the grid writes ONE moving window of the stash planes at a time;
    // contiguous runs per workgroup, 512 scattered write streams, cost 20 k cycles per wave in the delta stores and 12 us in the
    // k_wgrad that follows), then the Hr < 2 G left-over half-tiles as one more pair for the first Hr - G workgroups (if Hr > G)
    // and a single (second half skipped) for the others that get one.
    const int64_t Hn = (a.n + 31) >> 5;
    const int64_t G_ = gridDim.x, w_ = blockIdx.x;
    const int64_t R_ = Hn / (2 * G_), Hr = Hn - 2 * G_ * R_;
    const int64_t npair_x = Hr > G_ ? Hr - G_ : 0;                          // workgroups whose extra is a pair
    const int64_t nsing_x = Hr > G_ ? G_ - npair_x : Hr;                     // ... a single (the workgroups after those)
    const int extra = w_ < npair_x ? 2 : (w_ < npair_x + nsing_x ? 1 : 0);
    const int64_t ht_x = 2 * G_ * R_ + (w_ < npair_x ? 2 * w_ : 2 * npair_x + (w_ - npair_x));
    for (int64_t it_ = 0; it_ < R_ + (extra ? 1 : 0); ++it_) {
        const int64_t ht = it_ < R_ ? 2 * (it_ * G_ + w_) : ht_x;
        const bool two = it_ < R_ || extra == 2;      // workgroup-uniform: the second half exists
        // ---- sample inputs of both halves (kernarg scalars re-read per tile, as in k_fused)
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
        float x0[2], x1[2], x2[2];
        int64_t jidx[2];      // targets and loss weights are fetched at the loss (two workgroups per CU cover the latency; 16 registers less across the forward pass)
        bool valid[2];
        f32x16 acc[2][2];      // ONE 64-register array per wave: accumulators -> phases -> cos of the last layer -> deltas (in place throughout)
        // The 64 lanes draw the pair's 64 sample indices and coordinates ONCE (lane = sample: lanes 0..31 the first half, 32..63 the
        // second) and then hand every lane both halves' values for its column ln through the cross-lane network; computed per half as
        // in k_fused, the Philox draw, the 64-bit modulo and the grid coordinates ran twice (6 % of the kernel for this phase).
        {
            const int64_t n64 = ht * 32 + lane;
            const bool v64 = (lane < 32 || two) && n64 < a.n;
            int64_t j = 0;
            if (v64) j = k_idx ? k_idx[n64] : (k_pop ? philox_index(n64, k_pop, k_seed, k_step) : n64 + k_off);
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            if (v64) {
                if (k_co) {
                    c0 = k_co[j * cin];
                    c1 = k_co[j * cin + 1];
                    if (cin == 3) c2 = k_co[j * cin + 2];
                } else {
                    sample_coords<BOX>(kg, cin, j, c0, c1, c2);
                }
            }
            const int jl = (int)(uint32_t)(uint64_t)j, jh = (int)(uint32_t)((uint64_t)j >> 32);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int src = 32 * h + ln;
                x0[h] = __shfl(c0, src); x1[h] = __shfl(c1, src); x2[h] = __shfl(c2, src);
                jidx[h] = (int64_t)(((uint64_t)(uint32_t)__shfl(jh, src) << 32) | (uint32_t)__shfl(jl, src));
                valid[h] = (h == 0 || two) && (ht + h) * 32 + ln < a.n;
            }
        }
        X3Pre<8> x3pre;
        float4 bnext[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) bnext[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
#define X3T_LOAD_BIAS(layer)                                                                            \
    {                                                                                                   \
        const float *bp_ = pk + brief_pk_hidden(d, (layer)) + 2 * FP * FP;                              \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                 \
            const int mt = wm + 4 * t;                                                                  \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                               \
                bnext[t][q] = *reinterpret_cast<const float4 *>(bp_ + 32 * mt + 8 * q + 4 * hi);        \
        }                                                                                               \
    }
        // ---- layer 0 (exact f32): z0 = W0 x + b0 as two K=2 MFMAs per feature tile and half
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float b0 = hi ? x1[h] : x0[h];
            const float b1 = hi ? 1.0f : x2[h];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int mt = wm + 4 * t;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
                const float4 w = W0p[32 * mt + ln];
                acc[h][t] = MFMA(hi ? w.y : w.x, b0, acc[h][t]);
                acc[h][t] = MFMA(hi ? w.w : w.z, b1, acc[h][t]);
            }
        }
        STAMP(0)
        // ---- sine layers 0 .. L-2
        for (int l = 0; l <= L - 2; ++l) {
            const bool last = (l == L - 2);
            if (l > 0) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            acc[h][t][4 * q] = BRIEF_X3_FWD_SCALE * bnext[t][q].x; acc[h][t][4 * q + 1] = BRIEF_X3_FWD_SCALE * bnext[t][q].y;
                            acc[h][t][4 * q + 2] = BRIEF_X3_FWD_SCALE * bnext[t][q].z; acc[h][t][4 * q + 3] = BRIEF_X3_FWD_SCALE * bnext[t][q].w;
                        }
                __builtin_amdgcn_s_setprio(3);
                x3_chain2<true, !TRAIN>(acc, x3pre, rs_x3, (l - 1) * FP * FP * 4, x3_lo_bytes, X16, wm, lane, kit16, two);
                __builtin_amdgcn_s_setprio(0);
                STAMP(1)
                lds_barrier();   // every wave is done reading the previous images
                STAMP(2)
            }
            if (!last) {
                x3_preload<8>(x3pre, rs_x3, l * FP * FP * 4, x3_lo_bytes, wm, lane);      // ahead of this epilogue's stash stores
                X3T_LOAD_BIAS(l + 1)
            }
            float pph[2][4];      // (last layer) head partials of both halves
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int c = 0; c < 4; ++c) pph[h][c] = 0.f;
                if (h == 1 && !two) continue;
                const int voff = (int)(((ht + h) * 32) * (FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int mt = wm + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][t][r] = __builtin_amdgcn_fractf(l > 0 ? acc[h][t][r] * BRIEF_X3_FWD_UNSCALE : acc[h][t][r]);
                    f32x16 hv;
                    if (!last) {
                        if (TRAIN) {
                        const __amdgpu_buffer_rsrc_t rz =
                            __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)l * FP * npad), 0, stash_bytes, 0x00020000);
#pragma unroll
                        for (int r = 0; r < 16; ++r) bstore1s(acc[h][t][r], rz, voff, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) hv[r] = BRIEF_SIN_REV(acc[h][t][r]);
                        x3_write_tile<true>(X16 + h * HALF, hv, mt, lane);
                    } else {
                        // last sine layer: h feeds the head (from registers) and goes to this wave's transposed scratch for the head
                        // gradients (the images are dead: every wave is past the last chain's barrier); cos(phase) replaces the phase
#pragma unroll
                        for (int r = 0; r < 16; ++r) { hv[r] = BRIEF_SIN_REV(acc[h][t][r]); if (TRAIN) acc[h][t][r] = BRIEF_COS_REV(acc[h][t][r]); }
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (c < cout) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const float4 wv = *reinterpret_cast<const float4 *>(HW + c * FP + 32 * mt + 8 * q + 4 * hi);
                                    pph[h][c] = __fmaf_rn(wv.x, hv[4 * q], pph[h][c]); pph[h][c] = __fmaf_rn(wv.y, hv[4 * q + 1], pph[h][c]);
                                    pph[h][c] = __fmaf_rn(wv.z, hv[4 * q + 2], pph[h][c]); pph[h][c] = __fmaf_rn(wv.w, hv[4 * q + 3], pph[h][c]);
                                }
                            }
                        }
                        if (TRAIN) {
                            float *Th = T + (wave * 2 + h) * (K::TROWS * 33);
#pragma unroll
                            for (int r = 0; r < 16; ++r) Th[(32 * t + ROWMAP(r, hi)) * 33 + ln] = hv[r];
                        }
                    }
                }
                if (last) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) pph[h][c] += __shfl_xor(pph[h][c], 32);
                    if (hi == 0) PART[(h * 4 + wave) * 32 + ln] = make_float4(pph[h][0], pph[h][1], pph[h][2], pph[h][3]);
                }
            }
            STAMP(3)
            lds_barrier();      // images (or, last layer, the head partials) are published
            STAMP(4)
        }
        // ---- head: the waves' partial dot products (taken from the exact f32 activations above), summed in wave order
        float zo[2][4], yh[2][4], g[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 tot = PART[(h * 4) * 32 + ln];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 v = PART[(h * 4 + w) * 32 + ln];
                tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
            }
            const float tt[4] = {tot.x, tot.y, tot.z, tot.w};
            const int64_t n = (ht + h) * 32 + ln;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                zo[h][c] = 0.f; yh[h][c] = 0.f; g[h][c] = 0.f;
                if (c < cout) {
                    zo[h][c] = tt[c] + HW[4 * FP + c];
                    yh[h][c] = d.output_act ? brief_fast_sinf(d.w0_hidden * zo[h][c]) : zo[h][c];
                }
                if (!TRAIN) {
                    if (c < cout && valid[h] && wm == 0 && hi == 0) {
                        if (a.out_kind == BRIEF_OUT_F32) {
                            reinterpret_cast<float *>(a.out)[n * cout + c] = yh[h][c];
                        } else {
                            // utils/io.py:136-147: separate roundings, truncating cast
                            float t_ = __fsub_rn(yh[h][c], a.scale_min);
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
                if (c < cout && valid[h]) {
                    const float yvc = k_tg[jidx[h] * cout + c];
                    float we = k_wt ? k_wt[jidx[h] * cout + c] : 1.0f;
                    if (a.thr != 0.f && yh[h][c] <= a.thr) we = 1.0f;
                    const float df = yh[h][c] - yvc;
                    float li, gi;
                    if (a.loss_kind == BRIEF_LOSS_L2) { li = df * df; gi = 2.0f * df; }
                    else if (a.loss_kind == BRIEF_LOSS_SMOOTHL1) {
                        const float ad = fabsf(df);
                        if (ad < a.beta) { li = 0.5f * df * df / a.beta; gi = df / a.beta; }
                        else { li = ad - 0.5f * a.beta; gi = df < 0.f ? -1.0f : 1.0f; }
                    } else { li = 0.f; gi = 0.f; }
                    if (wm == 0 && hi == 0) lsum += li * we;
                    g[h][c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yvc : gi * we * a.inv_count;      // external: targets ARE dL/dyhat
                    if (d.output_act) g[h][c] *= d.w0_hidden * brief_fast_cosf(d.w0_hidden * zo[h][c]);
                    if (a.yhat_out && wm == 0 && hi == 0) a.yhat_out[n * cout + c] = yh[h][c];
                }
            }
        }
        STAMP(5)
        if (!TRAIN) continue;      // (the next tile's first LDS writes come after its own barriers; the partials were read above)
        // ---- head gradients, one half after the other, from the transposed h this wave parked in its scratch (lane <-> local feature)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) continue;
            // (no barriers here: the transposed scratch and G are this wave's own, LDS operations of one wave execute in order)
            if (hi == 0) *reinterpret_cast<float4 *>(Gw + ln * 4) = make_float4(g[h][0], g[h][1], g[h][2], g[h][3]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            {
                float4 sW = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
                const float *trow = T + (wave * 2 + h) * (K::TROWS * 33) + lane * 33;
                if (cout == 1) {
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
                accWh[0] += sW.x; accWh[1] += sW.y; accWh[2] += sW.z; accWh[3] += sW.w;
                accbh[0] += sb.x; accbh[1] += sb.y; accbh[2] += sb.z; accbh[3] += sb.w;
            }
        }
        // ---- delta of the last sine layer: om cos(phase) * (Wh^T g); the om rides on g
        {
            const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !two) continue;
                float gom[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) gom[c] = om_top * g[h][c];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int mt = wm + 4 * t;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (c < cout) {
                                const float4 wv = *reinterpret_cast<const float4 *>(HW + c * FP + 32 * mt + 8 * q + 4 * hi);
                                sacc.x = __fmaf_rn(wv.x, gom[c], sacc.x); sacc.y = __fmaf_rn(wv.y, gom[c], sacc.y);
                                sacc.z = __fmaf_rn(wv.z, gom[c], sacc.z); sacc.w = __fmaf_rn(wv.w, gom[c], sacc.w);
                            }
                        }
                        acc[h][t][4 * q] *= sacc.x; acc[h][t][4 * q + 1] *= sacc.y;
                        acc[h][t][4 * q + 2] *= sacc.z; acc[h][t][4 * q + 3] *= sacc.w;
                    }
                }
            }
        }
        STAMP(6)
        // ---- dgrad chain: layers L-2 .. 1
        for (int l = L - 2; l >= 1; --l) {
            const __amdgpu_buffer_rsrc_t rd =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.D + (int64_t)(l - 1) * FP * npad), 0, stash_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rzp =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)(l - 1) * FP * npad), 0, stash_bytes, 0x00020000);
            x3_preload<8>(x3pre, rs_x3, (l - 1) * FP * FP * 4 + FP * FP * 2, x3_lo_bytes, wm, lane);      // ahead of the delta stores
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !two) continue;
                const int voff_s = (int)(((ht + h) * 32) * (FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int mt = wm + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) bstore1s(acc[h][t][r], rd, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                }
            }
            STAMP(7)
            lds_barrier();   // transpose scratch / previous chain finished with the image region
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (h == 0 || two) x3_write_image<8, false>(X16 + h * HALF, acc[h], wm, lane);
            lds_barrier();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
            STAMP(8)
            __builtin_amdgcn_s_setprio(3);
            x3_chain2<false, false>(acc, x3pre, rs_x3, (l - 1) * FP * FP * 4 + FP * FP * 2, x3_lo_bytes, X16, wm, lane, kit16, two);
            __builtin_amdgcn_s_setprio(0);
            STAMP(9)
            // delta_{l-1} = acc * cos(phase_{l-1}): the phases come back from the stash after the chain, a half (32 requests) at a time
            // (all 64 at once: 152 B of scratch; a feature tile at a time: four exposed round trips per layer)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !two) continue;
                float zr[2][16];
                const int voff_s = (int)(((ht + h) * 32) * (FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int mt = wm + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) zr[t][r] = bload1s(rzp, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][t][r] *= BRIEF_COS_REV(zr[t][r]);
            }
        }
        STAMP(7)
        // ---- first-layer gradients from delta_0, one half after the other (lane <-> local feature)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) continue;
            if (h == 0) lds_barrier();      // the scratch aliases the images: every wave must be past the last dgrad chain
            float *Tf = Tw + h * (K::TROWS * 33);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) Tf[(32 * t + ROWMAP(r, hi)) * 33 + ln] = acc[h][t][r];
            if (hi == 1) *reinterpret_cast<float4 *>(Gw + 128 + ln * 4) = make_float4(x0[h], x1[h], x2[h], 1.0f);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // own-wave scratch: ordering only
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float *trow = Tf + lane * 33;
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const float dv = trow[s];
                const float4 xv = *reinterpret_cast<const float4 *>(Gw + 128 + s * 4);
                s0.x = __fmaf_rn(dv, xv.x, s0.x); s0.y = __fmaf_rn(dv, xv.y, s0.y);
                s0.z = __fmaf_rn(dv, xv.z, s0.z); s0.w = __fmaf_rn(dv, xv.w, s0.w);
            }
            acc0[0] += s0.x; acc0[1] += s0.y; acc0[2] += s0.z; acc0[3] += s0.w;
        }
        lds_barrier();
        STAMP(6)
    }
#undef X3T_LOAD_BIAS
    if (!TRAIN) return;
    float *rec = a.rec + ((int64_t)blockIdx.x * 4 + wave) * BRIEF_REC_FLOATS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        rec[lane * 4 + c] = acc0[c];                        // dW0[f_local][x0,x1,x2,bias]
        rec[BRIEF_REC_DWH + c * 128 + lane] = accWh[c];     // dWh[c][f_local]
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
#endif
    }
}
// ---------------------------------------------------------------------------------------------
// BRIEF_PREC_BF16X3 weight-gradient GEMM (FP = 256): the same split-K job as k_wgrad<8> on the same f32 stashes, with both
// operands split into hi + lo bf16 halves while they are staged (h = sin(2 pi phase) first) and three v_mfma_f32_32x32x16_bf16
// per fragment pair.  Panel rows are [32 samples hi | 32 samples lo | pad] = 144 B, the f32 kernel's conflict-free 36-dword
// stride; a fragment is 16 B of a row (8 consecutive samples).  Bias gradients: row sums of the f32 deltas, taken by the threads
// that stage them.  Same slab format as k_wgrad: k_reduce does not know the difference.
#ifndef BRIEF_X3W_DLY
#define BRIEF_X3W_DLY 0
#endif
__global__ __launch_bounds__(512, 2) void k_wgrad_x3(const WgradArgs a)
{
    constexpr int FP = 256, QT = 8, WNk = 4, TM = 4, TN = 2, LDSW = 36, NLD = 4, PANEL = FP * LDSW;
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2 buffers][A panel | B panel]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int wmk = wave / WNk, wnk = wave % WNk;
    const int l = 1 + (int)blockIdx.x / a.nsplit;                  // hidden layer 1..L-2
    const int split = (int)blockIdx.x % a.nsplit;
    const int64_t nchunks = a.npad / 32;
    const int64_t c0 = nchunks * split / a.nsplit, c1 = nchunks * (split + 1) / a.nsplit;
    const float *Dl = a.D + (int64_t)(l - 1) * FP * a.npad;
    const float *Zl = a.Z + (int64_t)(l - 1) * FP * a.npad;
    (void)QT;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jn][r] = 0.f;
    float bsum[NLD] = {0.f, 0.f, 0.f, 0.f};
    u32x4 ra[NLD], rb[NLD];      // kept as whole 128-bit tuples: as float4 structs the loop-carried components were shuffled
                                 // through copies behind s_waitcnt at the loop end, i.e. no prefetch across iterations
#ifdef BRIEF_X3W_NOLOAD      // diagnostic builds (timing only, results are garbage): no memory traffic / no MFMAs / no staging
    const int panel_bytes = 0;
#else
    const int panel_bytes = (int)((int64_t)FP * a.npad * 4);
#endif
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((void *)Dl, 0, panel_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsZ = __builtin_amdgcn_make_buffer_rsrc((void *)Zl, 0, panel_bytes, 0x00020000);
    int voffs[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + 512 * i;
        voffs[i] = e * 16;
    }
#define X3F(u_) __uint_as_float(u_)
#ifndef BRIEF_X3W_AUX
#define BRIEF_X3W_AUX 2      // streaming cache policy for the operand panels: read once (aux 0: 155 us, aux 2: 115 us)
#endif
#define X3W_LD(rs_, base_, voff_, soff_) __builtin_amdgcn_raw_buffer_load_b128(rs_, voff_, soff_, BRIEF_X3W_AUX)
#define X3W_ISSUE(cc)                                                                             \
    _Pragma("unroll") for (int i = 0; i < NLD; ++i) {                                             \
        ra[i] = X3W_LD(rsD, Dl, voffs[i], (int)((cc) * (FP * 128)));       \
        rb[i] = X3W_LD(rsZ, Zl, voffs[i], (int)((cc) * (FP * 128)));       \
    }
    // four f32 values of one row -> 4 hi + 4 lo bf16 (8 + 8 bytes) in the row's hi / lo halves
#define X3W_PUT(dst_, v_)                                                                         \
    {                                                                                             \
        union { uint2 u; __bf16 h[4]; } ph_, pl_;                                                 \
        const float f_[4] = {__uint_as_float((v_).x), __uint_as_float((v_).y), __uint_as_float((v_).z), __uint_as_float((v_).w)}; \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                        \
            ph_.h[j_] = (__bf16)f_[j_];                                                           \
            pl_.h[j_] = (__bf16)(f_[j_] - (float)ph_.h[j_]);                                      \
        }                                                                                         \
        *reinterpret_cast<uint2 *>(dst_) = ph_.u;                                                 \
        *reinterpret_cast<uint2 *>((dst_) + 16) = pl_.u;       /* + 64 bytes: the lo half */      \
    }
#define X3W_STAGE(buf, count_)                                                                    \
    _Pragma("unroll") for (int i = 0; i < NLD; ++i) {                                             \
        const int e = tid + 512 * i;                                                              \
        float *pa_ = smem + (buf) * 2 * PANEL + (e >> 3) * LDSW + (e & 7) * 2;                    \
        X3W_PUT(pa_, ra[i])                                                                       \
        if (count_) bsum[i] += (X3F(ra[i].x) + X3F(ra[i].y)) + (X3F(ra[i].z) + X3F(ra[i].w));     \
        u32x4 h_;                                                                                 \
        h_.x = __float_as_uint(BRIEF_SIN_REV(X3F(rb[i].x))); h_.y = __float_as_uint(BRIEF_SIN_REV(X3F(rb[i].y))); \
        h_.z = __float_as_uint(BRIEF_SIN_REV(X3F(rb[i].z))); h_.w = __float_as_uint(BRIEF_SIN_REV(X3F(rb[i].w))); \
        X3W_PUT(pa_ + PANEL, h_)                                                                  \
    }
    X3W_ISSUE(c0)
    X3W_STAGE(0, true)
    {
        const int64_t cn = c0 + 1 < c1 ? c0 + 1 : c1 - 1;
        X3W_ISSUE(cn)
    }
    lds_barrier();
    for (int64_t c = c0; c < c1; ++c) {
        const int cur = (int)(c - c0) & 1;
        const float *As = smem + cur * 2 * PANEL, *Bs = As + PANEL;
        // Chunk c + 1 is staged (its loads were issued an iteration ago) and chunk c + 2 requested BETWEEN this chunk's MFMA groups:
        // a bf16 MFMA hides ~4 VALU instructions of its own wave (profiles/r03_coissue.md), so the 16 groups of three MFMAs
        // carry the 4 x 4 staging sub-steps (pack delta | sines | pack h | next loads) instead of a separate VALU phase.  The
        // staged buffer is the one nobody reads this iteration.
        const float flag = c + 1 < c1 ? 1.0f : 0.0f;        // the clamped re-staging of the last chunk does not count in the bias sums
        const int64_t cn = c + 2 < c1 ? c + 2 : c1 - 1, cn1 = c + 1 < c1 ? c + 1 : c1 - 1;
        u32x4 hs = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // A fragments one row-tile ahead of their MFMAs (2 x 8 registers), B fragments for the whole k-step (16): with all four row
            // tiles' fragments resident (32) the allocator parked two of the prefetched operand tuples elsewhere and copied them back
            // behind s_waitcnt vmcnt(3) at the end of every iteration
            X3Frag ah[2], al[2], bh[TN], bl[TN];
            {
                const float *p_ = As + (32 * (wmk * TM) + ln) * LDSW + 8 * ks + 4 * hi;           // dwords: (16 ks + 8 hi) samples x 2 B
                ah[0].u = *reinterpret_cast<const uint4 *>(p_);
                al[0].u = *reinterpret_cast<const uint4 *>(p_ + 16);
            }
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
                const float *p_ = Bs + (32 * (wnk * TN + jn) + ln) * LDSW + 8 * ks + 4 * hi;
                bh[jn].u = *reinterpret_cast<const uint4 *>(p_);
                bl[jn].u = *reinterpret_cast<const uint4 *>(p_ + 16);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    if (jn == 0 && i + 1 < TM) {
                        const float *p_ = As + (32 * (wmk * TM + i + 1) + ln) * LDSW + 8 * ks + 4 * hi;
                        ah[(i + 1) & 1].u = *reinterpret_cast<const uint4 *>(p_);
                        al[(i + 1) & 1].u = *reinterpret_cast<const uint4 *>(p_ + 16);
                    }
#ifndef BRIEF_X3W_NOMFMA
                    acc[i][jn] = MFMA_X3(ah[i & 1].v, bh[jn].v, acc[i][jn]);
                    acc[i][jn] = MFMA_X3(ah[i & 1].v, bl[jn].v, acc[i][jn]);
                    acc[i][jn] = MFMA_X3(al[i & 1].v, bh[jn].v, acc[i][jn]);
#endif
                    __builtin_amdgcn_sched_barrier(0);
                    const int g = ks * (TM * TN) + i * TN + jn, slot = g >> 2, sub = g & 3;      // compile-time after unrolling
                    const int e = tid + 512 * slot;
                    float *pa_ = smem + (cur ^ 1) * 2 * PANEL + (e >> 3) * LDSW + (e & 7) * 2;
#ifndef BRIEF_X3W_NOSTAGE
                    // (the empty asm statements make the loop-carried values the load tuples themselves: left to the SLP vectoriser they
                    //  were component pairs across slots, copied into place behind s_waitcnt vmcnt(0) at the end of every iteration)
                    if (sub == 0) {
                        asm volatile("" : "+v"(ra[slot]));
                        X3W_PUT(pa_, ra[slot])
                        // (kept scalar and opaque: vectorised across slots, the sums were formed in place in the registers of
                        //  ra[0] / ra[2], whose reloads then went elsewhere and were copied back behind s_waitcnt vmcnt(3) at
                        //  the end of every iteration — five of the eight loads just issued had to land before the next chunk)
                        float rs_ = (X3F(ra[slot].x) + X3F(ra[slot].y)) + (X3F(ra[slot].z) + X3F(ra[slot].w));
                        asm volatile("" : "+v"(rs_));
                        bsum[slot] += flag * rs_;
                    } else if (sub == 1) {
                        asm volatile("" : "+v"(rb[slot]));
                        hs.x = __float_as_uint(BRIEF_SIN_REV(X3F(rb[slot].x))); hs.y = __float_as_uint(BRIEF_SIN_REV(X3F(rb[slot].y)));
                        hs.z = __float_as_uint(BRIEF_SIN_REV(X3F(rb[slot].z))); hs.w = __float_as_uint(BRIEF_SIN_REV(X3F(rb[slot].w)));
                    } else if (sub == 2) {
                        X3W_PUT(pa_ + PANEL, hs)
                    }
                    // the freed slot is re-requested BRIEF_X3W_DLY groups later (wrapping into the next iteration, ahead of the slot's
                    // staging there): the memory system delivers more with less in flight (tools/hbm_read_ubench.hip: 6.4 TB/s at
                    // 16-32 KB per CU, 5.5 at 64 KB and above)
                    {
                        const int gl = (g + 16 - 3 - BRIEF_X3W_DLY) & 15;      // the group whose slot is due now (compile-time after unrolling)
                        if ((gl & 3) == 0) {
                            const int sl = gl >> 2;
                            const int64_t cl = (4 * sl + 3 + BRIEF_X3W_DLY < 16) ? cn : cn1;
                            ra[sl] = X3W_LD(rsD, Dl, voffs[sl], (int)(cl * (FP * 128)));
                            rb[sl] = X3W_LD(rsZ, Zl, voffs[sl], (int)(cl * (FP * 128)));
                        }
                    }
#else
                    if (sub == 3) {
                        float rs_ = X3F(ra[slot].x) + X3F(rb[slot].x);
                        asm volatile("" : "+v"(rs_));
                        bsum[slot] += flag * rs_;
                        ra[slot] = X3W_LD(rsD, Dl, voffs[slot], (int)(cn * (FP * 128)));
                        rb[slot] = X3W_LD(rsZ, Zl, voffs[slot], (int)(cn * (FP * 128)));
                    }
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        lds_barrier();
    }
#undef X3W_ISSUE
#undef X3W_LD
#undef X3F
#undef X3W_PUT
#undef X3W_STAGE
    float *slab = a.slabs + ((int64_t)(l - 1) * a.nsplit + split) * ((int64_t)FP * FP + FP);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mt = wmk * TM + i;
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int nt = wnk * TN + jn;
#pragma unroll
            for (int r = 0; r < 16; ++r) slab[(int64_t)(32 * mt + ROWMAP(r, hi)) * FP + 32 * nt + ln] = acc[i][jn][r];
        }
    }
    // bias gradients: the eight threads that staged the eight 16-byte pieces of a row are neighbouring lanes
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        float v = bsum[i];
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
        if ((tid & 7) == 0) slab[(int64_t)FP * FP + (tid >> 3) + 64 * i] = v;
    }
}
