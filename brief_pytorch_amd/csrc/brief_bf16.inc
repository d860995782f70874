// brief_bf16.inc — BRIEF_PREC_BF16: the hidden F x F GEMMs of the SIREN fit on the bf16 matrix pipe.
// Included by brief_hip.hip (one translation unit: shares FusedArgs, the sampling / coordinate helpers,
// the f32 MFMA macro for the K = 3 first layer and the optimizer arithmetic).
//
// What stays f32: coordinates and the first layer (bf16 cannot tell neighbouring voxels of a 512-grid apart),
// biases, every accumulator, sin/cos, the head dot product, loss, gradient reductions, optimizer state and
// the master weights.  What is bf16: the A fragments of W / W^T, the activation and delta images the MFMAs
// read, and the delta stash.  The activations are stashed as ONE plane per sine layer: the phase theta = frac(om z / 2 pi)
// in fp16 (11 bits of a revolution: 1.5e-3 rad, below bf16's own 4e-3).  The dgrad chain takes cos(theta) of it and the
// weight-gradient GEMM sin(theta) while it stages its panels — transcendentals that ride in the bf16 MFMAs' issue gaps
// (profiles/r03_coissue.md), where round 2 stashed h AND cos as two bf16 planes: k16 is bound by its HBM bytes (4 MB per
// 128-sample tile at 8x512 against 246 k MFMA cycles), and a quarter of them were the cosine's round trip.
//
//   k16<NT,TRAIN>   512 threads = 8 waves, one workgroup per CU, 128-sample tiles.  Wave w owns feature tiles
//                   w*MTW .. (MTW = NT/8) for all four 32-sample tiles (acc[MTW][4] = 64 or 128 VGPRs), so every A
//                   fragment it fetches (16 B per lane, L2) feeds four MFMAs.  A converted accumulator tile is
//                   the next layer's B operand (registers 8s..8s+7 -> fragment of k-step s), published through a
//                   lane-linear LDS image [sample tile][kt][s][lane] x 16 B.
//                   Sample (lane n, tile st) is sample 4n + st of the workgroup tile: the four tiles of a lane are
//                   four NEIGHBOURING samples, so a stash row takes one 8-byte store per register instead of four
//                   2-byte ones.  Stashes are blocked [sample / 64][feature][64 samples]: a (feature, block) pair
//                   is one 128-byte line, a workgroup tile writes two contiguous FP x 128 B regions per plane,
//                   and the weight-gradient GEMM finds the four k-steps of a line next to each other.
//   k_wgrad16       dW_l = D_l H_{l-1}^T, first-layer and head gradients as two more (skinny) jobs, bias gradients
//                   through an all-ones B fragment.  Both operands are k(sample)-contiguous rows of the stashes:
//                   fragments are plain 16-byte global loads, no LDS, no transpose.
//   k_reduce16      fixed-order slab sums -> canonical gradients (+ optional fused optimizer and write-through to
//                   the f32 and bf16 fragment copies).

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
union Frag16 { uint4 u; bf16x8 v; };
union Pack4 { u32x2 u; bf16x4 v; };

__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

// NS = 32-sample tiles per workgroup tile: 4 in the body of a launch; a second launch walks what is left after the
// last full round of 256 workgroups with NS = 1 or 2 (quarter / half tiles spread over 4x / 2x as many CUs), so the
// tail of a 100 000-sample step costs a fraction of a round instead of a whole one.
// NW = waves per workgroup: 8 (one 512-thread workgroup per CU).  The kernel is also correct with NW = 4 (two 256-thread
// workgroups per CU running out of phase, MTW x NS = 8 accumulator tiles per wave: measured in round 2 and NOT kept —
// MFMA and VALU instructions do not overlap on a gfx950 SIMD even from different waves (tools/coexec_ubench.hip), so
// de-phasing buys nothing, and the 64-sample tiles of F = 512 double the weight traffic from L2 and halve the stash
// store width: 8x512 k16 1.35 ms against 1.21 ms).  Four waves with the whole 512-register file each (16 accumulator
// tiles per wave, one wave per SIMD) do not compile to anything useful from HIP source: hipcc keeps the VALU epilogue in
// the 256 architectural VGPRs and spills 407 registers to scratch.
template <int NT, int NS = 4, int NW = 8>
struct Cfg16 {
    static constexpr int MTW = NT / NW;                   // feature tiles per wave
    static constexpr int FP = 32 * NT;
    static constexpr int IMG_U4 = NS * NT * 2 * 64;       // uint4 elements of the B image
    static constexpr int HW_OFF = IMG_U4 * 4;             // floats
    static constexpr int HW_FLOATS = (4 * FP + 4 + 3) / 4 * 4;
    static constexpr int IN_OFF = HW_OFF + HW_FLOATS;     // INX | INY | INW : 3 x (32 NS) float4
    static constexpr int PART_OFF = IN_OFF + 3 * 32 * NS * 4; // head partials [NW waves][NS][32 n] float4
    static constexpr int TOTAL = PART_OFF + NW * NS * 32 * 4;
};

// Cache policy of the bf16 stash accesses: non-temporal (aux bit 1 = "nt" on gfx950).  The planes are written once and read once,
// 2.4 GB per 8x512 launch through 32 MB of L2; with the default policy the epilogue's stores hold the in-order vmcnt queue (the next
// chain's weight loads wait behind them) until L2 has made room.  Measured on one MI355X, same box, interleaved: 8x512 1.69 -> 1.40 ms
// per step with nt stores and loads (stores alone: 1.45), 4x256 0.351 -> 0.318 ms.  The fp32 path keeps the default policy (its k_fused
// gets 1.7 % slower with nt: k_wgrad finds part of the stash still cached), as do k_wgrad16's panel loads (neutral).
#ifndef BRIEF_STASH16_ST_AUX
#define BRIEF_STASH16_ST_AUX 2
#endif
#ifndef BRIEF_STASH16_LD_AUX
#define BRIEF_STASH16_LD_AUX 2
#endif
// the c = cos(phase) planes are the only ones the SAME kernel reads back (a tile's dgrad chain, one tile-lifetime after its forward
// pass wrote them): their policy is set separately
#ifndef BRIEF_STASH16_C_ST_AUX
#define BRIEF_STASH16_C_ST_AUX BRIEF_STASH16_ST_AUX
#endif
#ifndef BRIEF_STASH16_C_LD_AUX
#define BRIEF_STASH16_C_LD_AUX BRIEF_STASH16_LD_AUX
#endif
// NS neighbouring samples of a lane as one stash word of 2 NS bytes
template <int NS, int AUX = BRIEF_STASH16_ST_AUX>
__device__ __forceinline__ void stash_put(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float (&v)[NS])
{
    if constexpr (NS == 4) {
        Pack4 p;
#pragma unroll
        for (int i = 0; i < 4; ++i) p.v[i] = (__bf16)v[i];
        __builtin_amdgcn_raw_buffer_store_b64(p.u, r, voff, soff, AUX);
    } else if constexpr (NS == 2) {
        union { uint32_t u; bf16x2 v; } p;
        p.v[0] = (__bf16)v[0]; p.v[1] = (__bf16)v[1];
        __builtin_amdgcn_raw_buffer_store_b32(p.u, r, voff, soff, AUX);
    } else {
        union { unsigned short u; __bf16 h; } p;
        p.h = (__bf16)v[0];
        __builtin_amdgcn_raw_buffer_store_b16(p.u, r, voff, soff, AUX);
    }
}
template <int NS, int AUX = BRIEF_STASH16_C_LD_AUX>
__device__ __forceinline__ u32x2 stash_get(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    u32x2 w;
    if constexpr (NS == 4) w = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX);
    else if constexpr (NS == 2) { w.x = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX); w.y = 0; }
    else { w.x = __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, AUX); w.y = 0; }
    return w;
}
__device__ __forceinline__ float stash_val(u32x2 w, int st)
{
    return st == 0 ? bf16_lo(w.x) : (st == 1 ? bf16_hi(w.x) : (st == 2 ? bf16_lo(w.y) : bf16_hi(w.y)));
}
// the phase plane: NS neighbouring samples of a lane as fp16 (round to nearest), same word shape as the bf16 planes
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <int NS, int AUX = BRIEF_STASH16_ST_AUX>
__device__ __forceinline__ void theta_put(__amdgpu_buffer_rsrc_t r, int voff, int soff, const float (&v)[NS])
{
    union { uint32_t u; f16x2 h; } lo, hi2;
    lo.h[0] = (_Float16)v[0]; lo.h[1] = (_Float16)v[NS > 1 ? 1 : 0];
    if constexpr (NS == 4) {
        hi2.h[0] = (_Float16)v[2]; hi2.h[1] = (_Float16)v[3];
        u32x2 w; w.x = lo.u; w.y = hi2.u;
        __builtin_amdgcn_raw_buffer_store_b64(w, r, voff, soff, AUX);
    } else if constexpr (NS == 2) {
        __builtin_amdgcn_raw_buffer_store_b32(lo.u, r, voff, soff, AUX);
    } else {
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(lo.u & 0xFFFFu), r, voff, soff, AUX);
    }
}
__device__ __forceinline__ float theta_val(u32x2 w, int st)
{
    union { uint32_t u; f16x2 h; } p;
    p.u = st < 2 ? w.x : w.y;
    return (float)p.h[st & 1];
}
// eight phases (one 16-byte piece of a stash line) -> the bf16 activations h = sin(2 pi theta) the weight-gradient MFMAs read
__device__ __forceinline__ uint4 theta_to_h(uint4 w)
{
    union { uint4 u; f16x8 h; } in;
    in.u = w;
    Frag16 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out.v[j] = (__bf16)BRIEF_SIN_REV((float)in.h[j]);
    return out.u;
}

// one layer's GEMM: acc[t][st] += A(mt_t, :) * image(st), A fragments PD steps ahead from L2
// CPRE: once the chain has issued its last A loads, request the next epilogue's 16 stash words (c of the wave's
// first feature tile).  VMEM results return in order, so issued any earlier they would hold up the A fragments
// (L2 hits) behind an HBM round trip; issued here they have the last PD steps and nothing waits behind them.
template <int NT, int NS, int NW, bool CPRE, int MTW_ = NT / NW>
__device__ __forceinline__ void chain16(f32x16 (&acc)[MTW_][NS], __amdgpu_buffer_rsrc_t rs, int soff_block /*bytes*/,
                                        const uint4 *IMG, int wave, int lane,
                                        __amdgpu_buffer_rsrc_t rcn, int voff_c, u32x2 (&cpre)[16])
{
    using K = Cfg16<NT, NS, NW>;
    constexpr int NIT = NT * 2;      // (kt, s) steps
    constexpr int PD = K::MTW > 2 ? 2 : 4;
    const int voff = lane * 16;
    int soff_w = __builtin_amdgcn_readfirstlane(soff_block + wave * K::MTW * (NT * 2 * 1024));    // provably wave-uniform for the "+s" pin
    asm volatile("" : "+s"(soff_w));
    uint4 areg[NIT][K::MTW];
    uint4 breg[NS];
    // two LDS base addresses cover the whole image with 16-bit immediate offsets (sample tiles 0-1 | 2-3);
    // pinned so that the compiler does not materialise (and spill) one address register per far offset
    int o01 = lane * 16, o23 = lane * 16 + 2 * NT * 2 * 1024;          // byte offsets (opaque integers: the pointers stay LDS pointers)
    asm volatile("" : "+v"(o01));
    asm volatile("" : "+v"(o23));
    const uint4 *I01 = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(IMG) + o01);
    const uint4 *I23 = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(IMG) + o23);
#define IMG_AT(st, it) ((st) < 2 ? I01[((st) * NT * 2 + (it)) * 64] : I23[(((st) - 2) * NT * 2 + (it)) * 64])
#pragma unroll
    for (int it = 0; it < PD; ++it)
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + (t * NT * 2 + it) * 1024, 0);
            areg[it][t] = make_uint4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
    for (int st = 0; st < NS; ++st) breg[st] = IMG_AT(st, 0);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (it + PD < NIT) {
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + (t * NT * 2 + it + PD) * 1024, 0);
                areg[it + PD][t] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }
        if (CPRE && it + PD == NIT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cpre[r] = stash_get<NS>(rcn, voff_c, ((r & 3) + 8 * (r >> 2)) * 128);
        }
        __builtin_amdgcn_sched_barrier(0);
        // sample-tile major: once both feature tiles have used a B fragment its registers take the next step's
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            Frag16 fb; fb.u = breg[st];
#pragma unroll
            for (int t = 0; t < K::MTW; ++t) {
                Frag16 fa; fa.u = areg[it][t];
                acc[t][st] = MFMA16(fa.v, fb.v, acc[t][st]);
            }
            if (it + 1 < NIT) breg[st] = IMG_AT(st, it + 1);
        }
    }
#undef IMG_AT
}

// The chain of ONE of the wave's two feature tiles (MTW == 2), optionally with the forward epilogue of the OTHER tile riding in
// its MFMA gaps.  Measured (tools/coissue_ubench.hip, profiles/r03_coissue.md): a v_mfma_f32_32x32x16_bf16 occupies the matrix
// pipe for 32 cycles but the SIMD's issue port for ~8, and ~4 VALU instructions (or 2 transcendentals) issued behind it are free,
// from the same wave or from its SIMD mate.  An epilogue that runs AFTER its chain (round 2) has no MFMA to hide behind: every wave
// of the workgroup is between the same two barriers.  So the wave's chain is cut in two: tile 0 first, then tile 1 with tile 0's
// sines, cosines, bf16 packing and stash stores spread over its 32 k-steps (per MFMA: 1 transcendental + ~1 VALU + 1/4 store).
// Only tile 1's epilogue stays exposed, and the SIMD mate — whose chain the arbiter lets finish later — covers most of that.
// Price: the image is read twice (B fragments feed one feature tile instead of two: 128 instead of 64 B/clk/CU of LDS reads).
//   EPI == 0: plain chain.
//   EPI == 1: forward epilogue of `prev` (the other tile's finished accumulators = phases in revolutions): sin in place, cos,
//             stash h | c rows (TRAIN), bf16 fragments of h into fragw (they go to the image after the barrier that ends this chain).
template <int NT, int NS, int NW, bool TRAIN, int EPI>
__device__ __forceinline__ void chain16_tile(f32x16 (&acc)[NS], int tsel, __amdgpu_buffer_rsrc_t rs, int soff_block /*bytes*/,
                                             const uint4 *IMG, int wave, int lane,
                                             f32x16 (&prev)[NS], uint32_t (&fragw)[NS][8],
                                             __amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rc, int voff_s, int prev_row0 /* 32 * tile index of prev inside the wave */)
{
    constexpr int NIT = NT * 2;      // (kt, s) steps
    constexpr int PD = 8;            // one 1 KiB A fragment per step: eight steps = 1024 MFMA cycles of cover for an L2 hit
    const int voff = lane * 16;
    int soff_w = __builtin_amdgcn_readfirstlane(soff_block + (wave * 2 + tsel) * (NT * 2 * 1024));
    asm volatile("" : "+s"(soff_w));
    uint4 areg[NIT];
    uint4 breg[NS];
    int o01 = lane * 16, o23 = lane * 16 + 2 * NT * 2 * 1024;
    asm volatile("" : "+v"(o01));
    asm volatile("" : "+v"(o23));
    const uint4 *I01 = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(IMG) + o01);
    const uint4 *I23 = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(IMG) + o23);
#define IMG_AT(st, it) ((st) < 2 ? I01[((st) * NT * 2 + (it)) * 64] : I23[(((st) - 2) * NT * 2 + (it)) * 64])
#pragma unroll
    for (int it = 0; it < PD; ++it) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + it * 1024, 0);
        areg[it] = make_uint4(v.x, v.y, v.z, v.w);
    }
#pragma unroll
    for (int st = 0; st < NS; ++st) breg[st] = IMG_AT(st, 0);
    float ck[NS];                    // the phases of the NS neighbouring samples of one feature row: one stash word
#pragma unroll
    for (int st = 0; st < NS; ++st) ck[st] = 0.f;
    (void)rc;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (it + PD < NIT) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff_w + (it + PD) * 1024, 0);
            areg[it + PD] = make_uint4(v.x, v.y, v.z, v.w);
        }
        __builtin_amdgcn_sched_barrier(0);
        Frag16 fa; fa.u = areg[it];
        // One MFMA per slot, each slot closed by a scheduling barrier: left to itself hipcc issues the k-step's four MFMAs back to
        // back and puts all of the step's epilogue work into ONE gap (~100 issue cycles behind a 32-cycle MFMA), which hides
        // nothing.  Slot j of a k-step carries: fract + sine of one element (two k-steps per accumulator register r: the lower
        // half of the sample tiles first, then the rest), and on the register's second step the stash word of row r (its NS
        // phases as fp16) and (r odd) the packing of rows r - 1, r into the image fragments.
        const int r = it >> 1, half = it & 1;
        constexpr int H0 = (NS + 1) / 2;
        const int lo = half == 0 ? 0 : H0;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            Frag16 fb; fb.u = breg[st];
            acc[st] = MFMA16(fa.v, fb.v, acc[st]);
            if (it + 1 < NIT) breg[st] = IMG_AT(st, it + 1);
            if (EPI == 1 && it < 32) {
                const int e = lo + st;                       // the element this slot converts (if the half has that many)
                if (e < (half == 0 ? H0 : NS)) {
                    const float fr = __builtin_amdgcn_fractf(prev[e][r]);
                    if (TRAIN) ck[e] = fr;                     // the phase: what the stash keeps
                    prev[e][r] = BRIEF_SIN_REV(fr);
                }
                if (half == 1) {
                    const int soff = (prev_row0 + (r & 3) + 8 * (r >> 2)) * 128;
                    if (TRAIN && st == NS - 1) theta_put<NS>(rh, voff_s, soff, ck);
                    if ((r & 1) && st == NS - 1) {
#pragma unroll
                        for (int sx = 0; sx < NS; ++sx) {
                            union { uint32_t u; bf16x2 v; } pk2;
                            pk2.v[0] = (__bf16)prev[sx][r - 1]; pk2.v[1] = (__bf16)prev[sx][r];
                            fragw[sx][r >> 1] = pk2.u;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#undef IMG_AT
}

// registers 8s .. 8s+7 of an accumulator tile -> the bf16 fragment of k-step s
__device__ __forceinline__ uint4 pack_frag(const f32x16 &x, int s)
{
    Frag16 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = (__bf16)x[8 * s + j];
    return f.u;
}

template <int NT, int NS, int NW, int MTW_ = NT / NW>
__device__ __forceinline__ void write_image16(uint4 *IMG, const f32x16 (&h)[MTW_][NS], int wave, int lane)
{
    using K = Cfg16<NT, NS, NW>;
#pragma unroll
    for (int t = 0; t < K::MTW; ++t) {
        const int kt = wave * K::MTW + t;
#pragma unroll
        for (int st = 0; st < NS; ++st)
#pragma unroll
            for (int s = 0; s < 2; ++s) IMG[((st * NT + kt) * 2 + s) * 64 + lane] = pack_frag(h[t][st], s);
    }
}

template <int NT, bool TRAIN, int CO /* 1: data_channel == 1; 4: any */, int NS /* 32-sample tiles per workgroup tile */, int NW = 8,
          bool BOX = false /* inference over a box of the grid (box_coords) */>
__global__ __launch_bounds__(64 * NW, 1) void k16(const typename KArgsT<BOX>::type a)
{
    static_assert(!(TRAIN && BOX), "the box mapping is an inference instantiation");
#ifdef BRIEF_STAMPS
    float st_acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long st_last = clock64();
#endif
    using K = Cfg16<NT, NS, NW>;
    constexpr int MTW = K::MTW, FP = K::FP, TS = 32 * NS;      // TS: samples per workgroup tile
    static_assert(TS <= 64 * NW, "one thread per sample fetches the tile's inputs");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    uint4 *IMG = reinterpret_cast<uint4 *>(smem);
    float *HW = smem + K::HW_OFF;
    float4 *INX = reinterpret_cast<float4 *>(smem + K::IN_OFF);
    float4 *INY = INX + TS, *INW = INX + 2 * TS;
    float4 *PART = reinterpret_cast<float4 *>(smem + K::PART_OFF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const brief_siren_desc &d = a.d;
    const int L = d.layers, cin = d.cin, cout = CO == 1 ? 1 : d.cout;
    const int64_t npad = a.npad;
    const float *pk = a.pk;
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const int64_t pk16_bytes = (brief_pk_count(d) - brief_pk16_off(d, 1)) * 4;
    const __amdgpu_buffer_rsrc_t rs16 =
        __builtin_amdgcn_make_buffer_rsrc((void *)(pk + brief_pk16_off(d, 1)), 0, (int)pk16_bytes, 0x00020000);
    const int layer16_bytes = FP * FP * 4;               // Wf16 | Wb16 of one layer
    const int stash_bytes = (a.diag & 1) ? 0 : (int)((int64_t)FP * npad * 2);   // one plane [npad/64][FP][64] bf16 (host checks < 2^31)

    {
        const float *headp = pk + brief_pk_head(d);
        for (int e = tid; e < 4 * FP + 4; e += 64 * NW) HW[e] = headp[e];
    }
    float lsum = 0.f;
    float gsum[4] = {0.f, 0.f, 0.f, 0.f};
    const float inv_beta = 1.0f / a.beta;
    if (NW == 4) {
        // de-phase the two co-resident workgroups (as k_fused does): started together they would alternate between
        // their MFMA chains and their epilogues in lockstep
        const int slot = blockIdx.x / a.stagger_cus;
        for (int i = 0; i < slot * a.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    }
    __syncthreads();

    // this launch covers samples [n_begin, n_end), a multiple of TS apart; the last launch runs to the padded batch size
    // so that every stash column the weight-gradient GEMM reads has been written (padding samples carry delta = 0)
    const int64_t ntiles = a.n_end > a.n_begin ? (a.n_end - a.n_begin + TS - 1) / TS : 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = a.n_begin + tile * TS;
        // ---- inputs of the tile's samples, once per workgroup
        if (tid < TS) {
            float4 xi, yi, wi;
            small_inputs<BOX>((kargs_t)__builtin_amdgcn_kernarg_segment_ptr(), a.idx, a.rng_step, cin, cout, n0 + tid, xi, yi, wi);
            INX[tid] = xi; INY[tid] = yi; INW[tid] = wi;
            if (TRAIN) {
                // coordinates as the B operand of the first-layer gradient job: rows x0, x1, x2, 1
                __bf16 *X16 = reinterpret_cast<__bf16 *>(a.S16[3]);
                X16[0 * npad + n0 + tid] = (__bf16)xi.x;
                X16[1 * npad + n0 + tid] = (__bf16)xi.y;
                X16[2 * npad + n0 + tid] = (__bf16)xi.z;
                X16[3 * npad + n0 + tid] = (__bf16)1.0f;
            }
        }
        __syncthreads();
        f32x16 acc[MTW][NS];
        // ---- layer 0 in f32: two K=2 MFMAs against [x0 x1 | x2 1]
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            const float4 x = INX[NS * ln + st];
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                const float4 w = W0p[32 * (wave * MTW + t) + ln];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][st][r] = 0.f;
                acc[t][st] = MFMA(hi ? w.y : w.x, hi ? x.y : x.x, acc[t][st]);
                acc[t][st] = MFMA(hi ? w.w : w.z, hi ? 1.0f : x.z, acc[t][st]);
            }
        }
        // stash byte offset of this lane's 4 samples in feature row 4 hi: block (n0 + 4 ln) / 64, 128 B per row
        // (the wave's first feature row is folded in, so the per-register row offsets below are compile-time constants)
        STAMP(0)
        u32x2 cpre[16];          // c_l of this wave's first feature tile, requested one phase ahead (TRAIN)
        const int64_t s0 = n0 + NS * ln;                      // this lane's first sample
        const int voff_s = (int)((s0 >> 6) * (FP * 128)) + (int)(s0 & 63) * 2 + (hi * 4 + wave * MTW * 32) * 128;
        // ---- sine layers 0 .. L-2
        for (int l = 0; l <= L - 2; ++l) {
            // h = sin(theta) in place, theta = fract of the accumulator: the accumulator IS the phase in revolutions (the weights
            // carry om / 2 pi, brief_layout.h).  TRAIN: stash theta as fp16, four neighbouring samples per store.  The factor om of
            // om cos(om z) lives in the bf16 copy of W^T (k_repack).
            __amdgpu_buffer_rsrc_t rh, rc;
            if (TRAIN) rh = __builtin_amdgcn_make_buffer_rsrc((void *)(reinterpret_cast<_Float16 *>(a.S16[0]) + (int64_t)l * FP * npad), 0, stash_bytes, 0x00020000);
            else rh = rs16;
            rc = rh;
            constexpr bool SPLIT = MTW == 2 && NW == 8;      // tile 0's epilogue rides in tile 1's chain (chain16_tile)
            int t_first = 0;                                  // first feature tile whose epilogue still has to run below
            if (l > 0) {
                const float *bp_ = pk + brief_pk_hidden(d, l) + 2 * FP * FP;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 b4 = *reinterpret_cast<const float4 *>(bp_ + 32 * (wave * MTW + t) + 8 * q + 4 * hi);
#pragma unroll
                        for (int st = 0; st < NS; ++st) {
                            acc[t][st][4 * q] = b4.x; acc[t][st][4 * q + 1] = b4.y;
                            acc[t][st][4 * q + 2] = b4.z; acc[t][st][4 * q + 3] = b4.w;
                        }
                    }
                }
                if constexpr (SPLIT) {
                    uint32_t fragw[NS][8];
#pragma unroll
                    for (int st = 0; st < NS; ++st)
#pragma unroll
                        for (int j = 0; j < 8; ++j) fragw[st][j] = 0u;
                    chain16_tile<NT, NS, NW, TRAIN, 0>(acc[0], 0, rs16, (l - 1) * layer16_bytes, IMG, wave, lane, acc[0], fragw, rh, rc, voff_s, 0);
                    chain16_tile<NT, NS, NW, TRAIN, 1>(acc[1], 1, rs16, (l - 1) * layer16_bytes, IMG, wave, lane, acc[0], fragw, rh, rc, voff_s, 0);
                    STAMP(1)
                    lds_barrier();      // every wave is done reading the previous image
                    STAMP(2)
                    // tile 0's h fragments were packed inside the chain: publish them now
#pragma unroll
                    for (int st = 0; st < NS; ++st)
#pragma unroll
                        for (int sx = 0; sx < 2; ++sx)
                            IMG[((st * NT + wave * MTW) * 2 + sx) * 64 + lane] = make_uint4(fragw[st][4 * sx], fragw[st][4 * sx + 1], fragw[st][4 * sx + 2], fragw[st][4 * sx + 3]);
                    t_first = 1;
                } else {
                    chain16<NT, NS, NW, false>(acc, rs16, (l - 1) * layer16_bytes, IMG, wave, lane, rs16, 0, cpre);
                    STAMP(1)
                    lds_barrier();      // every wave is done reading the previous image
                    STAMP(2)
                }
            }
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                if (t < t_first) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float th[NS];
#pragma unroll
                    for (int st = 0; st < NS; ++st) {
                        th[st] = __builtin_amdgcn_fractf(acc[t][st][r]);
                        acc[t][st][r] = BRIEF_SIN_REV(th[st]);
                    }
                    if (TRAIN) theta_put<NS>(rh, voff_s, (32 * t + (r & 3) + 8 * (r >> 2)) * 128, th);
                }
                const int kt = wave * MTW + t;
#pragma unroll
                for (int st = 0; st < NS; ++st)
#pragma unroll
                    for (int sx = 0; sx < 2; ++sx) IMG[((st * NT + kt) * 2 + sx) * 64 + lane] = pack_frag(acc[t][st], sx);
            }
            STAMP(3)
            lds_barrier();
            STAMP(4)
        }
        if (TRAIN && (NS == 4 || NW == 4)) {
            const __amdgpu_buffer_rsrc_t rct =
                __builtin_amdgcn_make_buffer_rsrc((void *)(reinterpret_cast<_Float16 *>(a.S16[0]) + (int64_t)(L - 2) * FP * npad), 0, stash_bytes, 0x00020000);
#pragma unroll
            for (int r = 0; r < 16; ++r) cpre[r] = stash_get<NS>(rct, voff_s, ((r & 3) + 8 * (r >> 2)) * 128);
        }
        // ---- head: partial dot products over this wave's features, summed over the 8 waves through LDS
        {
            float p[NS][CO];
#pragma unroll
            for (int st = 0; st < NS; ++st)
#pragma unroll
                for (int c = 0; c < CO; ++c) p[st][c] = 0.f;
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                if (c < cout) {
#pragma unroll
                    for (int t = 0; t < MTW; ++t) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 wv = *reinterpret_cast<const float4 *>(HW + c * FP + 32 * (wave * MTW + t) + 8 * q + 4 * hi);
#pragma unroll
                            for (int st = 0; st < NS; ++st) {
                                p[st][c] = __fmaf_rn(wv.x, acc[t][st][4 * q], p[st][c]);
                                p[st][c] = __fmaf_rn(wv.y, acc[t][st][4 * q + 1], p[st][c]);
                                p[st][c] = __fmaf_rn(wv.z, acc[t][st][4 * q + 2], p[st][c]);
                                p[st][c] = __fmaf_rn(wv.w, acc[t][st][4 * q + 3], p[st][c]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int st = 0; st < NS; ++st) {
#pragma unroll
                for (int c = 0; c < CO; ++c) p[st][c] += __shfl_xor(p[st][c], 32);
                if (hi == 0) {
                    if (CO == 1) reinterpret_cast<float *>(PART)[(wave * NS + st) * 32 + ln] = p[st][0];
                    else PART[(wave * NS + st) * 32 + ln] = make_float4(p[st][0], p[st][CO > 1 ? 1 : 0], p[st][CO > 2 ? 2 : 0], p[st][CO > 3 ? 3 : 0]);
                }
            }
        }
        lds_barrier();
        float zo[NS][CO], yh[NS][CO], g[NS][CO];
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            if (CO == 1) {
                float sum = HW[4 * FP];
#pragma unroll
                for (int w = 0; w < NW; ++w) sum += reinterpret_cast<const float *>(PART)[(w * NS + st) * 32 + ln];
                zo[st][0] = sum;
            } else {
                float4 sum = make_float4(HW[4 * FP], HW[4 * FP + 1], HW[4 * FP + 2], HW[4 * FP + 3]);
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const float4 v = PART[(w * NS + st) * 32 + ln];
                    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
                }
                zo[st][0] = sum.x; zo[st][CO > 1 ? 1 : 0] = sum.y; zo[st][CO > 2 ? 2 : 0] = sum.z; zo[st][CO > 3 ? 3 : 0] = sum.w;
            }
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                yh[st][c] = d.output_act ? brief_fast_sinf(d.w0_hidden * zo[st][c]) : zo[st][c];
                g[st][c] = 0.f;
            }
        }
        if (!TRAIN) {
            if (wave == 0 && hi == 0) {
#pragma unroll
                for (int st = 0; st < NS; ++st) {
                    const int64_t n = n0 + NS * ln + st;
                    if (n < a.n) {
#pragma unroll
                        for (int c = 0; c < CO; ++c) {
                            if (c >= cout) break;
                            if (a.out_kind == BRIEF_OUT_F32) {
                                reinterpret_cast<float *>(a.out)[n * cout + c] = yh[st][c];
                            } else {
                                float t = __fsub_rn(yh[st][c], a.scale_min);
                                t = __fdiv_rn(t, a.den);
                                t = fminf(fmaxf(t, 0.f), 1.f);
                                const float u = __fadd_rn(__fmul_rn(t, a.span), a.vmin);
                                if (a.out_kind == BRIEF_OUT_U16) reinterpret_cast<uint16_t *>(a.out)[n * cout + c] = (uint16_t)(int)u;
                                else reinterpret_cast<uint8_t *>(a.out)[n * cout + c] = (uint8_t)(int)u;
                            }
                        }
                    }
                }
            }
            lds_barrier();      // IN / PART / image are rewritten by the next tile
            continue;
        }
        // ---- loss and dloss/dyhat (main.py:176-191); every wave needs g, wave 0 keeps the sums and the stash rows
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            const int64_t n = n0 + NS * ln + st;
            const float4 yv4 = INY[NS * ln + st], wv44 = INW[NS * ln + st];
            const float yv[4] = {yv4.x, yv4.y, yv4.z, yv4.w}, wv[4] = {wv44.x, wv44.y, wv44.z, wv44.w};
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                if (c < cout && n < a.n) {
                    float we = wv[c];
                    if (a.thr != 0.f && yh[st][c] <= a.thr) we = 1.0f;
                    const float df = yh[st][c] - yv[c];
                    float li, gi;
                    if (a.loss_kind == BRIEF_LOSS_L2) { li = df * df; gi = 2.0f * df; }
                    else if (a.loss_kind == BRIEF_LOSS_SMOOTHL1) {
                        const float ad = fabsf(df);
                        if (ad < a.beta) { li = 0.5f * df * df * inv_beta; gi = df * inv_beta; }
                        else { li = ad - 0.5f * a.beta; gi = df < 0.f ? -1.0f : 1.0f; }
                    } else { li = 0.f; gi = 0.f; }
                    g[st][c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yv[c] : gi * we * a.inv_count;
                    if (d.output_act) g[st][c] *= d.w0_hidden * brief_fast_cosf(d.w0_hidden * zo[st][c]);
                    if (wave == 0 && hi == 0) {
                        lsum += li * we;
                        gsum[c] += g[st][c];
                        if (a.yhat_out) a.yhat_out[n * cout + c] = yh[st][c];
                    }
                }
            }
        }
        if (wave == 0 && hi == 0) {
            __bf16 *G16 = reinterpret_cast<__bf16 *>(a.S16[4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int st = 0; st < NS; ++st) G16[c * npad + n0 + NS * ln + st] = (__bf16)(c < CO ? g[st][c < CO ? c : 0] : 0.f);
            }
        }
        // ---- delta of the last sine layer: c_{L-2} . (Wh^T g); then layers L-2 .. 1: stash delta, dgrad, times c_{l-1}
        const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int st = 0; st < NS; ++st) {
                    float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int c = 0; c < CO; ++c) {
                        if (c < cout) {
                            const float4 wv = *reinterpret_cast<const float4 *>(HW + c * FP + 32 * (wave * MTW + t) + 8 * q + 4 * hi);
                            sacc.x = __fmaf_rn(wv.x, g[st][c], sacc.x); sacc.y = __fmaf_rn(wv.y, g[st][c], sacc.y);
                            sacc.z = __fmaf_rn(wv.z, g[st][c], sacc.z); sacc.w = __fmaf_rn(wv.w, g[st][c], sacc.w);
                        }
                    }
                    // (deeper layers get their om through the scaled W^T copy, this one here)
                    acc[t][st][4 * q] = om_top * sacc.x; acc[t][st][4 * q + 1] = om_top * sacc.y;
                    acc[t][st][4 * q + 2] = om_top * sacc.z; acc[t][st][4 * q + 3] = om_top * sacc.w;
                }
            }
        }
        STAMP(5)
        for (int l = L - 2; l >= 0; --l) {
            // acc holds (W_{l+1}^T delta_{l+1}) (or Wh^T g): delta_l = acc . c_l.  c_l of the wave's first feature tile
            // was requested before the chain / the head (cpre), the second tile's is requested now and lands while
            // the first is being multiplied and stashed: the stash reads are HBM round trips, never waited on one by one
            {
                const __amdgpu_buffer_rsrc_t rc =
                    __builtin_amdgcn_make_buffer_rsrc((void *)(reinterpret_cast<_Float16 *>(a.S16[0]) + (int64_t)l * FP * npad), 0, stash_bytes, 0x00020000);
                const __amdgpu_buffer_rsrc_t rd =
                    __builtin_amdgcn_make_buffer_rsrc((void *)(reinterpret_cast<__bf16 *>(a.S16[2]) + (int64_t)l * FP * npad), 0, stash_bytes, 0x00020000);
                if (NS < 4 && NW == 8) {       // tail launches: no request-ahead (the compiler's backend rejects it inside the chain for these widths)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cpre[r] = stash_get<NS>(rc, voff_s, ((r & 3) + 8 * (r >> 2)) * 128);
                }
                // c of feature tile t + 1 is requested while tile t is multiplied and stashed
                u32x2 cnext[16];
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (t + 1 < MTW) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) cnext[r] = stash_get<NS>(rc, voff_s, (32 * (t + 1) + (r & 3) + 8 * (r >> 2)) * 128);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int soff = (32 * t + (r & 3) + 8 * (r >> 2)) * 128;
                        const u32x2 cw = cpre[r];
                        float dv[NS];
#pragma unroll
                        for (int st = 0; st < NS; ++st) { acc[t][st][r] *= BRIEF_COS_REV(theta_val(cw, st)); dv[st] = acc[t][st][r]; }
                        stash_put<NS>(rd, voff_s, soff, dv);
                    }
                    if (t + 1 < MTW) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) cpre[r] = cnext[r];
                    }
                }
            }
            STAMP(6)
            if (l == 0) break;
            lds_barrier();      // the previous chain (or the head) is done with the image
            write_image16<NT, NS, NW>(IMG, acc, wave, lane);
            lds_barrier();
            STAMP(7)
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int st = 0; st < NS; ++st)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][st][r] = 0.f;
            {
                const __amdgpu_buffer_rsrc_t rcn =
                    __builtin_amdgcn_make_buffer_rsrc((void *)(reinterpret_cast<_Float16 *>(a.S16[0]) + (int64_t)(l - 1) * FP * npad), 0, stash_bytes, 0x00020000);
                chain16<NT, NS, NW, NS == 4 || NW == 4>(acc, rs16, (l - 1) * layer16_bytes + FP * FP * 2, IMG, wave, lane, rcn, voff_s, cpre);
            }
            STAMP(8)
        }
        lds_barrier();          // IN / PART / image are rewritten by the next tile
        STAMP(9)
    }
    if (TRAIN && wave == 0) {
        float *rec = a.rec + ((int64_t)a.rec_base + blockIdx.x) * 8;      // [loss, dbh[4]] per workgroup
        for (int off = 16; off >= 1; off >>= 1) {
            lsum += __shfl_xor(lsum, off);
#pragma unroll
            for (int c = 0; c < 4; ++c) gsum[c] += __shfl_xor(gsum[c], off);
        }
        if (lane == 0) {
            rec[0] = lsum;
#pragma unroll
            for (int c = 0; c < 4; ++c) rec[1 + c] = gsum[c];
        }
    }
#ifdef BRIEF_STAMPS
    if (TRAIN && lane == 0) for (int i = 0; i < 10; ++i) a.rec[(int64_t)2 * a.stagger_cus * 8 + ((int64_t)blockIdx.x * NW + wave) * 10 + i] = st_acc[i];
#endif
}

// ---------------------------------------------------------------------------------------------
// weight gradients from the bf16 stashes.  Job j of a launch:
//   j = 0 .. hidden-1 : dW_{j+1}[fo][fi] = sum_n D_{j+1}[fo][n] H_j[fi][n]     (+ db_{j+1} = sum_n D_{j+1})
//   j = hidden        : dW_0[f][c]       = sum_n D_0[f][n] X[c][n]             (X = x0, x1, x2, 1: column 3 is db_0)
//   j = hidden + 1    : dWh^T[f][c]      = sum_n H_{L-2}[f][n] G[c][n]
// Workgroup = 4 waves as 2 x 2, wave tile 64 x 64 (hidden) or 64 x 32 (skinny), split-K over 64-sample blocks.
// A and B fragments are 16 contiguous bytes of a stash line (8 consecutive samples of one feature).  The 128-row
// panels of a block are contiguous 16 KB pieces of the stash: they are copied with fully coalesced loads, a
// block ahead, into double-buffered padded LDS panels, and the fragments come from there.
struct Wgrad16Args {
    brief_siren_desc d;
    const __bf16 *H, *D, *X, *G;
    int64_t npad;
    int nsplit, nsplit_s; // K splits of the hidden jobs / of the two skinny jobs
    int bias_jobs;        // 1: db_l comes from bias jobs of the skinny launch (FP = 512); 0: from the hidden kernel's ones-MFMA
    // k_wgrad16_big only: this launch covers the 64-sample blocks [kb_lo, kb_hi) in nsplit_here K splits, which fill the slabs split_lo ..
    // split_lo + nsplit_here - 1 of the nsplit every layer has (one launch: 0, npad / 64, 0, nsplit; the body / tail pair of the overlap plan:
    // brief_hip.hip, Split16Plan)
    int64_t kb_lo, kb_hi;
    int split_lo, nsplit_here;
    float *slabs;        // [(L-2)][nsplit][FP*FP + FP]  then  [nsplit_s][FP*4] (first layer)  then  [nsplit_s][FP*4] (head)
};

#define W16_LDSW 36                      // panel row stride in dwords (128 B of samples + 16 B pad): conflict-free ds_read_b128
#define W16_PANEL (128 * W16_LDSW)       // dwords per 128-row panel

// SKINNY = false: hidden-layer jobs on 128 x 128 output blocks, bias gradients through an all-ones B fragment in the
//                 first column of waves (used for FP = 256; FP = 512 goes to k_wgrad16_big).
// SKINNY = true : 64 x 32 wave tiles whose B fragments live in registers: the first-layer and head jobs (B = rows of
//                 X | G) and, for FP = 512 (bias_jobs), the hidden layers' bias gradients (B = all ones, written into
//                 the hidden slabs' bias rows: k_wgrad16_big has no registers left for them).
template <bool SKINNY>
__global__ __launch_bounds__(256, 2) void k_wgrad16(const Wgrad16Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [2 buffers][A panel | B panel]
    const brief_siren_desc &d = a.d;
    const int NT = brief_nt(d), FP = 32 * NT, hidden = d.layers - 2;
    const int nb = FP / 128;                                  // 128-row blocks per side
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 31, hi = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    // decode block -> (job, block row, block col, split)
    int b = blockIdx.x;
    int job, br, bc, split, nsplit;
    bool bias_job = false;
    if (!SKINNY) {
        const int per_hidden = nb * nb * a.nsplit;
        job = b / per_hidden; b %= per_hidden;
        split = b % a.nsplit; b /= a.nsplit;
        br = b / nb; bc = b % nb; nsplit = a.nsplit;
    } else if (a.bias_jobs && b < hidden * nb * a.nsplit) {
        bias_job = true;
        job = b / (nb * a.nsplit); b %= nb * a.nsplit;
        split = b % a.nsplit; br = b / a.nsplit; bc = 0; nsplit = a.nsplit;
    } else {
        if (a.bias_jobs) b -= hidden * nb * a.nsplit;
        job = hidden + b / (nb * a.nsplit_s); b %= nb * a.nsplit_s;
        split = b % a.nsplit_s; br = b / a.nsplit_s; bc = 0; nsplit = a.nsplit_s;
    }
    constexpr bool skinny = SKINNY;
    const int64_t npad = a.npad;
    const int64_t plane = (int64_t)FP * npad;
    const __bf16 *Ab, *Bb;
    if (job < hidden) { Ab = a.D + (int64_t)(job + 1) * plane; Bb = SKINNY ? a.X : a.H + (int64_t)job * plane; }
    else if (job == hidden) { Ab = a.D; Bb = a.X; }
    else { Ab = a.H + (int64_t)(d.layers - 2) * plane; Bb = a.G; }
    const bool a_is_theta = __builtin_amdgcn_readfirstlane(SKINNY && !bias_job && job == hidden + 1);      // the head job's A rows are the last sine layer's phases
    const int64_t nblk = npad / 64;                            // 64-sample blocks: one 128-byte line per (feature, block)
    const int64_t b0 = nblk * split / nsplit, b1 = nblk * (split + 1) / nsplit;     // b1 > b0 (host: nsplit <= nblk)

    // A 128-row panel of one block is 16 KB of contiguous stash: thread t copies uint4 t, t+256, t+512, t+768
    // (row = idx / 8, 16-byte chunk = idx % 8) into the padded LDS panel.  Skinny B operands (X, G: [4][npad]
    // rows) are read straight from global memory: 16 bytes per lane.
    const uint4 *Ag = reinterpret_cast<const uint4 *>(Ab) + (int64_t)br * 128 * 8;
    const uint4 *Bg = reinterpret_cast<const uint4 *>(Bb) + (int64_t)bc * 128 * 8;
    const int64_t blk_u4 = (int64_t)FP * 8;                    // uint4 per 64-sample block of a plane
    const uint4 *Bs = reinterpret_cast<const uint4 *>(Bb) + (int64_t)(ln & 3) * (npad / 8) + hi;
    const int lds_w0 = (tid >> 3) * W16_LDSW + (tid & 7) * 4;
    const int fa_off = (wm * 64 + ln) * W16_LDSW + hi * 4;     // + 32 i rows, + 8 p dwords
    const int fb_off = W16_PANEL + (wn * 64 + ln) * W16_LDSW + hi * 4;

    f32x16 acc[2][2], accb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][0][r] = 0.f; acc[i][1][r] = 0.f; accb[i][r] = 0.f; }
    }
    Frag16 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones.v[j] = (__bf16)1.0f;
    const bool want_bias = !skinny && bc == 0 && wn == 0;      // db_l = D_l . ones, by the first column of waves

    // staging registers as named scalars (arrays indexed in macro loops ended up in scratch)
    uint4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
#define W16_ISSUE(kb)                                                                         \
    {                                                                                         \
        const int64_t kk_ = (kb) < b1 ? (kb) : b1 - 1;   /* clamped: the redundant copy is never used */ \
        const uint4 *ap_ = Ag + kk_ * blk_u4 + tid;                                           \
        sa0 = ap_[0]; sa1 = ap_[256]; sa2 = ap_[512]; sa3 = ap_[768];                         \
        if (!skinny) {                                                                        \
            const uint4 *bp_ = Bg + kk_ * blk_u4 + tid;                                       \
            sb0 = bp_[0]; sb1 = bp_[256]; sb2 = bp_[512]; sb3 = bp_[768];                     \
        } else if (bias_job) {                                                                \
            sb0 = ones.u; sb1 = ones.u; sb2 = ones.u; sb3 = ones.u;                           \
        } else {                                                                              \
            const uint4 *bp_ = Bs + kk_ * 8;             /* k-steps 0..3 of the block */      \
            sb0 = bp_[0]; sb1 = bp_[2]; sb2 = bp_[4]; sb3 = bp_[6];                           \
        }                                                                                     \
    }
    /* the activation operand arrives as fp16 phases (k16's stash): h = sin(2 pi theta), taken on the way into LDS */ \
#define W16_STAGE(buf)                                                                        \
    {                                                                                         \
        float *pa_ = smem + (buf) * 2 * W16_PANEL + lds_w0;                                   \
        if (a_is_theta) { sa0 = theta_to_h(sa0); sa1 = theta_to_h(sa1); sa2 = theta_to_h(sa2); sa3 = theta_to_h(sa3); } \
        *reinterpret_cast<uint4 *>(pa_) = sa0;                                                \
        *reinterpret_cast<uint4 *>(pa_ + 32 * W16_LDSW) = sa1;                                \
        *reinterpret_cast<uint4 *>(pa_ + 64 * W16_LDSW) = sa2;                                \
        *reinterpret_cast<uint4 *>(pa_ + 96 * W16_LDSW) = sa3;                                \
        if (!skinny) {                                                                        \
            *reinterpret_cast<uint4 *>(pa_ + W16_PANEL) = theta_to_h(sb0);                    \
            *reinterpret_cast<uint4 *>(pa_ + W16_PANEL + 32 * W16_LDSW) = theta_to_h(sb1);    \
            *reinterpret_cast<uint4 *>(pa_ + W16_PANEL + 64 * W16_LDSW) = theta_to_h(sb2);    \
            *reinterpret_cast<uint4 *>(pa_ + W16_PANEL + 96 * W16_LDSW) = theta_to_h(sb3);    \
        }                                                                                     \
    }
    W16_ISSUE(b0)
    W16_STAGE(0)
    uint4 k0 = sb0, k1 = sb1, k2 = sb2, k3 = sb3;      // skinny: the B fragments of the block being multiplied
    lds_barrier();
    int cur = 0;
    for (int64_t kb = b0; kb < b1; ++kb) {
        W16_ISSUE(kb + 1)
        __builtin_amdgcn_sched_barrier(0);
        const float *pa = smem + cur * 2 * W16_PANEL;
#define W16_STEP(p, kf)                                                                       \
        {                                                                                     \
            Frag16 fa0, fa1, fb0, fb1;                                                        \
            fa0.u = *reinterpret_cast<const uint4 *>(pa + fa_off + 8 * (p));                  \
            fa1.u = *reinterpret_cast<const uint4 *>(pa + fa_off + 32 * W16_LDSW + 8 * (p));  \
            if (!skinny) {                                                                    \
                fb0.u = *reinterpret_cast<const uint4 *>(pa + fb_off + 8 * (p));              \
                fb1.u = *reinterpret_cast<const uint4 *>(pa + fb_off + 32 * W16_LDSW + 8 * (p)); \
            } else {                                                                          \
                fb0.u = (kf); fb1.u = (kf);                                                   \
            }                                                                                 \
            if (!skinny || wn == 0) {                                                         \
                acc[0][0] = MFMA16(fa0.v, fb0.v, acc[0][0]);                                  \
                acc[1][0] = MFMA16(fa1.v, fb0.v, acc[1][0]);                                  \
            }                                                                                 \
            if (!skinny) {                                                                    \
                acc[0][1] = MFMA16(fa0.v, fb1.v, acc[0][1]);                                  \
                acc[1][1] = MFMA16(fa1.v, fb1.v, acc[1][1]);                                  \
            }                                                                                 \
            if (!skinny && want_bias) {                                                       \
                accb[0] = MFMA16(fa0.v, ones.v, accb[0]);                                     \
                accb[1] = MFMA16(fa1.v, ones.v, accb[1]);                                     \
            }                                                                                 \
        }
        W16_STEP(0, k0) W16_STEP(1, k1) W16_STEP(2, k2) W16_STEP(3, k3)
#undef W16_STEP
        W16_STAGE(cur ^ 1)
        k0 = sb0; k1 = sb1; k2 = sb2; k3 = sb3;
        lds_barrier();
        cur ^= 1;
    }
#undef W16_ISSUE
#undef W16_STAGE
    const int64_t slab_h = (int64_t)FP * FP + FP;
    if (!skinny) {
        float *slab = a.slabs + ((int64_t)job * a.nsplit + split) * slab_h;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int jn = 0; jn < 2; ++jn)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(br * 128 + wm * 64 + 32 * i + ROWMAP(r, hi)) * FP + bc * 128 + wn * 64 + 32 * jn + ln] = acc[i][jn][r];
            if (want_bias && ln == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) slab[(int64_t)FP * FP + br * 128 + wm * 64 + 32 * i + ROWMAP(r, hi)] = accb[i][r];
            }
        }
    } else if (wn == 0) {
        if (bias_job) {
            float *slab = a.slabs + ((int64_t)job * a.nsplit + split) * slab_h + (int64_t)FP * FP;
            if (ln == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) slab[br * 128 + wm * 64 + 32 * i + ROWMAP(r, hi)] = acc[i][0][r];
            }
        } else {
            float *slab = a.slabs + (int64_t)hidden * a.nsplit * slab_h + ((int64_t)(job - hidden) * a.nsplit_s + split) * (FP * 4);
            if (ln < 4) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) slab[(br * 128 + wm * 64 + 32 * i + ROWMAP(r, hi)) * 4 + ln] = acc[i][0][r];
            }
        }
    }
}

// hidden-layer jobs for FP = 512: 256 x 256 output blocks, 512 threads = 8 waves as 4 (rows) x 2 (cols), wave tile
// 64 x 128.  Every stash plane is then read twice per layer instead of four times (this kernel is HBM-bound), and a
// fragment read from LDS feeds 1.33 MFMAs instead of 1 (94 instead of 170 B/clk/CU of LDS reads).  The first column of
// waves of the first block column also multiplies its delta rows with an all-ones fragment: db_l = D_l . 1 costs those
// waves 2 MFMAs more per k-step and no memory traffic (the separate bias jobs re-read every delta plane).
// Block order: the nb x nb blocks of one (layer, K split) get consecutive multiples of 8 apart in blockIdx, i.e. they are
// dispatched together onto ONE XCD (round-robin placement: speed only), so that the second reader of a panel finds it
// in that XCD's L2.
#define W16B_PANEL (256 * W16_LDSW)
__global__ __launch_bounds__(512, 1) void k_wgrad16_big(const Wgrad16Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [2 buffers][A panel | B panel], 256 rows each
    const brief_siren_desc &d = a.d;
    const int FP = 32 * brief_nt(d);
    const int nb = FP / 256;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 31, hi = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    // blockIdx = x + 8 (q + nq j): group g = x + 8 j (x: the XCD under round-robin placement), q = block inside the group;
    // the grid is padded to whole rounds of 8 groups, the surplus workgroups leave at once
    const int nq = nb * nb;
    int job, split, br, bc;
    {
        const int bid = blockIdx.x, x = bid & 7, rest = bid >> 3;
        const int q = rest % nq, g = x + 8 * (rest / nq);
        if (g >= (d.layers - 2) * a.nsplit_here) return;
        job = g / a.nsplit_here; split = g % a.nsplit_here;
        br = q / nb; bc = q % nb;
    }
    const int64_t npad = a.npad;
    const int64_t plane = (int64_t)FP * npad;
    const __bf16 *Ab = a.D + (int64_t)(job + 1) * plane, *Bb = a.H + (int64_t)job * plane;
    const int64_t nblk = a.kb_hi - a.kb_lo;
    const int64_t b0 = a.kb_lo + nblk * split / a.nsplit_here, b1 = a.kb_lo + nblk * (split + 1) / a.nsplit_here;      // b1 > b0 (host: nsplit_here <= blocks)
    const uint4 *Ag = reinterpret_cast<const uint4 *>(Ab) + (int64_t)br * 256 * 8;
    const uint4 *Bg = reinterpret_cast<const uint4 *>(Bb) + (int64_t)bc * 256 * 8;
    const int64_t blk_u4 = (int64_t)FP * 8;
    // thread t copies uint4 t + 512 i (i = 0..3) of a 256-row panel: row t/8 + 64 i, chunk t%8
    const int lds_w0 = (tid >> 3) * W16_LDSW + (tid & 7) * 4;
    const int fa_off = (wm * 64 + ln) * W16_LDSW + hi * 4;
    const int fb_off = W16B_PANEL + (wn * 128 + ln) * W16_LDSW + hi * 4;
    const bool want_bias = __builtin_amdgcn_readfirstlane(bc == 0);

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][0][r] = 0.f; acc[i][1][r] = 0.f; acc[i][2][r] = 0.f; acc[i][3][r] = 0.f; }
    // bias gradient db = row sums of the delta panel: taken by the thread that stages the row (4 rows x 8 samples per thread and
    // chunk) in the blocks of the first column — as two accumulator tiles of an all-ones MFMA it cost the 32 VGPRs that the second
    // staging register set below needs
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    // two staging register sets: the loads of chunk kb + 2 are in flight while chunk kb is multiplied and chunk kb + 1 is staged
    // (prefetch distance 2; together with leaving the fragment-read schedule to the compiler: -1.3 % on the 8x512 step, -2.4 % on
    // 5x384).  The kernel is memory-bound: without its loads, or without the staging that waits for them, it takes 202 us instead of
    // 377 us; it pulls 2.87 GB through L2 per launch, 1.9 GB of them from HBM (profiles/r02_bf16_c3_summary.md)
    uint4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
    uint4 ta0, ta1, ta2, ta3, tb0, tb1, tb2, tb3;
#define W16_ISSUE(kb, A, B)                                                                   \
    {                                                                                         \
        const int64_t kk_ = (kb) < b1 ? (kb) : b1 - 1;                                        \
        const uint4 *ap_ = Ag + kk_ * blk_u4 + tid;                                           \
        const uint4 *bp_ = Bg + kk_ * blk_u4 + tid;                                           \
        A##0 = ap_[0]; A##1 = ap_[512]; A##2 = ap_[1024]; A##3 = ap_[1536];                   \
        B##0 = bp_[0]; B##1 = bp_[512]; B##2 = bp_[1024]; B##3 = bp_[1536];                   \
    }
#define W16_ROWSUM(u) ((bf16_lo((u).x) + bf16_hi((u).x)) + (bf16_lo((u).y) + bf16_hi((u).y)) + ((bf16_lo((u).z) + bf16_hi((u).z)) + (bf16_lo((u).w) + bf16_hi((u).w))))
#define W16_STAGE(buf, A, B)                                                                  \
    {                                                                                         \
        float *pa_ = smem + (buf) * 2 * W16B_PANEL + lds_w0;                                  \
        *reinterpret_cast<uint4 *>(pa_) = A##0;                                               \
        *reinterpret_cast<uint4 *>(pa_ + 64 * W16_LDSW) = A##1;                               \
        *reinterpret_cast<uint4 *>(pa_ + 128 * W16_LDSW) = A##2;                              \
        *reinterpret_cast<uint4 *>(pa_ + 192 * W16_LDSW) = A##3;                              \
        *reinterpret_cast<uint4 *>(pa_ + W16B_PANEL) = B##0;                                  \
        *reinterpret_cast<uint4 *>(pa_ + W16B_PANEL + 64 * W16_LDSW) = B##1;                  \
        *reinterpret_cast<uint4 *>(pa_ + W16B_PANEL + 128 * W16_LDSW) = B##2;                 \
        *reinterpret_cast<uint4 *>(pa_ + W16B_PANEL + 192 * W16_LDSW) = B##3;                 \
        if (want_bias && count_rows) {                                                        \
            bsum[0] += W16_ROWSUM(A##0); bsum[1] += W16_ROWSUM(A##1);                         \
            bsum[2] += W16_ROWSUM(A##2); bsum[3] += W16_ROWSUM(A##3);                         \
        }                                                                                     \
    }
    /* MULTIPLY also turns the activation pieces of the NEXT staging set (fp16 phases, landed an iteration ago) into bf16     \
       h = sin(2 pi theta), one 16-byte piece per k-step: 8 transcendentals + 12 conversions behind 8 MFMAs ride in their      \
       issue gaps (profiles/r03_coissue.md); done at staging time they sat on the load -> LDS -> barrier path of a memory-bound \
       loop (444 us against 390) */                                                           \
#define W16_CONV(B, p) { if ((p) == 0) B##0 = theta_to_h(B##0); else if ((p) == 1) B##1 = theta_to_h(B##1); else if ((p) == 2) B##2 = theta_to_h(B##2); else B##3 = theta_to_h(B##3); }
#define W16_MULTIPLY(cur_, B)                                                                 \
    {                                                                                         \
        const float *pa = smem + (cur_) * 2 * W16B_PANEL;                                     \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                       \
            Frag16 fa0, fa1;                                                                  \
            fa0.u = *reinterpret_cast<const uint4 *>(pa + fa_off + 8 * p);                    \
            fa1.u = *reinterpret_cast<const uint4 *>(pa + fa_off + 32 * W16_LDSW + 8 * p);    \
            _Pragma("unroll") for (int jn = 0; jn < 4; ++jn) {                                \
                Frag16 fb;                                                                    \
                fb.u = *reinterpret_cast<const uint4 *>(pa + fb_off + 32 * jn * W16_LDSW + 8 * p); \
                acc[0][jn] = MFMA16(fa0.v, fb.v, acc[0][jn]);                                 \
                acc[1][jn] = MFMA16(fa1.v, fb.v, acc[1][jn]);                                 \
            }                                                                                 \
            W16_CONV(B, p)                                                                    \
        }                                                                                     \
    }
    // (the staged-row sums count a chunk when it is STAGED: the clamped re-loads past the last chunk are never staged twice,
    //  see the loop: every chunk b0 .. b1-1 passes through W16_STAGE exactly once)
    bool count_rows = true;                        // whether the chunk being staged is a new one (not the clamped re-load)
    W16_ISSUE(b0, sa, sb)
    sb0 = theta_to_h(sb0); sb1 = theta_to_h(sb1); sb2 = theta_to_h(sb2); sb3 = theta_to_h(sb3);
    W16_STAGE(0, sa, sb)
    W16_ISSUE(b0 + 1, sa, sb)
    lds_barrier();
    int cur = 0;
    for (int64_t kb = b0; kb < b1; kb += 2) {
        // every wave: request chunk kb + 2, multiply chunk kb (converting chunk kb + 1's phases in the MFMA gaps), stage chunk kb + 1
        count_rows = kb + 1 < b1;
        W16_ISSUE(kb + 2, ta, tb)                       // lands during this and the next half-iteration
        __builtin_amdgcn_sched_barrier(0);
        W16_MULTIPLY(cur, sb)
        W16_STAGE(cur ^ 1, sa, sb)                      // chunk kb + 1 (or, past the end, a copy nobody reads)
        lds_barrier();
        count_rows = kb + 2 < b1;
        W16_ISSUE(kb + 3, sa, sb)
        __builtin_amdgcn_sched_barrier(0);
        if (kb + 1 < b1) { W16_MULTIPLY(cur ^ 1, tb) }
        else { tb0 = theta_to_h(tb0); tb1 = theta_to_h(tb1); tb2 = theta_to_h(tb2); tb3 = theta_to_h(tb3); }
        W16_STAGE(cur, ta, tb)                          // chunk kb + 2
        lds_barrier();
    }
#undef W16_CONV
#undef W16_MULTIPLY
#undef W16_ROWSUM
#undef W16_ISSUE
#undef W16_STAGE
    float *slab = a.slabs + ((int64_t)job * a.nsplit + a.split_lo + split) * ((int64_t)FP * FP + FP);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int jn = 0; jn < 4; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                slab[(int64_t)(br * 256 + wm * 64 + 32 * i + ROWMAP(r, hi)) * FP + bc * 256 + wn * 128 + 32 * jn + ln] = acc[i][jn][r];
    }
    if (want_bias) {
        // the eight threads that staged the eight 16-byte pieces of a row are neighbouring lanes
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = bsum[i];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            if ((tid & 7) == 0) slab[(int64_t)FP * FP + br * 256 + (tid >> 3) + 64 * i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// first-layer / head / loss part of the reduction for the bf16 path (the hidden layers go through k_reduce)
struct Reduce16Args {
    brief_siren_desc d;
    const float *slabs;       // skinny region: [nsplit][FP*4] first layer, then [nsplit][FP*4] head
    int nsplit;
    const float *rec;         // [nwg][8]: loss, dbh[4]
    int nwg;
    float *grads, *loss_out;
    float inv_count;
    int update;
    OptimScalars opt;
    float *params, *s1, *s2, *pk;
};

__global__ __launch_bounds__(256) void k_reduce16(const Reduce16Args a)
{
    // one wave per item (parameter or the loss): lanes stride the partials, fixed-order butterfly
    const brief_siren_desc &d = a.d;
    const int F = d.features, cin = d.cin, cout = d.cout, FP = 32 * brief_nt(d);
    const int64_t l0_count = (int64_t)F * cin + F, head_w = (int64_t)cout * F;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t total = l0_count + head_w + cout + 1;
    if (item >= total) return;
    float s = 0.f;
    int64_t e = 0;
    int slot = -1;
    if (item < l0_count + head_w) {
        int f, c, which;
        if (item < (int64_t)F * cin) { f = (int)(item / cin); c = (int)(item % cin); which = 0; }
        else if (item < l0_count) { f = (int)(item - (int64_t)F * cin); c = 3; which = 0; }
        else { const int64_t r = item - l0_count; c = (int)(r / F); f = (int)(r % F); which = 1; }
        const float *base = a.slabs + (int64_t)which * a.nsplit * FP * 4 + f * 4 + c;
        for (int sp = lane; sp < a.nsplit; sp += 64) s += base[(int64_t)sp * FP * 4];
        e = which == 0 ? item : brief_canon_head_off(d) + (item - l0_count);
    } else {
        slot = item < total - 1 ? 1 + (int)(item - l0_count - head_w) : 0;      // dbh[c] | loss
        for (int w = lane; w < a.nwg; w += 64) s += a.rec[(int64_t)w * 8 + slot];
        e = brief_canon_head_off(d) + head_w + (slot - 1);
    }
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane != 0) return;
    if (slot == 0) { *a.loss_out = s * a.inv_count; return; }
    a.grads[e] = s;
    if (a.update) {
        const float pv = optim_apply(a.opt, s, a.params, a.s1, a.s2, e);
        if (item < (int64_t)F * cin) a.pk[(item / cin) * 4 + (item % cin)] = brief_phase_scale(d, 0) * pv;
        else if (item < l0_count) a.pk[(item - (int64_t)F * cin) * 4 + 3] = brief_phase_scale(d, 0) * pv;
        else {
            const int64_t r = item - l0_count;
            float *hp = a.pk + brief_pk_head(d);
            if (r < head_w) hp[(r / F) * FP + (r % F)] = pv;
            else hp[4 * (int64_t)FP + (r - head_w)] = pv;
        }
    }
}
