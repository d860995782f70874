// brief_lean.inc — k_lean<SH, MTW, NTC, TRAIN>: the exact-f32 fused forward / loss / dgrad walk in its LEAN form (included by
// brief_hip.hip; uses FusedArgs, the buffer-load helpers, philox_index, grid_coords and the record layout defined there).
//
// k_fused<NT> keeps four MTW x 16 register arrays per wave (accumulators, sines, cosines, deltas) and unrolls its chains over a
// compile-time width; that shape stops at 16 feature tiles (512 features: 4 tiles per wave x 4 arrays + prefetch = 512 VGPRs).
// This kernel is the same arithmetic around ONE state array per wave — accumulators -> phases -> cosines of the last sine layer
// -> deltas, in place throughout, the last layer's sines parked in the wave's transposed LDS scratch (the skeleton of
// k_fused_x3) — so that
//   * every width above 256 features fits: 4 waves x MTW <= 8 feature tiles of one 32-sample tile (SH = 1), the width a RUN-TIME
//     number of tiles nt = ceil(F / 32) in 9 .. 32 — and 3, 5, 6, 7 since the end of round 4, where this form beat k_fused<NT>
//     (brief_layout.h: brief_use_lean) — (NTC = 0: chains are rolled loops over k-tiles with a 4-step register ring of
//     weight fragments; tiles that nt % 4 leaves over are shared along K by the four waves, template parameter RM).  The image of a
//     1024-feature layer is 128 KB of LDS: one workgroup per CU above 512 features, two up to 512.  What SIREN.calc_features
//     (utils/Networks.py:299-314) solves for is whatever the byte budget gives — the reference has no width limit, and the shipped
//     opt/SingleTask/default.yaml on a 512^3 uint16 volume lands at F = 527;
//   * SH = 2 walks 64-sample tiles (two 32-sample halves per weight fragment, half-tiles dealt in strided pairs) with a
//     compile-time width NTC (fully unrolled chains): the f32 counterpart of k_fused_x3's walk.
// Records, stash planes and packed weights are those of k_fused: k_wgrad / k_reduce do not know which kernel ran.
#ifndef BRIEF_LEAN_KTAIL
#define BRIEF_LEAN_KTAIL 1      // the rolled chains stop at ceil(F / 8) steps instead of walking the last k-tile whole (0: A/B)
#endif
// ... except in the TRAIN kernel of two slots per wave (MTW = 2: 5 .. 7 tiles, three workgroups per CU on 168 registers): with the tail code behind the loop
// that kernel ran 17 - 22 % slower at EVERY width (4x160, which has no partial k-tile: 0.322 -> 0.394 ms), while the others gain what the skipped
// steps are worth (k_lean 4x264 0.603 -> 0.646 of the fp32 peak, 4x520 0.666 -> 0.693, 4x1000 0.772 -> 0.787; decode 4x130 0.505 -> 0.550, 4x264 0.704 -> 0.760)
constexpr bool lean_ktail(int MTW, bool train) { return BRIEF_LEAN_KTAIL && (!train || MTW != 2); }
struct LeanLds { int r, g_off, hw_off, part_off, total; };      // floats
__host__ __device__ inline LeanLds lean_lds(int SH, int MTW, int nt)
{
    LeanLds l;
    const int img = SH * nt * 1024, t = SH * 4 * 32 * MTW * 33;      // images | per-wave transposed scratch (aliases them)
    l.r = img > t ? img : t;
    l.g_off = l.r;
    l.hw_off = l.g_off + 4 * 256;
    l.part_off = l.hw_off + 4 * 32 * nt;      // (the head's four biases are read from the packed buffer: with them staged here a 16-tile workgroup took
                                              //  81 936 bytes and two of them missed the CU's 160 KB by 32 — 481 .. 512 features ran one workgroup per CU)
    l.total = l.part_off + SH * 4 * 32 * 4;
    return l;
}

// acc[h][t] += A(mt = wave + 4 t, :) * image_h, run-time width: a rolled loop over k-tiles, four (k-tile, q) steps per iteration,
// the weight fragments of step it + 4 requested into the ring slot step it has just freed.
//
// RM: what happens to the tiles left over when the tile count does not divide by the four waves.
//   0  nt % 4 == 0 (or 3 where RM 3 is not used): every slot t holds tile wave + 4 t; a wave that lacks the last one (only with nt % 4 == 3:
//      wave 3) computes it all the same, on the fragments of tile nt - 1 (never stored).
//   3  nt % 4 == 3: three left-over tiles S0, S1, S2 (owners: waves 0, 1, 2) for four waves, 3 / 4 of a tile pass each, in ONE instruction
//      stream: every wave skips position q = 3, works position 0 into a second accumulator px and positions 1, 2 into its last slot —
//        wave 0: S0 at all three       wave 1: S0 at position 0, S1 at 1, 2       wave 2: S2 at position 0, S1 at 1, 2       wave 3: S2 at all three
//      with rho = (1, 0, 2, 3), which makes the k-steps (mod 4) each tile receives a partition: S0 = {1, 2, 3} + {0}, S1 = {1, 2} + {3, 0},
//      S2 = {2} + {3, 0, 1}.  lean_fold3 hands wave 1's px to wave 0, wave 2's last slot to wave 1, wave 3's sum to wave 2.  (Under RM 0
//      wave 3 spent a whole pass on a duplicate tile while the others waited.)
//   1  nt % 4 == 1: the ONE left-over tile is shared by the four waves along K — wave w takes the k-steps it = w (mod 4) into its last
//      slot; the owner (wave 0) adds the three partial tiles after the chain (k_lean: through the slack behind the LDS image).  A 17-tile
//      layer (the shipped default.yaml on a 512^3 volume: F = 527) costs every wave 4.25 tile passes instead of 5 for wave 0 and a barrier
//      wait for the others.
//   2  nt % 4 == 2: two left-over tiles, tile nt - 2 shared by waves 0 and 2, tile nt - 1 by waves 1 and 3, each taking every second k-step.
// No predicate sits inside the loop (a wave-uniform branch around a load or an MFMA makes hipcc's s_waitcnt bookkeeping fall back to
// vmcnt(0) at the first MFMA of every step): each wave walks the four steps of a k-tile in an order ROTATED by rho(wave), chosen so
// that the steps it owns of the shared tile fall on fixed positions of the unrolled body (q = 3 for RM 1; q = 1, 3 for RM 2; q = 0, 1, 2
// for RM 3).  KTAIL: the loop covers the width's whole k-tiles, the 1 .. 3 real steps of a partial last one run behind it (lean_ktail);
// without it the up to three steps past ceil(F / 8) multiply zero weight columns with the zero activations of padding features.
// MTW = 1 exists for RM 3 only: a 3-tile net, whose three tiles are all "left over" (no wave owns a whole one).
template <int SH, int MTW, int RM, bool KTAIL>
__device__ __forceinline__ void lean_chain_rt(f32x16 (&acc)[SH][MTW], f32x16 &px, __amdgpu_buffer_rsrc_t rs, int soff_layer /*bytes*/, const float4 *X,
                                              int wave, int lane, int nt, int kit, bool two)
{
    constexpr int KF = RM == 0 ? MTW : MTW - 1;      // slots that hold a whole tile of this wave
    const int voff = lane * 16;
    const int HALF = nt * 256;
    const int rho = RM == 1 ? ((wave + 1) & 3) : (RM == 2 ? (((wave >> 1) + 1) & 1) : (RM == 3 ? ((0x3201 >> (4 * wave)) & 3) : 0));
    int soff_t[KF > 0 ? KF : 1];
#pragma unroll
    for (int t = 0; t < KF; ++t) {
        const int mt = wave + 4 * t;
        soff_t[t] = soff_layer + (mt < nt ? mt : nt - 1) * nt * 4096;
    }
    // the shared tile's fragments: RM 1, 2: one tile; RM 3: position 0 works on tile nt - 3 + (0, 0, 2, 2)[wave] (into px), positions 1 and 2
    // on tile nt - 3 + (0, 1, 1, 2)[wave] (into the last slot)
    const int soff_e = soff_layer + (RM == 1 ? nt - 1 : (RM == 2 ? nt - 2 + (wave & 1) : nt - 3 + ((wave + 1) >> 1))) * nt * 4096;
    const int soff_a = soff_layer + (nt - 3 + (wave & 2)) * nt * 4096;
    float4 areg[4][KF > 0 ? KF : 1];
    float4 aext[RM == 3 ? 3 : 2];                     // the shared tile's fragment(s): positions q = 3 (RM 1) / q = 1, 3 (RM 2) / q = 0, 1, 2 (RM 3)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int it0 = (q + rho) & 3;
#pragma unroll
        for (int t = 0; t < KF; ++t) areg[q][t] = bload4(rs, voff, soff_t[t] + it0 * 1024);
        if ((RM == 1 && q == 3) || (RM == 2 && (q & 1))) aext[q >> 1] = bload4(rs, voff, soff_e + it0 * 1024);
        if (RM == 3 && q < 3) aext[q] = bload4(rs, voff, (q == 0 ? soff_a : soff_e) + it0 * 1024);
        // keep the requests in step order: left alone, hipcc issues the ring's slots in reverse, step 0's fragments arrive last, and the
        // wait at the loop head — merged over the entry and the back edge — becomes vmcnt(0): every fourth step then drains the ring
        __builtin_amdgcn_sched_barrier(0);
    }
    // one position's MFMAs: the wave's whole tiles, and its share of the left-over tiles where this position carries one
#define LEAN_POS_MFMAS(q, B)                                                                                 \
    {                                                                                                        \
        _Pragma("unroll") for (int t = 0; t < KF; ++t) {                                                     \
            const float4 a = areg[q][t];                                                                     \
            _Pragma("unroll") for (int h = 0; h < SH; ++h) {                                                 \
                if (SH == 2 && h == 1 && !two) continue;                                                     \
                acc[h][t] = MFMA(a.x, B[h].x, acc[h][t]);                                                    \
                acc[h][t] = MFMA(a.y, B[h].y, acc[h][t]);                                                    \
                acc[h][t] = MFMA(a.z, B[h].z, acc[h][t]);                                                    \
                acc[h][t] = MFMA(a.w, B[h].w, acc[h][t]);                                                    \
            }                                                                                                \
        }                                                                                                    \
        if ((RM == 1 && q == 3) || (RM == 2 && (q & 1)) || (RM == 3 && (q == 1 || q == 2))) {                \
            const float4 a = aext[RM == 3 ? q : q >> 1];                                                     \
            _Pragma("unroll") for (int h = 0; h < SH; ++h) {                                                 \
                if (SH == 2 && h == 1 && !two) continue;                                                     \
                acc[h][MTW - 1] = MFMA(a.x, B[h].x, acc[h][MTW - 1]);                                        \
                acc[h][MTW - 1] = MFMA(a.y, B[h].y, acc[h][MTW - 1]);                                        \
                acc[h][MTW - 1] = MFMA(a.z, B[h].z, acc[h][MTW - 1]);                                        \
                acc[h][MTW - 1] = MFMA(a.w, B[h].w, acc[h][MTW - 1]);                                        \
            }                                                                                                \
        }                                                                                                    \
        if (RM == 3 && q == 0) {                                                                             \
            const float4 a = aext[0];                                                                        \
            px = MFMA(a.x, B[0].x, px); px = MFMA(a.y, B[0].y, px);                                          \
            px = MFMA(a.z, B[0].z, px); px = MFMA(a.w, B[0].w, px);                                          \
        }                                                                                                    \
    }
    float4 bcur[SH], bnxt[SH];
#pragma unroll
    for (int h = 0; h < SH; ++h) bcur[h] = X[h * HALF + rho * 64 + lane];
    const int nkt = KTAIL ? kit >> 2 : (kit + 3) >> 2;      // whole k-tiles (the width's last k-tile may hold 1 .. 3 real steps: below)
    for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // this position's k-step and the next position's (the first one of the next k-tile behind q = 3)
            const int it = kt * 4 + ((q + rho) & 3);
            const int itn = q < 3 ? kt * 4 + ((q + 1 + rho) & 3) : kt * 4 + 4 + rho;
#pragma unroll
            for (int h = 0; h < SH; ++h) bnxt[h] = X[h * HALF + itn * 64 + lane];
            __builtin_amdgcn_sched_barrier(0);
            LEAN_POS_MFMAS(q, bcur)
            __builtin_amdgcn_sched_barrier(0);
            // (fragments past the layer's last step are the next block's: requested, never used)
#pragma unroll
            for (int t = 0; t < KF; ++t) areg[q][t] = bload4(rs, voff, soff_t[t] + (it + 4) * 1024);
            if ((RM == 1 && q == 3) || (RM == 2 && (q & 1))) aext[q >> 1] = bload4(rs, voff, soff_e + (it + 4) * 1024);
            if (RM == 3 && q < 3) aext[q] = bload4(rs, voff, (q == 0 ? soff_a : soff_e) + (it + 4) * 1024);
#pragma unroll
            for (int h = 0; h < SH; ++h) bcur[h] = bnxt[h];
        }
    }
    // The width's last k-tile, when only 1 .. 3 of its steps hold real features (F = 527: 66 steps = 16 k-tiles + 2; F = 200: 25 = 6 + 1): the ring
    // already holds its fragments; the positions whose step lies past ceil(F / 8) are skipped — wave-uniform tests, but outside the loop, where
    // they cost one conservative wait instead of one per iteration.  (Those steps used to multiply zero weight columns with the zero activations of
    // padding features: up to 3 of 4 nt steps per chain, 12 % at 7 tiles.)
    if (KTAIL && (kit & 3)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = nkt * 4 + ((q + rho) & 3);
            if (it < kit) {
                float4 bt[SH];
#pragma unroll
                for (int h = 0; h < SH; ++h) bt[h] = X[h * HALF + it * 64 + lane];
                LEAN_POS_MFMAS(q, bt)
            }
        }
    }
#undef LEAN_POS_MFMAS
}

// After a chain with shared left-over tiles: the partners park their partial tile in the slack behind the LDS image (the tail of the
// transposed scratch, dead while the images are live; lean_lds: >= 3 tiles of room for every run-time width), one workgroup barrier,
// the owner adds them in wave order.  `PS`: that slack.  RM 0: just the barrier.
template <int SH, int MTW, int RM>
__device__ __forceinline__ void lean_fold_shared(f32x16 (&acc)[SH][MTW], float *PS, int wave, int lane, bool two)
{
    if (RM != 0) {
        const bool giver = RM == 1 ? wave != 0 : wave >= 2;
        const int slot = RM == 1 ? wave - 1 : wave - 2;
        if (giver) {
#pragma unroll
            for (int h = 0; h < SH; ++h) {
                if (SH == 2 && h == 1 && !two) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) PS[((h * 3 + slot) * 16 + r) * 64 + lane] = acc[h][MTW - 1][r];
            }
        }
    }
    lds_barrier();
    if (RM == 1 && wave == 0) {
#pragma unroll
        for (int h = 0; h < SH; ++h) {
            if (SH == 2 && h == 1 && !two) continue;
#pragma unroll
            for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][MTW - 1][r] += PS[((h * 3 + s3) * 16 + r) * 64 + lane];
        }
    }
    if (RM == 2 && wave < 2) {
#pragma unroll
        for (int h = 0; h < SH; ++h) {
            if (SH == 2 && h == 1 && !two) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][MTW - 1][r] += PS[((h * 3 + wave) * 16 + r) * 64 + lane];
        }
    }
}

// RM 3's fold: every partner parks ONE partial tile for its left neighbour.  The slack behind the image has room for one tile where three
// are needed (and no LDS is left to grow it at 15 and 31 tiles), so they are parked IN the dead image — tile w's 4 KB for owner w, which only
// wave w writes afterwards (its epilogue follows its add in program order).  That takes a barrier before (every wave is done reading the
// image) and one after the parking.  Afterwards the last slot of waves 0 .. 2 holds their whole left-over tile.
template <int MTW>
__device__ __forceinline__ void lean_fold3(f32x16 (&acc)[1][MTW], f32x16 &px, float *img, int wave, int lane)
{
    lds_barrier();
    if (wave == 3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) img[2048 + r * 64 + lane] = acc[0][MTW - 1][r] + px[r];
    } else if (wave == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { img[1024 + r * 64 + lane] = acc[0][MTW - 1][r]; acc[0][MTW - 1][r] = px[r]; }
    } else if (wave == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) img[r * 64 + lane] = px[r];
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][MTW - 1][r] += px[r];
    }
    lds_barrier();
    if (wave < 3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][MTW - 1][r] += img[wave * 1024 + r * 64 + lane];
    }
}

// compile-time width: fully unrolled, fragments four steps ahead in registers of their own (k_fused's chain, every A fragment
// against SH sample halves)
template <int SH, int MTW, int NTC>
__device__ __forceinline__ void lean_chain_ct(f32x16 (&acc)[SH][MTW], __amdgpu_buffer_rsrc_t rs, int soff_layer /*bytes*/, const float4 *X,
                                              int wave, int lane, int kit, bool two)
{
    constexpr int NT = NTC > 0 ? NTC : 1, NIT = NT * 4, PD = 4, HALF = NT * 256;
    constexpr bool EXACT = MTW * 4 == NT;
    const int voff = lane * 16;
    int soff_w = soff_layer + wave * (NT * 4 * 1024);
    asm volatile("" : "+s"(soff_w));
    float4 areg[NIT][MTW];
    float4 breg[NIT][SH];
#pragma unroll
    for (int it = 0; it < PD; ++it)
#pragma unroll
        for (int t = 0; t < MTW; ++t)
            if (EXACT || wave + 4 * t < NT) areg[it][t] = bload4(rs, voff, soff_w + (4 * t * NT * 4 + it) * 1024);
#pragma unroll
    for (int h = 0; h < SH; ++h) breg[0][h] = X[h * HALF + lane];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (it >= NIT - 3 && it >= kit) break;
        if (it + PD < NIT) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
                if (EXACT || wave + 4 * t < NT) areg[it + PD][t] = bload4(rs, voff, soff_w + (4 * t * NT * 4 + it + PD) * 1024);
        }
        if (it + 1 < NIT) {
#pragma unroll
            for (int h = 0; h < SH; ++h) breg[it + 1][h] = X[h * HALF + (it + 1) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
            if (EXACT || wave + 4 * t < NT) {
                const float4 a = areg[it][t];
#pragma unroll
                for (int h = 0; h < SH; ++h) {
                    if (h == 1 && !two) continue;      // a single half-tile at the end of a workgroup's run (wave-uniform)
                    const float4 b = breg[it][h];
                    acc[h][t] = MFMA(a.x, b.x, acc[h][t]);
                    acc[h][t] = MFMA(a.y, b.y, acc[h][t]);
                    acc[h][t] = MFMA(a.z, b.z, acc[h][t]);
                    acc[h][t] = MFMA(a.w, b.w, acc[h][t]);
                }
            }
        }
    }
}

// resident workgroups per CU the kernel is register-allocated for: the wide form owns a CU (128 KB image), the 64-sample form
// shares it with one mate (80 KB of LDS each)
#ifndef BRIEF_LEAN_WPE2
#define BRIEF_LEAN_WPE2 3      // resident workgroups per CU of the two-slot form (5 .. 7 tiles): 3 = 168 VGPRs (76 B of scratch with shared left-over tiles); experiment: 2
#endif
constexpr int lean_wpe(int SH, int MTW) { return SH == 1 && MTW <= 2 ? BRIEF_LEAN_WPE2 : (SH == 2 || MTW <= 4 ? 2 : 1); }

// RM: how the tiles left over by nt % 4 are dealt (lean_chain_rt, lean_chain_rt3): the host picks the instantiation nt % 4
template <int SH, int MTW, int NTC, bool TRAIN, int RM = 0, bool BOX = false>      // BOX: inference over a box of the grid (box_coords)
__global__ __launch_bounds__(256, lean_wpe(SH, MTW)) void k_lean(const typename KArgsT<BOX>::type a)
{
    static_assert(!(TRAIN && BOX), "the box mapping is an inference instantiation");
    static_assert(SH == 1 || SH == 2, "one or two 32-sample halves per tile");
    static_assert(RM == 0 || (NTC == 0 && SH == 1 && (MTW >= 2 || RM == 3)), "shared left-over tiles: run-time widths only (MTW = 1: the three tiles of a 3-tile net)");
    constexpr int TROWS = 32 * MTW;                    // local features one wave owns
    constexpr int RS = (TROWS + 63) / 64;              // local-feature slots per lane in the skinny-gradient passes
    constexpr int TR = MTW > 4 ? 256 : 128;            // rows of a record's dW0 / dWh sections (brief_layout.h: brief_rec_tr)
    const brief_siren_desc &d = a.d;
    const int nt = NTC > 0 ? NTC : brief_nt(d);
    const int FP = 32 * nt, HALF = nt * 256;           // HALF: float4 per sample-half image
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const LeanLds lds = lean_lds(SH, MTW, nt);
    float4 *X = reinterpret_cast<float4 *>(smem);
    float *T = smem;                                   // aliases the images
    float *G = smem + lds.g_off;
    float *HW = smem + lds.hw_off;                     // Whp[4][FP], bhp[4]
    float4 *PART = reinterpret_cast<float4 *>(smem + lds.part_off);      // head partials [SH][4 waves][32]
    const int lane = threadIdx.x & 63;
    // LOGICAL wave number: which feature tiles (wave + 4 t), scratch regions and record this wave owns.  Where two workgroups share a
    // CU (run-time widths up to 16 tiles), the second residency slot rotates the numbering by two: a tile count that does not divide by
    // four leaves the first waves one tile more (9 = 3/2/2/2, 14 = 4/4/3/3), and with both workgroups' heavy waves on the same SIMDs the
    // matrix pipes of the other two idle at every layer's barrier (14 tiles: 8 tile slots per SIMD and layer instead of 7).
    const int wave_hw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = (NTC == 0 && lean_wpe(SH, MTW) == 2) ? ((wave_hw + 2 * (((int)blockIdx.x / a.stagger_cus) & 1)) & 3) : wave_hw;
    const int hi = lane >> 5, ln = lane & 31;
    const int L = d.layers, cin = d.cin, cout = d.cout;
    const int kit = (d.features + 7) >> 3;             // chain steps that hold real (unpadded) features
    const int64_t npad = a.npad;
    const float *pk = a.pk;
    float *Gw = G + wave * 256;
    const float4 *W0p = reinterpret_cast<const float4 *>(pk + brief_pk_w0(d));
    const __amdgpu_buffer_rsrc_t rs_pk = __builtin_amdgcn_make_buffer_rsrc((void *)pk, 0, (int)(brief_pk_count(d) * 4), 0x00020000);
    const int stash_bytes = (int)((int64_t)FP * npad * 4);      // one layer's plane (host checks < 2^31)
    const int64_t hstride = brief_pk_hidden_stride(d);
    bool tv[MTW];                                      // this wave owns feature tile wave + 4 t
#pragma unroll
    for (int t = 0; t < MTW; ++t) tv[t] = wave + 4 * t < nt;
    {
        const float *headp = pk + brief_pk_head(d);
        for (int e = threadIdx.x; e < 4 * FP; e += 256) HW[e] = headp[e];
    }
    lds_barrier();
    float acc0[RS][4], accWh[RS][4];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc0[rs][c] = 0.f; accWh[rs][c] = 0.f; }
    float accbh[4] = {0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    // Work is dealt in 32-sample half-tiles.  SH = 1: workgroup w walks half-tiles w, w + G, ...  SH = 2: two at a time — R = Hn / (2 G)
    // full rounds of strided pairs (round r: half-tiles 2 (r G + w), + 1: the grid writes one moving window of the stash planes),
    // then the Hr < 2 G left-over half-tiles as one more pair for the first Hr - G workgroups (if Hr > G) and a single (second half
    // skipped) for the others that get one (k_fused_x3's plan).
    // (SH = 1, TRAIN: a launch may cover the tile range [n_begin / 32, ceil(n_end / 32)) only — the body / tail pair of the overlap plan, brief_hip.hip: fused_tail_plan —
    //  with its workgroups' records behind rec_base; n_begin = n_end = 0: the whole batch)
    const int64_t T0 = SH == 1 ? a.n_begin >> 5 : 0;
    const int64_t Hn = ((SH == 1 && a.n_end > 0 ? a.n_end : a.n) + 31) >> 5;
    const int64_t G_ = gridDim.x, w_ = blockIdx.x;
    const int64_t R_ = SH == 2 ? Hn / (2 * G_) : (Hn - T0 > w_ ? (Hn - T0 - w_ + G_ - 1) / G_ : 0);
    const int64_t Hr = Hn - 2 * G_ * R_;
    const int64_t npair_x = Hr > G_ ? Hr - G_ : 0;
    const int64_t nsing_x = Hr > G_ ? G_ - npair_x : Hr;
    const int extra = SH == 2 ? (w_ < npair_x ? 2 : (w_ < npair_x + nsing_x ? 1 : 0)) : 0;
    const int64_t ht_x = 2 * G_ * R_ + (w_ < npair_x ? 2 * w_ : 2 * npair_x + (w_ - npair_x));
    for (int64_t it_ = 0; it_ < R_ + (extra ? 1 : 0); ++it_) {
        const int64_t ht = SH == 2 ? (it_ < R_ ? 2 * (it_ * G_ + w_) : ht_x) : T0 + it_ * G_ + w_;
        const bool two = SH == 2 && (it_ < R_ || extra == 2);      // workgroup-uniform: the second half exists
        // ---- sample inputs (kernarg scalars re-read per tile through an opaque pointer, as in k_fused)
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
        float x0[SH], x1[SH], x2[SH];
        int64_t jidx[SH];      // targets and loss weights are fetched at the loss
        bool valid[SH];
        f32x16 acc[SH][MTW];   // THE state array: accumulators -> phases -> cosines of the last sine layer -> deltas
        f32x16 px;             // RM 3: the second partial accumulator of the left-over tiles (lean_chain_rt)
        {
            // SH = 2: the 64 lanes draw the pair's 64 indices / coordinates once (lane = sample) and hand every lane both halves' values
            // for its column; SH = 1: both lane halves compute their column's sample
            const int64_t n64 = ht * 32 + (SH == 2 ? lane : ln);
            const bool v64 = (SH == 1 || lane < 32 || two) && n64 < a.n;
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
            if (SH == 2) {
                const int jl = (int)(uint32_t)(uint64_t)j, jh = (int)(uint32_t)((uint64_t)j >> 32);
#pragma unroll
                for (int h = 0; h < SH; ++h) {
                    const int src = 32 * h + ln;
                    x0[h] = __shfl(c0, src); x1[h] = __shfl(c1, src); x2[h] = __shfl(c2, src);
                    jidx[h] = (int64_t)(((uint64_t)(uint32_t)__shfl(jh, src) << 32) | (uint32_t)__shfl(jl, src));
                    valid[h] = (h == 0 || two) && (ht + h) * 32 + ln < a.n;
                }
            } else {
                x0[0] = c0; x1[0] = c1; x2[0] = c2; jidx[0] = j; valid[0] = v64;
            }
        }
        // ---- layer 0: z0 = W0 x + b0 as two K=2 MFMAs per feature tile and half ([x0 x1 | x2 1] against W0p rows)
#pragma unroll
        for (int h = 0; h < SH; ++h) {
            const float b0 = hi ? x1[h] : x0[h];
            const float b1 = hi ? 1.0f : x2[h];
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
                if (tv[t]) {
                    const float4 w = W0p[32 * (wave + 4 * t) + ln];
                    acc[h][t] = MFMA(hi ? w.y : w.x, b0, acc[h][t]);
                    acc[h][t] = MFMA(hi ? w.w : w.z, b1, acc[h][t]);
                }
            }
        }
        // ---- sine layers 0 .. L-2
        for (int l = 0; l <= L - 2; ++l) {
            const bool last = (l == L - 2);
            if (l > 0) {
                const float *bp_ = pk + FP * 4 + (int64_t)(l - 1) * hstride + 2 * (int64_t)FP * FP;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (tv[t]) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 b4 = *reinterpret_cast<const float4 *>(bp_ + 32 * (wave + 4 * t) + 8 * q + 4 * hi);
#pragma unroll
                            for (int h = 0; h < SH; ++h) {
                                acc[h][t][4 * q] = b4.x; acc[h][t][4 * q + 1] = b4.y; acc[h][t][4 * q + 2] = b4.z; acc[h][t][4 * q + 3] = b4.w;
                            }
                        }
                    } else if (RM != 0 && t == MTW - 1) {
                        // a partner's share of a left-over tile starts from zero (the owner's carries the bias)
#pragma unroll
                        for (int h = 0; h < SH; ++h)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
                    }
                }
                const int soff_l = (int)((FP * 4 + (int64_t)(l - 1) * hstride) * 4);
                __builtin_amdgcn_s_setprio(3);
                if (RM == 3) {
                    // wave 2's own left-over tile (S2) accumulates in px, its last slot is a share of S1: the bias goes with the tile
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        px[r] = wave == 2 ? acc[0][MTW - 1][r] : 0.f;
                        if (wave == 2) acc[0][MTW - 1][r] = 0.f;
                    }
                }
                if (NTC > 0) lean_chain_ct<SH, MTW, NTC>(acc, rs_pk, soff_l, X, wave, lane, kit, two);
                else lean_chain_rt<SH, MTW, RM, lean_ktail(MTW, TRAIN)>(acc, px, rs_pk, soff_l, X, wave, lane, nt, kit, two);
                __builtin_amdgcn_s_setprio(0);
                if constexpr (RM == 3) lean_fold3<MTW>(acc, px, T, wave, lane);
                else lean_fold_shared<SH, MTW, RM>(acc, T + SH * nt * 1024, wave, lane, two);   // (its barrier: every wave is done reading the previous images)
                // the last layer's epilogue writes the sines into the transposed scratch, whose tail IS the slack the partial tiles were
                // parked in: the owners must have read them first (found by tools/fuzz_multifit.py: a co-trained 130-wide net differed from
                // its solo fit in one run of twenty)
                if (RM != 0 && TRAIN && last) lds_barrier();
            }
            float pph[SH][4];      // (last layer) head partials
#pragma unroll
            for (int h = 0; h < SH; ++h) {
#pragma unroll
                for (int c = 0; c < 4; ++c) pph[h][c] = 0.f;
                if (h == 1 && !two) continue;
                const int voff = (int)(((ht + h) * 32) * ((int64_t)FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wave + 4 * t;
                    // the accumulator IS the phase om z in revolutions (the weights carry om / 2 pi): keep its fraction
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][t][r] = __builtin_amdgcn_fractf(acc[h][t][r]);
                    f32x16 hv;
                    if (!last) {
                        if (TRAIN) {
                            const __amdgpu_buffer_rsrc_t rz =
                                __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)l * FP * npad), 0, stash_bytes, 0x00020000);
#pragma unroll
                            for (int r = 0; r < 16; ++r) bstore1(acc[h][t][r], rz, voff, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) hv[r] = BRIEF_SIN_REV(acc[h][t][r]);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            X[h * HALF + (mt * 4 + q) * 64 + lane] = make_float4(hv[4 * q], hv[4 * q + 1], hv[4 * q + 2], hv[4 * q + 3]);
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
                            float *Th = T + (wave * SH + h) * (TROWS * 33);
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
            lds_barrier();      // images (or, last layer, the head partials) are published
        }
        // ---- head: the waves' partial dot products, summed in wave order
        float zo[SH][4], yh[SH][4], g[SH][4];
#pragma unroll
        for (int h = 0; h < SH; ++h) {
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
                    zo[h][c] = tt[c] + pk[brief_pk_head(d) + 4 * (int64_t)FP + c];
                    yh[h][c] = d.output_act ? brief_fast_sinf(d.w0_hidden * zo[h][c]) : zo[h][c];
                }
                if (!TRAIN) {
                    if (c < cout && valid[h] && wave == 0 && hi == 0) {
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
                    if (wave == 0 && hi == 0) lsum += li * we;
                    g[h][c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yvc : gi * we * a.inv_count;      // external: targets ARE dL/dyhat
                    if (d.output_act) g[h][c] *= d.w0_hidden * brief_fast_cosf(d.w0_hidden * zo[h][c]);
                    if (a.yhat_out && wave == 0 && hi == 0) a.yhat_out[n * cout + c] = yh[h][c];
                }
            }
        }
        if (!TRAIN) {
            lds_barrier();      // the partials (and, for L = 2, nothing else) separate this tile's head from the next tile's epilogue
            continue;
        }
        // ---- head gradients, one half after the other, from the transposed h this wave parked in its scratch (lane <-> local feature;
        //      no barriers: the scratch and G are this wave's own, LDS operations of one wave execute in order)
#pragma unroll
        for (int h = 0; h < SH; ++h) {
            if (h == 1 && !two) continue;
            if (hi == 0) *reinterpret_cast<float4 *>(Gw + ln * 4) = make_float4(g[h][0], g[h][1], g[h][2], g[h][3]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int rs = 0; rs < RS; ++rs) {
                float4 sW = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
                const int row = lane + 64 * rs;
                const float *trow = T + (wave * SH + h) * (TROWS * 33) + (row < TROWS ? row : 0) * 33;
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
                if (row < TROWS) { accWh[rs][0] += sW.x; accWh[rs][1] += sW.y; accWh[rs][2] += sW.z; accWh[rs][3] += sW.w; }
                if (rs == 0) { accbh[0] += sb.x; accbh[1] += sb.y; accbh[2] += sb.z; accbh[3] += sb.w; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the next half overwrites G
        }
        // ---- delta of the last sine layer: om cos(phase) * (Wh^T g); the om rides on g
        {
            const float om_top = (L - 2) == 0 ? d.w0_first : d.w0_hidden;
#pragma unroll
            for (int h = 0; h < SH; ++h) {
                if (h == 1 && !two) continue;
                float gom[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) gom[c] = om_top * g[h][c];
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wave + 4 * t;
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
        // ---- dgrad chain: layers L-2 .. 1
        for (int l = L - 2; l >= 1; --l) {
            const __amdgpu_buffer_rsrc_t rd =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.D + (int64_t)(l - 1) * FP * npad), 0, stash_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rzp =
                __builtin_amdgcn_make_buffer_rsrc((void *)(a.Z + (int64_t)(l - 1) * FP * npad), 0, stash_bytes, 0x00020000);
#pragma unroll
            for (int h = 0; h < SH; ++h) {
                if (h == 1 && !two) continue;
                const int voff_s = (int)(((ht + h) * 32) * ((int64_t)FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wave + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) bstore1(acc[h][t][r], rd, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                }
            }
            lds_barrier();   // transposed scratch / previous chain finished with the image region
#pragma unroll
            for (int h = 0; h < SH; ++h) {
                if (h == 1 && !two) continue;
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (!tv[t]) continue;
                    const int mt = wave + 4 * t;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        X[h * HALF + (mt * 4 + q) * 64 + lane] = make_float4(acc[h][t][4 * q], acc[h][t][4 * q + 1], acc[h][t][4 * q + 2], acc[h][t][4 * q + 3]);
                }
            }
            lds_barrier();
#pragma unroll
            for (int h = 0; h < SH; ++h)
#pragma unroll
                for (int t = 0; t < MTW; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
            const int soff_b = (int)((FP * 4 + (int64_t)(l - 1) * hstride + (int64_t)FP * FP) * 4);
            __builtin_amdgcn_s_setprio(3);
            if (RM == 3) {
#pragma unroll
                for (int r = 0; r < 16; ++r) px[r] = 0.f;
            }
            if (NTC > 0) lean_chain_ct<SH, MTW, NTC>(acc, rs_pk, soff_b, X, wave, lane, kit, two);
            else lean_chain_rt<SH, MTW, RM, lean_ktail(MTW, TRAIN)>(acc, px, rs_pk, soff_b, X, wave, lane, nt, kit, two);
            __builtin_amdgcn_s_setprio(0);
            if constexpr (RM == 3) lean_fold3<MTW>(acc, px, T, wave, lane);                            // (two more barriers per layer than RM 0)
            else if (RM != 0) lean_fold_shared<SH, MTW, RM>(acc, T + SH * nt * 1024, wave, lane, two);      // (one more barrier per layer than RM 0)
            // delta_{l-1} = acc * cos(phase_{l-1}): the phases come back from the stash after the chain, two feature tiles (32 requests) at a time
#pragma unroll
            for (int h = 0; h < SH; ++h) {
                if (h == 1 && !two) continue;
                const int voff_s = (int)(((ht + h) * 32) * ((int64_t)FP * 4)) + ln * 4 + hi * 4 * 128;
#pragma unroll
                for (int t2 = 0; t2 < MTW; t2 += 2) {
                    float zr[2][16];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int t = t2 + u;
                        if (t < MTW && tv[t < MTW ? t : 0]) {
                            const int mt = wave + 4 * t;
#pragma unroll
                            for (int r = 0; r < 16; ++r) zr[u][r] = bload1s(rzp, voff_s, (32 * mt + (r & 3) + 8 * (r >> 2)) * 128);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int t = t2 + u;
                        if (t < MTW && tv[t < MTW ? t : 0]) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[h][t < MTW ? t : 0][r] *= BRIEF_COS_REV(zr[u][r]);
                        }
                    }
                }
            }
        }
        // ---- first-layer gradients from delta_0, one half after the other (lane <-> local feature)
#pragma unroll
        for (int h = 0; h < SH; ++h) {
            if (h == 1 && !two) continue;
            if (h == 0) lds_barrier();      // the scratch aliases the images: every wave must be past the last dgrad chain
            float *Tf = T + (wave * SH + h) * (TROWS * 33);
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) Tf[(32 * t + ROWMAP(r, hi)) * 33 + ln] = acc[h][t][r];
            if (hi == 1) *reinterpret_cast<float4 *>(Gw + 128 + ln * 4) = make_float4(x0[h], x1[h], x2[h], 1.0f);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // own-wave scratch: ordering only
#pragma unroll
            for (int rs = 0; rs < RS; ++rs) {
                float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
                const int row = lane + 64 * rs;
                const float *trow = Tf + (row < TROWS ? row : 0) * 33;
#pragma unroll 4
                for (int s = 0; s < 32; ++s) {
                    const float dv = trow[s];
                    const float4 xv = *reinterpret_cast<const float4 *>(Gw + 128 + s * 4);
                    s0.x = __fmaf_rn(dv, xv.x, s0.x); s0.y = __fmaf_rn(dv, xv.y, s0.y);
                    s0.z = __fmaf_rn(dv, xv.z, s0.z); s0.w = __fmaf_rn(dv, xv.w, s0.w);
                }
                if (row < TROWS) { acc0[rs][0] += s0.x; acc0[rs][1] += s0.y; acc0[rs][2] += s0.z; acc0[rs][3] += s0.w; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the next half overwrites the coordinates in G
        }
        lds_barrier();
    }
    if (!TRAIN) return;
    float *rec = a.rec + (((int64_t)blockIdx.x + a.rec_base) * 4 + wave) * (8 * TR + 32);
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) {
        const int row = lane + 64 * rs;
        if (row < TROWS) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                rec[row * 4 + c] = acc0[rs][c];                   // dW0[f_local][x0,x1,x2,bias]
                rec[4 * TR + c * TR + row] = accWh[rs][c];        // dWh[c][f_local]
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) rec[8 * TR + c] = accbh[c];
        rec[8 * TR + 4] = lsum;
    }
}
