// brief_wgrad.inc — k_wgrad: the weight-gradient GEMM of the stash path (part of the single translation unit brief_hip.hip, which includes it in this order;
// it uses what the parts before it define).
// ---------------------------------------------------------------------------------------------
// (the bf16 kernels are included after the optimizer helpers below)
// weight-gradient GEMM: dW_l[fo][fi] = sum_n D_l[fo][n] * sin(2 pi Z_{l-1}[fi][n]),  db_l = sum_n D_l   (Z: revolutions)
struct WgradArgs {
    brief_siren_desc d;
    const float *Z;
    const float *D;
    int64_t npad;
    int nsplit;
    // this launch covers the 32-sample chunks [kb_lo, kb_hi) in nsplit_here K splits, which fill the slabs split_lo .. split_lo + nsplit_here - 1 of the nsplit every
    // layer has (one launch: 0, npad / 32, 0, nsplit; the body / tail pair of the overlap plan of the wide nets: brief_hip.hip, fused_tail_plan).  k_wgrad_x3: unused
    int64_t kb_lo, kb_hi;
    int split_lo, nsplit_here;
    // uneven = 1 (the tail plan, brief_hip.hip: fused_tail_plan): the nsplit K splits of a layer are NOT equal — the first n_norm of them hold kfix_n / 2^16 chunks each, the
    // others (the SHORT splits, which also cover the fused kernel's tail tiles at the end of the chunk range) kfix_s / 2^16; split g covers chunks [bnd(g), bnd(g + 1)) of
    // [0, kb_hi), and the workgroups are numbered split-major (all layers of split g before split g + 1), so that the short splits' workgroups are dispatched last
    int uneven, n_norm;
    int64_t kfix_n, kfix_s;
    float *slabs;       // [(L-2)][nsplit][FP*FP + FP]
    float *stamps;      // diagnostic build (-DBRIEF_STAMPS) only: [blocks][8 waves][8]
};

// k_wgrad<NT> geometry.  Widths above 8 tiles are cut into NQ x NQ output quadrants of QT x QT tiles, one
// workgroup each (a 512x512 fp32 dW does not fit eight waves' registers); QT plays NT's role inside.
constexpr int wgrad_nq(int NT) { return (NT + 7) / 8; }
constexpr int wgrad_qt(int NT) { return (NT + wgrad_nq(NT) - 1) / wgrad_nq(NT); }      // exact for every compiled width (1 .. 8, 12, 16); above 16 tiles
                                                                                        // (run-time width) the last quadrant row / column may be short
// How the 8 waves of a k_wgrad workgroup cover a QT x QT tile block.  Rectangular form: WMk x WNk wave tiles of TM x TN 32 x 32 tiles each,
// times a WK-way split of every chunk's four k-groups (folded through LDS at the end) — 1, 2, 4, 6 and 8 tiles per side, where it leaves no
// slot empty (6: 2 x 2 waves x 3 x 3 tiles x two k-slices; 8: 2 x 4 waves x 4 x 2).  An odd side has no such grid (7: 64 slots for 49 tiles,
// 5: 36 for 25, 3: 16 for 9), so there the waves take UNEQUAL pieces, sized so that the four SIMDs (which carry waves w and w + 4) end up level:
//   LIST (3 and 5 per side)  wave w owns a run of floor(QT^2 / 8) tiles in row-major order; no k-split of those, no fold
//                            (4x96 step 0.392 -> 0.432 of the fp32 peak, 4x160 0.567 -> 0.608, 4x288 0.591 -> 0.649, 4x320 0.659 -> 0.710)
//   HET7 (7 per side)        wave w < 7 owns the first six tiles of tile row w, wave 7 the first six of tile column 6: 12 tiles per SIMD
//                            where 16 slots were (4x224 0.647 -> 0.677, 4x448 0.736 -> 0.770, 4x640 0.693 -> 0.739, 4x896 0.733 -> 0.783)
//   ... and the ONE tile that is left (9, 25, 49 = 8 n + 1: the corner tile) is split along K over waves 0 .. 3, one per SIMD: each takes one of the four k-groups of every
//   chunk into an extra accumulator, wave 0 adds the partners' three partial tiles through the dead LDS panels at the end (XS below).  Given whole to one wave it made
//   that wave's SIMD the slowest — 3 tiles against 2 at three per side, 7 against 6 at five, 13 against 12 at seven: step 4x65 0.2165 -> 0.2080 ms, 4x96 0.2327 -> 0.2216,
//   4x320 1.650 -> 1.614, 4x448 2.976 -> 2.948, 4x896 11.71 -> 11.64.
// Each role is a copy of the whole chunk loop (k_wgrad's chunk_loop): a role test inside the loop made the compiler carry two sets of
// accumulators across the merge and spill (measured 20 - 25 % slower than the rectangular form it was meant to beat).  LIST at 4 and 6 per
// side is a wash (+-1 %), at 7 it spills (two fragment reads per tile): BRIEF_WGRAD_LIST picks the sides at compile time for such A/B runs.
#ifndef BRIEF_WGRAD_XSPLIT
#define BRIEF_WGRAD_XSPLIT 1      // LIST / HET7: the one tile 8 waves leave over (9, 25, 49 = 8 n + 1) is split along K over waves 0 .. 3 (0: it goes whole to wave 7; A/B)
#endif
#ifndef BRIEF_WGRAD_LIST
#define BRIEF_WGRAD_LIST(QT) ((QT) == 3 || (QT) == 5)
#endif
// Round 5, rectangular layouts (1, 2, 4, 6, 8 tiles per side; the headline's k_wgrad<8>).  The loop's ISA showed two things the source did not:
//  (i)  the bias gradient db = row sums of the delta panel was taken from the A fragments by the first wave column only — `if (wnk == 0)`, which hipcc
//       if-converted: ALL eight waves ran its 61 adds, 63 moves and 16 selects per chunk (~10 % of the chunk's 128 MFMAs in issue cycles on a pipe that
//       serialises f32 MFMA and VALU).  BRIEF_WGRAD_STAGE_BIAS: the sums are taken by the thread that STAGES a row piece (3 adds per 16-byte piece, 4 pieces
//       per thread and chunk), reduced over the 8 threads of a row at the end — k_wgrad16_big's scheme;
//  (ii) every k-group's six fragment reads sat directly in front of its 32 MFMAs behind an lgkmcnt(0): after a chunk's barrier all eight waves read LDS at
//       once and all four matrix pipes waited.  BRIEF_WGRAD_FRAG_PIPE: the 8-tile layout reads k-group g + 1's fragments before it issues k-group g's MFMAs.
#ifndef BRIEF_WGRAD_STAGE_BIAS
#define BRIEF_WGRAD_STAGE_BIAS 1
#endif
#ifndef BRIEF_WGRAD_FRAG_PIPE
#define BRIEF_WGRAD_FRAG_PIPE 1
#endif
#ifndef BRIEF_WGRAD_FRAG_PIPE2
#define BRIEF_WGRAD_FRAG_PIPE2 1      // the same for the two-k-slice layouts (4 and 6 tiles per side): both of a wave's k-groups requested up front
#endif
// (the pipelined branch of the 8-tile layout takes no fragment-side bias sums: without the staged ones the hidden bias gradients would be silent zeros)
static_assert(!(BRIEF_WGRAD_FRAG_PIPE && !BRIEF_WGRAD_STAGE_BIAS), "BRIEF_WGRAD_FRAG_PIPE needs BRIEF_WGRAD_STAGE_BIAS: the pipelined 8-tile branch has no other bias sums");
// The operand feed of the compile-time 8-tile rectangular layout (the headline's k_wgrad<8>).  1: both panels of a chunk go global -> LDS by LDS-DMA
// (16 bytes per lane, no operand data in VGPRs), the sine and the bias sums are taken in place by the thread that fetched a piece.  0: the
// register-staged feed every other layout has (A/B builds).  The LDS image of the DMA feed has unpadded 128-byte rows — one wave-level DMA
// instruction writes 1 KiB at wave-uniform base + lane * 16, i.e. 8 whole rows — with the 16-byte piece index XOR-ed by (row >> 1) & 7: a
// ds_read_b128 is served in 16-lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (+ 32), whose rows must spread over the 16 (row parity, slot)
// pairs of the 256-byte bank row; row & 7 would put rows r and r + 24 of a group on one slot (2-way), (row >> 1) & 7 does not.  The swizzle is on
// the SOURCE address of the DMA and on the fragment reads; the LDS destination stays lane-linear.
#ifndef BRIEF_WGRAD_DMA_FEED
#define BRIEF_WGRAD_DMA_FEED 1
#endif
constexpr bool wgrad_dma_feed(int NT, int QT) { return BRIEF_WGRAD_DMA_FEED && BRIEF_WGRAD_FRAG_PIPE && NT != 0 && QT == 8 && !BRIEF_WGRAD_LIST(QT); }
constexpr int wgrad_wmk(int QT) { return QT >= 2 ? 2 : 1; }
constexpr int wgrad_wnk(int QT) { return QT >= 7 ? 4 : (QT >= 2 ? 2 : 1); }
constexpr bool wgrad_list(int QT) { return BRIEF_WGRAD_LIST(QT); }      // LIST mode (below): every wave owns a run of the QT^2 tiles in row-major order
constexpr int wgrad_wk(int QT) { return QT >= 7 || wgrad_list(QT) ? 1 : (QT >= 2 ? 2 : 4); }
// dynamic LDS in floats: two double-buffered panel pairs (the k-slice fold goes through them one row of wave tiles at a time)
constexpr int wgrad_lds_floats(int NT)
{
    const int QT = wgrad_qt(NT);
    const int WMk = wgrad_wmk(QT), WNk = wgrad_wnk(QT), WK = wgrad_wk(QT);
    const int NWv = WMk * WNk, TN = (QT + WNk - 1) / WNk;
    const int fold = (WK - 1) * NWv * TN * 1024 + (WK - 1) * NWv * 64, panels = 4 * 32 * QT * 36;
    return fold > panels ? fold : panels;
}
// ... of the compile-time widths' k_wgrad<NT>: the DMA-fed layout has unpadded rows (two buffers x two panels x 256 rows x 128 bytes = 128 KiB)
constexpr int wgrad_lds_floats_ct(int NT) { return wgrad_dma_feed(NT, wgrad_qt(NT)) ? 4 * 32 * wgrad_qt(NT) * 32 : wgrad_lds_floats(NT); }

// NT > 0: compile-time width.  NT == 0: run-time width above 16 tiles (k_lean's nets), QTR tiles per quadrant side, ceil(nt / 8)
// quadrants per side; the last quadrant row / column may hold fewer than QTR tiles (its missing rows are staged as zeros).
template <int NT, int QTR = 0>
__global__ __launch_bounds__(512, 2) void k_wgrad(const WgradArgs a)
{
    constexpr bool RTW = NT == 0;
    const int nt_w = RTW ? brief_nt(a.d) : NT;
    const int FP = 32 * nt_w;
    const int NQ = RTW ? (nt_w + 7) / 8 : wgrad_nq(NT);
    constexpr int QT = RTW ? QTR : wgrad_qt(NT), QP = 32 * QT;   // quadrants per side, tiles / rows per quadrant side
    // 8 waves = WMk x WNk output-tile grid x WK-way split of each chunk's four k-groups.  Wide nets spend
    // all 8 waves on output tiles; narrow ones (QT <= 4) would leave most waves without a tile, so they
    // split K instead and fold the partial accumulators through LDS at the end (fixed order).
    // LIST (5 tiles per side: 25 tiles): wave w owns tiles [3 w, 3 w + 3) of the block in row-major order, wave 7 four of them — 6, 6, 6 and 7
    // tiles on the four SIMDs where 2 x 2 waves x (3 x 3) x two k-slices carried 9; both fragments of a tile are read per tile (LDS has the room).
    constexpr bool LIST = wgrad_list(QT);
    constexpr int LCNT = QT * QT / 8, LREM = QT * QT % 8;      // tiles per wave; the last LREM waves (on different SIMDs, LREM <= 4) take one more
    constexpr bool HET7 = QT == 7 && !LIST;
    constexpr bool DMA_FEED = wgrad_dma_feed(NT, QT) && !LIST && !HET7;      // (= !RTW && QT == 8: see BRIEF_WGRAD_DMA_FEED)
    // XS: 9, 25 and 49 tiles are 8 n + 1.  Given whole to one wave, the odd tile makes that wave's SIMD the slowest (3 tiles against 2 at QT = 3, 7 against 6 at 5,
    // 13 against 12 at 7); instead waves 0 .. 3 — one per SIMD — each take ONE of the four k-groups of every chunk of it into an extra accumulator, and wave 0 adds the
    // three partners' partial tiles through the (by then dead) LDS panels at the end, in wave order.  Roles 0 .. 3: the wave number = the k-group; 4: no share; 5 (HET7): wave 7.
    constexpr bool XS = BRIEF_WGRAD_XSPLIT && (LIST || HET7) && QT * QT % 8 == 1;
    constexpr int XSLOT = LIST ? LCNT : 6;      // the accumulator slot of the shared tile (QT - 1, QT - 1)
    // 7 tiles per side (HET7): no rectangular grid of equal wave tiles covers 49 tiles with fewer than 64 slots, so the waves get UNEQUAL
    // pieces — wave w < 7 the first six tiles of tile row w, wave 7 the whole tile column 6: 12, 12, 12 and 13 tiles on the four SIMDs (a SIMD
    // carries waves w and w + 4) instead of 16, and at most 7 accumulator tiles per wave.
    constexpr int WMk = HET7 || LIST ? 2 : wgrad_wmk(QT), WNk = HET7 || LIST ? 4 : wgrad_wnk(QT);      // (HET7, LIST: all 8 waves in k-slice 0)
    constexpr int WK = wgrad_wk(QT);
    constexpr int NWv = WMk * WNk;                 // waves per k-slice
    constexpr int TM = HET7 || LIST ? 1 : (QT + WMk - 1) / WMk, TN = LIST ? LCNT + (LREM ? 1 : 0) : (HET7 ? 7 : (QT + WNk - 1) / WNk);
    constexpr bool MEX = QT % WMk == 0, NEX = QT % WNk == 0;   // every wave tile exists
    constexpr int LDSW = 36;                       // row stride (floats): conflict-free ds_read_b128
    constexpr int NLD = (QP * 8 + 511) / 512;      // float4 loads per thread per operand per chunk
    constexpr int PANEL = QP * LDSW;
    constexpr bool FULL = (QP * 8) % 512 == 0;     // every thread has a slot in every staging pass
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2 buffers][A panel | B panel]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int wk = wave / NWv, wrem = wave % NWv;
    const int wmk = wrem / WNk, wnk = wrem % WNk;
    const bool kactive = wk < WK;                  // QT == 1 uses 4 of the 8 waves for MFMA work
    const int quad = blockIdx.x % (NQ * NQ), bsl = blockIdx.x / (NQ * NQ);
    const int qm = quad / NQ, qn = quad % NQ;
    // (the uneven form exists in the run-time-width kernels only — the plan covers 9 .. 16 tiles — so that the compile-time ones, the headline's k_wgrad<8> among them,
    //  keep their register allocation: with it k_wgrad<8> went from 253 VGPRs to 256 + 24 bytes of scratch and the headline step lost 1.3 %)
    const bool uneven = RTW && a.uneven;
    const int hidden_l = a.d.layers - 2;
    const int l = uneven ? 1 + bsl % hidden_l : 1 + bsl / a.nsplit_here;         // hidden layer 1..L-2
    const int split = uneven ? bsl / hidden_l : bsl % a.nsplit_here;              // (local; slab a.split_lo + split)
    const int64_t nchunks = a.kb_hi - a.kb_lo;
    int64_t c0 = a.kb_lo + nchunks * split / a.nsplit_here, c1 = a.kb_lo + nchunks * (split + 1) / a.nsplit_here;   // c1 > c0 (host: nsplit_here <= chunks)
    if (uneven) {
        const int g0 = a.split_lo + split, g1 = g0 + 1;
        c0 = (g0 <= a.n_norm ? g0 * a.kfix_n : a.n_norm * a.kfix_n + (g0 - a.n_norm) * a.kfix_s) >> 16;
        c1 = g1 >= a.nsplit ? a.kb_hi : ((g1 <= a.n_norm ? g1 * a.kfix_n : a.n_norm * a.kfix_n + (g1 - a.n_norm) * a.kfix_s) >> 16);
    }
    // stash planes are [32-sample chunk][FP rows][32 samples]: this quadrant's rows of a chunk are QP * 128 contiguous bytes
    const float *Dl = a.D + (int64_t)(l - 1) * FP * a.npad + qm * QP * 32;     // this quadrant's delta rows (of chunk 0)
    const float *Zl = a.Z + (int64_t)(l - 1) * FP * a.npad + qn * QP * 32;     // ... and phase rows

    f32x16 acc[TM][TN];
    float dbacc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        dbacc[i] = 0.f;
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jn][r] = 0.f;
    }
    float dbl[LIST ? TN : 1];       // LIST: row sums of every tile's A fragments (the bias gradient where the tile sits in column 0)
    int lmt[LIST ? TN : 1], lnt[LIST ? TN : 1];
    if (LIST) {
        const int first = XS ? wave * LCNT : wave * LCNT + (wave > 8 - LREM ? wave - (8 - LREM) : 0);
#pragma unroll
        for (int k = 0; k < TN; ++k) {
            const int t = first + k < QT * QT ? first + k : QT * QT - 1;
            lmt[k] = t / QT; lnt[k] = t % QT; dbl[k] = 0.f;
        }
    }
    // bias gradients from the staged row pieces: 8 tiles per side only.  Measured interleaved on one box (tools/ab_step.sh, step time, old -> staged sums
    // [+ pipelined fragment reads at 8 per side]): 4x256 1.0024 -> 0.9881 ms, 4x1024 15.15 -> 14.91; but 4x96 (LIST 3) 0.2298 -> 0.2345, 4x160 (LIST 5)
    // 0.4817 -> 0.4901, 4x224 (HET7) 0.8554 -> 0.8699, 4x527 (6 per side, two k-slices) 4.751 -> 4.803, 4x192 0.632 -> 0.634: the other layouts keep the
    // fragment-side sums (their waves own one tile row each, or a k-slice: the sums ride in MFMA shadows there)
    constexpr bool SBIAS = BRIEF_WGRAD_STAGE_BIAS && QT == 8;
    const bool want_bias = SBIAS && qn == 0;                               // (block-uniform)
    float bsum[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) bsum[i] = 0.f;
    float4 ra[NLD], rb[NLD];
    // The loop body is branch-free: the prefetch of "chunk c+2" and the staging of "chunk c+1" are
    // clamped to the last chunk instead of being skipped (the redundant copies are never read).
    // thread e fetches 16 bytes at e * 16 of the quadrant's rows; the chunk offset is a scalar (no per-load 64-bit address
    // arithmetic on the VALU, which the f32 MFMA shares)
    const int panel_bytes = (int)((int64_t)FP * a.npad * 4) - (RTW ? 0 : (NQ - 1) * QP * 128);      // to the end of the last chunk's rows of the last quadrant
    const int rows_m = RTW ? FP - qm * QP : QP, rows_n = RTW ? FP - qn * QP : QP;      // rows this quadrant really has (run-time width: the last one may be short)
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((void *)Dl, 0, panel_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsZ = __builtin_amdgcn_make_buffer_rsrc((void *)Zl, 0, panel_bytes, 0x00020000);
    int voffs[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + 512 * i;
        voffs[i] = e * 16;
    }
#define WG_ISSUE(cc)                                                                              \
    _Pragma("unroll") for (int i = 0; i < NLD; ++i) {                                             \
        const int e = tid + 512 * i;                                                              \
        ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);                                                  \
        rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);                                                  \
        if (FULL || e < QP * 8) {                                                                 \
            if (!RTW || (e >> 3) < rows_m) ra[i] = bload4w(rsD, voffs[i], (int)((cc) * (FP * 128)));     \
            if (!RTW || (e >> 3) < rows_n) rb[i] = bload4w(rsZ, voffs[i], (int)((cc) * (FP * 128)));     \
        }                                                                                         \
    }
#define WG_STAGE_A(buf, i)                                                                        \
    {                                                                                             \
        const int e = tid + 512 * (i);                                                            \
        if (FULL || e < QP * 8)                                                                   \
            *reinterpret_cast<float4 *>(smem + (buf) * 2 * PANEL + (e >> 3) * LDSW + (e & 7) * 4) = ra[i]; \
    }
#define WG_STAGE_B(buf, i)                                                                        \
    {                                                                                             \
        const int e = tid + 512 * (i);                                                            \
        if (FULL || e < QP * 8) {                                                                 \
            float4 h;                                                                             \
            h.x = BRIEF_SIN_REV(rb[i].x); h.y = BRIEF_SIN_REV(rb[i].y);   /* the stash holds revolutions */ \
            h.z = BRIEF_SIN_REV(rb[i].z); h.w = BRIEF_SIN_REV(rb[i].w);                           \
            *reinterpret_cast<float4 *>(smem + (buf) * 2 * PANEL + PANEL + (e >> 3) * LDSW + (e & 7) * 4) = h; \
        }                                                                                         \
    }
// (branch-free inside the loops: a wave-uniform `if` around it splits the MFMA groups' scheduling region — cm_ is 1 for a new chunk, 0 for the
//  clamped re-load of the last one and for workgroups that owe no bias gradient)
#define WG_BIAS_M(i, cm_) { bsum[i] = __fmaf_rn((cm_), (ra[i].x + ra[i].y) + (ra[i].z + ra[i].w), bsum[i]); }      /* rows past a short quadrant's end were loaded as zeros */
#define WG_BIAS(i) WG_BIAS_M(i, 1.0f)
    // DMA feed (8 tiles per side, compile-time width).  Piece e = tid + 512 i of a panel is 16 bytes of row e >> 3; one wave's 64 pieces of a pass are
    // 8 whole rows, written lane-linear at float e * 4 of the panel.  The lane at slot e & 7 fetches piece (e & 7) ^ sw(row), sw(row) = (row >> 1) & 7 — the
    // same for every pass (512 pieces = 64 rows) — so piece p of a row sits at slot p ^ sw(row), where the fragment reads look for it.
    constexpr int PANEL_D = QP * 32;                                    // unpadded panel (floats); a buffer is [A panel | B panel]
    typedef __attribute__((address_space(3))) void wg_lds_void;
    const int voff_dma = ((tid >> 3) * 8 + ((tid & 7) ^ ((tid >> 4) & 7))) * 16;
#define WG_DMA_ISSUE(buf, cc)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < NLD; ++i) {                                                                  \
        float *dst_ = smem + (buf) * 2 * PANEL_D + (wave * 64 + 512 * i) * 4;      /* wave-uniform; the hardware adds lane * 16 */ \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (wg_lds_void *)dst_, 16, voff_dma, (int)((cc) * (FP * 128)) + i * 8192, 0, BRIEF_WGRAD_AUX); \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsZ, (wg_lds_void *)(dst_ + PANEL_D), 16, voff_dma, (int)((cc) * (FP * 128)) + i * 8192, 0, BRIEF_WGRAD_AUX); \
    }
// LDS-DMA data is ordered for a ds_read by the issuing wave's own vmcnt only (and, for the other waves, by a barrier behind it)
// (the sched_barrier pins the MFMAs written before the wait in front of it: register-only instructions are not ordered by the "memory" clobber, and the
//  wait would otherwise drift up to the DMA issue and stall the wave there for the whole fetch)
#define WG_DMA_WAIT() { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the thread that fetched a piece finishes it in place: delta piece -> bias sum (the add order of WG_BIAS: a row's eight sums meet in the XOR tree of the
// epilogue, which gives the same bits whichever lane holds which piece), phase piece -> sine, written back where it lies
#define WG_DMA_FINISH(buf, i)                                                                                          \
    {                                                                                                                  \
        float *pa_ = smem + (buf) * 2 * PANEL_D + (tid + 512 * (i)) * 4;                                               \
        if (want_bias) {                                                                                               \
            const float4 dv_ = *reinterpret_cast<const float4 *>(pa_);                                                 \
            bsum[i] += (dv_.x + dv_.y) + (dv_.z + dv_.w);                                                              \
        }                                                                                                              \
        float4 h_ = *reinterpret_cast<const float4 *>(pa_ + PANEL_D);                                                  \
        h_.x = BRIEF_SIN_REV(h_.x); h_.y = BRIEF_SIN_REV(h_.y);   /* the stash holds revolutions */                    \
        h_.z = BRIEF_SIN_REV(h_.z); h_.w = BRIEF_SIN_REV(h_.w);                                                        \
        *reinterpret_cast<float4 *>(pa_ + PANEL_D) = h_;                                                               \
    }
    if constexpr (DMA_FEED) {
        WG_DMA_ISSUE(0, c0)
        WG_DMA_WAIT();
#pragma unroll
        for (int i = 0; i < NLD; ++i) WG_DMA_FINISH(0, i)
    } else {
    WG_ISSUE(c0)
#pragma unroll
    for (int i = 0; i < NLD; ++i) { WG_STAGE_A(0, i) WG_STAGE_B(0, i) }
    if (want_bias) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) WG_BIAS(i)
    }
    {
        const int64_t cn = c0 + 1 < c1 ? c0 + 1 : c1 - 1;
        WG_ISSUE(cn)
    }
    }
    lds_barrier();
#ifdef BRIEF_STAMPS
    float st_acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long st_last = clock64();
#endif
// a k-group of the rectangular layouts: every tile of the wave's TM x TN block takes the group's four k-steps
#define WG_MFMAS(AF, BF)                                                                                               \
        {                                                                                                              \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                           \
                _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                                                    \
                    if ((MEX || wmk * TM + i < QT) && (NEX || wnk * TN + jn < QT)) {                                   \
                        acc[i][jn] = MFMA(AF[i].x, BF[jn].x, acc[i][jn]);                                              \
                        acc[i][jn] = MFMA(AF[i].y, BF[jn].y, acc[i][jn]);                                              \
                        acc[i][jn] = MFMA(AF[i].z, BF[jn].z, acc[i][jn]);                                              \
                        acc[i][jn] = MFMA(AF[i].w, BF[jn].w, acc[i][jn]);                                              \
                    }                                                                                                  \
                }                                                                                                      \
            }                                                                                                          \
        }
    if constexpr (LIST || HET7) {
    // (one copy of the whole chunk loop per role — a role test INSIDE the loop makes the compiler carry two sets of accumulators through
    //  the merge points and spill; every wave meets the same barriers in either copy.  The rectangular layouts below keep their plain
    //  loop: wrapped in the same lambda k_wgrad<8> grew from 204 to 244 VGPRs and 4 % more VALU instructions, for the same time within +-0.3 %)
    auto chunk_loop = [&](auto role_c) __attribute__((always_inline)) {
    constexpr int ROLE = decltype(role_c)::value;
    for (int64_t c = c0; c < c1; ++c) {
        const int cur = (int)(c - c0) & 1;
        const float *As = smem + cur * 2 * PANEL, *Bs = As + PANEL;
        const float cm_l = want_bias && c + 1 < c1 ? 1.0f : 0.0f;      // the chunk staged in this iteration is a new one (not the clamped re-load of the last)
        STAMP(0)
        if constexpr (LIST) {
            constexpr int CNT = XS ? LCNT : LCNT + ROLE;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
#pragma unroll
                for (int k = 0; k < CNT; ++k) {
                    const float4 a_ = *reinterpret_cast<const float4 *>(As + (32 * lmt[k] + ln) * LDSW + 8 * gq + 4 * hi);
                    const float4 b_ = *reinterpret_cast<const float4 *>(Bs + (32 * lnt[k] + ln) * LDSW + 8 * gq + 4 * hi);
                    if (!SBIAS) dbl[k] += (a_.x + a_.y) + (a_.z + a_.w);
                    acc[0][k] = MFMA(a_.x, b_.x, acc[0][k]); acc[0][k] = MFMA(a_.y, b_.y, acc[0][k]);
                    acc[0][k] = MFMA(a_.z, b_.z, acc[0][k]); acc[0][k] = MFMA(a_.w, b_.w, acc[0][k]);
                }
                if (XS && gq == ROLE) {      // this wave's k-group of the shared tile
                    const float4 a_ = *reinterpret_cast<const float4 *>(As + (32 * (QT - 1) + ln) * LDSW + 8 * gq + 4 * hi);
                    const float4 b_ = *reinterpret_cast<const float4 *>(Bs + (32 * (QT - 1) + ln) * LDSW + 8 * gq + 4 * hi);
                    acc[0][XSLOT] = MFMA(a_.x, b_.x, acc[0][XSLOT]); acc[0][XSLOT] = MFMA(a_.y, b_.y, acc[0][XSLOT]);
                    acc[0][XSLOT] = MFMA(a_.z, b_.z, acc[0][XSLOT]); acc[0][XSLOT] = MFMA(a_.w, b_.w, acc[0][XSLOT]);
                }
                if (gq >= 2) {
#pragma unroll
                    for (int i = 0; i < NLD; ++i)
                        if ((i & 1) == (gq & 1)) { WG_STAGE_A(cur ^ 1, i) WG_STAGE_B(cur ^ 1, i) if (SBIAS) WG_BIAS_M(i, cm_l) }
                }
            }
        } else if constexpr (HET7) {
            // two wave-uniform roles, each a straight-line stream of its own over the chunk's four k-groups (the role test sits OUTSIDE
            // the k-group loop so that each stream keeps its own software pipeline of fragment reads under the MFMAs)
#define WG_FRAG(P, row) (*reinterpret_cast<const float4 *>((P) + (32 * (row) + ln) * LDSW + 8 * gq + 4 * hi))
#define WG_MFMA4(k, A_, B_) { acc[0][k] = MFMA((A_).x, (B_).x, acc[0][k]); acc[0][k] = MFMA((A_).y, (B_).y, acc[0][k]); \
                              acc[0][k] = MFMA((A_).z, (B_).z, acc[0][k]); acc[0][k] = MFMA((A_).w, (B_).w, acc[0][k]); }
#define WG_STAGE_NEXT                                                                   \
            if (gq >= 2) {                                                              \
                _Pragma("unroll") for (int i = 0; i < NLD; ++i)                         \
                    if ((i & 1) == (gq & 1)) { WG_STAGE_A(cur ^ 1, i) WG_STAGE_B(cur ^ 1, i) if (SBIAS) WG_BIAS_M(i, cm_l) } \
            }
            if constexpr (XS ? ROLE < 5 : ROLE == 0) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const float4 a_ = WG_FRAG(As, wave);
                    if (!SBIAS) dbacc[0] += (a_.x + a_.y) + (a_.z + a_.w);
#pragma unroll
                    for (int jn = 0; jn < 6; ++jn) {
                        const float4 b_ = WG_FRAG(Bs, jn);
                        WG_MFMA4(jn, a_, b_)
                    }
                    if (XS && gq == ROLE) {      // this wave's k-group of the shared tile (6, 6)
                        const float4 a6 = WG_FRAG(As, 6), b6 = WG_FRAG(Bs, 6);
                        WG_MFMA4(6, a6, b6)
                    }
                    WG_STAGE_NEXT
                }
            } else {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const float4 b6 = WG_FRAG(Bs, 6);
#pragma unroll
                    for (int i = 0; i < (XS ? 6 : 7); ++i) {
                        const float4 a_ = WG_FRAG(As, i);
                        WG_MFMA4(i, a_, b6)
                    }
                    WG_STAGE_NEXT
                }
            }
#undef WG_FRAG
#undef WG_MFMA4
#undef WG_STAGE_NEXT
        }
        STAMP(1)
        {
            const int64_t cn = c + 2 < c1 ? c + 2 : c1 - 1, cn1 = c + 1 < c1 ? c + 1 : c1 - 1;
            WG_ISSUE(cn)
        }
        STAMP(2)
        lds_barrier();
        STAMP(3)
    }
    };
    if constexpr (XS) {
        if (wave == 0) chunk_loop(RoleC<0>{});
        else if (wave == 1) chunk_loop(RoleC<1>{});
        else if (wave == 2) chunk_loop(RoleC<2>{});
        else if (wave == 3) chunk_loop(RoleC<3>{});
        else if (HET7 && wave == 7) chunk_loop(RoleC<5>{});
        else chunk_loop(RoleC<4>{});
        // the shared tile's four partial sums: waves 1 .. 3 park theirs in the panels (dead: the loop ended on a barrier), wave 0 adds them in wave order
        if (wave >= 1 && wave <= 3) {
#pragma unroll
            for (int r = 0; r < 16; ++r) smem[(wave - 1) * 1024 + r * 64 + lane] = acc[0][XSLOT][r];
        }
        lds_barrier();
        if (wave == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][XSLOT][r] += smem[w * 1024 + r * 64 + lane];
        }
    } else {
        if (LIST ? (LREM > 0 && wave >= 8 - LREM) : wave == 7) chunk_loop(RoleC<1>{});
        else chunk_loop(RoleC<0>{});
    }
    } else if constexpr (DMA_FEED) {
    // After the barrier that ended chunk c - 1 every wave has left buffer cur ^ 1.  Chunk c + 1's sixteen DMA instructions per wave (eight per thread: 4 delta + 4
    // phase pieces) are issued into it BEHIND chunk c's last fragment read — behind the builtin hipcc waits vmcnt(0) in front of the next ds_read of any LDS
    // address, so issued at the top of the chunk they would stall every k-group's fragment reads for the whole fetch — and land under k-group 2's MFMAs; in the
    // shadow of k-group 3 the wave waits for its OWN pieces and finishes them in place; the chunk-end barrier (lgkmcnt(0) + s_barrier: it does not drain VMEM,
    // and nothing is in flight there) publishes the buffer, whose fragments are read one phase later.  No VGPR carries operand data from one iteration to the
    // next; the last chunk is its own copy of the body with nothing to stage.  (Measured beside it, profiles/r22_wgrad_feed.md: wait + finish behind k-group 3,
    // and the issue at the top of the chunk as a hand-written statement that hipcc does not count — both slower.)
    const int sw_d = ((ln >> 1) & 7) * 4;
#define WG_READ_FRAGS_D(gq_, AF, BF)                                                                                   \
        {                                                                                                              \
            const int fo_ = ln * 32 + ((8 * (gq_) + 4 * hi) ^ sw_d);                                                   \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) AF[i] = *reinterpret_cast<const float4 *>(As + 1024 * (wmk * TM + i) + fo_); \
            _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) BF[jn] = *reinterpret_cast<const float4 *>(Bs + 1024 * (wnk * TN + jn) + fo_); \
        }
#define WG_DMA_CHUNK(ST)                                                                                               \
    {                                                                                                                  \
        const int cur = (int)(c - c0) & 1;                                                                             \
        const float *As = smem + cur * 2 * PANEL_D, *Bs = As + PANEL_D;                                                \
        STAMP(0)                                                                                                       \
        float4 af0[TM], bf0[TN], af1[TM], bf1[TN];                                                                     \
        WG_READ_FRAGS_D(0, af0, bf0)                                                                                   \
        WG_READ_FRAGS_D(1, af1, bf1)                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        WG_MFMAS(af0, bf0)                                                                                             \
        WG_READ_FRAGS_D(2, af0, bf0)                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        WG_MFMAS(af1, bf1)                                                                                             \
        WG_READ_FRAGS_D(3, af1, bf1)                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        if (ST) { WG_DMA_ISSUE(cur ^ 1, c + 1) }                                                                       \
        WG_MFMAS(af0, bf0)                                                                                             \
        if (ST) { WG_DMA_WAIT(); WG_DMA_FINISH(cur ^ 1, 0) WG_DMA_FINISH(cur ^ 1, 2) }                                 \
        WG_MFMAS(af1, bf1)                                                                                             \
        if (ST) { WG_DMA_FINISH(cur ^ 1, 1) WG_DMA_FINISH(cur ^ 1, 3) }                                                \
        STAMP(1)                                                                                                       \
    }
    int64_t c = c0;
    for (; c + 1 < c1; ++c) {
        WG_DMA_CHUNK(1)
        lds_barrier();
        STAMP(3)
    }
    WG_DMA_CHUNK(0)
#undef WG_DMA_CHUNK
#undef WG_READ_FRAGS_D
    } else {
    for (int64_t c = c0; c < c1; ++c) {
        const int cur = (int)(c - c0) & 1;
        const float *As = smem + cur * 2 * PANEL, *Bs = As + PANEL;
        const float cm_r = want_bias && c + 1 < c1 ? 1.0f : 0.0f;      // the chunk staged in this iteration is a new one (not the clamped re-load of the last)
        STAMP(0)
#define WG_READ_FRAGS(gq_, AF, BF)                                                                                     \
        {                                                                                                              \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                           \
                const int mt = wmk * TM + i;                                                                           \
                AF[i] = make_float4(0.f, 0.f, 0.f, 0.f);                                                               \
                if (MEX || mt < QT) AF[i] = *reinterpret_cast<const float4 *>(As + (32 * mt + ln) * LDSW + 8 * (gq_) + 4 * hi); \
            }                                                                                                          \
            _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                                                        \
                const int nt = wnk * TN + jn;                                                                          \
                BF[jn] = make_float4(0.f, 0.f, 0.f, 0.f);                                                              \
                if (NEX || nt < QT) BF[jn] = *reinterpret_cast<const float4 *>(Bs + (32 * nt + ln) * LDSW + 8 * (gq_) + 4 * hi); \
            }                                                                                                          \
        }
        // The next chunk's staging rides in the shadow of the LAST two MFMA groups: its global loads were
        // issued at the end of the previous iteration and get the barrier + two groups to land.
#define WG_STAGE_NEXT(gq_)                                                                                             \
        if ((gq_) >= 2) {                                                                                              \
            _Pragma("unroll") for (int i = 0; i < NLD; ++i)                                                            \
                if ((i & 1) == ((gq_) & 1)) {                                                                          \
                    WG_STAGE_A(cur ^ 1, i) WG_STAGE_B(cur ^ 1, i)                                                      \
                    if (SBIAS) WG_BIAS_M(i, cm_r)                                                                      \
                }                                                                                                      \
        }
        if constexpr (BRIEF_WGRAD_FRAG_PIPE && WK == 1 && QT == 8) {
            // 8 tiles per side: every wave works all four k-groups; k-group g + 1's fragments are requested before k-group g's MFMAs issue
            float4 af0[TM], bf0[TN], af1[TM], bf1[TN];
            WG_READ_FRAGS(0, af0, bf0)
            WG_READ_FRAGS(1, af1, bf1)
            __builtin_amdgcn_sched_barrier(0);
            WG_MFMAS(af0, bf0)
            WG_READ_FRAGS(2, af0, bf0)
            __builtin_amdgcn_sched_barrier(0);
            WG_MFMAS(af1, bf1)
            WG_READ_FRAGS(3, af1, bf1)
            __builtin_amdgcn_sched_barrier(0);
            WG_MFMAS(af0, bf0)
            WG_STAGE_NEXT(2)
            WG_MFMAS(af1, bf1)
            WG_STAGE_NEXT(3)
        } else if constexpr (BRIEF_WGRAD_FRAG_PIPE2 && WK == 2 && QT >= 4) {
            // two k-slices (4 and 6 tiles per side): a wave works k-groups wk and wk + 2; both groups' fragments are requested up front
            float4 af0[TM], bf0[TN], af1[TM], bf1[TN];
            WG_READ_FRAGS(wk, af0, bf0)
            WG_READ_FRAGS(wk + 2, af1, bf1)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
                if (wnk == 0) {      // (k-group wk, then wk + 2: the order of the un-pipelined loop, bit for bit)
                    dbacc[i] += (af0[i].x + af0[i].y) + (af0[i].z + af0[i].w);
                    dbacc[i] += (af1[i].x + af1[i].y) + (af1[i].z + af1[i].w);
                }
            WG_MFMAS(af0, bf0)
            WG_STAGE_NEXT(2)
            WG_MFMAS(af1, bf1)
            WG_STAGE_NEXT(3)
        } else {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            if (kactive && (WK == 1 || (gq % WK) == wk)) {
                float4 af[TM], bf[TN];
                WG_READ_FRAGS(gq, af, bf)
                if (!SBIAS) {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
                        if (wnk == 0) dbacc[i] += (af[i].x + af[i].y) + (af[i].z + af[i].w);
                }
                WG_MFMAS(af, bf)
            }
            WG_STAGE_NEXT(gq)
        }
        }
#undef WG_READ_FRAGS
#undef WG_MFMAS
#undef WG_STAGE_NEXT
        STAMP(1)
        {
            const int64_t cn = c + 2 < c1 ? c + 2 : c1 - 1, cn1 = c + 1 < c1 ? c + 1 : c1 - 1;
            WG_ISSUE(cn)
        }
        STAMP(2)
        lds_barrier();
        STAMP(3)
    }
    }
#ifdef BRIEF_STAMPS
    if (lane == 0 && a.stamps) for (int i = 0; i < 4; ++i) a.stamps[((int64_t)blockIdx.x * 8 + wave) * 8 + i] = st_acc[i];
#endif
#undef WG_ISSUE
#undef WG_STAGE_A
#undef WG_STAGE_B
#undef WG_BIAS
#undef WG_BIAS_M
#undef WG_DMA_ISSUE
#undef WG_DMA_WAIT
#undef WG_DMA_FINISH
    if (WK > 1) {
        // fold the k-slices, one row of wave tiles at a time: slices 1..WK-1 park accumulator row i in LDS (the panels are dead now:
        // the loop ended on a barrier), slice 0 adds them in slice order (row by row so that the area never exceeds the panels)
        float *red = smem;
        float *redb = smem + (WK - 1) * NWv * TN * 1024;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i > 0) lds_barrier();      // slice 0 is done with the previous row's partials
            if (kactive && wk > 0) {
#pragma unroll
                for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[(((wk - 1) * NWv + wrem) * TN + jn) * 1024 + r * 64 + lane] = acc[i][jn][r];
                redb[((wk - 1) * NWv + wrem) * 64 + lane] = dbacc[i];
            }
            lds_barrier();
            if (wk == 0) {
                for (int w = 1; w < WK; ++w) {
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            acc[i][jn][r] += red[(((w - 1) * NWv + wrem) * TN + jn) * 1024 + r * 64 + lane];
                    dbacc[i] += redb[((w - 1) * NWv + wrem) * 64 + lane];
                }
            }
        }
    }
    float *slab = a.slabs + ((int64_t)(l - 1) * a.nsplit + a.split_lo + split) * ((int64_t)FP * FP + FP);
    if (want_bias) {
        // the eight threads that staged the eight 16-byte pieces of a row are neighbouring lanes: fixed-order tree over them
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 512 * i;
            if (FULL || e < QP * 8) {
                float v = bsum[i];
                v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                if ((tid & 7) == 0 && (e >> 3) < rows_m) slab[(int64_t)FP * FP + qm * QP + (e >> 3)] = v;
            }
        }
    }
    if (wk != 0) return;
    if (LIST) {
        const int cnt = XS ? LCNT + (wave == 0 ? 1 : 0) : LCNT + (LREM > 0 && wave >= 8 - LREM ? 1 : 0);
#pragma unroll
        for (int k = 0; k < TN; ++k) {
            if (k >= cnt) break;
            const int mt = XS && k == LCNT ? QT - 1 : lmt[k], nt = XS && k == LCNT ? QT - 1 : lnt[k];      // (XS: wave 0's extra slot is the shared tile)
            if ((!RTW || qm * QT + mt < nt_w) && (!RTW || qn * QT + nt < nt_w)) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(qm * QP + 32 * mt + ROWMAP(r, hi)) * FP + qn * QP + 32 * nt + ln] = acc[0][k][r];
            }
            if (!SBIAS && qn == 0 && nt == 0 && !(XS && k == LCNT)) {
                const float tot = dbl[k] + __shfl_xor(dbl[k], 32);
                if (hi == 0 && (!RTW || qm * QT + mt < nt_w)) slab[(int64_t)FP * FP + qm * QP + 32 * mt + ln] = tot;
            }
        }
        return;
    }
    if (HET7) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            int mt = wave < 7 ? wave : k, nt = wave < 7 ? k : 6;
            if (XS) {
                if (k == 6) { if (wave != 0) continue; mt = 6; nt = 6; }      // the shared tile, summed in wave 0's slot 6
            } else if (wave < 7 && k == 6) continue;
            if ((!RTW || qm * QT + mt < nt_w) && (!RTW || qn * QT + nt < nt_w)) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(qm * QP + 32 * mt + ROWMAP(r, hi)) * FP + qn * QP + 32 * nt + ln] = acc[0][k][r];
            }
        }
        if (!SBIAS && qn == 0 && wave < 7) {      // bias gradients: tile row w from wave w
            const float tot = dbacc[0] + __shfl_xor(dbacc[0], 32);
            if (hi == 0 && (!RTW || qm * QT + wave < nt_w)) slab[(int64_t)FP * FP + qm * QP + 32 * wave + ln] = tot;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mt = wmk * TM + i;
        if (mt < QT && (!RTW || qm * QT + mt < nt_w)) {
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
                const int nt = wnk * TN + jn;
                if (nt < QT && (!RTW || qn * QT + nt < nt_w)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        slab[(int64_t)(qm * QP + 32 * mt + ROWMAP(r, hi)) * FP + qn * QP + 32 * nt + ln] = acc[i][jn][r];
                }
            }
            if (!SBIAS && wnk == 0 && qn == 0) {
                const float tot = dbacc[i] + __shfl_xor(dbacc[i], 32);
                if (hi == 0) slab[(int64_t)FP * FP + qm * QP + 32 * mt + ln] = tot;
            }
        }
    }
}
