// brief_device.inc — shared device-side definitions: MFMA / row maps, KCfg, kernel argument structs, coordinate synthesis, buffer loads, the unrolled chain, Philox index stream, build-time knobs (part of the single translation unit brief_hip.hip, which includes it in this order;
// it uses what the parts before it define).
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// row of accumulator register r (0..15) inside a 32x32 tile, for lane half hi
#define ROWMAP(r, hi) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hi))
template <int V> struct RoleC { static constexpr int value = V; };

template <int NT, bool INFER = false>      // INFER: the inference kernels' wave mapping (brief_layout.h: brief_wm / brief_wm_infer)
struct KCfg {
    static constexpr int WM = INFER ? brief_wm_infer(NT) : brief_wm(NT);           // waves along the feature dimension
    static constexpr int WS = 4 / WM;                 // 32-sample tiles per workgroup
    static constexpr int MTW = (NT + WM - 1) / WM;    // feature tiles owned by one wave
    static constexpr bool EXACT = (NT % WM) == 0;
    static constexpr int FP = 32 * NT;
    static constexpr int XS_FLOATS = WS * NT * 1024;  // activation image(s)
    static constexpr int TROWS = 32 * MTW;            // local features one wave owns
    static constexpr int RS = (TROWS + 63) / 64;      // local-feature slots per lane in the skinny-gradient pass
    static constexpr int T_FLOATS = 4 * TROWS * 33;   // per-wave transposed scratch
    static constexpr int G_FLOATS = 4 * 256;          // per-wave g[4][32] + xs[32][4]
};

struct GridArgs {
    int ndim;
    int64_t dims[3];
    float lo, hi;
    float step[3];
    int fast;               // the grid has fewer than 2^32 points: 32-bit indices, division by multiplication
    uint64_t magic[3];      // floor(2^64 / dims[a]) + 1   (exact quotients for every 32-bit numerator)
};

// a strided box of a grid (brief_siren_forward_box): box voxel (i0, i1, i2), in (d,h,w) order, is grid voxel start + step * i on
// every axis; box-linear index b = (i0 * extent[1] + i1) * extent[2] + i2.  Axes past cin are unused.
struct BoxArgs {
    int64_t start[3], step[3], extent[3];
    uint64_t magic[3];      // floor(2^64 / extent[a]) + 1
    int fast;               // the box has fewer than 2^32 voxels: 32-bit split (every grid dim is below 2^31, whatever the grid's size)
};

// n / dv for a loop-invariant divisor (Lemire's fastdiv: one 64-bit multiply-high instead of ~100 VALU
// instructions of 64-bit division; the VALU is what the f32 MFMA competes with)
__device__ __forceinline__ uint32_t fast_div(uint32_t nn, uint64_t magic, uint32_t dv)
{
    return dv == 1 ? nn : (uint32_t)__umul64hi(magic, (uint64_t)nn);
}

struct FusedArgs {
    brief_siren_desc d;
    const float *pk;
    const float *coords;
    const float *targets;
    const float *weights;
    const int64_t *idx;
    int64_t offset;
    int64_t n;
    uint64_t rng_pop, rng_seed, rng_step;   // idx == NULL && rng_pop > 0: sample j in-kernel (Philox)
    GridArgs grid;
    int loss_kind;
    float thr, beta, inv_count;
    float *Z;            // [(L-2)][npad/32][FP][32]   phases (om z reduced to revolutions) of layers 0..L-3, tile-blocked: a 32-sample tile's rows are 128 B apart
    float *D;            // [(L-2)][npad/32][FP][32]   deltas of layers 1..L-2, same layout
    int64_t npad;
    float *rec;          // [gridDim.x*4][BRIEF_REC_FLOATS]
    int64_t n_begin, n_end;   // the sample range of this launch (body / tail launches: bf16 path; k_lean / k_wide TRAIN under the overlap plan; 0, 0: the whole batch)
    int rec_base;             // first record slot (workgroup number) of this launch
    void *S16[5];        // bf16 path: stashes THETA (fp16 phases) | unused | D (bf16 deltas) ([(L-1)][FP][npad] each), X [4][npad], G [4][npad]
    float *slabs;        // k_small: [(L-2)][gridDim.x][FP*FP + FP] per-workgroup hidden-layer gradient partials; k_wide<.., true>: [gridDim.x][2][FP*32] image-ordered planes
    float *yhat_out;     // [n][cout] or NULL
    void *out;           // forward output
    int out_kind;
    float scale_min, den, span, vmin;   // fused invnormalize
    int stagger_cus;     // workgroups per residency slot (= CU count)
    int stagger;         // s_sleep(127) units of start delay per slot
    int pers_wgs;        // k_fused: workgroups [0, pers_wgs) walk tiles b, b + pers_wgs, ... < pers_tiles (the persistent body);
    int64_t pers_tiles;  //          workgroup b >= pers_wgs takes the single tile pers_tiles + b - pers_wgs (see fused_plan)
    int diag;            // timing diagnostics only (BRIEF_DIAG): bit 0 = stash descriptors with zero records (the range check then
                         // drops every stash load and store: results are wrong, the instruction stream is unchanged)
};
// The argument of the box instantiations (<.., BOX = true>, inference only): sample j = offset + n is box voxel j (box_coords).  The box
// lives in a struct of its own behind FusedArgs, so that every other instantiation keeps its kernel-argument segment (and with it the
// offsets of the hidden arguments behind it) exactly as it was.
struct FusedBoxArgs : FusedArgs {
    BoxArgs box;
};
template <bool BOX> struct KArgsT { using type = FusedArgs; };
template <> struct KArgsT<true> { using type = FusedBoxArgs; };
// the kernel's only argument, read through the constant address space (what the BOX instantiations read the box from)
typedef const __attribute__((address_space(4))) FusedBoxArgs *kargs_box;

// Workgroup barrier for LDS hand-offs only.  __syncthreads() also emits s_waitcnt vmcnt(0), which
// drains every global load / store still in flight (register prefetches, stash stores) at each
// barrier; all cross-wave traffic in these kernels goes through LDS, so waiting for the LDS queue is
// enough (cdna_hip_programming.md, 'Pipelining across barriers').
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// torch.linspace as torch-CPU evaluates it (utils/dataset.py:28-32; SURVEY.md a11)
__device__ __forceinline__ float lin_coord(const GridArgs &g, int a, int64_t i)
{
    const int64_t nn = g.dims[a];
    if (nn == 1) return g.lo;
    return i < nn / 2 ? __fmaf_rn(g.step[a], (float)i, g.lo) : __fmaf_rn(-g.step[a], (float)(nn - 1 - i), g.hi);
}

__device__ __forceinline__ float lin_coord32(const GridArgs &g, int a, uint32_t i)
{
    const uint32_t nn = (uint32_t)g.dims[a];
    if (nn == 1) return g.lo;
    return i < nn / 2 ? __fmaf_rn(g.step[a], (float)i, g.lo) : __fmaf_rn(-g.step[a], (float)(nn - 1 - i), g.hi);
}

// voxel index -> coordinates of the flattened (d,h,w) / (h,w) grid (create_flattened_coords, utils/dataset.py:36-62)
__device__ __forceinline__ void grid_coords(const GridArgs &g, int cin, int64_t j, float &x0, float &x1, float &x2)
{
    if (cin == 3) {
        int64_t id, ih, iw;
        if (g.fast) {
            const uint32_t ju = (uint32_t)j, d2 = (uint32_t)g.dims[2], d1 = (uint32_t)g.dims[1];
            const uint32_t t2 = fast_div(ju, g.magic[2], d2);
            const uint32_t t1 = fast_div(t2, g.magic[1], d1);
            x0 = lin_coord32(g, 0, t1);
            x1 = lin_coord32(g, 1, t2 - t1 * d1);
            x2 = lin_coord32(g, 2, ju - t2 * d2);
            return;
        } else {
            iw = j % g.dims[2];
            const int64_t t2 = j / g.dims[2];
            ih = t2 % g.dims[1]; id = t2 / g.dims[1];
        }
        x0 = lin_coord(g, 0, id);
        x1 = lin_coord(g, 1, ih);
        x2 = lin_coord(g, 2, iw);
    } else {
        int64_t ih, iw;
        if (g.fast) {
            const uint32_t ju = (uint32_t)j, d1 = (uint32_t)g.dims[1];
            const uint32_t t1 = fast_div(ju, g.magic[1], d1);
            x0 = lin_coord32(g, 0, t1);
            x1 = lin_coord32(g, 1, ju - t1 * d1);
            return;
        } else {
            iw = j % g.dims[1]; ih = j / g.dims[1];
        }
        x0 = lin_coord(g, 0, ih);
        x1 = lin_coord(g, 1, iw);
    }
}

// box-linear index b -> coordinates of grid voxel start + step * i (the box of the kernel argument, see BoxArgs).  The full index on
// each axis is below 2^31, so the coordinate is lin_coord32 of it: the same float the whole-grid decode gives that voxel, bit for bit.
__device__ __forceinline__ void box_coords(const GridArgs &g, int cin, int64_t b, float &x0, float &x1, float &x2)
{
    kargs_box ap = (kargs_box)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    uint32_t i0, i1, i2 = 0u;
    if (cin == 3) {
        const uint32_t e2 = (uint32_t)ap->box.extent[2], e1 = (uint32_t)ap->box.extent[1];
        if (ap->box.fast) {
            const uint32_t bu = (uint32_t)b;
            const uint32_t t2 = fast_div(bu, ap->box.magic[2], e2);
            const uint32_t t1 = fast_div(t2, ap->box.magic[1], e1);
            i0 = t1; i1 = t2 - t1 * e1; i2 = bu - t2 * e2;
        } else {
            const int64_t t2 = b / (int64_t)e2, t1 = t2 / (int64_t)e1;
            i0 = (uint32_t)t1; i1 = (uint32_t)(t2 - t1 * e1); i2 = (uint32_t)(b - t2 * e2);
        }
    } else {
        const uint32_t e1 = (uint32_t)ap->box.extent[1];
        if (ap->box.fast) {
            const uint32_t bu = (uint32_t)b;
            const uint32_t t1 = fast_div(bu, ap->box.magic[1], e1);
            i0 = t1; i1 = bu - t1 * e1;
        } else {
            const int64_t t1 = b / (int64_t)e1;
            i0 = (uint32_t)t1; i1 = (uint32_t)(b - t1 * e1);
        }
    }
    x0 = lin_coord32(g, 0, (uint32_t)ap->box.start[0] + (uint32_t)ap->box.step[0] * i0);
    x1 = lin_coord32(g, 1, (uint32_t)ap->box.start[1] + (uint32_t)ap->box.step[1] * i1);
    if (cin == 3) x2 = lin_coord32(g, 2, (uint32_t)ap->box.start[2] + (uint32_t)ap->box.step[2] * i2);
}

// the coordinate synthesis of a kernel instantiation: the whole flattened grid, or (BOX, inference only) a box of it.  BOX = false compiles
// to grid_coords alone, so the instantiations without the box (every TRAIN one) carry no instruction of it.
template <bool BOX>
__device__ __forceinline__ void sample_coords(const GridArgs &g, int cin, int64_t j, float &x0, float &x1, float &x2)
{
    if constexpr (BOX) box_coords(g, cin, j, x0, x1, x2);
    else grid_coords(g, cin, j, x0, x1, x2);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 16-byte buffer load: one VGPR byte offset per lane + a scalar byte offset, so no per-block
// 64-bit address VGPRs exist for the compiler to hoist and spill (cdna_hip_programming.md T8).
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
#ifndef BRIEF_WGRAD_AUX
#define BRIEF_WGRAD_AUX 0      // cache policy of k_wgrad's operand panels (2: streaming)
#endif
__device__ __forceinline__ float4 bload4w(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, BRIEF_WGRAD_AUX);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
__device__ __forceinline__ void bstore1(float v, __amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, voff, soff, 0);
}
// the split-precision fused kernel's stash accesses, with a cache-policy knob of their own (see BRIEF_X3W_AUX for the reader's side)
#ifndef BRIEF_STASH_LD_AUX
#define BRIEF_STASH_LD_AUX 0      // phase reloads of the dgrad chains (k_fused and k_fused_x3): read once (experiment: 2)
#endif
#ifndef BRIEF_X3_STASH_AUX
#define BRIEF_X3_STASH_AUX 0      // k_fused_x3's own stash stores / phase reloads: the streaming policy costs it 9-10 us (measured), default policy
#endif
__device__ __forceinline__ float bload1s(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, BRIEF_STASH_LD_AUX));
}
__device__ __forceinline__ void bstore1s(float v, __amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, voff, soff, BRIEF_X3_STASH_AUX);
}

// One layer's GEMM for the feature tiles this wave owns:  acc[t] += A(mt,:) * image.
// A fragments stream from the packed weight buffer (L2 resident) PD (kt,q)-steps ahead of use.
// kit: (k-tile, q) steps that hold real features, ceil(F / 8): the steps above it multiply zero weight columns with the
// zero activations of the padding features, so skipping them changes nothing but the time (F = 22 runs 3 of its 4 steps)
template <int NT, bool INFER = false>
__device__ __forceinline__ void chain(f32x16 (&acc)[(KCfg<NT, INFER>::MTW)], __amdgpu_buffer_rsrc_t rs, int soff_layer /*bytes*/,
                                      const float4 *Xs, int wm, int lane, int kit)
{
    using K = KCfg<NT, INFER>;
    constexpr int NIT = NT * 4;
    constexpr int PD = NIT < 4 ? NIT : 4;
    const int voff = lane * 16;
    int soff_w = soff_layer + wm * (NT * 4 * 1024);
    // opaque to the optimiser: otherwise all 2*NT*4 per-block scalar offsets are hoisted out of the tile
    // loop, spilled to VGPR lanes and fetched back with v_readlane (a VALU op the f32 MFMA has to wait for)
    asm volatile("" : "+s"(soff_w));
    constexpr int smul = 1024;
    float4 areg[NIT][K::MTW];
    float4 breg[NIT];
    // padding is at most 31 features = the last three steps: only those carry a run-time check (on their MFMAs)
#pragma unroll
    for (int it = 0; it < PD; ++it)
#pragma unroll
        for (int t = 0; t < K::MTW; ++t)
            if (K::EXACT || wm + K::WM * t < NT) areg[it][t] = bload4(rs, voff, soff_w + (K::WM * t * NT * 4 + it) * smul);
    breg[0] = Xs[lane];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (it >= NIT - 3 && it >= kit) break;
        // (the prefetch is not predicated on kit: behind a wave-uniform branch the s_waitcnt bookkeeping counts the load as possibly
        //  missing and waits one step early — prefetch depth 3, 2, 1 over steps NIT-7 .. NIT-5; the padded steps hold zero fragments)
        if (it + PD < NIT) {
#pragma unroll
            for (int t = 0; t < K::MTW; ++t)
                if (K::EXACT || wm + K::WM * t < NT) {
                    areg[it + PD][t] = bload4(rs, voff, soff_w + (K::WM * t * NT * 4 + it + PD) * smul);
                }
        }
        if (it + 1 < NIT) breg[it + 1] = Xs[(it + 1) * 64 + lane];
        // pin the prefetch above this step's MFMAs: left alone, the scheduler sinks each load to
        // just before its use (one register set, vmcnt(0) per step, L2 latency fully exposed)
        __builtin_amdgcn_sched_barrier(0);
        const float4 b = breg[it];
#pragma unroll
        for (int t = 0; t < K::MTW; ++t) {
            if (K::EXACT || wm + K::WM * t < NT) {
                const float4 a = areg[it][t];
                acc[t] = MFMA(a.x, b.x, acc[t]);
                acc[t] = MFMA(a.y, b.y, acc[t]);
                acc[t] = MFMA(a.z, b.z, acc[t]);
                acc[t] = MFMA(a.w, b.w, acc[t]);
            }
        }
    }
}

template <int NT, bool INFER = false>
__device__ __forceinline__ void write_image(float4 *Xs, const f32x16 (&h)[(KCfg<NT, INFER>::MTW)], int wm, int lane)
{
    using K = KCfg<NT, INFER>;
#pragma unroll
    for (int t = 0; t < K::MTW; ++t) {
        const int mt = wm + K::WM * t;
        if (K::EXACT || mt < NT) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Xs[(mt * 4 + q) * 64 + lane] = make_float4(h[t][4 * q], h[t][4 * q + 1], h[t][4 * q + 2], h[t][4 * q + 3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 voxel-index stream (stands in for the CPU torch.randint of main.py:156)
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

__device__ __forceinline__ int64_t philox_index(int64_t i, uint64_t pop, uint64_t seed, uint64_t step)
{
    uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t r64 = ((uint64_t)c[0] << 32) | c[1];
    return (int64_t)__umul64hi(r64, pop);      // multiply-shift: bias < pop / 2^64
}

// LDS map of k_fused (floats):  R = max(image, transpose scratch) | G (per-wave g / coords) | HW (head weights)
//   image  X : WS x NT x 1024            activation register image(s)
//   scratch T: 4 waves x 32*MTW x 33      per-wave [feature][sample] transpose (aliases X: used only while
//                                         no wave reads the image, see the barriers below)
#ifndef BRIEF_FUSED64
#ifndef BRIEF_LEAN_RM3
#define BRIEF_LEAN_RM3 1     // nt % 4 == 3: the three left-over tiles shared along K (lean_chain_rt3); 0: wave 3 computes a duplicate (A/B)
#endif
#define BRIEF_FUSED64 0      // 1: the 8-tile TRAIN step walks 64-sample tiles (k_lean<2, 2, 8>) instead of k_fused<8>'s 32-sample tiles
#endif
#ifndef BRIEF_KERNARG_RELOAD
#define BRIEF_KERNARG_RELOAD 1
#endif
#ifndef BRIEF_TRAIN_WPE
#define BRIEF_TRAIN_WPE 2   // waves per SIMD the TRAIN variant is register-allocated for
#endif
#if defined(BRIEF_STAMPS) && BRIEF_STAMPS + 0 != 2      /* -DBRIEF_STAMPS=2: only the start / end clock pair (the product instruction stream otherwise) */
#define STAMP(slot) { const long long t_ = clock64(); st_acc[slot] += (float)(t_ - st_last); st_last = t_; }
#else
#define STAMP(slot)
#endif
