// brief_mfn.inc — the multiplicative filter networks MFNFourier / MFNGabor (Fathony et al., ICLR 2021): k_mfn_fwd<MTW, TRAIN, BOX,
// GABOR>, k_mfn_wgrad, k_mfn_repack (part of the single translation unit brief_hip.hip, included after brief_nerf.inc; the reduction
// is that file's k_ffn_reduce with bv = 0).  Only new kernels: no existing kernel, device function or argument struct is changed.
//
// Net (reference utils/Networks.py:648-799), L = layers, F = features, x = coordinates:
//   filter i = 0 .. L-2:  a_i = Wf_i x + bf_i,  g_i = sin(a_i)  (Fourier)  or  sin(a_i) exp(-0.5 D_i gamma_i),
//                         D_i = |x|^2 + |mu_i|^2 - 2 x.mu_i  (Gabor, the reference's expanded form)
//   z_0 = g_0,  u_i = W_i z_{i-1} + b_i,  z_i = g_i . u_i  (i = 1 .. L-2),  out = Wo z_{L-2} + bo  (sin(out) with output_act)
// No activation sits between the layers: every hidden GEMM's epilogue multiplies its accumulators by the filter of the (feature,
// sample) elements the lane holds.  Filters use brief_sincosf (brief_math.h, 3-term Cody-Waite reduction: |err| <= 1.2e-7 for the
// few hundred radians the default init reaches) and the accurate expf.  The backward recomputes sin / cos / envelope from x instead
// of stashing them (profiles/r09_mfn.md).
//
// LDS per workgroup: the hidden image [FP rows][32 samples] plus 32 x float4 (x_0, x_1, x_2, |x|^2) of the tile; z_0 is written
// straight into the image.  F = 525: 70 144 bytes (two workgroups per CU); F = 1024: 131 584 (one).
//
// Packed layout (floats; FP = 32 nt, fragment block (mt, step) = 64 lanes x float4, A[32 mt + i][8 step + 4 hi + j]):
//   per hidden layer l = 1 .. L-2:  Wf [nt][FP / 8][64][4] (W_l), Wb [nt][FP / 8][64][4] (W_l^T), b [FP]
//   Whf  [1][FP / 8][64][4]  (rows >= cout zero),  Whb [nt][4][64][4]  (Wo^T, columns >= cout zero),  bh [32] (rows >= cout zero)
//   per filter i = 0 .. L-2:  FW [FP][4] = (w_0, w_1, w_2, b)  and, Gabor only, FG [FP][4] = (mu_0, mu_1, mu_2, gamma), FQ [FP] = |mu|^2
//   (features >= F and coordinates >= cin zero)
// Train stash (workspace, [rows][npad] feature-major planes): Z_i (i = 0 .. L-2), U_i and DU_i = dL/du_i (i = 1 .. L-2), DA_i = dL/da_i
// and, Gabor only, Q_i = dL/dg_i . sin(a_i) . e_i (i = 0 .. L-2), XP [5][npad] = (x_0, x_1, [x_2,] |x|^2, 1) per sample, G [4][npad] =
// dL/d(out) (the head's pre-activation).

struct MfnLayout {
    int nt, FP;
    int64_t hid, hid_stride, whf, whb, bh, filt, filt_stride, total;
};
BL_HD MfnLayout mfn_layout(const brief_mfn_desc &d)
{
    MfnLayout o;
    o.nt = (d.features + 31) / 32; o.FP = 32 * o.nt;
    o.hid = 0;
    o.hid_stride = 2 * (int64_t)o.FP * o.FP + o.FP;
    o.whf = o.hid + (int64_t)(d.layers - 2) * o.hid_stride;
    o.whb = o.whf + 32 * (int64_t)o.FP;
    o.bh = o.whb + 32 * (int64_t)o.FP;
    o.filt = o.bh + 32;
    o.filt_stride = (d.filter ? 9 : 4) * (int64_t)o.FP;
    o.total = o.filt + (int64_t)(d.layers - 1) * o.filt_stride;
    return o;
}
// canonical offsets (floats, state_dict order): (W_l [F][F] b_l [F]) x (L-2) | Wo [cout][F] bo [cout] | per filter: [mu [F][cin]
// gamma [F]] Wf [F][cin] bf [F]
BL_HD int64_t mfn_canon_hidden(const brief_mfn_desc &d, int l /*1..L-1*/) { const int64_t F = d.features; return (int64_t)(l - 1) * (F * F + F); }
BL_HD int64_t mfn_canon_head(const brief_mfn_desc &d) { return mfn_canon_hidden(d, d.layers - 1); }
BL_HD int64_t mfn_canon_filter(const brief_mfn_desc &d, int i /*0..L-1*/)
{
    const int64_t F = d.features;
    return mfn_canon_head(d) + (int64_t)d.cout * F + d.cout + (int64_t)i * (d.filter ? 2 : 1) * (d.cin * F + F);
}
BL_HD int64_t mfn_canon_filter_w(const brief_mfn_desc &d, int i) { return mfn_canon_filter(d, i) + (d.filter ? (int64_t)d.cin * d.features + d.features : 0); }
BL_HD int64_t mfn_canon_count(const brief_mfn_desc &d) { return mfn_canon_filter(d, d.layers - 1); }

struct MfnArgs {
    brief_mfn_desc d;
    int nt;
    const float *pk;
    const float *coords, *targets, *weights;
    const int64_t *idx;
    int64_t offset, n;
    uint64_t rng_pop, rng_seed, rng_step;
    GridArgs grid;
    BoxArgs box;
    int loss_kind;
    float thr, beta, inv_count;
    float *Z, *U, *DU, *DA, *Q, *XP, *G;   // train stash (see above)
    float *lpart;                          // [gridDim.x] loss partial per workgroup
    int64_t npad;
    float *yhat_out;
    void *out;
    int out_kind;
    float scale_min, den, span, vmin;
};

// ---- the tile helpers (mfn_box_coords .. mfn_frag): the one text of brief_tile.inc, compiled here under the mfn_ prefix; functions of
// this family's own, because one set of functions called by every family changes the code of existing kernels (88 of 330: the note in
// brief_nerf.inc).  Nothing stayed a copy.
#define TILE_(name) mfn_##name
#include "brief_tile.inc"

// filter of feature f at x = (x_0, x_1, x_2, |x|^2): sin(a), cos(a) and the envelope e (1 for Fourier); fb: the filter's packed block
template <bool GABOR>
__device__ __forceinline__ void mfn_filter(const float *__restrict__ fb, int FP, int f, const float4 x, float &sv, float &cv, float &ev)
{
    const float4 w = *reinterpret_cast<const float4 *>(fb + 4 * f);
    float a = x.x * w.x;
    a = fmaf(x.y, w.y, a);
    a = fmaf(x.z, w.z, a);
    a = a + w.w;
    brief_sincosf(a, &sv, &cv);
    ev = 1.f;
    if (GABOR) {
        const float4 m = *reinterpret_cast<const float4 *>(fb + 4 * (int64_t)FP + 4 * f);
        const float msq = fb[8 * (int64_t)FP + f];
        float xm = x.x * m.x;
        xm = fmaf(x.y, m.y, xm);
        xm = fmaf(x.z, m.z, xm);
        const float D = (x.w + msq) - 2.f * xm;
        ev = expf((-0.5f * D) * m.w);
    }
}

// One 32-sample tile per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles wv, wv + 4, ...
// TRAIN: forward, loss, dgrad chain and the stash for k_mfn_wgrad.  Inference: forward and the out_kind epilogue (BOX: box voxels).
template <int MTW, bool TRAIN, bool BOX, bool GABOR>
__global__ __launch_bounds__(256) void k_mfn_fwd(const MfnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nt = a.nt, FP = 32 * nt;
    float4 *Xh = reinterpret_cast<float4 *>(smem);                     // hidden image: FP rows
    float *xsh = smem + 32 * FP;                                       // [32][4] (x_0, x_1, x_2, |x|^2) of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers, F = a.d.features;
    const int kf = (F + 7) / 8;                                        // K steps that hold real features
    const MfnLayout lay = mfn_layout(a.d);
    const int64_t ntiles = (a.n + 31) / 32;
    float lsum = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t col0 = tile * 32;
        // ---- sample selection (wave 0, lanes 0..31 keep their sample's target for the loss)
        const int64_t n = col0 + s;
        const bool valid = n < a.n;
        float yv[4] = {0.f, 0.f, 0.f, 0.f}, wv4[4] = {1.f, 1.f, 1.f, 1.f};
        if (tid < 32) {
            float x0 = 0.f, x1 = 0.f, x2 = 0.f;
            if (valid) {
                int64_t j = a.idx ? a.idx[n] : (a.rng_pop ? philox_index(n, a.rng_pop, a.rng_seed, a.rng_step) : n + a.offset);
                if (TRAIN) {
                    for (int c = 0; c < cout; ++c) {
                        yv[c] = a.targets[j * cout + c];
                        if (a.weights) wv4[c] = a.weights[j * cout + c];
                    }
                }
                if (a.coords) {
                    x0 = a.coords[j * cin];
                    x1 = a.coords[j * cin + 1];
                    if (cin == 3) x2 = a.coords[j * cin + 2];
                } else if (BOX) {
                    mfn_box_coords(a.grid, a.box, cin, j, x0, x1, x2);
                } else {
                    grid_coords(a.grid, cin, j, x0, x1, x2);
                }
            }
            const float xsq = (x0 * x0 + x1 * x1) + x2 * x2;      // (x ** 2).sum(-1)
            *reinterpret_cast<float4 *>(xsh + 4 * s) = make_float4(x0, x1, x2, xsq);
            if (TRAIN) {
                float *xp = a.XP + col0 + s;
                xp[0] = x0;
                xp[a.npad] = x1;
                if (cin == 3) xp[2 * a.npad] = x2;
                xp[(int64_t)cin * a.npad] = xsq;
                xp[(int64_t)(cin + 1) * a.npad] = valid ? 1.f : 0.f;
            }
        }
        __syncthreads();
        const float4 xs = *reinterpret_cast<const float4 *>(xsh + 4 * s);
        // ---- z_0 = g_0 (built in registers in the accumulator layout), then u_l = W_l z_{l-1} + b_l, z_l = g_l . u_l
        f32x16 acc[MTW];
        for (int l = 0; l <= L - 2; ++l) {
            const float *fb = a.pk + lay.filt + (int64_t)l * lay.filt_stride;
            if (l == 0) {
#pragma unroll
                for (int t = 0; t < MTW; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = 1.f;
            } else {
                const float *Wf = a.pk + lay.hid + (int64_t)(l - 1) * lay.hid_stride;
                mfn_bias(acc, Wf + 2 * (int64_t)FP * FP, nt, wv, hi);
                mfn_chain(acc, Wf, FP / 8, kf, nt, Xh, wv, lane);
                if (TRAIN) mfn_stash(a.U + (int64_t)(l - 1) * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            }
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                const int mt = wv + 4 * t;
                if (mt < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float sv, cv, ev;
                        mfn_filter<GABOR>(fb, FP, 32 * mt + ROWMAP(r, hi), xs, sv, cv, ev);
                        acc[t][r] = (sv * ev) * acc[t][r];
                    }
                }
            }
            if (TRAIN) mfn_stash(a.Z + (int64_t)l * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            __syncthreads();
            mfn_write_image(Xh, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        mfn_bias(hacc, a.pk + lay.bh, 1, wv, hi);
        if (wv == 0) {
            mfn_chain(hacc, a.pk + lay.whf, FP / 8, kf, 1, Xh, wv, lane);
        }
        float yh[4], yc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            yh[c] = hacc[0][c];
            yc[c] = 1.f;
            if (a.d.output_act) brief_sincosf(hacc[0][c], &yh[c], &yc[c]);     // out = sin(out): plain torch.sin, no w0
        }
        if (!TRAIN) {
            if (tid < 32 && valid) {
                for (int c = 0; c < cout; ++c) {
                    if (a.out_kind == BRIEF_OUT_F32) {
                        reinterpret_cast<float *>(a.out)[n * cout + c] = yh[c];
                    } else {
                        // utils/io.py:136-147: separate roundings, truncating cast (the SIREN kernels' epilogue)
                        float t = __fsub_rn(yh[c], a.scale_min);
                        t = __fdiv_rn(t, a.den);
                        t = fminf(fmaxf(t, 0.f), 1.f);
                        const float u = __fadd_rn(__fmul_rn(t, a.span), a.vmin);
                        if (a.out_kind == BRIEF_OUT_U16) reinterpret_cast<uint16_t *>(a.out)[n * cout + c] = (uint16_t)(int)u;
                        else reinterpret_cast<uint8_t *>(a.out)[n * cout + c] = (uint8_t)(int)u;
                    }
                }
            }
            __syncthreads();      // the image is re-used by the next tile
            continue;
        }
        // ---- loss and dL/dyhat (main.py:176-191), the SIREN kernels' arithmetic; then through sin' when output_act is set
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (tid < 32 && valid) {
            for (int c = 0; c < cout; ++c) {
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
                lsum += li * we;
                g[c] = a.loss_kind == BRIEF_LOSS_EXTERNAL ? yv[c] : gi * we * a.inv_count;
                if (a.d.output_act) g[c] = g[c] * yc[c];
                if (a.yhat_out) a.yhat_out[n * cout + c] = yh[c];
            }
        }
        if (tid < 32) {
#pragma unroll
            for (int c = 0; c < 4; ++c) a.G[(int64_t)c * a.npad + col0 + s] = g[c];
        }
        __syncthreads();      // every wave is past its reads of the last hidden image
        if (tid < 64) Xh[lane] = hi == 0 ? make_float4(g[0], g[1], g[2], g[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        // ---- dgrad chain, l = L-2 .. 0: dZ_l = W_{l+1}^T dU_{l+1} (Wo^T dOut for l = L-2); dU_l = dZ_l . g_l, dG_l = dZ_l . u_l
        // (dG_0 = dZ_0), dA_l = dG_l . cos(a_l) . e_l, Q_l = dG_l . sin(a_l) . e_l
        for (int l = L - 2; l >= 0; --l) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            if (l == L - 2) mfn_chain(acc, a.pk + lay.whb, 4, 1, nt, Xh, wv, lane);
            else mfn_chain(acc, a.pk + lay.hid + (int64_t)l * lay.hid_stride + (int64_t)FP * FP, FP / 8, kf, nt, Xh, wv, lane);
            const float *fb = a.pk + lay.filt + (int64_t)l * lay.filt_stride;
            const float *Ul = l > 0 ? a.U + (int64_t)(l - 1) * FP * a.npad : nullptr;
            float *DAl = a.DA + (int64_t)l * FP * a.npad;
            float *Ql = GABOR ? a.Q + (int64_t)l * FP * a.npad : nullptr;
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                const int mt = wv + 4 * t;
                if (mt < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int f = 32 * mt + ROWMAP(r, hi);
                        const int64_t e = (int64_t)f * a.npad + col0 + s;
                        float sv, cv, ev;
                        mfn_filter<GABOR>(fb, FP, f, xs, sv, cv, ev);
                        const float dz = acc[t][r];
                        float dg = dz;
                        if (l > 0) {
                            dg = dz * Ul[e];
                            acc[t][r] = dz * (sv * ev);
                        }
                        DAl[e] = (dg * cv) * ev;
                        if (GABOR) Ql[e] = (dg * sv) * ev;
                    }
                }
            }
            if (l > 0) {
                mfn_stash(a.DU + (int64_t)(l - 1) * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
                __syncthreads();
                mfn_write_image(Xh, acc, nt, wv, lane);
                __syncthreads();
            }
        }
        __syncthreads();      // the image is re-used by the next tile
    }
    if (TRAIN) {
        // per-workgroup loss partial: the 32 sample lanes of wave 0, fixed shuffle tree
        if (tid < 64) {
            float v = tid < 32 ? lsum : 0.f;
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            if (tid == 0) a.lpart[blockIdx.x] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// weight gradients: dW = sum_s A[row][s] B[col][s] over the planes of one weight block, split-K over sample chunks (blockIdx.y), each
// wave one 64 x 64 block (2 x 2 accumulator tiles; the second column tile is skipped when B has at most 32 rows), partial sums into
// slabs[split][canonical index]; the bias gradient (row sums of A) by the waves of the first column block of the blocks that carry it.
// Blocks: hidden layer l (A = DU_l, B = Z_{l-1}), head (A = G, B = Z_{L-2}), filter i (A = DA_i, B = XP rows 0 .. cin-1, bias) and,
// Gabor only, filter i's mu / gamma (A = Q_i, B = XP rows 0 .. cin+1 = (x, |x|^2, 1)): with S_c = sum q x_c, S_r = sum q |x|^2,
// S_q = sum q the epilogue forms dmu = -gamma (mu S_q - S_x) and dgamma = -(|mu|^2 S_q + S_r - 2 mu.S_x) / 2 (linear in the sums,
// so each split's slab holds its own share and the reduction adds them).
struct MfnWgradBlock {
    const float *A, *B;     // [rows][npad] planes
    int arows, brows;       // rows that hold data (A: F or cout; B: F, cin or cin + 2)
    int mb, nb;             // 64-row / 64-column blocks
    int wave_begin;         // first wave job of this block
    int64_t w_off, b_off;   // canonical offsets of dW (column 0 of this block) and db (b_off < 0: no bias)
    int ldw;                // row length of dW in the canonical buffer
    int gabor;              // mu / gamma block: w_off = mu, b_off unused, fg: the filter's FG block in the packed copy
    const float *fg;
};
#define MFN_WGRAD_BLOCKS 32       // blocks per k_mfn_wgrad launch (deeper nets take several launches)
struct MfnWgradArgs {
    MfnWgradBlock blk[MFN_WGRAD_BLOCKS];
    int nblocks, waves, cin, FP;
    int64_t npad, chunk, mlp;
    float *slabs;
};

__global__ __launch_bounds__(256) void k_mfn_wgrad(const MfnWgradArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, i = lane & 31;
    const int w = blockIdx.x * 4 + (tid >> 6);
    if (w >= a.waves) return;
    int l = 0;
    while (l + 1 < a.nblocks && a.blk[l + 1].wave_begin <= w) ++l;
    const MfnWgradBlock &L = a.blk[l];
    const int wl = w - L.wave_begin, mb = wl / L.nb, nb = wl % L.nb;
    const bool bias = L.b_off >= 0 && nb == 0 && !L.gabor;
    const bool y1 = 64 * nb + 32 < L.brows;      // the second column tile holds data
    const int64_t k0 = (int64_t)blockIdx.y * a.chunk;
    int64_t k1 = k0 + a.chunk;
    if (k1 > a.npad) k1 = a.npad;
    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
    float bsum[2] = {0.f, 0.f};
    const int ra[2] = {64 * mb + i, 64 * mb + 32 + i}, rb[2] = {64 * nb + i, 64 * nb + 32 + i};
    const bool va[2] = {ra[0] < L.arows, ra[1] < L.arows}, vb[2] = {rb[0] < L.brows, rb[1] < L.brows};
    const float *pa[2] = {L.A + (int64_t)(va[0] ? ra[0] : 0) * a.npad, L.A + (int64_t)(va[1] ? ra[1] : 0) * a.npad};
    const float *pb[2] = {L.B + (int64_t)(vb[0] ? rb[0] : 0) * a.npad, L.B + (int64_t)(vb[1] ? rb[1] : 0) * a.npad};
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // operands of step k + 8 are loaded while step k's MFMAs run
    float4 an[2], bn[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        an[x] = va[x] && k0 < k1 ? *reinterpret_cast<const float4 *>(pa[x] + k0 + 4 * hi) : z4;
        bn[x] = vb[x] && k0 < k1 ? *reinterpret_cast<const float4 *>(pb[x] + k0 + 4 * hi) : z4;
    }
    for (int64_t k = k0; k < k1; k += 8) {
        float4 av[2], bv[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) { av[x] = an[x]; bv[x] = bn[x]; }
        if (k + 8 < k1) {
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                an[x] = va[x] ? *reinterpret_cast<const float4 *>(pa[x] + k + 8 + 4 * hi) : z4;
                bn[x] = vb[x] ? *reinterpret_cast<const float4 *>(pb[x] + k + 8 + 4 * hi) : z4;
            }
        }
        if (bias) {
#pragma unroll
            for (int x = 0; x < 2; ++x) bsum[x] += (av[x].x + av[x].y) + (av[x].z + av[x].w);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            acc[x][0] = MFMA(av[x].x, bv[0].x, acc[x][0]);
            acc[x][0] = MFMA(av[x].y, bv[0].y, acc[x][0]);
            acc[x][0] = MFMA(av[x].z, bv[0].z, acc[x][0]);
            acc[x][0] = MFMA(av[x].w, bv[0].w, acc[x][0]);
            if (y1) {
                acc[x][1] = MFMA(av[x].x, bv[1].x, acc[x][1]);
                acc[x][1] = MFMA(av[x].y, bv[1].y, acc[x][1]);
                acc[x][1] = MFMA(av[x].z, bv[1].z, acc[x][1]);
                acc[x][1] = MFMA(av[x].w, bv[1].w, acc[x][1]);
            }
        }
    }
    float *slab = a.slabs + (int64_t)blockIdx.y * a.mlp;
    if (L.gabor) {
        // columns 0 .. cin-1: S_x, cin: S_r, cin + 1: S_q of row (64 mb + 32 x + ROWMAP(r, hi)), held by lanes 32 hi + col
        const int cin = a.cin;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[x][0][r];
                const int base = 32 * hi;
                const float s0 = __shfl(v, base), s1 = __shfl(v, base + 1), s2 = __shfl(v, base + 2);
                const float sr = __shfl(v, base + cin), sq = __shfl(v, base + cin + 1);
                const int row = 64 * mb + 32 * x + ROWMAP(r, hi);
                if (row < L.arows && i <= cin) {
                    const float4 m = *reinterpret_cast<const float4 *>(L.fg + 4 * row);
                    if (i < cin) {
                        const float mc = i == 0 ? m.x : (i == 1 ? m.y : m.z);
                        slab[L.w_off + (int64_t)row * cin + i] = -m.w * (mc * sq - v);
                    } else {
                        const float msq = L.fg[4 * (int64_t)a.FP + row];
                        float md = m.x * s0;
                        md = fmaf(m.y, s1, md);
                        if (cin == 3) md = fmaf(m.z, s2, md);
                        slab[L.w_off + (int64_t)L.arows * cin + row] = -0.5f * ((msq * sq + sr) - 2.f * md);
                    }
                }
            }
        return;
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int col = 64 * nb + 32 * y + i;
            if (col >= L.brows) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 64 * mb + 32 * x + ROWMAP(r, hi);
                if (row < L.arows) slab[L.w_off + (int64_t)row * L.ldw + col] = acc[x][y][r];
            }
        }
    if (bias) {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float v = bsum[x] + __shfl_xor(bsum[x], 32);
            if (hi == 0 && va[x]) slab[L.b_off + ra[x]] = v;
        }
    }
}

// canonical -> packed (see the layout at the top of this file)
__global__ void k_mfn_repack(const brief_mfn_desc d, const float *__restrict__ params, float *__restrict__ pk)
{
    const MfnLayout lay = mfn_layout(d);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= lay.total) return;
    const int F = d.features, cin = d.cin, cout = d.cout, FP = lay.FP;
    float v = 0.f;
    int row, k;
    if (e < lay.whf) {
        const int l = 1 + (int)((e - lay.hid) / lay.hid_stride);
        const int64_t r = (e - lay.hid) % lay.hid_stride;
        const float *W = params + mfn_canon_hidden(d, l);
        if (r < 2 * (int64_t)FP * FP) {
            const bool bwd = r >= (int64_t)FP * FP;
            mfn_frag(bwd ? r - (int64_t)FP * FP : r, FP / 8, row, k);
            if (row < F && k < F) v = bwd ? W[(int64_t)k * F + row] : W[(int64_t)row * F + k];
        } else {
            const int f = (int)(r - 2 * (int64_t)FP * FP);
            if (f < F) v = W[(int64_t)F * F + f];
        }
    } else if (e < lay.whb) {
        mfn_frag(e - lay.whf, FP / 8, row, k);
        if (row < cout && k < F) v = params[mfn_canon_head(d) + (int64_t)row * F + k];
    } else if (e < lay.bh) {
        mfn_frag(e - lay.whb, 4, row, k);
        if (row < F && k < cout) v = params[mfn_canon_head(d) + (int64_t)k * F + row];
    } else if (e < lay.filt) {
        const int c = (int)(e - lay.bh);
        if (c < cout) v = params[mfn_canon_head(d) + (int64_t)cout * F + c];
    } else {
        const int fi = (int)((e - lay.filt) / lay.filt_stride);
        const int64_t r = (e - lay.filt) % lay.filt_stride;
        const float *W = params + mfn_canon_filter_w(d, fi), *mu = params + mfn_canon_filter(d, fi);
        if (r < 8 * (int64_t)FP) {
            const int f = (int)((r >> 2) % FP), j = (int)(r & 3);
            const bool fg = r >= 4 * (int64_t)FP;          // (mu_0, mu_1, mu_2, gamma) instead of (w_0, w_1, w_2, b)
            if (f < F) {
                if (j < cin) v = fg ? mu[(int64_t)f * cin + j] : W[(int64_t)f * cin + j];
                else if (j == 3) v = fg ? mu[(int64_t)F * cin + f] : W[(int64_t)F * cin + f];
            }
        } else {
            const int f = (int)(r - 8 * (int64_t)FP);
            if (f < F) {
                // (mu ** 2).sum(-1)
                const float *m = mu + (int64_t)f * cin;
                float q = m[0] * m[0] + m[1] * m[1];
                if (cin == 3) q = q + m[2] * m[2];
                v = q;
            }
        }
    }
    pk[e] = v;
}
