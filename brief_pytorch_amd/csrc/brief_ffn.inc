// brief_ffn.inc — the FFN (Fourier-feature) network: k_ffn_fwd<MTW, TRAIN, BOX>, k_ffn_wgrad, k_ffn_reduce, k_ffn_repack (part of the single
// translation unit brief_hip.hip, which includes it in this order; it uses what the parts before it define).  Only new kernels: no SIREN
// kernel, device function or argument struct is changed by this file.
//
// Same transposed form as the SIREN kernels: Z^T[feature][sample] = W[feature][k] * H^T[k][sample] on v_mfma_f32_32x32x2_f32 (exact f32),
// the weights as A fragments streamed from the fragment-ordered copy (L2 resident), the activations as one LDS register image per
// 32-sample tile.  Image element (k, s) of a tile: float ((k >> 3) * 64 + 32 * ((k >> 2) & 1) + s) * 4 + (k & 3), the layout of an
// accumulator tile written back as the next MFMA's B operand.
//
// Packed layout (floats; FP = 32 nt features, EP = 32 ceil(E / 32), K0 = 2 EP, fragment block (mt, step) = 64 lanes x float4):
//   W0f  [nt][K0 / 8 steps][64][4]   A[32 mt + i][8 step + 4 hi + j] = W0[32 mt + i][col(k)], k < EP: col e = k, k >= EP: col E + (k - EP)
//   b0   [FP]
//   per hidden layer l = 1 .. L-2:  Wf [nt][FP / 8][64][4] (W_l), Wb [nt][FP / 8][64][4] (W_l^T), b [FP]
//   Whf  [1][FP / 8][64][4]  (rows >= cout zero),  Whb [nt][4][64][4]  (Wh^T, columns >= cout zero),  bh [32] (rows >= cout zero)
//   Bv   [EP][4]  bvals rows (cin entries, rest zero)
// Train stash (workspace, [rows][npad] feature-major planes, sample-contiguous): H_l (post-ReLU output of layer l, l = 0 .. L-2),
// D_l (delta of layer l's pre-activation), EMB [K0][npad] (the embedding the first layer saw), G [4][npad] (dL/dyhat).  The embedding
// is stashed, not recomputed, so the first layer's weight gradient sees exactly the values of the forward pass.

struct FfnLayout {
    int nt, FP, EP, K0;
    int64_t w0f, b0, hid, hid_stride, whf, whb, bh, bv, total;
};
BL_HD FfnLayout ffn_layout(const brief_ffn_desc &d)
{
    FfnLayout o;
    o.nt = (d.features + 31) / 32; o.FP = 32 * o.nt;
    o.EP = 32 * ((d.embsize + 31) / 32); o.K0 = 2 * o.EP;
    o.w0f = 0;
    o.b0 = (int64_t)o.FP * o.K0;
    o.hid = o.b0 + o.FP;
    o.hid_stride = 2 * (int64_t)o.FP * o.FP + o.FP;
    o.whf = o.hid + (int64_t)(d.layers - 2) * o.hid_stride;
    o.whb = o.whf + 32 * (int64_t)o.FP;
    o.bh = o.whb + 32 * (int64_t)o.FP;
    o.bv = o.bh + 32;
    o.total = o.bv + 4 * (int64_t)o.EP;
    return o;
}
// canonical offsets (floats): bvals | W0 b0 | hidden | head
BL_HD int64_t ffn_canon_w0(const brief_ffn_desc &d) { return (int64_t)d.embsize * d.cin; }
BL_HD int64_t ffn_canon_hidden(const brief_ffn_desc &d, int l /*1..L-2*/)
{
    const int64_t F = d.features;
    return ffn_canon_w0(d) + 2 * (int64_t)d.embsize * F + F + (int64_t)(l - 1) * (F * F + F);
}
BL_HD int64_t ffn_canon_head(const brief_ffn_desc &d) { return ffn_canon_hidden(d, d.layers - 1); }
BL_HD int64_t ffn_canon_count(const brief_ffn_desc &d) { return ffn_canon_head(d) + (int64_t)d.cout * d.features + d.cout; }

struct FfnArgs {
    brief_ffn_desc d;
    int nt, EP;
    const float *pk;
    const float *coords, *targets, *weights;
    const int64_t *idx;
    int64_t offset, n;
    uint64_t rng_pop, rng_seed, rng_step;
    GridArgs grid;
    BoxArgs box;
    int loss_kind;
    float thr, beta, inv_count;
    float *H, *D, *EMB, *G;   // train stash (see above)
    float *lpart;             // [gridDim.x] loss partial per workgroup
    int64_t npad;
    float *yhat_out;
    void *out;
    int out_kind;
    float scale_min, den, span, vmin;
};

// the tile helpers ffn_box_coords, ffn_chain, ffn_bias, ffn_write_image, ffn_stash and ffn_frag: the one text of brief_tile.inc, compiled
// here under the ffn_ prefix (every family includes it under its own; the note at its top says why they are not one set of functions)
#define TILE_(name) ffn_##name
#include "brief_tile.inc"

// the embedding of one (coordinate, frequency row) pair: t = sum_c x_c B[e][c] as an fma chain in c order, in revolutions
__device__ __forceinline__ void ffn_embed(float x0, float x1, float x2, float4 b, int cin, float &s, float &c)
{
    float t = x0 * b.x;
    t = __fmaf_rn(x1, b.y, t);
    if (cin == 3) t = __fmaf_rn(x2, b.z, t);
    const float f = __builtin_amdgcn_fractf(t);
    s = BRIEF_SIN_REV(f);
    c = BRIEF_COS_REV(f);
}

// One 32-sample tile per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles wv, wv + 4, ...
// TRAIN: forward, loss, dgrad chain and the stash for k_ffn_wgrad.  Inference: forward and the out_kind epilogue (BOX: box voxels).
template <int MTW, bool TRAIN, bool BOX>
__global__ __launch_bounds__(256) void k_ffn_fwd(const FfnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *Xs = reinterpret_cast<float4 *>(smem);                     // image: max(K0, FP) rows x 32 samples
    const int K0 = 2 * a.EP, nt = a.nt, FP = 32 * nt;
    float *xsh = smem + 32 * (K0 > FP ? K0 : FP);                      // [32][4] coordinates of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers, F = a.d.features, E = a.d.embsize;
    const int kf = (F + 7) / 8;                                        // K steps that hold real features
    const FfnLayout lay = ffn_layout(a.d);
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
                    ffn_box_coords(a.grid, a.box, cin, j, x0, x1, x2);
                } else {
                    grid_coords(a.grid, cin, j, x0, x1, x2);
                }
            }
            *reinterpret_cast<float4 *>(xsh + 4 * s) = make_float4(x0, x1, x2, 0.f);
        }
        __syncthreads();
        // ---- embedding image (and its stash): rows e (sin) and EP + e (cos); padding rows are zero
        for (int q = tid; q < a.EP * 32; q += 256) {
            const int e = q >> 5, sc = q & 31;
            float sv = 0.f, cv = 0.f;
            if (e < E) {
                const float4 x = *reinterpret_cast<const float4 *>(xsh + 4 * sc);
                ffn_embed(x.x, x.y, x.z, *reinterpret_cast<const float4 *>(a.pk + lay.bv + 4 * e), cin, sv, cv);
            }
            const int k1 = e, k2 = a.EP + e;
            smem[((k1 >> 3) * 64 + 32 * ((k1 >> 2) & 1) + sc) * 4 + (k1 & 3)] = sv;
            smem[((k2 >> 3) * 64 + 32 * ((k2 >> 2) & 1) + sc) * 4 + (k2 & 3)] = cv;
            if (TRAIN) {
                a.EMB[(int64_t)k1 * a.npad + col0 + sc] = sv;
                a.EMB[(int64_t)k2 * a.npad + col0 + sc] = cv;
            }
        }
        __syncthreads();
        // ---- first layer (K = K0) and the hidden layers, ReLU
        f32x16 acc[MTW];
        for (int l = 0; l <= L - 2; ++l) {
            const float *Wf = l == 0 ? a.pk + lay.w0f : a.pk + lay.hid + (int64_t)(l - 1) * lay.hid_stride;
            const float *bb = l == 0 ? a.pk + lay.b0 : Wf + 2 * (int64_t)FP * FP;
            ffn_bias(acc, bb, nt, wv, hi);
            if (l == 0) ffn_chain(acc, Wf, K0 / 8, K0 / 8, nt, Xs, wv, lane);
            else ffn_chain(acc, Wf, FP / 8, kf, nt, Xs, wv, lane);
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = fmaxf(acc[t][r], 0.f);
            if (TRAIN) ffn_stash(a.H + (int64_t)l * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            __syncthreads();
            ffn_write_image(Xs, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        ffn_bias(hacc, a.pk + lay.bh, 1, wv, hi);
        if (wv == 0) {
            ffn_chain(hacc, a.pk + lay.whf, FP / 8, kf, 1, Xs, wv, lane);
        }
        float yh[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) yh[c] = hacc[0][c];
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
        // ---- loss and dL/dyhat (main.py:176-191), the SIREN kernels' arithmetic
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
                if (a.yhat_out) a.yhat_out[n * cout + c] = yh[c];
            }
        }
        if (tid < 32) {
#pragma unroll
            for (int c = 0; c < 4; ++c) a.G[(int64_t)c * a.npad + col0 + s] = g[c];
        }
        __syncthreads();      // every wave is past its reads of the last hidden image
        if (tid < 64) Xs[lane] = hi == 0 ? make_float4(g[0], g[1], g[2], g[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        // ---- dgrad chain: delta_l = (W_{l+1}^T delta_{l+1}) . (h_l > 0), l = L-2 .. 0 (none into the embedding)
        for (int l = L - 2; l >= 0; --l) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            if (l == L - 2) ffn_chain(acc, a.pk + lay.whb, 4, 1, nt, Xs, wv, lane);
            else ffn_chain(acc, a.pk + lay.hid + (int64_t)l * lay.hid_stride + (int64_t)FP * FP, FP / 8, kf, nt, Xs, wv, lane);
            const float *Hl = a.H + (int64_t)l * FP * a.npad;
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                const int mt = wv + 4 * t;
                if (mt < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (!(Hl[(int64_t)(32 * mt + ROWMAP(r, hi)) * a.npad + col0 + s] > 0.f)) acc[t][r] = 0.f;
                }
            }
            ffn_stash(a.D + (int64_t)l * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            if (l > 0) {
                __syncthreads();
                ffn_write_image(Xs, acc, nt, wv, lane);
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
// weight gradients: dW = sum_s A[row][s] B[col][s] over the planes of one layer, split-K over sample chunks (blockIdx.y), each wave one
// 64 x 64 block (2 x 2 accumulator tiles), partial sums into slabs[split][MLP canonical index]; the bias gradient (row sums of A) by the
// waves of the first column block.
struct FfnWgradLayer {
    const float *A, *B;     // [rows][npad] planes
    int arows, brows;       // rows that hold data (A: F or cout; B: F or K0)
    int mb, nb;             // 64-row / 64-column blocks
    int wave_begin;         // first wave job of this layer
    int64_t w_off, b_off;   // canonical MLP offsets (relative to the MLP span) of dW and db
    int ldw;                // row length of dW in the canonical buffer
    int emb;                // B is the embedding plane: column k maps to canonical column k < EP ? k : E + (k - EP)
};
#define FFN_WGRAD_LAYERS 32      // layers per k_ffn_wgrad launch (deeper nets take several launches)
struct FfnWgradArgs {
    FfnWgradLayer lay[FFN_WGRAD_LAYERS];
    int nlayers, waves, EP, E;
    int64_t npad, chunk, mlp;
    float *slabs;
};

__global__ __launch_bounds__(256) void k_ffn_wgrad(const FfnWgradArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, i = lane & 31;
    const int w = blockIdx.x * 4 + (tid >> 6);
    if (w >= a.waves) return;
    int l = 0;
    while (l + 1 < a.nlayers && a.lay[l + 1].wave_begin <= w) ++l;
    const FfnWgradLayer &L = a.lay[l];
    const int wl = w - L.wave_begin, mb = wl / L.nb, nb = wl % L.nb;
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
        if (nb == 0) {
#pragma unroll
            for (int x = 0; x < 2; ++x) bsum[x] += (av[x].x + av[x].y) + (av[x].z + av[x].w);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                acc[x][y] = MFMA(av[x].x, bv[y].x, acc[x][y]);
                acc[x][y] = MFMA(av[x].y, bv[y].y, acc[x][y]);
                acc[x][y] = MFMA(av[x].z, bv[y].z, acc[x][y]);
                acc[x][y] = MFMA(av[x].w, bv[y].w, acc[x][y]);
            }
    }
    float *slab = a.slabs + (int64_t)blockIdx.y * a.mlp;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int col = 64 * nb + 32 * y + i;
            if (col >= L.brows) continue;
            int ccol = col;
            if (L.emb) {
                if (col < a.EP) { if (col >= a.E) continue; }
                else { if (col - a.EP >= a.E) continue; ccol = a.E + (col - a.EP); }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 64 * mb + 32 * x + ROWMAP(r, hi);
                if (row < L.arows) slab[L.w_off + (int64_t)row * L.ldw + ccol] = acc[x][y][r];
            }
        }
    if (nb == 0) {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float v = bsum[x] + __shfl_xor(bsum[x], 32);
            if (hi == 0 && va[x]) slab[L.b_off + ra[x]] = v;
        }
    }
}

// sum of the slabs in split order -> canonical gradients (bvals span zero), optional fused optimizer update on the MLP span; loss
// = sum of the workgroup partials in order * inv_count (thread 0)
__global__ __launch_bounds__(256) void k_ffn_reduce(const float *__restrict__ slabs, int nsplit, int64_t mlp, int64_t bv, float *__restrict__ grads,
                                                    const float *__restrict__ lpart, int nparts, float inv_count, float *__restrict__ loss_out,
                                                    int update, OptimScalars o, float *__restrict__ params, float *__restrict__ s1, float *__restrict__ s2)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) {
        float ls = 0.f;
        for (int w = 0; w < nparts; ++w) ls += lpart[w];
        *loss_out = ls * inv_count;
    }
    if (p < bv) grads[p] = 0.f;
    if (p >= mlp) return;
    float g = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) g += slabs[(int64_t)sp * mlp + p];
    grads[bv + p] = g;
    if (update) optim_apply(o, g, params, s1, s2, bv + p);
}

// canonical -> packed (see the layout at the top of this file)
__global__ void k_ffn_repack(const brief_ffn_desc d, const float *__restrict__ params, float *__restrict__ pk)
{
    const FfnLayout lay = ffn_layout(d);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= lay.total) return;
    const int F = d.features, E = d.embsize, cin = d.cin, cout = d.cout, FP = lay.FP;
    float v = 0.f;
    int row, k;
    if (e < lay.b0) {
        ffn_frag(e - lay.w0f, lay.K0 / 8, row, k);
        const int col = k < lay.EP ? (k < E ? k : -1) : (k - lay.EP < E ? E + (k - lay.EP) : -1);
        if (row < F && col >= 0) v = params[ffn_canon_w0(d) + (int64_t)row * 2 * E + col];
    } else if (e < lay.hid) {
        const int f = (int)(e - lay.b0);
        if (f < F) v = params[ffn_canon_w0(d) + (int64_t)F * 2 * E + f];
    } else if (e < lay.whf) {
        const int l = 1 + (int)((e - lay.hid) / lay.hid_stride);
        const int64_t r = (e - lay.hid) % lay.hid_stride;
        const float *W = params + ffn_canon_hidden(d, l);
        if (r < 2 * (int64_t)FP * FP) {
            const bool bwd = r >= (int64_t)FP * FP;
            ffn_frag(bwd ? r - (int64_t)FP * FP : r, FP / 8, row, k);
            if (row < F && k < F) v = bwd ? W[(int64_t)k * F + row] : W[(int64_t)row * F + k];
        } else {
            const int f = (int)(r - 2 * (int64_t)FP * FP);
            if (f < F) v = W[(int64_t)F * F + f];
        }
    } else if (e < lay.whb) {
        ffn_frag(e - lay.whf, FP / 8, row, k);
        if (row < cout && k < F) v = params[ffn_canon_head(d) + (int64_t)row * F + k];
    } else if (e < lay.bh) {
        ffn_frag(e - lay.whb, 4, row, k);
        if (row < F && k < cout) v = params[ffn_canon_head(d) + (int64_t)k * F + row];
    } else if (e < lay.bv) {
        const int c = (int)(e - lay.bh);
        if (c < cout) v = params[ffn_canon_head(d) + (int64_t)cout * F + c];
    } else {
        const int64_t r = e - lay.bv;
        const int er = (int)(r >> 2), c = (int)(r & 3);
        if (er < E && c < cin) v = params[(int64_t)er * cin + c];
    }
    pk[e] = v;
}
