// brief_taper.inc — tapered SIRENs (SIREN_Pyramid, SIRENFT, SIRENPS): k_taper_fwd<MTW, TRAIN, BOX>, k_taper_wgrad, k_taper_repack (part of
// the single translation unit brief_hip.hip, included after brief_mfn.inc; the reduction is brief_ffn.inc's k_ffn_reduce with bv = 0).
// Only new kernels: no SIREN, FFN, NeRF or MFN kernel, device function or argument struct is changed by this file.
//
// Net (reference utils/Networks.py:316-552): a SIREN whose every Linear has its own width and every sine its own w0:
//   h_0 = sin(w0_0 (W_0 x + b_0)),  h_l = sin(w0_l (W_l h_{l-1} + b_l))  (l = 1 .. L-2),  y = Wh h_{L-2} + bh  [sin(w0_{L-1} y) with
//   output_act].  W_l is [out_l][in_l], in_l = out_{l-1}.
// Phase rule (k_fused's): the forward weights and biases of layer l carry s_l = w0_l / 2 pi, so the accumulator IS the phase in
// revolutions; its fraction (v_fract) goes to v_sin / v_cos.  The backward copies W_l^T carry w0_{l-1}, so the dgrad chain's
// accumulator times cos(phase_{l-1}) is dL/du_{l-1} (u: the Linear's output before w0).
//
// Every layer is padded on its own: OP_l = 32 ceil(out_l / 32) output rows, K steps of 8 rows: ks_l = ceil(in_l / 8) forward,
// kb_l = ceil(out_l / 8) backward.  Padded rows / columns and biases are zero: a padded unit has phase 0, emits sin(0) = 0 and receives
// a zero gradient.  The tile helpers are the one text of brief_tile.inc compiled under the taper_ prefix (not functions shared with
// the other families: that changes the code of 88 of the 330 kernels, see the note in brief_nerf.inc); the chain is that file's
// TILE_CHAIN_PACKED form, a layer's fragment rows being exactly ksteps steps long.  Nothing stayed a copy.
//
// LDS per workgroup: the image [max_l OP_l rows][32 samples] plus 32 x float4 of coordinates (1024 rows: 131 584 bytes).
//
// Packed layout (floats; fragment block (mt, step) = 64 lanes x float4, A[32 mt + i][8 step + 4 hi + j]):
//   layer 0:            W0p [OP_0][4] = s_0 (w_0, w_1, w_2 | 0, b)      (layer 0 runs on the VALU)
//   layer l = 1 .. L-2: Wf [nt_l][ks_l][64][4] (s_l W_l),  Wb [nt_{l-1}][kb_l][64][4] (w0_{l-1} W_l^T),  b [OP_l] (s_l b_l)
//   head (l = L-1):     Wf [1][ks][64][4] (rows >= cout zero),  Wb [nt_{L-2}][1][64][4] (w0_{L-2} Wh^T),  bh [32]
// Train stash (workspace, feature-major planes of each layer's own height): Z_l [OP_l][npad] (fraction of the phase, revolutions),
// D_l [OP_l][npad] (dL/du_l), X [4][npad] (coordinates), G [4][npad] (dL/dy).

struct TaperLayout {
    int L, ntmax, rows;                         // rows: sum of OP_l over the sine layers (height of the Z / D stash)
    int out[BRIEF_TAPER_MAX_LAYERS], in[BRIEF_TAPER_MAX_LAYERS], nt[BRIEF_TAPER_MAX_LAYERS];
    int ks[BRIEF_TAPER_MAX_LAYERS], kb[BRIEF_TAPER_MAX_LAYERS], row0[BRIEF_TAPER_MAX_LAYERS];
    int64_t wf[BRIEF_TAPER_MAX_LAYERS], wb[BRIEF_TAPER_MAX_LAYERS], bias[BRIEF_TAPER_MAX_LAYERS], canon[BRIEF_TAPER_MAX_LAYERS];
    int64_t total, count;                       // floats of the packed / the canonical buffer
};
BL_HD TaperLayout taper_layout(const brief_taper_desc &d)
{
    TaperLayout o;
    const int L = d.layers;
    o.L = L; o.ntmax = 1; o.rows = 0;
    int64_t pk = 0, cn = 0;
    for (int l = 0; l < BRIEF_TAPER_MAX_LAYERS; ++l) {
        o.out[l] = o.in[l] = o.nt[l] = o.ks[l] = o.kb[l] = o.row0[l] = 0;
        o.wf[l] = o.wb[l] = o.bias[l] = o.canon[l] = 0;
    }
    for (int l = 0; l < L; ++l) {
        o.out[l] = l == L - 1 ? d.cout : d.widths[l];
        o.in[l] = l == 0 ? d.cin : o.out[l - 1];
        o.nt[l] = (o.out[l] + 31) / 32;
        o.ks[l] = (o.in[l] + 7) / 8;
        o.kb[l] = (o.out[l] + 7) / 8;
        o.canon[l] = cn;
        cn += (int64_t)o.out[l] * o.in[l] + o.out[l];
        if (l < L - 1) {
            o.row0[l] = o.rows;
            o.rows += 32 * o.nt[l];
            if (o.nt[l] > o.ntmax) o.ntmax = o.nt[l];
        }
        o.wf[l] = pk;
        if (l == 0) {
            pk += 4 * 32 * (int64_t)o.nt[0];
            o.wb[0] = o.bias[0] = pk;
        } else {
            pk += (int64_t)o.nt[l] * o.ks[l] * 256;
            o.wb[l] = pk;
            pk += (int64_t)o.nt[l - 1] * o.kb[l] * 256;
            o.bias[l] = pk;
            pk += 32 * (int64_t)o.nt[l];
        }
    }
    o.total = pk; o.count = cn;
    return o;
}

struct TaperArgs {
    brief_taper_desc d;
    TaperLayout lay;
    const float *pk;
    const float *coords, *targets, *weights;
    const int64_t *idx;
    int64_t offset, n;
    uint64_t rng_pop, rng_seed, rng_step;
    GridArgs grid;
    BoxArgs box;
    int loss_kind;
    float thr, beta, inv_count;
    float *Z, *D, *X, *G;     // train stash (see above)
    float *lpart;             // [gridDim.x] loss partial per workgroup
    int64_t npad;
    float *yhat_out;
    void *out;
    int out_kind;
    float scale_min, den, span, vmin;
};

#define TILE_CHAIN_PACKED
#define TILE_(name) taper_##name
#include "brief_tile.inc"

// One 32-sample tile per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles wv, wv + 4, ... of
// every layer (fewer of them in a narrower layer).  TRAIN: forward, loss, dgrad chain and the stash for k_taper_wgrad.  Inference:
// forward and the out_kind epilogue (BOX: box voxels).
template <int MTW, bool TRAIN, bool BOX>
__global__ __launch_bounds__(256) void k_taper_fwd(const TaperArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *Xh = reinterpret_cast<float4 *>(smem);                     // image: 32 ntmax rows
    float *xsh = smem + 1024 * a.lay.ntmax;                            // [32][4] coordinates of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers;
    const int64_t ntiles = (a.n + 31) / 32;
    const float w0h = a.d.w0[L - 1];
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
#pragma unroll
                    for (int c = 0; c < 4; ++c) {      // (static indices: the per-channel arrays stay in registers)
                        if (c < cout) {
                            yv[c] = a.targets[j * cout + c];
                            if (a.weights) wv4[c] = a.weights[j * cout + c];
                        }
                    }
                }
                if (a.coords) {
                    x0 = a.coords[j * cin];
                    x1 = a.coords[j * cin + 1];
                    if (cin == 3) x2 = a.coords[j * cin + 2];
                } else if (BOX) {
                    taper_box_coords(a.grid, a.box, cin, j, x0, x1, x2);
                } else {
                    grid_coords(a.grid, cin, j, x0, x1, x2);
                }
            }
            *reinterpret_cast<float4 *>(xsh + 4 * s) = make_float4(x0, x1, x2, 0.f);
            if (TRAIN) {
                a.X[col0 + s] = x0; a.X[a.npad + col0 + s] = x1; a.X[2 * a.npad + col0 + s] = x2; a.X[3 * a.npad + col0 + s] = 0.f;
            }
        }
        __syncthreads();
        const float4 x = *reinterpret_cast<const float4 *>(xsh + 4 * s);
        // ---- sine layers 0 .. L-2: layer 0 on the VALU (K = cin), the others as MFMA chains over their own tiles and K steps
        f32x16 acc[MTW];
        for (int l = 0; l <= L - 2; ++l) {
            const int nt = a.lay.nt[l];
            if (l == 0) {
                const float4 *W0p = reinterpret_cast<const float4 *>(a.pk + a.lay.wf[0]);
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    const int mt = wv + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = 0.f;
                        if (mt < nt) {
                            const float4 w = W0p[32 * mt + ROWMAP(r, hi)];
                            v = __fmaf_rn(w.x, x.x, __fmaf_rn(w.y, x.y, __fmaf_rn(w.z, x.z, w.w)));
                        }
                        acc[t][r] = v;
                    }
                }
            } else {
                taper_bias(acc, a.pk + a.lay.bias[l], nt, wv, hi);
                taper_chain(acc, a.pk + a.lay.wf[l], a.lay.ks[l], nt, Xh, wv, lane);
            }
            // the accumulator is the phase in revolutions; its fraction is what sin and cos are taken of (here, in the dgrad chain and
            // in k_taper_wgrad)
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = __builtin_amdgcn_fractf(acc[t][r]);
            if (TRAIN) taper_stash(a.Z + (int64_t)a.lay.row0[l] * a.npad, a.npad, col0, acc, nt, wv, hi, s);
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = BRIEF_SIN_REV(acc[t][r]);
            __syncthreads();
            taper_write_image(Xh, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        taper_bias(hacc, a.pk + a.lay.bias[L - 1], 1, wv, hi);
        if (wv == 0) taper_chain(hacc, a.pk + a.lay.wf[L - 1], a.lay.ks[L - 1], 1, Xh, wv, lane);
        float yh[4], zo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            zo[c] = hacc[0][c];
            yh[c] = a.d.output_act ? brief_fast_sinf(w0h * zo[c]) : zo[c];
        }
        if (!TRAIN) {
            if (tid < 32 && valid) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= cout) break;
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
        // ---- loss and dL/dy (main.py:176-191), the SIREN kernels' arithmetic
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (tid < 32 && valid) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= cout) break;
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
                if (a.d.output_act) g[c] *= w0h * brief_fast_cosf(w0h * zo[c]);
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
        // ---- dgrad chain: dL/du_l = (w0_l W_{l+1}^T dL/du_{l+1}) . cos(phase_l), l = L-2 .. 0 (the head's K is one step)
        for (int l = L - 2; l >= 0; --l) {
            const int nt = a.lay.nt[l];
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            taper_chain(acc, a.pk + a.lay.wb[l + 1], a.lay.kb[l + 1], nt, Xh, wv, lane);
            const float *Zl = a.Z + (int64_t)a.lay.row0[l] * a.npad;
#pragma unroll
            for (int t = 0; t < MTW; ++t) {
                const int mt = wv + 4 * t;
                if (mt < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[t][r] *= BRIEF_COS_REV(Zl[(int64_t)(32 * mt + ROWMAP(r, hi)) * a.npad + col0 + s]);
                }
            }
            taper_stash(a.D + (int64_t)a.lay.row0[l] * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            if (l > 0) {
                __syncthreads();
                taper_write_image(Xh, acc, nt, wv, lane);
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
// weight gradients: dW_l = sum_s A[row][s] B[col][s] over the planes of one rectangular [out_l x in_l] block, split-K over sample
// chunks (blockIdx.y), each wave one 64 x 64 block (2 x 2 accumulator tiles), partial sums into slabs[split][canonical index]; the bias
// gradient (row sums of A) by the waves of the first column block.  A = D_l (G for the head); B = the coordinates (layer 0) or the
// stashed phase of layer l-1, whose sine is taken as the operand is loaded (bsin).
struct TaperWgradBlock {
    const float *A, *B;     // [rows][npad] planes
    int arows, brows;       // rows that hold data
    int mb, nb;             // 64-row / 64-column blocks
    int wave_begin;         // first wave job of this block
    int bsin;               // B holds phases in revolutions: the operand is sin(2 pi B)
    int64_t w_off, b_off;   // canonical offsets of dW and db
    int ldw;                // row length of dW in the canonical buffer
};
struct TaperWgradArgs {
    TaperWgradBlock blk[BRIEF_TAPER_MAX_LAYERS];
    int nblocks, waves;
    int64_t npad, chunk, mlp;
    float *slabs;
};

__device__ __forceinline__ float4 taper_sin4(float4 v)
{
    return make_float4(BRIEF_SIN_REV(v.x), BRIEF_SIN_REV(v.y), BRIEF_SIN_REV(v.z), BRIEF_SIN_REV(v.w));
}

__global__ __launch_bounds__(256) void k_taper_wgrad(const TaperWgradArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, i = lane & 31;
    const int w = blockIdx.x * 4 + (tid >> 6);
    if (w >= a.waves) return;
    int l = 0;
    while (l + 1 < a.nblocks && a.blk[l + 1].wave_begin <= w) ++l;
    const TaperWgradBlock &L = a.blk[l];
    const int wl = w - L.wave_begin, mb = wl / L.nb, nb = wl % L.nb;
    const bool bias = nb == 0, bsin = L.bsin != 0;
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
        if (bsin) {
#pragma unroll
            for (int x = 0; x < 2; ++x) bv[x] = taper_sin4(bv[x]);       // rows past brows hold phase 0: sin 0 = 0
        }
        if (bias) {
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

// canonical (state_dict order: W_l [out_l][in_l] b_l [out_l] per layer) -> packed (see the layout at the top of this file)
__global__ void k_taper_repack(const brief_taper_desc d, const TaperLayout lay, const float *__restrict__ params, float *__restrict__ pk)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= lay.total) return;
    const int L = lay.L;
    int l = 0;
    while (l + 1 < L && lay.wf[l + 1] <= e) ++l;
    const int out = lay.out[l], in = lay.in[l];
    const float *W = params + lay.canon[l], *b = W + (int64_t)out * in;
    const float sf = l < L - 1 ? d.w0[l] * 0.15915494309189535f : 1.0f;      // w0_l / 2 pi (the head is not scaled)
    float v = 0.f;
    int row, k;
    if (l == 0) {
        const int64_t q = e - lay.wf[0];
        row = (int)(q >> 2); k = (int)(q & 3);
        if (row < out) {
            if (k < in) v = W[(int64_t)row * in + k] * sf;
            else if (k == 3) v = b[row] * sf;
        }
    } else if (e < lay.wb[l]) {
        taper_frag(e - lay.wf[l], lay.ks[l], row, k);
        if (row < out && k < in) v = W[(int64_t)row * in + k] * sf;
    } else if (e < lay.bias[l]) {
        taper_frag(e - lay.wb[l], lay.kb[l], row, k);
        if (row < in && k < out) v = W[(int64_t)k * in + row] * d.w0[l - 1];
    } else {
        const int f = (int)(e - lay.bias[l]);
        if (f < out) v = b[f] * sf;
    }
    pk[e] = v;
}
