// brief_nerf.inc — the NeRF positional-encoding network: k_nerf_fwd<MTW, TRAIN, BOX>, k_nerf_wgrad, k_nerf_repack (part of the single
// translation unit brief_hip.hip, included after brief_ffn.inc; the reduction is that file's k_ffn_reduce with bv = 0).  Only new
// kernels: no SIREN or FFN kernel, device function or argument struct is changed by this file.
//
// Net (reference utils/Networks.py:64-136): enc = [x_0 .. x_{cin-1}, sin(2^0 pi x_0), cos(2^0 pi x_0), sin(2^0 pi x_1), ..., cos(2^{Lf-1}
// pi x_{cin-1})] (d = cin (1 + 2 Lf) columns), Linear(d, F) + ReLU, (layers - 2) x (Linear(F, F) + ReLU), Linear(F, cout); with skip the
// hidden layer sl = (layers - 1) / 2 is Linear(d + F, F) on cat[enc, h].
// Phase rule: the reference evaluates torch.sin((2 ** i) * math.pi * c) in fp32, i.e. the sine of the exact float 2^i * fl32(fl32(pi) x).
// The kernel forms p = fl32(pi) * x as one rounded fp32 multiply (no contraction), scales it exactly by 2^i and evaluates the accurate
// full-range ocml sincosf on it (about 1 ulp).
//
// LDS per workgroup: the image [DP + FP rows][32 samples] plus 32 x float4 of coordinates, DP = d padded to the 8-row fragment step.  The
// encoding rows 0 .. DP-1 stay resident for the whole tile (the skip layer reads them again); the hidden activations live in rows DP ..
// DP+FP-1.  F = 1024, Lf = 10, cin = 3: (64 + 1024) * 128 + 512 = 139 776 bytes (one workgroup per CU); F = 507: 74 240 bytes (two).
//
// Packed layout (floats; FP = 32 nt, DP = 8 ceil(d / 8), fragment block (mt, step) = 64 lanes x float4, A[32 mt + i][8 step + 4 hi + j]):
//   W0f  [nt][DP / 8][64][4]   (W0, columns >= d zero)
//   b0   [FP]
//   per hidden layer l = 1 .. L-2:  Wf [nt][FP / 8][64][4] (the hidden columns of W_l), Wb [nt][FP / 8][64][4] (their transpose), b [FP]
//   Whf  [1][FP / 8][64][4]  (rows >= cout zero),  Whb [nt][4][64][4]  (Wh^T, columns >= cout zero),  bh [32] (rows >= cout zero)
//   Wse  [nt][DP / 8][64][4]  the encoding columns of the skip layer (skip only; absent otherwise)
// Train stash (workspace, [rows][npad] feature-major planes): H_l (post-ReLU output of layer l, l = 0 .. L-2), D_l (delta of layer l's
// pre-activation), ENC [DP][npad] (the encoding the first and the skip layer saw), G [4][npad] (dL/dyhat).

#define NERF_PI_F 3.14159274101257324f      // fl32(pi): math.pi as torch multiplies it into a float32 tensor

struct NerfLayout {
    int nt, FP, d, DP, sl;      // sl: skip layer index (0 = none)
    int64_t w0f, b0, hid, hid_stride, whf, whb, bh, wse, total;
};
BL_HD int nerf_d(const brief_nerf_desc &d) { return d.cin * (1 + 2 * d.frequencies); }
BL_HD NerfLayout nerf_layout(const brief_nerf_desc &d)
{
    NerfLayout o;
    o.nt = (d.features + 31) / 32; o.FP = 32 * o.nt;
    o.d = nerf_d(d); o.DP = 8 * ((o.d + 7) / 8);
    o.sl = d.skip ? (d.layers - 1) / 2 : 0;
    o.w0f = 0;
    o.b0 = (int64_t)o.FP * o.DP;
    o.hid = o.b0 + o.FP;
    o.hid_stride = 2 * (int64_t)o.FP * o.FP + o.FP;
    o.whf = o.hid + (int64_t)(d.layers - 2) * o.hid_stride;
    o.whb = o.whf + 32 * (int64_t)o.FP;
    o.bh = o.whb + 32 * (int64_t)o.FP;
    o.wse = o.bh + 32;
    o.total = o.wse + (o.sl ? (int64_t)o.FP * o.DP : 0);
    return o;
}
// canonical offsets (floats, state_dict order): W0 [F][d] b0 [F] | W_l [F][ldw_l] b_l [F] (ldw = d + F for the skip layer) | Wh bh
BL_HD int64_t nerf_canon_hidden(const brief_nerf_desc &d, int l /*1..L-1*/)
{
    const int64_t F = d.features, dd = nerf_d(d);
    const int sl = d.skip ? (d.layers - 1) / 2 : 0;
    return dd * F + F + (int64_t)(l - 1) * (F * F + F) + (sl && l > sl ? dd * F : 0);
}
BL_HD int64_t nerf_canon_head(const brief_nerf_desc &d) { return nerf_canon_hidden(d, d.layers - 1); }
BL_HD int64_t nerf_canon_count(const brief_nerf_desc &d) { return nerf_canon_head(d) + (int64_t)d.cout * d.features + d.cout; }

struct NerfArgs {
    brief_nerf_desc d;
    int nt, DP;
    const float *pk;
    const float *coords, *targets, *weights;
    const int64_t *idx;
    int64_t offset, n;
    uint64_t rng_pop, rng_seed, rng_step;
    GridArgs grid;
    BoxArgs box;
    int loss_kind;
    float thr, beta, inv_count;
    float *H, *D, *ENC, *G;   // train stash (see above)
    float *lpart;             // [gridDim.x] loss partial per workgroup
    int64_t npad;
    float *yhat_out;
    void *out;
    int out_kind;
    float scale_min, den, span, vmin;
};

// ---- the tile helpers nerf_box_coords, nerf_chain, nerf_bias, nerf_write_image, nerf_stash and nerf_frag: the one text of brief_tile.inc,
// compiled here under the nerf_ prefix.  One text, not one set of functions: with the NeRF, MFN and taper kernels calling the ffn_*
// helpers, 88 of the 330 kernels compiled to other code, 24 k_ffn_fwd instantiations whose source did not change among them.  No
// family keeps a copy; only brief_jac.inc has a frag lambda of its own.
#define TILE_(name) nerf_##name
#include "brief_tile.inc"

// image element (k, s) of a 32-sample tile (the layout of brief_ffn.inc)
__device__ __forceinline__ int nerf_img(int k, int s) { return ((k >> 3) * 64 + 32 * ((k >> 2) & 1) + s) * 4 + (k & 3); }

// One 32-sample tile per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles wv, wv + 4, ...
// TRAIN: forward, loss, dgrad chain and the stash for k_nerf_wgrad.  Inference: forward and the out_kind epilogue (BOX: box voxels).
template <int MTW, bool TRAIN, bool BOX>
__global__ __launch_bounds__(256) void k_nerf_fwd(const NerfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int DP = a.DP, nt = a.nt, FP = 32 * nt;
    float4 *Xe = reinterpret_cast<float4 *>(smem);                     // encoding image: rows 0 .. DP-1
    float4 *Xh = Xe + (DP / 8) * 64;                                   // hidden image: FP rows
    float *xsh = smem + 32 * (DP + FP);                                // [32][4] coordinates of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers, F = a.d.features, Lf = a.d.frequencies;
    const int kf = (F + 7) / 8;                                        // K steps that hold real features
    const NerfLayout lay = nerf_layout(a.d);
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
                    nerf_box_coords(a.grid, a.box, cin, j, x0, x1, x2);
                } else {
                    grid_coords(a.grid, cin, j, x0, x1, x2);
                }
            }
            *reinterpret_cast<float4 *>(xsh + 4 * s) = make_float4(x0, x1, x2, 0.f);
        }
        __syncthreads();
        // ---- encoding image (and its stash): rows c < cin the coordinates, pair q = i cin + c -> rows cin + 2 q (sin), cin + 2 q + 1
        // (cos), rows d .. DP-1 zero
        const int npair = cin * Lf, nfix = DP - 2 * npair;             // nfix: coordinate rows and padding rows
        for (int q = tid; q < (npair + nfix) * 32; q += 256) {
            const int e = q >> 5, sc = q & 31;
            const float4 x = *reinterpret_cast<const float4 *>(xsh + 4 * sc);
            if (e < npair) {
                const int i = e / cin, c = e - i * cin;
                const float xc = c == 0 ? x.x : (c == 1 ? x.y : x.z);
                const float p = ldexpf(__fmul_rn(NERF_PI_F, xc), i);   // the exact float 2^i fl32(fl32(pi) x)
                float sv, cv;
                sincosf(p, &sv, &cv);
                const int k1 = cin + 2 * e, k2 = k1 + 1;
                smem[nerf_img(k1, sc)] = sv;
                smem[nerf_img(k2, sc)] = cv;
                if (TRAIN) {
                    a.ENC[(int64_t)k1 * a.npad + col0 + sc] = sv;
                    a.ENC[(int64_t)k2 * a.npad + col0 + sc] = cv;
                }
            } else {
                const int r = e - npair, k = r < cin ? r : 2 * npair + r;
                const float v = r < cin ? (r == 0 ? x.x : (r == 1 ? x.y : x.z)) : 0.f;
                smem[nerf_img(k, sc)] = v;
                if (TRAIN) a.ENC[(int64_t)k * a.npad + col0 + sc] = v;
            }
        }
        __syncthreads();
        // ---- first layer (K = DP, the encoding), the hidden layers (the skip layer: encoding rows, then the hidden image), ReLU
        f32x16 acc[MTW];
        for (int l = 0; l <= L - 2; ++l) {
            const float *Wf = l == 0 ? a.pk + lay.w0f : a.pk + lay.hid + (int64_t)(l - 1) * lay.hid_stride;
            const float *bb = l == 0 ? a.pk + lay.b0 : Wf + 2 * (int64_t)FP * FP;
            nerf_bias(acc, bb, nt, wv, hi);
            if (l == 0) {
                nerf_chain(acc, Wf, DP / 8, DP / 8, nt, Xe, wv, lane);
            } else {
                if (l == lay.sl) nerf_chain(acc, a.pk + lay.wse, DP / 8, DP / 8, nt, Xe, wv, lane);
                nerf_chain(acc, Wf, FP / 8, kf, nt, Xh, wv, lane);
            }
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = fmaxf(acc[t][r], 0.f);
            if (TRAIN) nerf_stash(a.H + (int64_t)l * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            __syncthreads();
            nerf_write_image(Xh, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        nerf_bias(hacc, a.pk + lay.bh, 1, wv, hi);
        if (wv == 0) {
            nerf_chain(hacc, a.pk + lay.whf, FP / 8, kf, 1, Xh, wv, lane);
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
        if (tid < 64) Xh[lane] = hi == 0 ? make_float4(g[0], g[1], g[2], g[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        // ---- dgrad chain: delta_l = (W_{l+1}^T delta_{l+1}) . (h_l > 0), l = L-2 .. 0; the skip layer's W^T is its hidden half (nothing
        // flows into the encoding)
        for (int l = L - 2; l >= 0; --l) {
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            if (l == L - 2) nerf_chain(acc, a.pk + lay.whb, 4, 1, nt, Xh, wv, lane);
            else nerf_chain(acc, a.pk + lay.hid + (int64_t)l * lay.hid_stride + (int64_t)FP * FP, FP / 8, kf, nt, Xh, wv, lane);
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
            nerf_stash(a.D + (int64_t)l * FP * a.npad, a.npad, col0, acc, nt, wv, hi, s);
            if (l > 0) {
                __syncthreads();
                nerf_write_image(Xh, acc, nt, wv, lane);
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
// wave one 64 x 64 block (2 x 2 accumulator tiles), partial sums into slabs[split][canonical index]; the bias gradient (row sums of A)
// by the waves of the first column block of the blocks that carry it.  The skip layer is two blocks: its encoding columns (B = ENC,
// no bias) and its hidden columns (B = H_{sl-1}, column offset d, with the bias).
struct NerfWgradBlock {
    const float *A, *B;     // [rows][npad] planes
    int arows, brows;       // rows that hold data (A: F or cout; B: F or d)
    int mb, nb;             // 64-row / 64-column blocks
    int wave_begin;         // first wave job of this block
    int64_t w_off, b_off;   // canonical offsets of dW (column 0 of this block) and db (b_off < 0: no bias)
    int ldw;                // row length of dW in the canonical buffer
};
#define NERF_WGRAD_BLOCKS 32      // blocks per k_nerf_wgrad launch (deeper nets take several launches)
struct NerfWgradArgs {
    NerfWgradBlock blk[NERF_WGRAD_BLOCKS];
    int nblocks, waves;
    int64_t npad, chunk, mlp;
    float *slabs;
};

__global__ __launch_bounds__(256) void k_nerf_wgrad(const NerfWgradArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, i = lane & 31;
    const int w = blockIdx.x * 4 + (tid >> 6);
    if (w >= a.waves) return;
    int l = 0;
    while (l + 1 < a.nblocks && a.blk[l + 1].wave_begin <= w) ++l;
    const NerfWgradBlock &L = a.blk[l];
    const int wl = w - L.wave_begin, mb = wl / L.nb, nb = wl % L.nb;
    const bool bias = L.b_off >= 0 && nb == 0;
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

// canonical -> packed (see the layout at the top of this file)
__global__ void k_nerf_repack(const brief_nerf_desc d, const float *__restrict__ params, float *__restrict__ pk)
{
    const NerfLayout lay = nerf_layout(d);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= lay.total) return;
    const int F = d.features, dd = lay.d, cout = d.cout, FP = lay.FP;
    float v = 0.f;
    int row, k;
    if (e < lay.b0) {
        nerf_frag(e - lay.w0f, lay.DP / 8, row, k);
        if (row < F && k < dd) v = params[(int64_t)row * dd + k];
    } else if (e < lay.hid) {
        const int f = (int)(e - lay.b0);
        if (f < F) v = params[(int64_t)F * dd + f];
    } else if (e < lay.whf) {
        const int l = 1 + (int)((e - lay.hid) / lay.hid_stride);
        const int64_t r = (e - lay.hid) % lay.hid_stride;
        const int coff = l == lay.sl ? dd : 0, ldw = F + coff;
        const float *W = params + nerf_canon_hidden(d, l);
        if (r < 2 * (int64_t)FP * FP) {
            const bool bwd = r >= (int64_t)FP * FP;
            nerf_frag(bwd ? r - (int64_t)FP * FP : r, FP / 8, row, k);
            if (row < F && k < F) v = bwd ? W[(int64_t)k * ldw + coff + row] : W[(int64_t)row * ldw + coff + k];
        } else {
            const int f = (int)(r - 2 * (int64_t)FP * FP);
            if (f < F) v = W[(int64_t)F * ldw + f];
        }
    } else if (e < lay.whb) {
        nerf_frag(e - lay.whf, FP / 8, row, k);
        if (row < cout && k < F) v = params[nerf_canon_head(d) + (int64_t)row * F + k];
    } else if (e < lay.bh) {
        nerf_frag(e - lay.whb, 4, row, k);
        if (row < F && k < cout) v = params[nerf_canon_head(d) + (int64_t)k * F + row];
    } else if (e < lay.wse) {
        const int c = (int)(e - lay.bh);
        if (c < cout) v = params[nerf_canon_head(d) + (int64_t)cout * F + c];
    } else {
        nerf_frag(e - lay.wse, lay.DP / 8, row, k);
        if (row < F && k < dd) v = params[nerf_canon_hidden(d, lay.sl) + (int64_t)row * (dd + F) + k];
    }
    pk[e] = v;
}
