// brief_jac.inc — spatial-gradient decode of an fp32 SIREN: k_jac_fwd<MTW, BOX>, k_jac_repack (part of the single translation unit
// brief_hip.hip, included behind brief_quant.inc so that its kernels are named last; the host entries are brief_jac_host.inc).
// No kernel or device function of another file is changed.  The tile helpers jac_box_coords, jac_chain, jac_bias_col, jac_fetch and
// jac_write_image are the one text of brief_tile.inc compiled under the jac_ prefix (TILE_CHAIN_PACKED form; not functions shared with the
// families: that changes the code of 88 of the 330 kernels, see the note in brief_nerf.inc); the Hessian decode (brief_hess.inc) compiles
// the same text under hess_, and its HessArgs derives from this file's JacArgs.  The frag lambda of k_jac_repack (it captures ks) is this
// file's own; the included jac_bias, jac_stash and jac_frag are unused.
//
// Forward mode: the value and its cin tangents travel through the layers together,
//   z_0 = W_0 x + b_0,            dz_0/dx_a = W_0[:, a]
//   h_l = sin(w0_l z_l),          dh_l = w0_l cos(w0_l z_l) . dz_l
//   z_{l+1} = W_{l+1} h_l + b,    dz_{l+1} = W_{l+1} dh_l          (head: y = Wh h + bh, dy = Wh dh; output_act: y <- sin(w0 y), dy <- w0 cos(w0 y) dy)
// Quad layout: the 32 columns of an MFMA tile are 8 samples x 4 quantities, column 4 j + q = sample j, q = 0 the phase / value and
// q = 1 .. cin the tangent along axis q - 1 (cin == 2: column q = 3 is zero).  One chain acc += A(mt, step) . image advances all four; a
// bias goes into column q = 0 only.  The LDS image of a layer stays [32 nt rows][32 columns] (128 KB at 1024 features, plus the tile's
// coordinates), as in the family kernels.
// Phase rule (k_fused's): the forward weights and biases of sine layer l carry s_l = w0_l / 2 pi, so the accumulator of column 0 IS the
// phase in revolutions and a tangent column is its derivative; with f = fract(phase), h = sin_rev(f) and dh = 2 pi cos_rev(f) dz.  The
// phase of a tangent's sample sits in the same register of lane (lane & ~3): a DPP quad broadcast, no LDS round trip.
//
// Packed layout (floats; fragment block (mt, step) = 64 lanes x float4, A[32 mt + i][8 step + 4 hi + j]; OP = 32 nt, ks = ceil(F / 8)):
//   layer 0:            W0p [OP][4] = s_0 (w_0, w_1, w_2 | 0, b)                   (layer 0 runs on the VALU)
//   layer l = 1 .. L-2: Wf [nt][ks][64][4] (s_l W_l),  b [OP] (s_l b_l)
//   head:               Wf [1][ks][64][4] (rows >= cout zero, unscaled),  bh [32]
// Padded rows / columns and biases are zero: a padded unit has phase 0, value sin(0) = 0 and tangent 2 pi cos(0) . 0 = 0.

struct JacLayout {
    int L, F, nt, ks;
    int64_t hid, hid_stride, head, total;       // packed offsets: first hidden layer, floats per hidden layer, head, size
    int64_t c_hid, c_stride, c_head;            // canonical offsets: first hidden layer, floats per hidden layer, head
};
BL_HD JacLayout jac_layout(const brief_siren_desc &d)
{
    JacLayout o;
    o.L = d.layers; o.F = d.features;
    o.nt = (d.features + 31) / 32;
    o.ks = (d.features + 7) / 8;
    o.hid = 128 * (int64_t)o.nt;
    o.hid_stride = (int64_t)o.nt * o.ks * 256 + 32 * (int64_t)o.nt;
    o.head = o.hid + (int64_t)(d.layers - 2) * o.hid_stride;
    o.total = o.head + (int64_t)o.ks * 256 + 32;
    const int64_t F = d.features;
    o.c_hid = F * d.cin + F;
    o.c_stride = F * F + F;
    o.c_head = o.c_hid + (int64_t)(d.layers - 2) * o.c_stride;
    return o;
}

struct JacArgs {
    brief_siren_desc d;
    JacLayout lay;
    const float *pk;
    const float *coords;
    const int64_t *idx;
    int64_t offset, n;
    GridArgs grid;
    BoxArgs box;
    float *value;             // [n][cout] or NULL
    float *jac;               // [n][cout][cin]
};

#define TILE_CHAIN_PACKED
#define TILE_(name) jac_##name
#include "brief_tile.inc"

// the value lane 4 (lane / 4) holds, in every lane of its quad (DPP quad_perm [0, 0, 0, 0]); call it from wave-uniform control flow
__device__ __forceinline__ float jac_quad0(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x00, 0xf, 0xf, false));
}

// One tile of 8 samples x 4 quantities per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles
// wv, wv + 4, ... of every layer.  Samples past n in the last tile compute on zeros and store nothing.
template <int MTW, bool BOX>
__global__ __launch_bounds__(256) void k_jac_fwd(const JacArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *Xh = reinterpret_cast<float4 *>(smem);                     // image: 32 nt rows x 32 columns
    float *xsh = smem + 1024 * a.lay.nt;                               // [8][4] coordinates of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int sj = s >> 2, q = s & 3;                                  // column s: sample sj of the tile, quantity q
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers, nt = a.lay.nt, ks = a.lay.ks;
    const int64_t ntiles = (a.n + 7) / 8;
    const float w0h = a.d.w0_hidden;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t col0 = tile * 8;
        // ---- sample selection: the sources of the family decode kernels
        if (tid < 8) *reinterpret_cast<float4 *>(xsh + 4 * tid) = jac_fetch<BOX>(a, cin, col0 + tid);
        __syncthreads();
        const float4 x = *reinterpret_cast<const float4 *>(xsh + 4 * sj);
        // ---- sine layers 0 .. L-2: layer 0 on the VALU (K = cin), the others as MFMA chains
        f32x16 acc[MTW];
        for (int l = 0; l <= L - 2; ++l) {
            if (l == 0) {
                const float4 *W0p = reinterpret_cast<const float4 *>(a.pk);
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    const int mt = wv + 4 * t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = 0.f;
                        if (mt < nt) {
                            const float4 w = W0p[32 * mt + ROWMAP(r, hi)];
                            const float ph = __fmaf_rn(w.x, x.x, __fmaf_rn(w.y, x.y, __fmaf_rn(w.z, x.z, w.w)));
                            v = q == 0 ? ph : (q == 1 ? w.x : (q == 2 ? w.y : w.z));      // (cin == 2: w.z is zero)
                        }
                        acc[t][r] = v;
                    }
                }
            } else {
                const float *pl = a.pk + a.lay.hid + (int64_t)(l - 1) * a.lay.hid_stride;
                jac_bias_col(acc, pl + (int64_t)nt * ks * 256, nt, wv, hi, q == 0);
                jac_chain(acc, pl, ks, nt, Xh, wv, lane);
            }
            // column 0 holds the phase in revolutions, columns 1 .. 3 its derivatives: h = sin_rev(f), dh = 2 pi cos_rev(f) dz
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float f = __builtin_amdgcn_fractf(jac_quad0(acc[t][r]));
                    acc[t][r] = q == 0 ? BRIEF_SIN_REV(f) : 6.2831853071795865f * BRIEF_COS_REV(f) * acc[t][r];
                }
            __syncthreads();
            jac_write_image(Xh, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        const float *ph = a.pk + a.lay.head;
        jac_bias_col(hacc, ph + (int64_t)ks * 256, 1, wv, hi, q == 0);
        if (wv == 0) jac_chain(hacc, ph, ks, 1, Xh, wv, lane);
        float yo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y = hacc[0][c], y0 = jac_quad0(y);
            if (a.d.output_act) yo[c] = q == 0 ? brief_fast_sinf(w0h * y) : w0h * brief_fast_cosf(w0h * y0) * y;
            else yo[c] = y;
        }
        const int64_t n = col0 + sj;
        if (tid < 32 && n < a.n) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= cout) break;
                if (q == 0) {
                    if (a.value) a.value[n * cout + c] = yo[c];
                } else if (q - 1 < cin) {
                    a.jac[(n * cout + c) * cin + (q - 1)] = yo[c];
                }
            }
        }
        __syncthreads();      // the image and the coordinates are re-used by the next tile
    }
}

// canonical (state_dict order: W_l [out_l][in_l] b_l [out_l] per layer) -> packed (see the layout at the top of this file)
__global__ void k_jac_repack(const brief_siren_desc d, const JacLayout lay, const float *__restrict__ params, float *__restrict__ pk)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= lay.total) return;
    const int F = lay.F, cin = d.cin, cout = d.cout, ks = lay.ks;
    const float s0 = d.w0_first * 0.15915494309189535f, sh = d.w0_hidden * 0.15915494309189535f;      // w0_l / 2 pi (the head is not scaled)
    // fragment element p of a block sequence with ks steps per row tile: (row, k)
    auto frag = [ks](int64_t p, int &row, int &k) {
        const int j = (int)(p & 3), lanei = (int)((p >> 2) & 63);
        const int64_t blk = p >> 8;
        const int step = (int)(blk % ks), mt = (int)(blk / ks);
        row = 32 * mt + (lanei & 31);
        k = 8 * step + 4 * (lanei >> 5) + j;
    };
    float v = 0.f;
    int row, k;
    if (e < lay.hid) {
        row = (int)(e >> 2); k = (int)(e & 3);
        if (row < F) {
            if (k < cin) v = params[(int64_t)row * cin + k] * s0;
            else if (k == 3) v = params[(int64_t)F * cin + row] * s0;
        }
    } else if (e < lay.head) {
        const int64_t l1 = (e - lay.hid) / lay.hid_stride, p = (e - lay.hid) % lay.hid_stride, nw = (int64_t)lay.nt * ks * 256;
        const float *W = params + lay.c_hid + l1 * lay.c_stride, *b = W + (int64_t)F * F;
        if (p < nw) {
            frag(p, row, k);
            if (row < F && k < F) v = W[(int64_t)row * F + k] * sh;
        } else if (p - nw < F) {
            v = b[p - nw] * sh;
        }
    } else {
        const int64_t p = e - lay.head, nw = (int64_t)ks * 256;
        const float *W = params + lay.c_head, *b = W + (int64_t)cout * F;
        if (p < nw) {
            frag(p, row, k);
            if (row < cout && k < F) v = W[(int64_t)row * F + k];
        } else if (p - nw < cout) {
            v = b[p - nw];
        }
    }
    pk[e] = v;
}
