// brief_hess.inc — Hessian decode of an fp32 SIREN: k_hess_fwd<MTW, BOX> and its host entries brief_siren_hess_forward / _forward_box
// (part of the single translation unit brief_hip.hip, included last, behind brief_view.inc, so that its kernels are the last ones named).
// No kernel or device function of another file is changed.  The tile helpers hess_box_coords, hess_chain, hess_bias_col, hess_fetch and
// hess_write_image are the one text of brief_tile.inc compiled under the hess_ prefix (TILE_CHAIN_PACKED form, as brief_jac.inc has them
// under jac_); the included hess_bias, hess_stash and hess_frag are unused.  HessArgs is brief_jac.inc's JacArgs and one pointer; the host
// entries are the driver of brief_jac_host.inc over HessDecode.  The weights are the Jacobian kernel's packed fragment copy (k_jac_repack,
// JacLayout): there is no second repack.  The two kernels stay two texts: their column layouts, the layer-0 block, the sine rule and the
// head differ in every line that is not a helper call (profiles/r21_derivative_decode.md).
//
// Forward mode of second order: the value, its cin tangents and its cin (cin + 1) / 2 distinct second derivatives travel together,
//   z_0 = W_0 x + b_0,      d_a z_0 = W_0[:, a],       d_ab z_0 = 0
//   h = sin(w0 z),          d_a h = w0 cos(w0 z) d_a z,    d_ab h = w0 cos(w0 z) d_ab z - w0^2 sin(w0 z) d_a z d_b z
//   z' = W h + b,           d_a z' = W d_a h,          d_ab z' = W d_ab h       (one chain over all columns; the bias in the value column)
//   head: y = Wh h + bh unscaled; output_act: the sine rule with w0_hidden on y.
// Phase rule (k_jac_fwd's): the weights carry s_l = w0_l / 2 pi, so the value column IS the phase p in revolutions and the other columns
// are its derivatives; with f = fract(p): h = sin_rev(f), d_a h = 2 pi cos_rev(f) d_a p, d_ab h = 2 pi cos_rev(f) d_ab p -
// (2 pi)^2 sin_rev(f) d_a p d_b p.
//
// Slot layout: the 32 columns of an MFMA tile are SPT samples x SLOT columns, SLOT = 1 + cin + nh = 10 (cin == 3: SPT = 3 samples per
// tile) or 6 (cin == 2: SPT = 5); column SLOT j + c, j < SPT, belongs to sample j of the tile and
//   c = 0                     the phase / value
//   c = 1 .. cin              the tangent along axis c - 1
//   c = cin + 1 .. cin + nh   the second derivative h = c - cin - 1 in the order (00, 01, 02, 11, 12, 22)  (cin == 2: (00, 01, 11))
// Columns 30 and 31 belong to no sample: exact zeros at every layer.  (Power-of-two slots, 16 / 8 columns and 2 / 4 samples per tile,
// would leave 12 / 8 of the 32 columns idle; the lane arithmetic below does not need them.)
// A second-derivative column needs the phase and two tangents of its own sample; they sit in the same register of the lanes lane0,
// lane0 + 1 + a and lane0 + 1 + b, lane0 = 32 hi + SLOT j: three lane permutes (ds_bpermute) per register with byte addresses
// computed once per thread, no LDS round trip.  The LDS image of a layer stays [32 nt rows][32 columns] (128 KB at 1024 features)
// plus the tile's coordinates, as in k_jac_fwd.

struct HessArgs : JacArgs {
    float *hess;              // [n][cout][nh]; the base's jac may be NULL here
};

#define TILE_CHAIN_PACKED
#define TILE_(name) hess_##name
#include "brief_tile.inc"

// register v of lane addr / 4 (ds_bpermute); call it from wave-uniform control flow
__device__ __forceinline__ float hess_lane(int addr, float v)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// One tile of SPT samples per workgroup iteration (persistent grid over the tiles), 4 waves; wave wv owns feature tiles wv, wv + 4,
// ... of every layer.  Samples past n in the last tile compute on zeros and store nothing.
template <int MTW, bool BOX>
__global__ __launch_bounds__(256) void k_hess_fwd(const HessArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4 *Xh = reinterpret_cast<float4 *>(smem);                     // image: 32 nt rows x 32 columns
    float *xsh = smem + 1024 * a.lay.nt;                               // [spt][4] coordinates of the tile
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, hi = lane >> 5, s = lane & 31;
    const int cin = a.d.cin, cout = a.d.cout, L = a.d.layers, nt = a.lay.nt, ks = a.lay.ks;
    const int nh = cin == 3 ? 6 : 3, slot = 1 + cin + nh, spt = 32 / slot;      // 10 columns x 3 samples, or 6 columns x 5 samples
    const bool used = s < spt * slot;                                  // columns 30 and 31 belong to no sample
    const int sj = used ? s / slot : 0, c = used ? s - slot * sj : slot;      // column s: sample sj of the tile, column c of its slot
    const int kind = c == 0 ? 0 : (c <= cin ? 1 : (c < slot ? 2 : 3));      // value, tangent, second derivative, unused
    const int h2 = c - cin - 1;                                        // the second derivative's index (kind == 2)
    int ha = 0, hb = 0;                                                // its two axes
    if (kind == 2) {
        if (cin == 3) { ha = h2 < 3 ? 0 : (h2 < 5 ? 1 : 2); hb = h2 < 3 ? h2 : (h2 < 5 ? h2 - 2 : 2); }
        else          { ha = h2 < 2 ? 0 : 1; hb = h2 < 1 ? 0 : 1; }
    }
    const int lane0 = 32 * hi + slot * sj;
    const int src0 = 4 * lane0, srcA = 4 * (lane0 + 1 + ha), srcB = 4 * (lane0 + 1 + hb);      // ds_bpermute byte addresses
    const int64_t ntiles = (a.n + spt - 1) / spt;
    const float w0h = a.d.w0_hidden;
    const float tau = 6.2831853071795865f, tau2 = 39.478417604357434f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t col0 = tile * spt;
        // ---- sample selection: the sources of the family decode kernels
        if (tid < spt) *reinterpret_cast<float4 *>(xsh + 4 * tid) = hess_fetch<BOX>(a, cin, col0 + tid);
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
                            v = c == 0 ? ph : (c == 1 ? w.x : (c == 2 ? w.y : (c == 3 && cin == 3 ? w.z : 0.f)));      // d_ab p = 0
                        }
                        acc[t][r] = v;
                    }
                }
            } else {
                const float *pl = a.pk + a.lay.hid + (int64_t)(l - 1) * a.lay.hid_stride;
                hess_bias_col(acc, pl + (int64_t)nt * ks * 256, nt, wv, hi, c == 0);
                hess_chain(acc, pl, ks, nt, Xh, wv, lane);
            }
            // the sine rule on the phase p (column 0), its tangents and its second derivatives
#pragma unroll
            for (int t = 0; t < MTW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[t][r];
                    const float p = hess_lane(src0, v), da = hess_lane(srcA, v), db = hess_lane(srcB, v);
                    const float f = __builtin_amdgcn_fractf(p);
                    const float sn = BRIEF_SIN_REV(f), first = tau * BRIEF_COS_REV(f) * v;
                    const float second = __fmaf_rn(-(tau2 * sn) * da, db, first);
                    acc[t][r] = kind == 0 ? sn : (kind == 1 ? first : (kind == 2 ? second : 0.f));
                }
            __syncthreads();
            hess_write_image(Xh, acc, nt, wv, lane);
            __syncthreads();
        }
        // ---- head (one 32-row tile: wave 0), rows 0..cout-1 are in registers 0..3 of lanes 0..31
        f32x16 hacc[1];
        const float *ph = a.pk + a.lay.head;
        hess_bias_col(hacc, ph + (int64_t)ks * 256, 1, wv, hi, c == 0);
        if (wv == 0) hess_chain(hacc, ph, ks, 1, Xh, wv, lane);
        float yo[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const float y = hacc[0][ch];
            if (a.d.output_act) {
                const float y0 = hess_lane(src0, y), ya = hess_lane(srcA, y), yb = hess_lane(srcB, y);
                const float sn = brief_fast_sinf(w0h * y0), first = w0h * brief_fast_cosf(w0h * y0) * y;
                const float second = __fmaf_rn(-(w0h * w0h * sn) * ya, yb, first);
                yo[ch] = kind == 0 ? sn : (kind == 1 ? first : second);
            } else {
                yo[ch] = y;
            }
        }
        const int64_t n = col0 + sj;
        if (tid < 32 && n < a.n) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (ch >= cout) break;
                if (kind == 0) {
                    if (a.value) a.value[n * cout + ch] = yo[ch];
                } else if (kind == 1) {
                    if (a.jac) a.jac[(n * cout + ch) * cin + (c - 1)] = yo[ch];
                } else if (kind == 2) {
                    a.hess[(n * cout + ch) * nh + h2] = yo[ch];
                }
            }
        }
        __syncthreads();      // the image and the coordinates are re-used by the next tile
    }
}

// ---- host side: the driver of brief_jac_host.inc (its checks, their order and the sample sources) over this decode's traits; `packed`
// is brief_siren_jac_repack's buffer.

static void deriv_set_hess(HessArgs &a, float *hess) { a.hess = hess; }

template <bool BOX>
struct HessFwd { template <int M> static auto fn() { return k_hess_fwd<M, BOX>; } };

struct HessDecode {
    typedef HessArgs Args;
    static constexpr const char *label = "spatial hessian", *too_wide = "spatial hessian: features must be 1..1024",
                                *null_buffer = "spatial hessian: null buffer (packed and hess are required)";
    static float *required(float *, float *hess) { return hess; }
    // the persistent grid over tiles of 3 (cin == 3) or 5 (cin == 2) samples: family_grid counts tiles of 32
    template <bool BOX>
    static int launch(const Args &a, hipStream_t st)
    {
        const int lds = jac_lds_bytes(a.lay);
        const int64_t spt = a.d.cin == 3 ? 3 : 5;
        return launch_fwd_mtw<HessFwd<BOX> >((a.lay.nt + 3) / 4, a, family_grid(lds, 32 * ((a.n + spt - 1) / spt)), lds, st, too_wide);
    }
};

extern "C" {

int brief_siren_hess_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                             float *value, float *jac, float *hess, void *stream)
{
    return deriv_forward<HessDecode>(d, packed, grid, batch, value, jac, hess, stream);
}

int brief_siren_hess_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                                 float *value, float *jac, float *hess, void *stream)
{
    return deriv_forward_box<HessDecode>(d, packed, box, offset, n, value, jac, hess, stream);
}

}   // extern "C"

