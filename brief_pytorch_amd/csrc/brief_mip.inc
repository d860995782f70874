// brief_mip.inc — k_mip_rows, k_mip_cols: max-intensity projections of a decoded box (part of the single translation unit brief_hip.hip).
// A dense box src[e0][e1][e2][C] of uint8 / uint16 is folded by elementwise MAX into three images that live in a larger frame
// (I0, I1, I2) at `origin` (o0, o1, o2):
//   mip_d[I1][I2][C] <- max over axis 0,   mip_h[I0][I2][C] <- max over axis 1,   mip_w[I0][I1][C] <- max over axis 2.
// All three are read-modify-write (img = max(img, new)): the chunks of one region, and the blocks of a partition, meet in them.
//
// There are NO atomics.  The hardware has no 8- or 16-bit atomic max, so an atomic on an image element would be a compare-and-swap on
// the 32-bit word around it (and at an image's last bytes on memory that does not belong to it).  Instead every destination has ONE
// owner within a launch, who reduces everything that lands on it on chip and then does one plain read-modify-write:
//   k_mip_rows   a workgroup owns a box row index y: mip_d[y][all x] and mip_w[all z][y].  Its waves split z.  A lane holds 16 bytes of
//                the row (L = e2 C elements per row, 64 lanes = one 1-KiB segment); per segment a wave keeps the max over its z in
//                registers (mip_d; the waves' partials meet in LDS, wave 0 writes), and per row (z, y) folds its vector to the C
//                channel maxima and reduces them over the wave with a butterfly (mip_w; lane c writes channel c, for every segment
//                of the row in turn: the same lane, so in program order).
//   k_mip_cols   a workgroup owns (z, segment): mip_h[z][segment].  Its waves split y; registers over y, LDS over the waves.
// So the box is read twice (once per kernel; the second read of a chunk finds it in the caches) and each image element touched
// by a launch is read once and written once.  16-byte loads are used when src is 16-byte aligned and a row is a whole number of
// 16-byte vectors; otherwise the same vectors are assembled from element loads.  Max is exact and order-independent: every run
// gives the same bits.  Indices are 64-bit throughout.
static const int kMipMaxWaves = 16;
static const int kMipUnroll = 4;                                   // rows a wave has in flight

__device__ __forceinline__ uint32_t mip_pkmax16(uint32_t a, uint32_t b)       // max of the two 16-bit halves, each on its own (v_pk_max_u16)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const us2 r = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
    return __builtin_bit_cast(uint32_t, r);
}
template <typename T>
__device__ __forceinline__ uint32_t mip_wmax(uint32_t a, uint32_t b)          // elementwise max of the T's packed in a word
{
    if (sizeof(T) == 2) return mip_pkmax16(a, b);
    // bytes: the even and the odd ones as two sets of 16-bit numbers (an odd byte with a zero below it compares as the byte does)
    return mip_pkmax16(a & 0x00ff00ffu, b & 0x00ff00ffu) | mip_pkmax16(a & 0xff00ff00u, b & 0xff00ff00u);
}
template <typename T>
__device__ __forceinline__ uint4 mip_vmax(const uint4 &a, const uint4 &b)
{
    return make_uint4(mip_wmax<T>(a.x, b.x), mip_wmax<T>(a.y, b.y), mip_wmax<T>(a.z, b.z), mip_wmax<T>(a.w, b.w));
}

// 16 bytes of a row of L elements from element e; elements at and beyond L read as 0 (the identity of max) and are never touched.
// vec: the row's base and e * sizeof(T) are multiples of 16.
template <typename T>
__device__ __forceinline__ uint4 mip_load(const T *__restrict__ row, int64_t e, int64_t L, bool vec)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    if (vec && e + VEC <= L) return *reinterpret_cast<const uint4 *>(row + e);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (e + j < L) w[j * (int)sizeof(T) / 4] |= (uint32_t)row[e + j] << (8 * ((j * (int)sizeof(T)) & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// img[0 .. nvalid) = max(img, the first nvalid elements of v): the owner's plain read-modify-write
template <typename T>
__device__ __forceinline__ void mip_rmw(T *img, const uint4 &v, int nvalid)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    if (nvalid == VEC && ((uintptr_t)img & 15) == 0) {
        uint4 *p = reinterpret_cast<uint4 *>(img);
        *p = mip_vmax<T>(*p, v);
        return;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (j < nvalid) {
            const int x = corr_elem<T>(v, j);
            if (x > (int)img[j]) img[j] = (T)x;
        }
}

// the C channel maxima of a lane's vector, whose element j belongs to channel (ph + j) % C.  VEC is a multiple of 1, 2 and 4, so
// ph is 0 there; with C = 3 it is the lane's own, and each of its three values gets its unrolled copy.
template <typename T, int C>
__device__ __forceinline__ void mip_fold(const uint4 &v, int ph, int (&m)[4])
{
    constexpr int VEC = 16 / (int)sizeof(T);
#pragma unroll
    for (int p = 0; p < (C == 3 ? 3 : 1); ++p)
        if (C != 3 || ph == p) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int x = corr_elem<T>(v, j);
                m[(p + j) % C] = x > m[(p + j) % C] ? x : m[(p + j) % C];
            }
        }
}

template <typename T, int C>
__global__ __launch_bounds__(64 * kMipMaxWaves) void k_mip_rows(const T *__restrict__ src, int64_t e0, int64_t e1, int64_t L, int vec,
                                                                 T *__restrict__ mip_d, T *__restrict__ mip_w, int64_t o0, int64_t o1, int64_t o2,
                                                                 int64_t I1, int64_t I2)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ uint4 s_acc[kMipMaxWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t nseg = (L + 64 * VEC - 1) / (64 * VEC);
    for (int64_t y = blockIdx.x; y < e1; y += gridDim.x) {
        for (int64_t seg = 0; seg < nseg; ++seg) {
            const int64_t e = (seg * 64 + lane) * VEC;              // the lane's first element within a row
            const int ph = C == 3 ? (int)(e % 3) : 0;
            uint4 acc = make_uint4(0u, 0u, 0u, 0u);
            for (int64_t zb = wave; zb < e0; zb += (int64_t)kMipUnroll * nw) {
                uint4 v[kMipUnroll];
#pragma unroll
                for (int k = 0; k < kMipUnroll; ++k) {
                    const int64_t z = zb + (int64_t)k * nw;
                    v[k] = z < e0 ? mip_load<T>(src + (z * e1 + y) * L, e, L, vec != 0) : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (int k = 0; k < kMipUnroll; ++k) {
                    const int64_t z = zb + (int64_t)k * nw;
                    if (z >= e0) break;                             // (wave-uniform)
                    acc = mip_vmax<T>(acc, v[k]);
                    int m[4] = {0, 0, 0, 0};
                    mip_fold<T, C>(v[k], ph, m);
                    uint32_t p0 = (uint32_t)m[0] | ((uint32_t)m[1] << 16), p1 = (uint32_t)m[2] | ((uint32_t)m[3] << 16);
                    for (int off = 32; off >= 1; off >>= 1) {
                        p0 = mip_pkmax16(p0, (uint32_t)__shfl_xor((int)p0, off));
                        if (C > 2) p1 = mip_pkmax16(p1, (uint32_t)__shfl_xor((int)p1, off));
                    }
                    if (lane < C) {
                        const uint32_t pw = lane < 2 ? p0 : p1;
                        const int x = (int)((lane & 1) ? pw >> 16 : pw & 0xffffu);
                        T *d = mip_w + ((o0 + z) * I1 + o1 + y) * C + lane;
                        if (x > (int)*d) *d = (T)x;
                    }
                }
            }
            s_acc[wave][lane] = acc;
            __syncthreads();
            if (wave == 0 && e < L) {
                for (int w = 1; w < nw; ++w) acc = mip_vmax<T>(acc, s_acc[w][lane]);
                const int64_t left = L - e;
                mip_rmw<T>(mip_d + ((o1 + y) * I2 + o2) * C + e, acc, left < VEC ? (int)left : VEC);
            }
            __syncthreads();                                        // (s_acc is rewritten for the next segment)
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kMipMaxWaves) void k_mip_cols(const T *__restrict__ src, int64_t e0, int64_t e1, int64_t L, int vec,
                                                                 T *__restrict__ mip_h, int64_t o0, int64_t o2, int64_t I2, int C)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ uint4 s_acc[kMipMaxWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t nseg = (L + 64 * VEC - 1) / (64 * VEC), total = e0 * nseg;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t z = t / nseg, seg = t - z * nseg;
        const int64_t e = (seg * 64 + lane) * VEC;
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
        for (int64_t yb = wave; yb < e1; yb += (int64_t)kMipUnroll * nw) {
            uint4 v[kMipUnroll];
#pragma unroll
            for (int k = 0; k < kMipUnroll; ++k) {
                const int64_t y = yb + (int64_t)k * nw;
                v[k] = y < e1 ? mip_load<T>(src + (z * e1 + y) * L, e, L, vec != 0) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int k = 0; k < kMipUnroll; ++k) acc = mip_vmax<T>(acc, v[k]);
        }
        s_acc[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && e < L) {
            for (int w = 1; w < nw; ++w) acc = mip_vmax<T>(acc, s_acc[w][lane]);
            const int64_t left = L - e;
            mip_rmw<T>(mip_h + ((o0 + z) * I2 + o2) * C + e, acc, left < VEC ? (int)left : VEC);
        }
        __syncthreads();                                            // (s_acc is rewritten for the workgroup's next piece)
    }
}
