// brief_correct.inc — k_correct_count, k_correct_emit, k_correct_apply: the error-bounded mode (part of the single translation unit
// brief_hip.hip).  After a fit the stored artefact is decoded and compared with the volume; every element off by more than the
// bound eps gets a stored correction, and every decode adds the corrections back, so that max |x - x^| <= eps holds exactly.
//
//   m = 2 eps + 1,  d = x - y^ (integers),  q = floor((d + eps) / m)   (FLOOR division)
//   q != 0  <=>  |d| > eps,   |d - q m| <= eps always;   the decoder computes clamp(y^ + q m, 0, type max).
//
// Finding the corrections is a stream compaction in two passes over the two volumes, with NO atomics, so that the output (and the
// file written from it) is the same on every run and ascending in the element index:
//   k_correct_count   a workgroup owns fixed contiguous chunks of kCorrChunkBytes of each array (chunk c = elements
//                     [c E, (c + 1) E), E = kCorrChunkBytes / sizeof(T)), reads both with 16-byte loads and writes the chunk's number
//                     of q != 0 elements; an exclusive scan of those counts (the caller's) gives every chunk's first output slot
//   k_correct_emit    the same walk again.  A chunk is dealt to the four waves as four contiguous quarters, a quarter to the
//                     lanes as kCorrIters rounds of one 16-byte vector per lane; a first pass over the quarter keeps one hit bit
//                     per element and gives the wave's total.  Rank of an element among the chunk's hits:
//                     hits of earlier waves (LDS prefix over the waves' totals) + hits of the wave's earlier rounds (a running
//                     wave-uniform sum) + hits of lower lanes in this round (mbcnt of the 64-bit ballot, summed over the vector's
//                     positions) + hits at lower positions of the lane's own vector.
//   k_correct_apply   one thread per correction: out[idx - base] = clamp(out[idx - base] + q m, 0, type max).
// Element indices are 64-bit throughout; `base` (the index of element 0 of the arrays in the volume they are a part of) is an
// argument, so a small array "at" an offset above 2^32 runs the very code a volume of that size runs.
static const int kCorrIters = 8;                                 // 16-byte vectors per lane and chunk
static const int kCorrChunkBytes = 256 * 16 * kCorrIters;        // of each array: 32 KiB
static const int kCorrWaveBytes = kCorrChunkBytes / 4;

// 16 bytes of `p` from element e0 (e0 * sizeof(T) is a multiple of 16); elements at and beyond n read as 0 in BOTH arrays, i.e.
// d = 0, never a hit.  Only the last vector of the arrays can be partial.
template <typename T>
__device__ __forceinline__ uint4 corr_load(const T *__restrict__ p, int64_t e0, int64_t n)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    if (e0 + VEC <= n) return *reinterpret_cast<const uint4 *>(p + e0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (e0 + j < n) w[j * (int)sizeof(T) / 4] |= (uint32_t)p[e0 + j] << (8 * ((j * (int)sizeof(T)) & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <typename T>
__device__ __forceinline__ int corr_elem(const uint4 &v, int j)      // j is a compile-time constant at every call site
{
    const uint32_t w = (j * (int)sizeof(T) / 4) == 0 ? v.x : ((j * (int)sizeof(T) / 4) == 1 ? v.y : ((j * (int)sizeof(T) / 4) == 2 ? v.z : v.w));
    return (int)((w >> (8 * ((j * (int)sizeof(T)) & 3))) & (sizeof(T) == 1 ? 0xffu : 0xffffu));
}
// floor((d + eps) / m) for a hit (|d| > eps): C's division truncates, so the negative side is divided as a positive number
__device__ __forceinline__ int corr_q(int d, int eps, int m)
{
    const int num = d + eps;
    return num >= 0 ? num / m : -((m - 1 - num) / m);
}

template <typename T>
__global__ __launch_bounds__(256) void k_correct_count(const T *__restrict__ dec, const T *__restrict__ src, int64_t n, int eps, int64_t nchunks,
                                                       int32_t *__restrict__ counts)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int64_t E = kCorrChunkBytes / (int)sizeof(T), EW = kCorrWaveBytes / (int)sizeof(T);
    __shared__ int s_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t e_wave = c * E + wave * EW;
        int hits = 0;
#pragma unroll
        for (int it = 0; it < kCorrIters; ++it) {
            const int64_t e0 = e_wave + ((int64_t)it * 64 + lane) * VEC;
            if (e0 < n) {
                const uint4 a = corr_load(dec, e0, n), b = corr_load(src, e0, n);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int d = corr_elem<T>(b, j) - corr_elem<T>(a, j);
                    hits += (d > eps || d < -eps) ? 1 : 0;
                }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) hits += __shfl_xor(hits, off);
        if (lane == 0) s_tot[wave] = hits;
        __syncthreads();
        if (threadIdx.x == 0) counts[c] = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
        __syncthreads();
    }
}

// element j of a vector for a RUN-TIME j (the emit pass walks a lane's hits bit by bit)
template <typename T>
__device__ __forceinline__ int corr_elem_dyn(const uint4 &v, int j)
{
    const int word = j * (int)sizeof(T) / 4;
    const uint32_t w = word == 0 ? v.x : (word == 1 ? v.y : (word == 2 ? v.z : v.w));
    return (int)((w >> (8 * ((j * (int)sizeof(T)) & 3))) & (sizeof(T) == 1 ? 0xffu : 0xffffu));
}

template <typename T>
__global__ __launch_bounds__(256) void k_correct_emit(const T *__restrict__ dec, const T *__restrict__ src, int64_t n, int eps, int64_t base,
                                                      int64_t nchunks, const int64_t *__restrict__ offsets, int64_t total,
                                                      int64_t *__restrict__ idx_out, int32_t *__restrict__ q_out)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int64_t E = kCorrChunkBytes / (int)sizeof(T), EW = kCorrWaveBytes / (int)sizeof(T);
    __shared__ int s_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = 2 * eps + 1;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t e_wave = c * E + wave * EW;
        // pass 1: the wave's quarter streamed once; what is kept is one hit bit per element (VEC bits per lane and round)
        uint32_t hit[kCorrIters];
        int wave_hits = 0;
#pragma unroll
        for (int it = 0; it < kCorrIters; ++it) {
            const int64_t e0 = e_wave + ((int64_t)it * 64 + lane) * VEC;
            hit[it] = 0u;
            if (e0 < n) {
                const uint4 a = corr_load(dec, e0, n), b = corr_load(src, e0, n);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int d = corr_elem<T>(b, j) - corr_elem<T>(a, j);
                    hit[it] |= (d > eps || d < -eps) ? (1u << j) : 0u;
                }
            }
            wave_hits += __popc(hit[it]);
        }
        for (int off = 32; off >= 1; off >>= 1) wave_hits += __shfl_xor(wave_hits, off);
        if (lane == 0) s_tot[wave] = wave_hits;
        __syncthreads();
        int64_t slot = offsets[c];                                  // first output slot of the chunk, then of this wave
        for (int w = 0; w < wave; ++w) slot += s_tot[w];
        __syncthreads();                                            // (s_tot is rewritten for the workgroup's next chunk)
        // pass 2: ranks from the hit bits; only lanes that hold a hit read their vectors again (from the caches) for q
#pragma unroll
        for (int it = 0; it < kCorrIters; ++it) {
            uint32_t h = hit[it];
            int below = 0, round_hits = 0;                          // hits of lower lanes / of the whole wave in this round
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const unsigned long long mask = __ballot((h >> j) & 1u);
                below += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                round_hits += __popcll(mask);
            }
            if (h) {
                const int64_t e0 = e_wave + ((int64_t)it * 64 + lane) * VEC;
                const uint4 a = corr_load(dec, e0, n), b = corr_load(src, e0, n);
                int64_t k = slot + below;
                while (h) {
                    const int j = __ffs((int)h) - 1;
                    h &= h - 1;
                    if (k < total) {                                // (always true for offsets that are the scan of k_correct_count's counts)
                        idx_out[k] = base + e0 + j;
                        q_out[k] = corr_q(corr_elem_dyn<T>(b, j) - corr_elem_dyn<T>(a, j), eps, m);
                    }
                    ++k;
                }
            }
            slot += round_hits;
        }
    }
}

template <typename T>
__global__ void k_correct_apply(T *__restrict__ out, int64_t n, const int64_t *__restrict__ idx, const int32_t *__restrict__ q, int64_t count,
                                int m, int64_t base)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int64_t i = idx[k] - base;
    if (i < 0 || i >= n) return;                                    // (refused on the host where it can be seen; never written out of bounds)
    constexpr int64_t TMAX = sizeof(T) == 1 ? 255 : 65535;
    int64_t v = (int64_t)out[i] + (int64_t)q[k] * m;
    v = v < 0 ? 0 : (v > TMAX ? TMAX : v);
    out[i] = (T)v;
}
