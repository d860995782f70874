// brief_quant.inc — k_quant_minmax, k_quant_fold, k_quant_apply, k_quant_decode: the weight quantiser of the quantised artefact and of the
// quantised fine-tune (part of the single translation unit brief_hip.hip; the arithmetic is brief_quant.h's, bit for bit numpy's).
//
// A tensor is a span {offset, count} of the canonical parameter buffer.  The spans travel BY VALUE in the kernel arguments (at most
// BRIEF_QUANT_MAX_TENSORS of them: a 16-layer tapered net has 32), cut into chunks: workgroup b owns chunk b of the launch and finds its
// span by a binary search over the spans' first chunks — wave-uniform, scalar loads of the argument segment.  There is no device table.
//
//   k_quant_minmax   one workgroup per kQuantRangeChunk (16 Ki) elements of a tensor: partial (min, max) -> workspace[chunk]
//   k_quant_fold     one workgroup per tensor: folds its partials, writes lo and step = (hi - lo) / (2^bits - 1) computed on the device
//   k_quant_apply    one workgroup per kQuantApplyChunk elements of a segment: qparams = deq(code(params)), codes = code(params); a
//                    segment that is a GAP between two spans is copied through to qparams
//   k_quant_decode   one workgroup per kQuantApplyChunk elements of a tensor: params_out = deq(codes)
// No atomics and no host round trip: min / max do not depend on the order they are folded in, everything else is elementwise.
// Spans start at arbitrary offsets: a chunk is walked as an unaligned scalar head (up to 3 elements), a body of 16-byte vectors and a
// scalar tail; the vector body is taken only where every array the kernel touches is 16-byte aligned at the same element.
#include "brief_quant.h"

static const int kQuantRangeChunk = 16384;                     // elements per workgroup of k_quant_minmax
static const int kQuantApplyChunk = 2048;                      // ... of k_quant_apply / k_quant_decode: two 16-byte vectors per thread
static const int kQuantMaxSegs = 2 * BRIEF_QUANT_MAX_TENSORS - 1;      // the spans in offset order and the gaps between them

struct QuantSegs {
    int64_t off[kQuantMaxSegs], cnt[kQuantMaxSegs];
    int32_t first_chunk[kQuantMaxSegs + 1];                    // chunk index of every segment's first chunk; [n]: chunks of the launch
    int16_t tensor[kQuantMaxSegs];                             // row of lo_step (the caller's tensor index); -1: a gap
    int32_t n;
};

// segment of chunk b: the last s with first_chunk[s] <= b
__device__ __forceinline__ int quant_seg_of(const QuantSegs &q, int b)
{
    int lo = 0, hi = q.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (q.first_chunk[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// elements in front of the first 16-byte boundary of p (p is 4-byte aligned), at most len
__device__ __forceinline__ int quant_head(const void *p, int len)
{
    const int h = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    return h < len ? h : len;
}

__global__ __launch_bounds__(256) void k_quant_minmax(const QuantSegs q, const float *__restrict__ params, float2 *__restrict__ partial)
{
    __shared__ float s_lo[4], s_hi[4];
    const int b = (int)blockIdx.x, s = quant_seg_of(q, b);
    const int64_t e0 = (int64_t)(b - q.first_chunk[s]) * kQuantRangeChunk;
    const int64_t left = q.cnt[s] - e0;
    const int len = (int)(left < kQuantRangeChunk ? left : kQuantRangeChunk);
    const float *p = params + q.off[s] + e0;
    const int head = quant_head(p, len), nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    const int tid = (int)threadIdx.x;
    float lo = p[0], hi = p[0];                                // (len >= 1: a span is never empty)
    if (tid < head) { const float v = p[tid]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    const float4 *pv = reinterpret_cast<const float4 *>(p + head);
    for (int i = tid; i < nvec; i += 256) {
        const float4 v = pv[i];
        lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    if (tail0 + tid < len) { const float v = p[tail0 + tid]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    for (int o = 32; o >= 1; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0)
        partial[b] = make_float2(fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])), fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])));
}

__global__ __launch_bounds__(64) void k_quant_fold(const QuantSegs q, const float2 *__restrict__ partial, int bits, float2 *__restrict__ lo_step)
{
    const int s = (int)blockIdx.x, c0 = q.first_chunk[s], c1 = q.first_chunk[s + 1];
    float lo = partial[c0].x, hi = partial[c0].y;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) { const float2 v = partial[c]; lo = fminf(lo, v.x); hi = fmaxf(hi, v.y); }
    for (int o = 32; o >= 1; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if (threadIdx.x == 0) lo_step[q.tensor[s]] = make_float2(lo, brief_quant_step(lo, hi, bits));
}

__device__ __forceinline__ void quant_one(float w, float lo, float step, float top, bool gap, float &dq, float &code)
{
    code = gap ? 0.f : brief_quant_code(w, lo, step, top);
    dq = gap ? w : brief_quant_deq(code, lo, step);
}

__global__ __launch_bounds__(256) void k_quant_apply(const QuantSegs q, const float *__restrict__ params, int bits, const float2 *__restrict__ lo_step,
                                                     float *__restrict__ qparams, uint16_t *__restrict__ codes)
{
    const int b = (int)blockIdx.x, s = quant_seg_of(q, b);
    const int64_t e0 = q.off[s] + (int64_t)(b - q.first_chunk[s]) * kQuantApplyChunk;
    const int64_t left = q.off[s] + q.cnt[s] - e0;
    const int len = (int)(left < kQuantApplyChunk ? left : kQuantApplyChunk);
    const int t = q.tensor[s];
    const bool gap = t < 0;
    if (gap && !qparams) return;                               // (a gap has no codes)
    const float2 ls = gap ? make_float2(0.f, 0.f) : lo_step[t];
    const float top = (float)((1 << bits) - 1);
    const float *p = params + e0;
    float *qp = qparams ? qparams + e0 : nullptr;
    uint16_t *cp = (codes && !gap) ? codes + e0 : nullptr;
    const int tid = (int)threadIdx.x;
    int head = quant_head(p, len);
    // the vector body needs qparams 16-byte aligned where params is; the four codes of a vector are 8 bytes
    const bool vec_ok = !qp || (((uintptr_t)(qp + head)) & 15) == 0;
    if (!vec_ok) head = len;
    const int nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    const bool code_vec = cp && (((uintptr_t)(cp + head)) & 7) == 0;
    for (int i = tid; i < head; i += 256) {
        float dq, cd;
        quant_one(p[i], ls.x, ls.y, top, gap, dq, cd);
        if (qp) qp[i] = dq;
        if (cp) cp[i] = (uint16_t)cd;
    }
    const float4 *pv = reinterpret_cast<const float4 *>(p + head);
    for (int i = tid; i < nvec; i += 256) {
        const float4 v = pv[i];
        float4 dq, cd;
        quant_one(v.x, ls.x, ls.y, top, gap, dq.x, cd.x);
        quant_one(v.y, ls.x, ls.y, top, gap, dq.y, cd.y);
        quant_one(v.z, ls.x, ls.y, top, gap, dq.z, cd.z);
        quant_one(v.w, ls.x, ls.y, top, gap, dq.w, cd.w);
        if (qp) reinterpret_cast<float4 *>(qp + head)[i] = dq;
        if (cp) {
            const uint32_t c01 = (uint32_t)cd.x | ((uint32_t)cd.y << 16), c23 = (uint32_t)cd.z | ((uint32_t)cd.w << 16);
            if (code_vec) reinterpret_cast<uint2 *>(cp + head)[i] = make_uint2(c01, c23);
            else {
                uint16_t *c4 = cp + head + 4 * i;
                c4[0] = (uint16_t)cd.x; c4[1] = (uint16_t)cd.y; c4[2] = (uint16_t)cd.z; c4[3] = (uint16_t)cd.w;
            }
        }
    }
    if (tail0 + tid < len) {                                   // (at most three elements)
        float dq, cd;
        quant_one(p[tail0 + tid], ls.x, ls.y, top, gap, dq, cd);
        if (qp) qp[tail0 + tid] = dq;
        if (cp) cp[tail0 + tid] = (uint16_t)cd;
    }
}

__global__ __launch_bounds__(256) void k_quant_decode(const QuantSegs q, const uint16_t *__restrict__ codes, const float2 *__restrict__ lo_step,
                                                      float *__restrict__ out)
{
    const int b = (int)blockIdx.x, s = quant_seg_of(q, b);
    const int64_t e0 = q.off[s] + (int64_t)(b - q.first_chunk[s]) * kQuantApplyChunk;
    const int64_t left = q.off[s] + q.cnt[s] - e0;
    const int len = (int)(left < kQuantApplyChunk ? left : kQuantApplyChunk);
    const float2 ls = lo_step[q.tensor[s]];
    const uint16_t *cp = codes + e0;
    float *op = out + e0;
    const int tid = (int)threadIdx.x;
    int head = quant_head(op, len);
    if ((((uintptr_t)(cp + head)) & 7) != 0) head = len;       // the four codes of an output vector are read as 8 bytes
    const int nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    for (int i = tid; i < head; i += 256) op[i] = brief_quant_deq((float)cp[i], ls.x, ls.y);
    for (int i = tid; i < nvec; i += 256) {
        const uint2 c = reinterpret_cast<const uint2 *>(cp + head)[i];
        float4 v;
        v.x = brief_quant_deq((float)(c.x & 0xffffu), ls.x, ls.y);
        v.y = brief_quant_deq((float)(c.x >> 16), ls.x, ls.y);
        v.z = brief_quant_deq((float)(c.y & 0xffffu), ls.x, ls.y);
        v.w = brief_quant_deq((float)(c.y >> 16), ls.x, ls.y);
        reinterpret_cast<float4 *>(op + head)[i] = v;
    }
    if (tail0 + tid < len) op[tail0 + tid] = brief_quant_deq((float)cp[tail0 + tid], ls.x, ls.y);
}
