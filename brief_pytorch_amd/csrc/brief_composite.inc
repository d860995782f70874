// brief_composite.inc — composite view: front-to-back emission-absorption rendering through a transfer table, k_composite_fold and
// k_composite_finish and their C-ABI entries brief_view_composite_* (part of the single translation unit brief_hip.hip, included at its
// very end: kernels and host code of a feature that touches no other kernel).  The arithmetic is csrc/brief_composite.h, compiled here
// for the device and for brief_view_composite_host alike; clip, scan, coordinates and the list layout are the view's (brief_view.inc).
//
//   k_composite_fold    k_view_fold's walk: a ray belongs to a group of G = 2^lg adjacent lanes, and in every PASS the group touches G
//                       consecutive samples of the ray-major list.  Per pass a lane loads its sample's value, looks (tau, eR, eG, eB) up,
//                       the group takes an inclusive scan of tau over its lanes (lg shuffles of width G), adds the ray's running carry
//                       to get the saturated exclusive prefix P_i, and adds W(P_i) * e_c to three uint64 sums of its own; the carry
//                       advances by the pass's total.  After the passes the sums are butterflied over the group and lane 0 does one
//                       plain read-modify-write of the pixel's state: tau_run[r] (the saturated running optical depth, which is also the
//                       carry-in of the ray's next chunk), acc[r][3] and hits[r].
//   k_composite_finish  the RGBA image from that state (brief_composite_pixel).
// No atomics: within a launch a pixel has one owner.  The chunks of a view follow the list's order on one stream, so the earlier part
// of a ray is always folded first and tau_run[r] is the prefix of everything before the chunk.  Every sum is an integer sum, and
// the prefix a sample gets depends on its place along the ray alone: the image does not depend on G, on the chunking or on the run.
//
// The table is read through the cache with plain 16-byte loads, whatever its size (4 KiB for a uint8 table, 64 KiB at the default
// b = 12 of uint16, 1 MiB at b = 16).  A copy of a small table in LDS, gathered there, was measured against this and bought nothing
// (profiles/r20_composite.md: 1.58 against 1.59 ms behind a 4x22 net, inside the spread), so there is one path.
//
// The composite of a partition follows these, and at the very end the SHADED composite (k_composite_select, k_composite_pick,
// k_composite_shade_fold and their entries): copies of the fold's structure that leave the kernels above as they are.
#include "brief_composite.h"

struct CompositeTable { int32_t channel, shift; };      // index = value[channel] >> shift: below 2^tf_bits for every value of the dtype
struct CompositeBg { int32_t c[3]; };

__device__ __forceinline__ unsigned long long composite_shfl_xor(unsigned long long x, int o)
{
    return (unsigned long long)__shfl_xor((long long)x, o);
}

// hits: int32 [rays], tau_run: int32 [rays], acc: uint64 [rays][3], all caller-initialised to 0
template <typename T>
__global__ __launch_bounds__(256) void k_composite_fold(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                        const T *__restrict__ vals, int C, CompositeTable tb, const int4 *__restrict__ tf,
                                                        int32_t *__restrict__ hits, int32_t *__restrict__ tau_run,
                                                        unsigned long long *__restrict__ acc)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        uint32_t carry = (uint32_t)tau_run[q.r];                     // (read by the whole group before its lane 0 writes it, below)
        int n = 0;
        unsigned long long m[3] = {0, 0, 0};
        for (int64_t sb = q.lo; sb < q.hi; sb += G) {                // a pass; q.lo and q.hi are the group's: its lanes stay together
            const int64_t s = sb + sub;
            int4 e = make_int4(0, 0, 0, 0);
            if (s < q.hi) {
                const int32_t k = kb + (int32_t)(s - q.a);
                if (brief_view_inside(v, brief_view_at(v, 0, q.base[0], k), brief_view_at(v, 1, q.base[1], k), brief_view_at(v, 2, q.base[2], k))) {
                    ++n;
                    e = tf[(int)vals[(s - ch.s0) * C + tb.channel] >> tb.shift];
                }
            }
            uint32_t incl = (uint32_t)e.x;                           // at most G * TAU_SAT <= 2^27: no overflow before the saturation
            for (int o = 1; o < G; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, G);
                if (sub >= o) incl += y;
            }
            const unsigned long long w = brief_composite_w(brief_composite_add(carry, incl - (uint32_t)e.x));
            m[0] += w * (unsigned long long)(uint32_t)e.y;
            m[1] += w * (unsigned long long)(uint32_t)e.z;
            m[2] += w * (unsigned long long)(uint32_t)e.w;
            carry = brief_composite_add(carry, (uint32_t)__shfl((int)incl, G - 1, G));
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] += composite_shfl_xor(m[c], o);
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner
            hits[q.r] += n;
            tau_run[q.r] = (int32_t)carry;
            unsigned long long *d = acc + q.r * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += m[c];
        }
    }
}

__global__ __launch_bounds__(256) void k_composite_finish(int64_t rays, CompositeBg bg, const int32_t *__restrict__ tau_run,
                                                          const unsigned long long *__restrict__ acc, uchar4 *__restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t a[3] = {acc[r * 3], acc[r * 3 + 1], acc[r * 3 + 2]};
        uint8_t px[4];
        brief_composite_pixel((uint32_t)tau_run[r], a, bg.c, px);
        out[r] = make_uchar4(px[0], px[1], px[2], px[3]);
    }
}

// ---- host side
static int check_composite_table(int elem_kind, int32_t channels, int32_t channel, const void *tf, int32_t tf_bits, CompositeTable *tb)
{
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "composite: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "composite: channels must be 1..4");
    if (channel < 0 || channel >= channels) return fail(BRIEF_ERR_INVALID, "composite: channel must be 0 .. channels - 1");
    if (!tf) return fail(BRIEF_ERR_INVALID, "composite: null transfer table");
    if ((uintptr_t)tf & 15) return fail(BRIEF_ERR_INVALID, "composite: the transfer table must be 16-byte aligned (an entry is read as one int4)");
    const int bits = elem_kind == BRIEF_OUT_U8 ? 8 : 16;
    if (tf_bits < 1 || tf_bits > bits) return fail(BRIEF_ERR_INVALID, "composite: tf_bits must be 1 .. 8 for uint8 and 1 .. 16 for uint16");
    tb->channel = channel; tb->shift = bits - tf_bits;
    return 0;
}

static int check_composite_bg(const int32_t *background, CompositeBg *bg)
{
    if (!background) return fail(BRIEF_ERR_INVALID, "composite: null background");
    for (int c = 0; c < 3; ++c) {
        if (background[c] < 0 || background[c] > 255) return fail(BRIEF_ERR_INVALID, "composite: background must be 0 .. 255 per channel");
        bg->c[c] = background[c];
    }
    return 0;
}

extern "C" {

int brief_view_composite_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                              int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                              int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream)
{
    ViewChunk ch;
    CompositeTable tb;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !hits || !tau_run || !acc) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define COMPOSITE_FOLD(T) hipLaunchKernelGGL((k_composite_fold<T>), grid, block, 0, st, *view, ch, k0, off, (const T *)vals, (int)channels, tb, \
                                             (const int4 *)tf, hits, tau_run, (unsigned long long *)acc)
    if (elem_kind == BRIEF_OUT_U8) COMPOSITE_FOLD(uint8_t); else COMPOSITE_FOLD(uint16_t);
#undef COMPOSITE_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_composite_finish(const brief_view_desc *view, const int32_t *background, const int32_t *hits, const int32_t *tau_run, const uint64_t *acc,
                                uint8_t *out, void *stream)
{
    CompositeBg bg;
    if (int rc = check_view(view)) return rc;
    if (!hits || !tau_run || !acc || !out) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if ((uintptr_t)out & 3) return fail(BRIEF_ERR_INVALID, "composite: the image must be 4-byte aligned (a pixel is written as one uchar4)");
    if (int rc = check_composite_bg(background, &bg)) return rc;
    const int64_t rays = (int64_t)view->rows * view->cols;
    if (rays > kViewMaxRays) return fail(BRIEF_ERR_INVALID, "view: more than 2^40 rays");
    hipLaunchKernelGGL(k_composite_finish, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, rays, bg, tau_run,
                       (const unsigned long long *)acc, (uchar4 *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same fold and finish on the host CPU, sample after sample: no GPU call.  Every buffer is host memory; vals holds the WHOLE list.
int brief_view_composite_host(const brief_view_desc *view, const int32_t *k0, const int64_t *off, const void *vals, int elem_kind, int32_t channels,
                              int32_t channel, const int32_t *tf, int32_t tf_bits, const int32_t *background, int32_t *hits, int32_t *tau_run,
                              uint64_t *acc, uint8_t *out)
{
    CompositeTable tb;
    CompositeBg bg;
    if (int rc = check_view(view)) return rc;
    if (!k0 || !off || !vals || !out) return fail(BRIEF_ERR_INVALID, "composite: null buffer (hits, tau_run and acc alone may be NULL)");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    if (int rc = check_composite_bg(background, &bg)) return rc;
    for (int32_t i = 0; i < (int32_t)1 << tf_bits; ++i) {
        const int32_t *e = tf + 4 * (int64_t)i;
        if (e[0] < 0 || e[0] > BRIEF_COMPOSITE_TAU_SAT) return fail(BRIEF_ERR_INVALID, "composite: a table entry's tau lies outside 0 .. TAU_SAT (32 * 65536)");
        for (int c = 1; c < 4; ++c)
            if (e[c] < 0 || e[c] > BRIEF_COMPOSITE_E_MAX) return fail(BRIEF_ERR_INVALID, "composite: a table entry's emission lies outside 0 .. 65280");
    }
    const int64_t rays = (int64_t)view->rows * view->cols;
    if (off[0] != 0) return fail(BRIEF_ERR_INVALID, "composite: off[0] must be 0 (vals holds the whole list)");
    for (int64_t r = 0; r < rays; ++r) {
        const int64_t cnt = off[r + 1] - off[r];
        if (cnt < 0 || k0[r] < 0 || cnt > (int64_t)view->depth - k0[r])
            return fail(BRIEF_ERR_INVALID, "composite: off must not decrease, and a ray's samples k0 .. k0 + cnt - 1 must lie inside 0 .. depth - 1");
    }
    for (int64_t r = 0; r < rays; ++r) {
        const int32_t row = (int32_t)(r / view->cols), col = (int32_t)(r - (int64_t)row * view->cols);
        float base[3];
        for (int a = 0; a < 3; ++a) base[a] = brief_view_base(*view, a, row, col);
        uint32_t run = 0;
        uint64_t sum[3] = {0, 0, 0};
        int32_t n = 0;
        for (int64_t s = off[r]; s < off[r + 1]; ++s) {
            const int32_t k = k0[r] + (int32_t)(s - off[r]);
            if (!brief_view_inside(*view, brief_view_at(*view, 0, base[0], k), brief_view_at(*view, 1, base[1], k), brief_view_at(*view, 2, base[2], k)))
                continue;
            ++n;
            const int64_t at = s * channels + channel;
            const int value = elem_kind == BRIEF_OUT_U8 ? (int)((const uint8_t *)vals)[at] : (int)((const uint16_t *)vals)[at];
            const int32_t *e = tf + 4 * (int64_t)(value >> tb.shift);
            const uint64_t w = brief_composite_w(run);
            for (int c = 0; c < 3; ++c) sum[c] += w * (uint64_t)e[1 + c];
            run = brief_composite_add(run, (uint32_t)e[0]);
        }
        if (hits) hits[r] = n;
        if (tau_run) tau_run[r] = (int32_t)run;
        if (acc)
            for (int c = 0; c < 3; ++c) acc[r * 3 + c] = sum[c];
        brief_composite_pixel(run, sum, bg.c, out + r * 4);
    }
    return 0;
}

}   // extern "C"

// ---- composite view of a partition: the prefix is carried across blocks (csrc/brief_composite.h "the composite of a PARTITION";
// composite.render_composite_partition; DESIGN.md "Composite view of a partition").
//   k_composite_part_fold    k_composite_fold on one block's list: view_part_ray's walk and k_view_part_fold's exact test (clip box and
//                            cell).  Its state is indexed by WINDOW ray within the block's slice: hits_w, tau_w (carry-in and carry-out)
//                            and acc_w[3].  Pass A runs it on zeroed state, pass B over the second-pass counts with tau_w preloaded with C.
//   k_composite_part_carry   one thread per window ray of all blocks: C and cnt2 (brief_composite_carry), a loop over the table of windows.
//   k_composite_part_gather  one thread per pixel: the pixel's hits, tau_run and acc from its segments (brief_composite_gather).
// No atomics: a window ray has one owner in a launch, and the chunks of a block follow each other on one stream.
template <typename T>
__global__ __launch_bounds__(256) void k_composite_part_fold(brief_view_desc v, brief_view_part pt, ViewChunk ch, const int32_t *__restrict__ k0,
                                                             const int64_t *__restrict__ off, const T *__restrict__ vals, int C, CompositeTable tb,
                                                             const int4 *__restrict__ tf, int32_t *__restrict__ hits_w, int32_t *__restrict__ tau_w,
                                                             unsigned long long *__restrict__ acc_w)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_part_ray(v, pt, ch, off, g).q;
        const int32_t kb = k0[q.r];
        uint32_t carry = (uint32_t)tau_w[q.r];                       // (read by the whole group before its lane 0 writes it, below)
        int n = 0;
        unsigned long long m[3] = {0, 0, 0};
        for (int64_t sb = q.lo; sb < q.hi; sb += G) {                // a pass; q.lo and q.hi are the group's: its lanes stay together
            const int64_t s = sb + sub;
            int4 e = make_int4(0, 0, 0, 0);
            if (s < q.hi) {
                const int32_t k = kb + (int32_t)(s - q.a);
                const float p0 = brief_view_at(v, 0, q.base[0], k), p1 = brief_view_at(v, 1, q.base[1], k), p2 = brief_view_at(v, 2, q.base[2], k);
                if (brief_view_inside(v, p0, p1, p2) && brief_view_part_owned(pt, p0, p1, p2)) {
                    ++n;
                    e = tf[(int)vals[(s - ch.s0) * C + tb.channel] >> tb.shift];
                }
            }
            uint32_t incl = (uint32_t)e.x;                           // at most G * TAU_SAT <= 2^27: no overflow before the saturation
            for (int o = 1; o < G; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, G);
                if (sub >= o) incl += y;
            }
            const unsigned long long w = brief_composite_w(brief_composite_add(carry, incl - (uint32_t)e.x));
            m[0] += w * (unsigned long long)(uint32_t)e.y;
            m[1] += w * (unsigned long long)(uint32_t)e.z;
            m[2] += w * (unsigned long long)(uint32_t)e.w;
            carry = brief_composite_add(carry, (uint32_t)__shfl((int)incl, G - 1, G));
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] += composite_shfl_xor(m[c], o);
        }
        if (sub == 0 && n > 0) {                                     // the window ray's owner
            if (hits_w) hits_w[q.r] += n;
            tau_w[q.r] = (int32_t)carry;
            unsigned long long *d = acc_w + q.r * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += m[c];
        }
    }
}

struct CompositeWins { const brief_composite_window *wins; int32_t blocks; int64_t window_rays; };

__global__ __launch_bounds__(256) void k_composite_part_carry(CompositeWins t, const int32_t *__restrict__ k0, const int32_t *__restrict__ cnt,
                                                              const int32_t *__restrict__ tau_w, int32_t *__restrict__ carry, int32_t *__restrict__ cnt2)
{
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < t.window_rays; w += (int64_t)gridDim.x * blockDim.x) {
        int32_t c, n;
        brief_composite_carry(t.wins, t.blocks, k0, cnt, tau_w, w, c, n);
        carry[w] = c;
        cnt2[w] = n;
    }
}

__global__ __launch_bounds__(256) void k_composite_part_gather(int32_t cols, int64_t rays, CompositeWins t, const int32_t *__restrict__ hits_w,
                                                               const int32_t *__restrict__ tau_w, const unsigned long long *__restrict__ acc_w,
                                                               const int32_t *__restrict__ carry, const unsigned long long *__restrict__ acc_w2,
                                                               int32_t *__restrict__ hits, int32_t *__restrict__ tau_run,
                                                               unsigned long long *__restrict__ acc)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = (int32_t)(r / cols), col = (int32_t)(r - (int64_t)row * cols);
        int32_t n;
        uint32_t run;
        uint64_t a[3];
        brief_composite_gather(t.wins, t.blocks, row, col, hits_w, tau_w, (const uint64_t *)acc_w, carry, (const uint64_t *)acc_w2, n, run, a);
        hits[r] = n;
        tau_run[r] = (int32_t)run;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r * 3 + c] = a[c];
    }
}

// ---- host side of the partition entries
static const int64_t kCompositeMaxWindowRays = (int64_t)1 << 46;      // 2^40 rays of up to 2^6 blocks each and more: far above any memory

static int check_composite_wins(const brief_view_desc *view, const void *wins, int32_t blocks, int64_t window_rays, int64_t *rays)
{
    if (int rc = check_view(view)) return rc;
    *rays = (int64_t)view->rows * view->cols;
    if (*rays > kViewMaxRays) return fail(BRIEF_ERR_INVALID, "view: more than 2^40 rays");
    if (!wins) return fail(BRIEF_ERR_INVALID, "composite: null table of windows");
    if (blocks < 1) return fail(BRIEF_ERR_INVALID, "composite: blocks must be >= 1");
    if (window_rays < 1 || window_rays > kCompositeMaxWindowRays) return fail(BRIEF_ERR_INVALID, "composite: window_rays must be 1 .. 2^46");
    return 0;
}

// the table itself, where it is host memory
static int check_composite_wins_host(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays)
{
    int64_t at = 0;
    for (int32_t b = 0; b < blocks; ++b) {
        const brief_composite_window &w = wins[b];
        if (w.base != at) return fail(BRIEF_ERR_INVALID, "composite: the windows' bases must be 0 and then each the end of the slice before");
        if (w.wrows < 0 || w.wcols < 0 || (w.wrows == 0) != (w.wcols == 0))
            return fail(BRIEF_ERR_INVALID, "composite: a window must be at least 1 x 1, or 0 x 0 where the block meets no ray");
        if (w.wrows > 0 && (w.row0 < 0 || w.col0 < 0 || w.row0 > view->rows - w.wrows || w.col0 > view->cols - w.wcols))
            return fail(BRIEF_ERR_INVALID, "composite: a block's window must lie inside the image rows x cols");
        at += (int64_t)w.wrows * w.wcols;
    }
    if (at != window_rays) return fail(BRIEF_ERR_INVALID, "composite: the windows must hold window_rays rays together");
    return 0;
}

extern "C" {

int brief_view_composite_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0,
                                   int64_t s1, int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels,
                                   int32_t channel, const int32_t *tf, int32_t tf_bits, int32_t *hits_w, int32_t *tau_w, uint64_t *acc_w,
                                   void *stream)
{
    ViewChunk ch;
    CompositeTable tb;
    if (int rc = check_view_part_chunk(view, part, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !tau_w || !acc_w) return fail(BRIEF_ERR_INVALID, "composite: null buffer (hits_w alone may be NULL)");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define COMPOSITE_PART_FOLD(T) hipLaunchKernelGGL((k_composite_part_fold<T>), grid, block, 0, st, *view, *part, ch, k0, off, (const T *)vals, \
                                                  (int)channels, tb, (const int4 *)tf, hits_w, tau_w, (unsigned long long *)acc_w)
    if (elem_kind == BRIEF_OUT_U8) COMPOSITE_PART_FOLD(uint8_t); else COMPOSITE_PART_FOLD(uint16_t);
#undef COMPOSITE_PART_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_composite_part_carry(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                    const int32_t *k0, const int32_t *cnt, const int32_t *tau_w, int32_t *carry, int32_t *cnt2, void *stream)
{
    int64_t rays;
    if (int rc = check_composite_wins(view, wins, blocks, window_rays, &rays)) return rc;
    if (!k0 || !cnt || !tau_w || !carry || !cnt2) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    const CompositeWins t = {wins, blocks, window_rays};
    hipLaunchKernelGGL(k_composite_part_carry, dim3(view_blocks(window_rays)), dim3(256), 0, (hipStream_t)stream, t, k0, cnt, tau_w, carry, cnt2);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_composite_part_gather(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                     const int32_t *hits_w, const int32_t *tau_w, const uint64_t *acc_w, const int32_t *carry,
                                     const uint64_t *acc_w2, int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream)
{
    int64_t rays;
    if (int rc = check_composite_wins(view, wins, blocks, window_rays, &rays)) return rc;
    if (!hits_w || !tau_w || !acc_w || !carry || !acc_w2 || !hits || !tau_run || !acc) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    const CompositeWins t = {wins, blocks, window_rays};
    hipLaunchKernelGGL(k_composite_part_gather, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, view->cols, rays, t, hits_w, tau_w,
                       (const unsigned long long *)acc_w, carry, (const unsigned long long *)acc_w2, hits, tau_run, (unsigned long long *)acc);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same fold on the host CPU, sample after sample: no GPU call.  Every buffer is host memory; off has wrows * wcols + 1 entries in
// any numbering (a slice of one scan over all blocks), vals holds the block's WHOLE list, sample s at s - off[0].
int brief_view_composite_part_fold_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off,
                                        const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                                        int32_t *hits_w, int32_t *tau_w, uint64_t *acc_w)
{
    CompositeTable tb;
    if (int rc = check_view_part(view, part)) return rc;
    if (!k0 || !off || !vals || !tau_w || !acc_w) return fail(BRIEF_ERR_INVALID, "composite: null buffer (hits_w alone may be NULL)");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    const int64_t wrays = (int64_t)part->wrows * part->wcols;
    for (int64_t r = 0; r < wrays; ++r) {
        const int64_t cnt = off[r + 1] - off[r];
        if (cnt < 0 || k0[r] < 0 || cnt > (int64_t)view->depth - k0[r])
            return fail(BRIEF_ERR_INVALID, "composite: off must not decrease, and a ray's samples k0 .. k0 + cnt - 1 must lie inside 0 .. depth - 1");
        if (tau_w[r] < 0 || tau_w[r] > BRIEF_COMPOSITE_TAU_SAT) return fail(BRIEF_ERR_INVALID, "composite: a carry-in tau_w lies outside 0 .. TAU_SAT (32 * 65536)");
    }
    for (int64_t r = 0; r < wrays; ++r) {
        const int32_t wr = (int32_t)(r / part->wcols);
        const int32_t row = part->row0 + wr, col = part->col0 + (int32_t)(r - (int64_t)wr * part->wcols);
        float base[3];
        for (int a = 0; a < 3; ++a) base[a] = brief_view_base(*view, a, row, col);
        uint32_t run = (uint32_t)tau_w[r];
        uint64_t sum[3] = {0, 0, 0};
        int32_t n = 0;
        for (int64_t s = off[r]; s < off[r + 1]; ++s) {
            const int32_t k = k0[r] + (int32_t)(s - off[r]);
            const float p0 = brief_view_at(*view, 0, base[0], k), p1 = brief_view_at(*view, 1, base[1], k), p2 = brief_view_at(*view, 2, base[2], k);
            if (!(brief_view_inside(*view, p0, p1, p2) && brief_view_part_owned(*part, p0, p1, p2))) continue;
            ++n;
            const int64_t at = (s - off[0]) * channels + channel;
            const int value = elem_kind == BRIEF_OUT_U8 ? (int)((const uint8_t *)vals)[at] : (int)((const uint16_t *)vals)[at];
            const int32_t *e = tf + 4 * (int64_t)(value >> tb.shift);
            const uint64_t w = brief_composite_w(run);
            for (int c = 0; c < 3; ++c) sum[c] += w * (uint64_t)(uint32_t)e[1 + c];
            run = brief_composite_add(run, (uint32_t)e[0]);
        }
        if (n > 0) {
            if (hits_w) hits_w[r] += n;
            tau_w[r] = (int32_t)run;
            for (int c = 0; c < 3; ++c) acc_w[r * 3 + c] += sum[c];
        }
    }
    return 0;
}

int brief_view_composite_part_carry_host(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                         const int32_t *k0, const int32_t *cnt, const int32_t *tau_w, int32_t *carry, int32_t *cnt2)
{
    int64_t rays;
    if (int rc = check_composite_wins(view, wins, blocks, window_rays, &rays)) return rc;
    if (!k0 || !cnt || !tau_w || !carry || !cnt2) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (int rc = check_composite_wins_host(view, wins, blocks, window_rays)) return rc;
    for (int64_t w = 0; w < window_rays; ++w) brief_composite_carry(wins, blocks, k0, cnt, tau_w, w, carry[w], cnt2[w]);
    return 0;
}

int brief_view_composite_part_gather_host(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                          const int32_t *hits_w, const int32_t *tau_w, const uint64_t *acc_w, const int32_t *carry,
                                          const uint64_t *acc_w2, int32_t *hits, int32_t *tau_run, uint64_t *acc)
{
    int64_t rays;
    if (int rc = check_composite_wins(view, wins, blocks, window_rays, &rays)) return rc;
    if (!hits_w || !tau_w || !acc_w || !carry || !acc_w2 || !hits || !tau_run || !acc) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (int rc = check_composite_wins_host(view, wins, blocks, window_rays)) return rc;
    for (int64_t r = 0; r < rays; ++r) {
        const int32_t row = (int32_t)(r / view->cols), col = (int32_t)(r - (int64_t)row * view->cols);
        uint32_t run;
        brief_composite_gather(wins, blocks, row, col, hits_w, tau_w, acc_w, carry, acc_w2, hits[r], run, acc + r * 3);
        tau_run[r] = (int32_t)run;
    }
    return 0;
}

}   // extern "C"

// ---- shaded composite: every sample's emission lit by the net's analytic gradient (csrc/brief_composite.h "SHADED composite";
// composite.render_composite with shade; DESIGN.md "Shaded composite").
//   k_composite_select      k_composite_fold's walk, lookup and scan with the ray's carry read from tau_run[r]: need[s - s0] = the sample
//                           is inside, emits and its prefix is below TAU_SAT (brief_composite_need).  It writes nothing else.
//   k_composite_pick        coords_sel[slot[i]] = coords[i] where need[i]: the needed samples, in the list's order.
//   k_composite_shade_fold  k_composite_fold with e scaled by s_q (brief_composite_shade_q of the sample's Jacobian row, read only where
//                           need is 1: at slot[s - s0], or at s - s0 for a dense jac).  A sample that needs no gradient adds 0 as it is.
// The kernels are copies of the fold's structure: the plain fold stays as it was.
template <typename T>
__global__ __launch_bounds__(256) void k_composite_select(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                          const T *__restrict__ vals, int C, CompositeTable tb, const int4 *__restrict__ tf,
                                                          const int32_t *__restrict__ tau_run, int32_t *__restrict__ need)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the scan below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        uint32_t carry = (uint32_t)tau_run[q.r];
        for (int64_t sb = q.lo; sb < q.hi; sb += G) {                // a pass; q.lo and q.hi are the group's: its lanes stay together
            const int64_t s = sb + sub;
            int4 e = make_int4(0, 0, 0, 0);
            bool inside = false;
            if (s < q.hi) {
                const int32_t k = kb + (int32_t)(s - q.a);
                inside = brief_view_inside(v, brief_view_at(v, 0, q.base[0], k), brief_view_at(v, 1, q.base[1], k), brief_view_at(v, 2, q.base[2], k));
                if (inside) e = tf[(int)vals[(s - ch.s0) * C + tb.channel] >> tb.shift];
            }
            uint32_t incl = (uint32_t)e.x;                           // at most G * TAU_SAT <= 2^27: no overflow before the saturation
            for (int o = 1; o < G; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, G);
                if (sub >= o) incl += y;
            }
            const uint32_t prefix = brief_composite_add(carry, incl - (uint32_t)e.x);
            if (s < q.hi) need[s - ch.s0] = brief_composite_need(inside, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w, prefix) ? 1 : 0;
            carry = brief_composite_add(carry, (uint32_t)__shfl((int)incl, G - 1, G));
        }
    }
}

__global__ __launch_bounds__(256) void k_composite_pick(int64_t n, const int32_t *__restrict__ need, const int64_t *__restrict__ slot,
                                                        const float *__restrict__ coords, float *__restrict__ coords_sel)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!need[i]) continue;
        const int64_t at = slot[i];
        if (at < 0 || at >= n) continue;                             // (a scan of need never gives one)
#pragma unroll
        for (int a = 0; a < 3; ++a) coords_sel[at * 3 + a] = coords[i * 3 + a];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_composite_shade_fold(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                              const T *__restrict__ vals, int C, CompositeTable tb, const int4 *__restrict__ tf,
                                                              const int32_t *__restrict__ need, const int64_t *__restrict__ slot,
                                                              const float *__restrict__ jac, brief_composite_shade sh,
                                                              int32_t *__restrict__ hits, int32_t *__restrict__ tau_run,
                                                              unsigned long long *__restrict__ acc)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        uint32_t carry = (uint32_t)tau_run[q.r];                     // (read by the whole group before its lane 0 writes it, below)
        int n = 0;
        unsigned long long m[3] = {0, 0, 0};
        for (int64_t sb = q.lo; sb < q.hi; sb += G) {                // a pass; q.lo and q.hi are the group's: its lanes stay together
            const int64_t s = sb + sub;
            int4 e = make_int4(0, 0, 0, 0);
            if (s < q.hi) {
                const int32_t k = kb + (int32_t)(s - q.a);
                if (brief_view_inside(v, brief_view_at(v, 0, q.base[0], k), brief_view_at(v, 1, q.base[1], k), brief_view_at(v, 2, q.base[2], k))) {
                    ++n;
                    e = tf[(int)vals[(s - ch.s0) * C + tb.channel] >> tb.shift];
                    if (need[s - ch.s0]) {                           // the only samples whose emission reaches the pixel
                        const int64_t row = slot ? slot[s - ch.s0] : s - ch.s0;
                        const float *jp = jac + (row * C + tb.channel) * 3;
                        const float j[3] = {jp[0], jp[1], jp[2]};
                        const int32_t s_q = brief_composite_shade_q(j, sh.gscale, sh.light, sh.ka_q, sh.kd_q);
                        e.y = (int)brief_composite_lit((uint32_t)e.y, s_q);
                        e.z = (int)brief_composite_lit((uint32_t)e.z, s_q);
                        e.w = (int)brief_composite_lit((uint32_t)e.w, s_q);
                    }
                }
            }
            uint32_t incl = (uint32_t)e.x;                           // at most G * TAU_SAT <= 2^27: no overflow before the saturation
            for (int o = 1; o < G; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, G);
                if (sub >= o) incl += y;
            }
            const unsigned long long w = brief_composite_w(brief_composite_add(carry, incl - (uint32_t)e.x));
            m[0] += w * (unsigned long long)(uint32_t)e.y;
            m[1] += w * (unsigned long long)(uint32_t)e.z;
            m[2] += w * (unsigned long long)(uint32_t)e.w;
            carry = brief_composite_add(carry, (uint32_t)__shfl((int)incl, G - 1, G));
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] += composite_shfl_xor(m[c], o);
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner
            hits[q.r] += n;
            tau_run[q.r] = (int32_t)carry;
            unsigned long long *d = acc + q.r * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += m[c];
        }
    }
}

// ---- host side of the shaded entries
static int check_composite_shade(const brief_composite_shade *sh)
{
    if (!sh) return fail(BRIEF_ERR_INVALID, "composite: null shade descriptor");
    if (sh->ka_q < 0 || sh->ka_q > 256 || sh->kd_q < 0 || sh->kd_q > 256)
        return fail(BRIEF_ERR_INVALID, "composite: ka_q and kd_q must be 0 .. 256 (round(256 * KA), round(256 * KD) of KA, KD in [0, 1])");
    for (int a = 0; a < 3; ++a)
        if (sh->gscale[a] - sh->gscale[a] != 0.f || sh->light[a] - sh->light[a] != 0.f)
            return fail(BRIEF_ERR_INVALID, "composite: gscale and light must be finite");
    return 0;
}

extern "C" {

int brief_view_composite_select(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                                int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                                const int32_t *tau_run, int32_t *need, void *stream)
{
    ViewChunk ch;
    CompositeTable tb;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !tau_run || !need) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define COMPOSITE_SELECT(T) hipLaunchKernelGGL((k_composite_select<T>), grid, block, 0, st, *view, ch, k0, off, (const T *)vals, (int)channels, tb, \
                                               (const int4 *)tf, tau_run, need)
    if (elem_kind == BRIEF_OUT_U8) COMPOSITE_SELECT(uint8_t); else COMPOSITE_SELECT(uint16_t);
#undef COMPOSITE_SELECT
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_composite_pick(const int32_t *need, const int64_t *slot, const float *coords, int64_t n, float *coords_sel, void *stream)
{
    if (!need || !slot || !coords || !coords_sel) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (n < 1) return fail(BRIEF_ERR_INVALID, "composite: n must be >= 1");
    hipLaunchKernelGGL(k_composite_pick, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, need, slot, coords, coords_sel);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_composite_shade_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0,
                                    int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel,
                                    const int32_t *tf, int32_t tf_bits, const int32_t *need, const int64_t *slot, const float *jac,
                                    const brief_composite_shade *shade, int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream)
{
    ViewChunk ch;
    CompositeTable tb;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !need || !jac || !hits || !tau_run || !acc) return fail(BRIEF_ERR_INVALID, "composite: null buffer (slot alone may be NULL: a dense jac)");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    if (int rc = check_composite_shade(shade)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define COMPOSITE_SHADE_FOLD(T) hipLaunchKernelGGL((k_composite_shade_fold<T>), grid, block, 0, st, *view, ch, k0, off, (const T *)vals, (int)channels, tb, \
                                                   (const int4 *)tf, need, slot, jac, *shade, hits, tau_run, (unsigned long long *)acc)
    if (elem_kind == BRIEF_OUT_U8) COMPOSITE_SHADE_FOLD(uint8_t); else COMPOSITE_SHADE_FOLD(uint16_t);
#undef COMPOSITE_SHADE_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

// select, shade_fold and finish on the host CPU, sample after sample: no GPU call.  Every buffer is host memory; vals and the dense jac
// hold the WHOLE list.
int brief_view_composite_shade_host(const brief_view_desc *view, const int32_t *k0, const int64_t *off, const void *vals, int elem_kind,
                                    int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits, const int32_t *background,
                                    const float *jac, const brief_composite_shade *shade, int32_t *need, int32_t *hits, int32_t *tau_run,
                                    uint64_t *acc, uint8_t *out)
{
    CompositeTable tb;
    CompositeBg bg;
    if (int rc = check_view(view)) return rc;
    if (!k0 || !off || !vals || !jac || !out) return fail(BRIEF_ERR_INVALID, "composite: null buffer (need, hits, tau_run and acc alone may be NULL)");
    if (int rc = check_composite_table(elem_kind, channels, channel, tf, tf_bits, &tb)) return rc;
    if (int rc = check_composite_bg(background, &bg)) return rc;
    if (int rc = check_composite_shade(shade)) return rc;
    for (int32_t i = 0; i < (int32_t)1 << tf_bits; ++i) {
        const int32_t *e = tf + 4 * (int64_t)i;
        if (e[0] < 0 || e[0] > BRIEF_COMPOSITE_TAU_SAT) return fail(BRIEF_ERR_INVALID, "composite: a table entry's tau lies outside 0 .. TAU_SAT (32 * 65536)");
        for (int c = 1; c < 4; ++c)
            if (e[c] < 0 || e[c] > BRIEF_COMPOSITE_E_MAX) return fail(BRIEF_ERR_INVALID, "composite: a table entry's emission lies outside 0 .. 65280");
    }
    const int64_t rays = (int64_t)view->rows * view->cols;
    if (off[0] != 0) return fail(BRIEF_ERR_INVALID, "composite: off[0] must be 0 (vals and jac hold the whole list)");
    for (int64_t r = 0; r < rays; ++r) {
        const int64_t cnt = off[r + 1] - off[r];
        if (cnt < 0 || k0[r] < 0 || cnt > (int64_t)view->depth - k0[r])
            return fail(BRIEF_ERR_INVALID, "composite: off must not decrease, and a ray's samples k0 .. k0 + cnt - 1 must lie inside 0 .. depth - 1");
    }
    for (int64_t r = 0; r < rays; ++r) {
        const int32_t row = (int32_t)(r / view->cols), col = (int32_t)(r - (int64_t)row * view->cols);
        float base[3];
        for (int a = 0; a < 3; ++a) base[a] = brief_view_base(*view, a, row, col);
        uint32_t run = 0;
        uint64_t sum[3] = {0, 0, 0};
        int32_t n = 0;
        for (int64_t s = off[r]; s < off[r + 1]; ++s) {
            const int32_t k = k0[r] + (int32_t)(s - off[r]);
            if (need) need[s] = 0;
            if (!brief_view_inside(*view, brief_view_at(*view, 0, base[0], k), brief_view_at(*view, 1, base[1], k), brief_view_at(*view, 2, base[2], k)))
                continue;
            ++n;
            const int64_t at = s * channels + channel;
            const int value = elem_kind == BRIEF_OUT_U8 ? (int)((const uint8_t *)vals)[at] : (int)((const uint16_t *)vals)[at];
            const int32_t *e = tf + 4 * (int64_t)(value >> tb.shift);
            if (brief_composite_need(true, (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3], run)) {
                if (need) need[s] = 1;
                const int32_t s_q = brief_composite_shade_q(jac + at * 3, shade->gscale, shade->light, shade->ka_q, shade->kd_q);
                const uint64_t w = brief_composite_w(run);
                for (int c = 0; c < 3; ++c) sum[c] += w * (uint64_t)brief_composite_lit((uint32_t)e[1 + c], s_q);
            }
            run = brief_composite_add(run, (uint32_t)e[0]);
        }
        if (hits) hits[r] = n;
        if (tau_run) tau_run[r] = (int32_t)run;
        if (acc)
            for (int c = 0; c < 3; ++c) acc[r * 3 + c] = sum[c];
        brief_composite_pixel(run, sum, bg.c, out + r * 4);
    }
    return 0;
}

int brief_composite_shade_q_host(const float *jac, int64_t n, const brief_composite_shade *shade, int32_t *s_q)
{
    if (!jac || !s_q) return fail(BRIEF_ERR_INVALID, "composite: null buffer");
    if (n < 1) return fail(BRIEF_ERR_INVALID, "composite: n must be >= 1");
    if (int rc = check_composite_shade(shade)) return rc;
    for (int64_t i = 0; i < n; ++i) s_q[i] = brief_composite_shade_q(jac + i * 3, shade->gscale, shade->light, shade->ka_q, shade->kd_q);
    return 0;
}

}   // extern "C"
