// brief_view.inc — orthographic view decode: k_view_clip, k_view_coords, k_view_fold, k_view_finish and their C-ABI entries brief_view_*
// (part of the single translation unit brief_hip.hip, included at its very end: kernels and host code of a feature that touches no
// other kernel); behind them k_view_part_clip / _coords / _fold, the same for one block of a partition, and the surface view.  The geometry is csrc/brief_view.h, compiled here for the device and for the host entries alike.
//
// A view is rows x cols rays of `depth` samples each.  The net is evaluated by its own forward entry on explicit coordinates; these
// kernels only say WHERE (clip, coords) and reduce WHAT came back (fold, finish):
//   k_view_clip    one thread per ray: the interval [k0, k0 + cnt) of its samples inside the clip box (brief_view_ray_range).
//   (caller)       off = exclusive scan of cnt (int64, rays + 1 entries): the COMPACTED SAMPLE LIST.
//   k_view_coords  the [n][3] fp32 coordinates of the samples [s0, s1) of that list.
//   (caller)       the net's forward entry on those coordinates, integer output kind: vals [n][C] uint8 / uint16.
//   k_view_fold    reduces vals into the per-pixel accumulators; k_view_finish writes the image.
//
// Layout of the compacted list: RAY-MAJOR, a ray's samples contiguous and ascending in k — sample off[r] + j is (row, col, k0[r] + j)
// with r = row * cols + col.  Rays that are neighbours in the image are neighbours in the list.  Both kernels that walk it give a ray
// to a GROUP of G = 2^lg adjacent lanes (G = 1 .. 64, chosen by the caller near the mean samples per ray; 64 / G rays per wave): lane
// `sub` of the group takes the samples lo + sub, lo + sub + G, ...  So in every pass the G lanes of a group touch G consecutive
// samples, and the groups of a wave touch consecutive rays, whose samples follow each other in the list: a wave's 12-byte coordinate
// stores and its 1..8-byte value loads fall into one contiguous span of the chunk (whole cache lines, apart from the span's ends),
// whether a ray holds one sample (a slice: G = 1, lane = ray = sample) or hundreds (a projection: G = 64, a wave per ray).
//
// There are NO atomics: within a launch a pixel has ONE owner, its group.  The group applies the exact inside test to every sample,
// reduces over its lanes in registers (a butterfly of lg steps within the group) and lane 0 does one plain read-modify-write of the
// pixel's accumulators: hits (int32) and the running max / min (int32) or sum (int64) per channel.  Launches of one view follow each
// other on one stream.  Everything folded is an integer: the result is exact and does not depend on G, on the chunking or on the run.
#include <type_traits>
#include "brief_view.h"

struct ViewChunk {
    int64_t s0, s1;      // the samples of the compacted list this launch covers
    int64_t r0, r1;      // the rays that may hold one of them: off[r + 1] > s0 and off[r] < s1 for r0 <= r < r1
    int lg;              // log2 of the lanes per ray
    float step[3];       // brief_view_step per axis, from the host (fill_grid's own float)
};

__global__ __launch_bounds__(256) void k_view_clip(brief_view_desc v, int32_t *__restrict__ k0, int32_t *__restrict__ cnt)
{
    const int64_t rays = (int64_t)v.rows * v.cols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = (int32_t)(r / v.cols), col = (int32_t)(r - (int64_t)row * v.cols);
        int32_t b, n;
        brief_view_ray_range(v, row, col, b, n);
        k0[r] = b;
        cnt[r] = n;
    }
}

// the part of the walk both list kernels share: the group's ray of iteration `it` and its samples within the chunk, [lo, hi) (empty
// for a group beyond the last ray), the ray's first list index `a` and its foot `base`
struct ViewRay { int64_t r, a, lo, hi; float base[3]; };
__device__ __forceinline__ ViewRay view_ray(const brief_view_desc &v, const ViewChunk &ch, const int64_t *__restrict__ off, int64_t g)
{
    ViewRay q;
    const bool live = g < ch.r1 - ch.r0;
    q.r = ch.r0 + (live ? g : 0);
    q.a = off[q.r];
    const int64_t b = off[q.r + 1];
    q.lo = q.a > ch.s0 ? q.a : ch.s0;
    q.hi = live ? (b < ch.s1 ? b : ch.s1) : q.lo;
    const int32_t row = (int32_t)(q.r / v.cols), col = (int32_t)(q.r - (int64_t)row * v.cols);
#pragma unroll
    for (int a = 0; a < 3; ++a) q.base[a] = brief_view_base(v, a, row, col);
    return q;
}

__global__ __launch_bounds__(256) void k_view_coords(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                     float *__restrict__ coords)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg; g < ch.r1 - ch.r0; g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            float *x = coords + (s - ch.s0) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = brief_view_coord(v, a, ch.step[a], brief_view_at(v, a, q.base[a], k));
        }
    }
}

// MODE 0: max, 1: min, 2: sum (mean).  acc: int32 [rays][C] (max, min) or int64 [rays][C] (sum), caller-initialised to the fold's
// identity (0, INT32_MAX, 0); hits: int32 [rays], caller-initialised to 0.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_view_fold(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                   const T *__restrict__ vals, int C, int32_t *__restrict__ hits, void *__restrict__ acc)
{
    typedef typename std::conditional<MODE == 2, long long, int>::type A;
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        int n = 0;
        A m[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = MODE == 1 ? (A)INT32_MAX : (A)0;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            if (!brief_view_inside(v, brief_view_at(v, 0, q.base[0], k), brief_view_at(v, 1, q.base[1], k), brief_view_at(v, 2, q.base[2], k)))
                continue;
            ++n;
            const T *x = vals + (s - ch.s0) * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = (A)x[c];
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = __shfl_xor(m[c], o);
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner
            hits[q.r] += n;
            A *d = (A *)acc + q.r * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) d[c] = MODE == 0 ? (m[c] > d[c] ? m[c] : d[c]) : (MODE == 1 ? (m[c] < d[c] ? m[c] : d[c]) : d[c] + m[c]);
        }
    }
}

// out[r][c]: the running value in the source dtype (T, max / min / slice) or the mean as float ((float)((double)sum / hits)); a pixel
// without an inside sample is 0
template <typename T, bool MEAN>
__global__ __launch_bounds__(256) void k_view_finish(int64_t rays, int C, const int32_t *__restrict__ hits, const void *__restrict__ acc, void *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rays * C; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t h = hits[i / C];
        if (MEAN) ((float *)out)[i] = h > 0 ? (float)((double)((const long long *)acc)[i] / (double)h) : 0.f;
        else ((T *)out)[i] = h > 0 ? (T)((const int *)acc)[i] : (T)0;
    }
}

// ---- host side
static const int32_t kViewMaxCount = 1 << 24;      // rows, cols and depth travel as floats
static const int64_t kViewMaxRays = (int64_t)1 << 40;

static int check_view(const brief_view_desc *v)
{
    if (!v) return fail(BRIEF_ERR_INVALID, "view: null descriptor");
    if (v->rows < 1 || v->cols < 1 || v->depth < 1 || v->rows >= kViewMaxCount || v->cols >= kViewMaxCount || v->depth >= kViewMaxCount)
        return fail(BRIEF_ERR_INVALID, "view: rows, cols and depth must be 1 .. 2^24 - 1 (a float holds them exactly)");
    if (!(v->lo == v->lo && v->hi == v->hi) || v->lo - v->lo != 0.f || v->hi - v->hi != 0.f) return fail(BRIEF_ERR_INVALID, "view: lo and hi must be finite");
    for (int a = 0; a < 3; ++a) {
        if (v->dims[a] < 2 || v->dims[a] >= ((int64_t)1 << 31)) return fail(BRIEF_ERR_INVALID, "view: every grid dim must be 2 .. 2^31 - 1");
        const float f[6] = {v->origin[a], v->drow[a], v->dcol[a], v->ddepth[a], v->box_lo[a], v->box_hi[a]};
        for (int i = 0; i < 6; ++i)
            if (f[i] - f[i] != 0.f) return fail(BRIEF_ERR_INVALID, "view: origin, steps and clip box must be finite");
        if (!(v->box_lo[a] >= 0.f && v->box_lo[a] <= v->box_hi[a] && v->box_hi[a] <= (float)(v->dims[a] - 1)))
            return fail(BRIEF_ERR_INVALID, "view: the clip box must satisfy 0 <= box_lo <= box_hi <= dims - 1 on every axis");
    }
    return 0;
}

static int view_blocks(int64_t threads)
{
    const int64_t want = (threads + 255) / 256, cap = (int64_t)kCUs * 64;
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

static int check_view_chunk(const brief_view_desc *v, const void *k0, const void *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1, int32_t lanes,
                            ViewChunk *ch)
{
    if (int rc = check_view(v)) return rc;
    if (!k0 || !off) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    const int64_t rays = (int64_t)v->rows * v->cols;
    if (s0 < 0 || s1 <= s0) return fail(BRIEF_ERR_INVALID, "view: an empty or negative sample range");
    if (r0 < 0 || r1 <= r0 || r1 > rays) return fail(BRIEF_ERR_INVALID, "view: the ray range must lie inside 0 .. rows * cols");
    int lg = 0;
    while (lg < 6 && (1 << lg) < lanes) ++lg;
    if (lanes < 1 || lanes > 64 || (1 << lg) != lanes) return fail(BRIEF_ERR_INVALID, "view: lanes per ray must be a power of two, 1 .. 64");
    ch->s0 = s0; ch->s1 = s1; ch->r0 = r0; ch->r1 = r1; ch->lg = lg;
    for (int a = 0; a < 3; ++a) ch->step[a] = brief_view_step(*v, a);
    return 0;
}

extern "C" {

int brief_view_clip(const brief_view_desc *view, int32_t *k0, int32_t *cnt, void *stream)
{
    if (int rc = check_view(view)) return rc;
    if (!k0 || !cnt) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    const int64_t rays = (int64_t)view->rows * view->cols;
    if (rays > kViewMaxRays) return fail(BRIEF_ERR_INVALID, "view: more than 2^40 rays");
    hipLaunchKernelGGL(k_view_clip, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, *view, k0, cnt);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_coords(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                      int32_t lanes, float *coords, void *stream)
{
    ViewChunk ch;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!coords) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    hipLaunchKernelGGL(k_view_coords, dim3(view_blocks((r1 - r0) << ch.lg)), dim3(256), 0, (hipStream_t)stream, *view, ch, k0, off, coords);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                    int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits, void *acc, void *stream)
{
    ViewChunk ch;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !hits || !acc) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "view: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "view: channels must be 1..4");
    if (mode < BRIEF_VIEW_MAX || mode > BRIEF_VIEW_SLICE) return fail(BRIEF_ERR_INVALID, "view: mode must be BRIEF_VIEW_MAX, _MIN, _MEAN or _SLICE");
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int m = mode == BRIEF_VIEW_SLICE ? 0 : mode;      // a slice has at most one inside sample per ray: its max is that sample
#define VIEW_FOLD(T, M) hipLaunchKernelGGL((k_view_fold<T, M>), grid, block, 0, st, *view, ch, k0, off, (const T *)vals, (int)channels, hits, acc)
    if (elem_kind == BRIEF_OUT_U8) {
        if (m == 0) VIEW_FOLD(uint8_t, 0); else if (m == 1) VIEW_FOLD(uint8_t, 1); else VIEW_FOLD(uint8_t, 2);
    } else {
        if (m == 0) VIEW_FOLD(uint16_t, 0); else if (m == 1) VIEW_FOLD(uint16_t, 1); else VIEW_FOLD(uint16_t, 2);
    }
#undef VIEW_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_finish(const brief_view_desc *view, int elem_kind, int32_t channels, int32_t mode, const int32_t *hits, const void *acc, void *out,
                      void *stream)
{
    if (int rc = check_view(view)) return rc;
    if (!hits || !acc || !out) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "view: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "view: channels must be 1..4");
    if (mode < BRIEF_VIEW_MAX || mode > BRIEF_VIEW_SLICE) return fail(BRIEF_ERR_INVALID, "view: mode must be BRIEF_VIEW_MAX, _MIN, _MEAN or _SLICE");
    const int64_t rays = (int64_t)view->rows * view->cols;
    const dim3 grid(view_blocks(rays * channels)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (mode == BRIEF_VIEW_MEAN) hipLaunchKernelGGL((k_view_finish<uint16_t, true>), grid, block, 0, st, rays, (int)channels, hits, acc, out);
    else if (elem_kind == BRIEF_OUT_U8) hipLaunchKernelGGL((k_view_finish<uint8_t, false>), grid, block, 0, st, rays, (int)channels, hits, acc, out);
    else hipLaunchKernelGGL((k_view_finish<uint16_t, false>), grid, block, 0, st, rays, (int)channels, hits, acc, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same header on the host CPU: no GPU call
int brief_view_sample_host(const brief_view_desc *view, const int32_t *row, const int32_t *col, const int32_t *k, int64_t n, float *pos, float *coord,
                           uint8_t *inside)
{
    if (int rc = check_view(view)) return rc;
    if (!row || !col || !k || n < 0) return fail(BRIEF_ERR_INVALID, "view: null index buffer or negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_step(*view, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= view->rows || col[i] < 0 || col[i] >= view->cols || k[i] < 0 || k[i] >= view->depth)
            return fail(BRIEF_ERR_INVALID, "view: a sample index outside rows x cols x depth");
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = brief_view_pos(*view, a, row[i], col[i], k[i]);
        if (pos) { pos[3 * i] = p[0]; pos[3 * i + 1] = p[1]; pos[3 * i + 2] = p[2]; }
        if (coord)
            for (int a = 0; a < 3; ++a) coord[3 * i + a] = brief_view_coord(*view, a, step[a], p[a]);
        if (inside) inside[i] = brief_view_inside(*view, p[0], p[1], p[2]) ? 1 : 0;
    }
    return 0;
}

int brief_view_clip_host(const brief_view_desc *view, int32_t *k0, int32_t *cnt)
{
    if (int rc = check_view(view)) return rc;
    if (!k0 || !cnt) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    for (int32_t row = 0; row < view->rows; ++row)
        for (int32_t col = 0; col < view->cols; ++col) {
            const int64_t r = (int64_t)row * view->cols + col;
            brief_view_ray_range(*view, row, col, k0[r], cnt[r]);
        }
    return 0;
}

}   // extern "C"

// ---- view of a partition: the nearest block owns a sample (csrc/brief_view.h "a view of a PARTITION"; view.render_partition).
//   k_view_part_clip    one thread per WINDOW ray: the interval of its samples inside the clip box and the block's cell.
//   k_view_part_coords  k_view_coords on the block's compacted list, giving block-local coordinates.
//   k_view_part_fold    k_view_fold with the exact test (clip box and cell) on every sample.
// The layout is that of k_view_coords / k_view_fold: ray-major list, a group of G = 2^lg lanes per ray, contiguous spans per wave.
// k0 and off are indexed by window ray, hits and acc by image ray (the pixel).  No atomics: within a launch a pixel has one owner, and
// the launches of a view, block after block, follow each other on one stream.
struct ViewPartRay { ViewRay q; int64_t pixel; };
__device__ __forceinline__ ViewPartRay view_part_ray(const brief_view_desc &v, const brief_view_part &pt, const ViewChunk &ch,
                                                     const int64_t *__restrict__ off, int64_t g)
{
    ViewPartRay w;
    ViewRay &q = w.q;
    const bool live = g < ch.r1 - ch.r0;
    q.r = ch.r0 + (live ? g : 0);
    q.a = off[q.r];
    const int64_t b = off[q.r + 1];
    q.lo = q.a > ch.s0 ? q.a : ch.s0;
    q.hi = live ? (b < ch.s1 ? b : ch.s1) : q.lo;
    const int32_t wr = (int32_t)(q.r / pt.wcols);
    const int32_t row = pt.row0 + wr, col = pt.col0 + (int32_t)(q.r - (int64_t)wr * pt.wcols);
    w.pixel = (int64_t)row * v.cols + col;
#pragma unroll
    for (int a = 0; a < 3; ++a) q.base[a] = brief_view_base(v, a, row, col);
    return w;
}

__global__ __launch_bounds__(256) void k_view_part_clip(brief_view_desc v, brief_view_part pt, int32_t *__restrict__ k0, int32_t *__restrict__ cnt)
{
    const int64_t rays = (int64_t)pt.wrows * pt.wcols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t wr = (int32_t)(r / pt.wcols);
        int32_t b, n;
        brief_view_part_ray_range(v, pt, pt.row0 + wr, pt.col0 + (int32_t)(r - (int64_t)wr * pt.wcols), b, n);
        k0[r] = b;
        cnt[r] = n;
    }
}

__global__ __launch_bounds__(256) void k_view_part_coords(brief_view_desc v, brief_view_part pt, ViewChunk ch, const int32_t *__restrict__ k0,
                                                          const int64_t *__restrict__ off, float *__restrict__ coords)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg; g < ch.r1 - ch.r0; g += groups) {
        const ViewRay q = view_part_ray(v, pt, ch, off, g).q;
        const int32_t kb = k0[q.r];
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            float *x = coords + (s - ch.s0) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a)      // (ch.step: the BLOCK grid's step, brief_view_part_step)
                x[a] = brief_view_part_coord(v, pt, a, ch.step[a], brief_view_part_local(pt, a, brief_view_at(v, a, q.base[a], k)));
        }
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_view_part_fold(brief_view_desc v, brief_view_part pt, ViewChunk ch, const int32_t *__restrict__ k0,
                                                        const int64_t *__restrict__ off, const T *__restrict__ vals, int C, int32_t *__restrict__ hits,
                                                        void *__restrict__ acc)
{
    typedef typename std::conditional<MODE == 2, long long, int>::type A;
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewPartRay w = view_part_ray(v, pt, ch, off, g);
        const ViewRay &q = w.q;
        const int32_t kb = k0[q.r];
        int n = 0;
        A m[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = MODE == 1 ? (A)INT32_MAX : (A)0;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            const float p0 = brief_view_at(v, 0, q.base[0], k), p1 = brief_view_at(v, 1, q.base[1], k), p2 = brief_view_at(v, 2, q.base[2], k);
            if (!(brief_view_inside(v, p0, p1, p2) && brief_view_part_owned(pt, p0, p1, p2))) continue;
            ++n;
            const T *x = vals + (s - ch.s0) * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = (A)x[c];
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = __shfl_xor(m[c], o);
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner in this launch
            hits[w.pixel] += n;
            A *d = (A *)acc + w.pixel * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) d[c] = MODE == 0 ? (m[c] > d[c] ? m[c] : d[c]) : (MODE == 1 ? (m[c] < d[c] ? m[c] : d[c]) : d[c] + m[c]);
        }
    }
}

// ---- host side of the partition entries
static const int64_t kViewPartMaxDim = (int64_t)1 << 23;      // s - 0.5 and e + 0.5 are exact floats below it

static int check_view_part(const brief_view_desc *v, const brief_view_part *pt)
{
    if (int rc = check_view(v)) return rc;
    if (!pt) return fail(BRIEF_ERR_INVALID, "view: null block descriptor");
    for (int a = 0; a < 3; ++a) {
        if (v->dims[a] >= kViewPartMaxDim)
            return fail(BRIEF_ERR_INVALID, "view: a partition needs every axis of the volume below 2^23 (the cell bounds s - 0.5 and e + 0.5 must be exact floats)");
        if (pt->start[a] < 0 || pt->dims[a] < 2 || pt->start[a] > v->dims[a] - pt->dims[a])
            return fail(BRIEF_ERR_INVALID, "view: a block needs start >= 0, dims >= 2 and start + dims <= the volume's dims on every axis");
    }
    if (pt->row0 < 0 || pt->col0 < 0 || pt->wrows < 1 || pt->wcols < 1 || pt->row0 > v->rows - pt->wrows || pt->col0 > v->cols - pt->wcols)
        return fail(BRIEF_ERR_INVALID, "view: a block's window must be at least 1 x 1 and lie inside the image rows x cols");
    return 0;
}

static int check_view_part_chunk(const brief_view_desc *v, const brief_view_part *pt, const void *k0, const void *off, int64_t s0, int64_t s1, int64_t r0,
                                 int64_t r1, int32_t lanes, ViewChunk *ch)
{
    if (int rc = check_view_part(v, pt)) return rc;
    if (int rc = check_view_chunk(v, k0, off, s0, s1, 0, 1, lanes, ch)) return rc;
    if (r0 < 0 || r1 <= r0 || r1 > (int64_t)pt->wrows * pt->wcols) return fail(BRIEF_ERR_INVALID, "view: the ray range must lie inside 0 .. wrows * wcols of the block's window");
    ch->r0 = r0; ch->r1 = r1;
    for (int a = 0; a < 3; ++a) ch->step[a] = brief_view_part_step(*v, *pt, a);
    return 0;
}

extern "C" {

int brief_view_part_clip(const brief_view_desc *view, const brief_view_part *part, int32_t *k0, int32_t *cnt, void *stream)
{
    if (int rc = check_view_part(view, part)) return rc;
    if (!k0 || !cnt) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    hipLaunchKernelGGL(k_view_part_clip, dim3(view_blocks((int64_t)part->wrows * part->wcols)), dim3(256), 0, (hipStream_t)stream, *view, *part, k0, cnt);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_part_coords(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                           int64_t r0, int64_t r1, int32_t lanes, float *coords, void *stream)
{
    ViewChunk ch;
    if (int rc = check_view_part_chunk(view, part, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!coords) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    hipLaunchKernelGGL(k_view_part_coords, dim3(view_blocks((r1 - r0) << ch.lg)), dim3(256), 0, (hipStream_t)stream, *view, *part, ch, k0, off, coords);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_view_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                         int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits,
                         void *acc, void *stream)
{
    ViewChunk ch;
    if (int rc = check_view_part_chunk(view, part, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !hits || !acc) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "view: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "view: channels must be 1..4");
    if (mode < BRIEF_VIEW_MAX || mode > BRIEF_VIEW_SLICE) return fail(BRIEF_ERR_INVALID, "view: mode must be BRIEF_VIEW_MAX, _MIN, _MEAN or _SLICE");
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int m = mode == BRIEF_VIEW_SLICE ? 0 : mode;      // a slice has at most one sample per ray over ALL blocks: its max is that sample
#define VIEW_PART_FOLD(T, M) hipLaunchKernelGGL((k_view_part_fold<T, M>), grid, block, 0, st, *view, *part, ch, k0, off, (const T *)vals, (int)channels, hits, acc)
    if (elem_kind == BRIEF_OUT_U8) {
        if (m == 0) VIEW_PART_FOLD(uint8_t, 0); else if (m == 1) VIEW_PART_FOLD(uint8_t, 1); else VIEW_PART_FOLD(uint8_t, 2);
    } else {
        if (m == 0) VIEW_PART_FOLD(uint16_t, 0); else if (m == 1) VIEW_PART_FOLD(uint16_t, 1); else VIEW_PART_FOLD(uint16_t, 2);
    }
#undef VIEW_PART_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same header on the host CPU: no GPU call
int brief_view_part_clip_host(const brief_view_desc *view, const brief_view_part *part, int32_t *k0, int32_t *cnt)
{
    if (int rc = check_view_part(view, part)) return rc;
    if (!k0 || !cnt) return fail(BRIEF_ERR_INVALID, "view: null buffer");
    for (int32_t wr = 0; wr < part->wrows; ++wr)
        for (int32_t wc = 0; wc < part->wcols; ++wc) {
            const int64_t r = (int64_t)wr * part->wcols + wc;
            brief_view_part_ray_range(*view, *part, part->row0 + wr, part->col0 + wc, k0[r], cnt[r]);
        }
    return 0;
}

int brief_view_part_sample_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *row, const int32_t *col, const int32_t *k,
                                int64_t n, float *pos, float *local, float *coord, uint8_t *inside, uint8_t *owned)
{
    if (int rc = check_view_part(view, part)) return rc;
    if (!row || !col || !k || n < 0) return fail(BRIEF_ERR_INVALID, "view: null index buffer or negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_part_step(*view, *part, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= view->rows || col[i] < 0 || col[i] >= view->cols || k[i] < 0 || k[i] >= view->depth)
            return fail(BRIEF_ERR_INVALID, "view: a sample index outside rows x cols x depth");
        float p[3], q[3];
        for (int a = 0; a < 3; ++a) {
            p[a] = brief_view_pos(*view, a, row[i], col[i], k[i]);
            q[a] = brief_view_part_local(*part, a, p[a]);
        }
        if (pos) { pos[3 * i] = p[0]; pos[3 * i + 1] = p[1]; pos[3 * i + 2] = p[2]; }
        if (local) { local[3 * i] = q[0]; local[3 * i + 1] = q[1]; local[3 * i + 2] = q[2]; }
        if (coord)
            for (int a = 0; a < 3; ++a) coord[3 * i + a] = brief_view_part_coord(*view, *part, a, step[a], q[a]);
        if (inside) inside[i] = brief_view_inside(*view, p[0], p[1], p[2]) ? 1 : 0;
        if (owned) owned[i] = brief_view_part_owned(*part, p[0], p[1], p[2]) ? 1 : 0;
    }
    return 0;
}

}   // extern "C"

// ---- surface view: the first sample of every ray at which one channel of the integer decode crosses a level, a sub-sample bisection
// of that crossing, and a Lambert shading from the net's analytic Jacobian at the hit (view.render_surface; DESIGN.md "Surface view").
//   k_surface_fold     k_view_fold's walk, folding first[r] = the smallest inside k whose value passes the side test (int32, caller-
//                      initialised to INT32_MAX) and hits[r]; one owner per pixel, a butterfly min within the group, no atomics.
//   k_surface_bracket  t_lo / t_hi per ray: (first - 1, first) where first > k0 (the sample before the hit is inside and fails the test),
//                      (first, first) for a CUT ray (first == k0: the clip box slices the object open), (NaN, NaN) without a hit.
//   k_surface_coords   DENSE [rays][3] coordinates (and positions) at the bracket's midpoint, or at t_hi (the hit itself).
//   (caller)           the net's forward entry on them, integer output kind.
//   k_surface_step     t_hi = t_mid where the value at t_mid passes the test, t_lo = t_mid otherwise.
//   k_surface_shade    the unit normal and the Lambert term of every pixel from the Jacobian at the hits.
// The side test compares decoded integers, and the bracket moves by it alone: first, t_lo and t_hi are exact and do not depend on the
// lanes per ray, on the chunking or on the run.
struct SurfaceTest { int32_t channel, level, below; };      // passes: value[channel] >= level (above) or <= level (below)
struct SurfaceVec { float v[3]; };

__device__ __forceinline__ bool surface_pass(const SurfaceTest &t, int32_t y) { return t.below ? y <= t.level : y >= t.level; }

template <typename T>
__global__ __launch_bounds__(256) void k_surface_fold(brief_view_desc v, ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                      const T *__restrict__ vals, int C, SurfaceTest test, int32_t *__restrict__ hits,
                                                      int32_t *__restrict__ first)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewRay q = view_ray(v, ch, off, g);
        const int32_t kb = k0[q.r];
        int n = 0;
        int32_t f = INT32_MAX;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            if (!brief_view_inside(v, brief_view_at(v, 0, q.base[0], k), brief_view_at(v, 1, q.base[1], k), brief_view_at(v, 2, q.base[2], k)))
                continue;
            ++n;
            if (k < f && surface_pass(test, (int32_t)vals[(s - ch.s0) * C + test.channel])) f = k;      // (a lane's k ascend: its first pass)
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {
            n += __shfl_xor(n, o);
            const int32_t y = __shfl_xor(f, o);
            f = y < f ? y : f;
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner
            hits[q.r] += n;
            if (f < first[q.r]) first[q.r] = f;
        }
    }
}

__global__ __launch_bounds__(256) void k_surface_bracket(int64_t rays, const int32_t *__restrict__ k0, const int32_t *__restrict__ first,
                                                         float *__restrict__ t_lo, float *__restrict__ t_hi)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t f = first[r];
        const bool hit = f >= 0 && f != INT32_MAX;
        const float hi = hit ? (float)f : __builtin_nanf("");
        t_hi[r] = hi;
        t_lo[r] = hit && f > k0[r] ? (float)(f - 1) : hi;
    }
}

// the depth a round evaluates: the midpoint of a bracket, else t_hi (a cut ray's hit; NaN without a hit)
__device__ __forceinline__ float surface_t(float lo, float hi, bool mid) { return mid && lo < hi ? brief_view_mid(lo, hi) : hi; }

__global__ __launch_bounds__(256) void k_surface_coords(brief_view_desc v, SurfaceVec step, int mid, const float *__restrict__ t_lo,
                                                        const float *__restrict__ t_hi, float *__restrict__ coords, float *__restrict__ pos)
{
    const int64_t rays = (int64_t)v.rows * v.cols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = (int32_t)(r / v.cols), col = (int32_t)(r - (int64_t)row * v.cols);
        const float t = surface_t(t_lo[r], t_hi[r], mid != 0);
        const bool hit = t == t;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // a ray without a hit gets the clip box's corner: a valid coordinate whose value nobody reads
            const float p = hit ? brief_view_at_t(v, a, brief_view_base(v, a, row, col), t) : v.box_lo[a];
            coords[r * 3 + a] = brief_view_coord(v, a, step.v[a], p);
            if (pos) pos[r * 3 + a] = hit ? p : t;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_surface_step(int64_t rays, const T *__restrict__ vals, int C, SurfaceTest test, float *__restrict__ t_lo,
                                                      float *__restrict__ t_hi)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const float lo = t_lo[r], hi = t_hi[r];
        if (!(lo < hi)) continue;                                    // cut, or no hit: never refined
        const float t = brief_view_mid(lo, hi);
        if (surface_pass(test, (int32_t)vals[r * C + test.channel])) t_hi[r] = t; else t_lo[r] = t;
    }
}

// g_a = jac[r][channel][a] * gscale_a (grey levels per physical unit); n = -g / |g| above (out of a bright object), +g / |g| below;
// shade = max(0, -(n . light)), light the unit direction the light travels.  |g| == 0 or no hit: normal 0, shade 0.
__global__ __launch_bounds__(256) void k_surface_shade(int64_t rays, const float *__restrict__ t, const float *__restrict__ jac, int C, SurfaceTest test,
                                                       SurfaceVec gscale, SurfaceVec light, float *__restrict__ normal, float *__restrict__ shade)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        float n[3] = {0.f, 0.f, 0.f}, s = 0.f;
        if (t[r] == t[r]) {
            const float *j = jac + (r * C + test.channel) * 3;
            const float g0 = j[0] * gscale.v[0], g1 = j[1] * gscale.v[1], g2 = j[2] * gscale.v[2];
            const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
            if (len > 0.f && len - len == 0.f) {
                const float sign = test.below ? 1.f : -1.f;
                n[0] = sign * g0 / len; n[1] = sign * g1 / len; n[2] = sign * g2 / len;
                const float d = -(n[0] * light.v[0] + n[1] * light.v[1] + n[2] * light.v[2]);
                s = d > 0.f ? d : 0.f;
            }
        }
        normal[r * 3] = n[0]; normal[r * 3 + 1] = n[1]; normal[r * 3 + 2] = n[2];
        shade[r] = s;
    }
}

static int check_surface_test(int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side, SurfaceTest *t)
{
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "surface: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "surface: channels must be 1..4");
    if (channel < 0 || channel >= channels) return fail(BRIEF_ERR_INVALID, "surface: channel must be 0 .. channels - 1");
    if (level < 0 || level > (elem_kind == BRIEF_OUT_U8 ? 255 : 65535))
        return fail(BRIEF_ERR_INVALID, "surface: level must lie in the range of the integer decode (0 .. 255 for uint8, 0 .. 65535 for uint16)");
    if (side != BRIEF_SURFACE_ABOVE && side != BRIEF_SURFACE_BELOW) return fail(BRIEF_ERR_INVALID, "surface: side must be BRIEF_SURFACE_ABOVE (0) or BRIEF_SURFACE_BELOW (1)");
    t->channel = channel; t->level = level; t->below = side == BRIEF_SURFACE_BELOW;
    return 0;
}

static int check_surface_rays(const brief_view_desc *v, int64_t *rays)
{
    if (int rc = check_view(v)) return rc;
    *rays = (int64_t)v->rows * v->cols;
    if (*rays > kViewMaxRays) return fail(BRIEF_ERR_INVALID, "view: more than 2^40 rays");
    return 0;
}

extern "C" {

int brief_surface_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                       int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side, int32_t *hits,
                       int32_t *first, void *stream)
{
    ViewChunk ch;
    SurfaceTest t;
    if (int rc = check_view_chunk(view, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !hits || !first) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(elem_kind, channels, channel, level, side, &t)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_kind == BRIEF_OUT_U8) hipLaunchKernelGGL((k_surface_fold<uint8_t>), grid, block, 0, st, *view, ch, k0, off, (const uint8_t *)vals, (int)channels, t, hits, first);
    else hipLaunchKernelGGL((k_surface_fold<uint16_t>), grid, block, 0, st, *view, ch, k0, off, (const uint16_t *)vals, (int)channels, t, hits, first);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_bracket(const brief_view_desc *view, const int32_t *k0, const int32_t *first, float *t_lo, float *t_hi, void *stream)
{
    int64_t rays;
    if (int rc = check_surface_rays(view, &rays)) return rc;
    if (!k0 || !first || !t_lo || !t_hi) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    hipLaunchKernelGGL(k_surface_bracket, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, rays, k0, first, t_lo, t_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_coords(const brief_view_desc *view, const float *t_lo, const float *t_hi, int32_t midpoint, float *coords, float *pos, void *stream)
{
    int64_t rays;
    if (int rc = check_surface_rays(view, &rays)) return rc;
    if (!t_lo || !t_hi || !coords) return fail(BRIEF_ERR_INVALID, "surface: null buffer (pos alone may be NULL)");
    if (midpoint != 0 && midpoint != 1) return fail(BRIEF_ERR_INVALID, "surface: midpoint must be 0 (the hit, t_hi) or 1 (the bracket's midpoint)");
    SurfaceVec step;
    for (int a = 0; a < 3; ++a) step.v[a] = brief_view_step(*view, a);
    hipLaunchKernelGGL(k_surface_coords, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, *view, step, (int)midpoint, t_lo, t_hi, coords, pos);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_step(const brief_view_desc *view, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                       float *t_lo, float *t_hi, void *stream)
{
    int64_t rays;
    SurfaceTest t;
    if (int rc = check_surface_rays(view, &rays)) return rc;
    if (!vals || !t_lo || !t_hi) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(elem_kind, channels, channel, level, side, &t)) return rc;
    const dim3 grid(view_blocks(rays)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_kind == BRIEF_OUT_U8) hipLaunchKernelGGL((k_surface_step<uint8_t>), grid, block, 0, st, rays, (const uint8_t *)vals, (int)channels, t, t_lo, t_hi);
    else hipLaunchKernelGGL((k_surface_step<uint16_t>), grid, block, 0, st, rays, (const uint16_t *)vals, (int)channels, t, t_lo, t_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_shade(const brief_view_desc *view, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                        const float *gscale, const float *light, float *normal, float *shade, void *stream)
{
    int64_t rays;
    SurfaceTest test;
    if (int rc = check_surface_rays(view, &rays)) return rc;
    if (!t || !jac || !gscale || !light || !normal || !shade) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(BRIEF_OUT_U16, channels, channel, 0, side, &test)) return rc;
    SurfaceVec g, l;
    for (int a = 0; a < 3; ++a) {
        g.v[a] = gscale[a]; l.v[a] = light[a];
        if (g.v[a] - g.v[a] != 0.f || l.v[a] - l.v[a] != 0.f) return fail(BRIEF_ERR_INVALID, "surface: gscale and light must be finite");
    }
    hipLaunchKernelGGL(k_surface_shade, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, rays, t, jac, (int)channels, test, g, l, normal, shade);
    HIP_TRY(hipGetLastError());
    return 0;
}

// brief_view_sample_host at a real depth t, 0 <= t <= depth - 1: the positions the refinement evaluates, on the host CPU
int brief_view_sample_t_host(const brief_view_desc *view, const int32_t *row, const int32_t *col, const float *t, int64_t n, float *pos, float *coord,
                             uint8_t *inside)
{
    if (int rc = check_view(view)) return rc;
    if (!row || !col || !t || n < 0) return fail(BRIEF_ERR_INVALID, "view: null index buffer or negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_step(*view, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= view->rows || col[i] < 0 || col[i] >= view->cols || !(t[i] >= 0.f && t[i] <= (float)(view->depth - 1)))
            return fail(BRIEF_ERR_INVALID, "view: a sample outside rows x cols x [0, depth - 1]");
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = brief_view_at_t(*view, a, brief_view_base(*view, a, row[i], col[i]), t[i]);
        if (pos) { pos[3 * i] = p[0]; pos[3 * i + 1] = p[1]; pos[3 * i + 2] = p[2]; }
        if (coord)
            for (int a = 0; a < 3; ++a) coord[3 * i + a] = brief_view_coord(*view, a, step[a], p[a]);
        if (inside) inside[i] = brief_view_inside(*view, p[0], p[1], p[2]) ? 1 : 0;
    }
    return 0;
}

}   // extern "C"
