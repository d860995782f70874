// brief_rays.inc — the ray view: a view whose rays come from a device table, six floats per ray (a perspective camera, or any bundle a
// caller fills in).  k_rays_clip, k_rays_coords, k_rays_fold, k_rays_surface_fold, k_rays_surface_coords, k_rays_surface_shade and their
// C-ABI entries brief_rays_* (part of the single translation unit brief_hip.hip, included at its very end: kernels and host code of a
// feature that touches no other kernel).  The geometry is csrc/brief_rays.h, compiled here for the device and for the host entries alike.
//
// The walk is brief_view.inc's: the compacted RAY-MAJOR sample list (sample off[r] + j is sample k0[r] + j of ray r), a group of
// G = 2^lg adjacent lanes per ray, no atomics, one owner per pixel, integer folds.  What differs:
//   k_rays_clip / k_rays_coords  read the ray's foot and step from the table where the orthographic kernels compute them from the
//                                lattice: one 24-byte row per ray, read once per ray and launch.
//   k_rays_fold / k_rays_surface_fold  are GEOMETRY-FREE.  The list k_rays_clip makes is exact (it holds every inside sample and nothing
//                                else), so no sample is tested again and the folds never read the table: hits[r] grows by the samples
//                                of the chunk that belong to ray r.
// brief_view_finish, brief_surface_bracket and brief_surface_step read rows x cols of their descriptor only: a ray view calls them with
// brief_rays_view()'s descriptor.  The table is device memory the caller filled; it is trusted (brief_rays.h "Ray range" says what a bad
// one can and cannot do), the host entries check theirs for finiteness.
#include "brief_rays.h"

// the part of the walk the list kernels share: the group's ray of iteration `it` and its samples within the chunk, [lo, hi) (empty for
// a group beyond the last ray), and the ray's first list index `a`
struct RaysRay { int64_t r, a, lo, hi; };
__device__ __forceinline__ RaysRay rays_ray(const ViewChunk &ch, const int64_t *__restrict__ off, int64_t g)
{
    RaysRay q;
    const bool live = g < ch.r1 - ch.r0;
    q.r = ch.r0 + (live ? g : 0);
    q.a = off[q.r];
    const int64_t b = off[q.r + 1];
    q.lo = q.a > ch.s0 ? q.a : ch.s0;
    q.hi = live ? (b < ch.s1 ? b : ch.s1) : q.lo;
    return q;
}

__global__ __launch_bounds__(256) void k_rays_clip(brief_view_desc v, const float *__restrict__ rays, int32_t *__restrict__ k0, int32_t *__restrict__ cnt)
{
    const int64_t n = (int64_t)v.rows * v.cols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        float ray[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) ray[i] = rays[r * 6 + i];
        int32_t b, c;
        brief_rays_ray_range(v, ray, b, c);
        k0[r] = b;
        cnt[r] = c;
    }
}

__global__ __launch_bounds__(256) void k_rays_coords(brief_view_desc v, ViewChunk ch, const float *__restrict__ rays, const int32_t *__restrict__ k0,
                                                     const int64_t *__restrict__ off, float *__restrict__ coords)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg; g < ch.r1 - ch.r0; g += groups) {
        const RaysRay q = rays_ray(ch, off, g);
        const int32_t kb = k0[q.r];
        float ray[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) ray[i] = rays[q.r * 6 + i];
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            float *x = coords + (s - ch.s0) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = brief_view_coord(v, a, ch.step[a], brief_rays_at(ray, a, k));
        }
    }
}

// k_view_fold without the inside test.  MODE 0: max, 1: min, 2: sum (mean); acc and hits as k_view_fold's.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_rays_fold(ViewChunk ch, const int64_t *__restrict__ off, const T *__restrict__ vals, int C,
                                                   int32_t *__restrict__ hits, void *__restrict__ acc)
{
    typedef typename std::conditional<MODE == 2, long long, int>::type A;
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const RaysRay q = rays_ray(ch, off, g);
        A m[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = MODE == 1 ? (A)INT32_MAX : (A)0;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const T *x = vals + (s - ch.s0) * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = (A)x[c];
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const A y = __shfl_xor(m[c], o);
                    m[c] = MODE == 0 ? (y > m[c] ? y : m[c]) : (MODE == 1 ? (y < m[c] ? y : m[c]) : m[c] + y);
                }
        }
        if (sub == 0 && q.hi > q.lo) {                               // the pixel's owner; the ray's samples in this chunk are q.hi - q.lo
            hits[q.r] += (int32_t)(q.hi - q.lo);
            A *d = (A *)acc + q.r * C;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) d[c] = MODE == 0 ? (m[c] > d[c] ? m[c] : d[c]) : (MODE == 1 ? (m[c] < d[c] ? m[c] : d[c]) : d[c] + m[c]);
        }
    }
}

// k_surface_fold without the inside test: first[r] = the smallest k of the ray's list whose value passes the side test
template <typename T>
__global__ __launch_bounds__(256) void k_rays_surface_fold(ViewChunk ch, const int32_t *__restrict__ k0, const int64_t *__restrict__ off,
                                                           const T *__restrict__ vals, int C, SurfaceTest test, int32_t *__restrict__ hits,
                                                           int32_t *__restrict__ first)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const RaysRay q = rays_ray(ch, off, g);
        const int32_t kb = k0[q.r];
        int32_t f = INT32_MAX;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            if (k < f && surface_pass(test, (int32_t)vals[(s - ch.s0) * C + test.channel])) f = k;      // (a lane's k ascend: its first pass)
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {
            const int32_t y = __shfl_xor(f, o);
            f = y < f ? y : f;
        }
        if (sub == 0 && q.hi > q.lo) {                               // the pixel's owner
            hits[q.r] += (int32_t)(q.hi - q.lo);
            if (f < first[q.r]) first[q.r] = f;
        }
    }
}

// k_surface_coords at the per-ray real depth
__global__ __launch_bounds__(256) void k_rays_surface_coords(brief_view_desc v, SurfaceVec step, int mid, const float *__restrict__ rays,
                                                             const float *__restrict__ t_lo, const float *__restrict__ t_hi, float *__restrict__ coords,
                                                             float *__restrict__ pos)
{
    const int64_t n = (int64_t)v.rows * v.cols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const float t = surface_t(t_lo[r], t_hi[r], mid != 0);
        const bool hit = t == t;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // a ray without a hit gets the clip box's corner: a valid coordinate whose value nobody reads
            const float p = hit ? brief_rays_at_t(rays + r * 6, a, t) : v.box_lo[a];
            coords[r * 3 + a] = brief_view_coord(v, a, step.v[a], p);
            if (pos) pos[r * 3 + a] = hit ? p : t;
        }
    }
}

// k_surface_shade's arithmetic with the light of ray r, light[r][3]
__global__ __launch_bounds__(256) void k_rays_surface_shade(int64_t n_rays, const float *__restrict__ t, const float *__restrict__ jac, int C, SurfaceTest test,
                                                            SurfaceVec gscale, const float *__restrict__ light, float *__restrict__ normal,
                                                            float *__restrict__ shade)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rays; r += (int64_t)gridDim.x * blockDim.x) {
        float n[3] = {0.f, 0.f, 0.f}, s = 0.f;
        if (t[r] == t[r]) {
            const float *j = jac + (r * C + test.channel) * 3;
            const float g0 = j[0] * gscale.v[0], g1 = j[1] * gscale.v[1], g2 = j[2] * gscale.v[2];
            const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
            if (len > 0.f && len - len == 0.f) {
                const float sign = test.below ? 1.f : -1.f;
                n[0] = sign * g0 / len; n[1] = sign * g1 / len; n[2] = sign * g2 / len;
                const float d = -(n[0] * light[r * 3] + n[1] * light[r * 3 + 1] + n[2] * light[r * 3 + 2]);
                s = d > 0.f ? d : 0.f;
            }
        }
        normal[r * 3] = n[0]; normal[r * 3 + 1] = n[1]; normal[r * 3 + 2] = n[2];
        shade[r] = s;
    }
}

// ---- host side
static int check_rays(const brief_rays_desc *d, brief_view_desc *v, int64_t *n_rays)
{
    if (!d) return fail(BRIEF_ERR_INVALID, "rays: null descriptor");
    *v = brief_rays_view(*d);
    if (int rc = check_view(v)) return rc;
    const int64_t n = (int64_t)v->rows * v->cols;
    if (n > kViewMaxRays) return fail(BRIEF_ERR_INVALID, "view: more than 2^40 rays");
    if (n_rays) *n_rays = n;
    return 0;
}

static int check_rays_chunk(const brief_rays_desc *d, const void *k0, const void *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1, int32_t lanes,
                            brief_view_desc *v, ViewChunk *ch)
{
    if (int rc = check_rays(d, v, nullptr)) return rc;
    return check_view_chunk(v, k0, off, s0, s1, r0, r1, lanes, ch);
}

static int check_rays_table(const float *rays, int64_t r)
{
    for (int i = 0; i < 6; ++i)
        if (rays[r * 6 + i] - rays[r * 6 + i] != 0.f) return fail(BRIEF_ERR_INVALID, "rays: every base and step of the ray table must be finite");
    return 0;
}

extern "C" {

int brief_rays_clip(const brief_rays_desc *desc, const float *rays, int32_t *k0, int32_t *cnt, void *stream)
{
    brief_view_desc v;
    int64_t n;
    if (int rc = check_rays(desc, &v, &n)) return rc;
    if (!rays || !k0 || !cnt) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    hipLaunchKernelGGL(k_rays_clip, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, v, rays, k0, cnt);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_rays_coords(const brief_rays_desc *desc, const float *rays, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0,
                      int64_t r1, int32_t lanes, float *coords, void *stream)
{
    brief_view_desc v;
    ViewChunk ch;
    if (int rc = check_rays_chunk(desc, k0, off, s0, s1, r0, r1, lanes, &v, &ch)) return rc;
    if (!rays || !coords) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    hipLaunchKernelGGL(k_rays_coords, dim3(view_blocks((r1 - r0) << ch.lg)), dim3(256), 0, (hipStream_t)stream, v, ch, rays, k0, off, coords);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_rays_fold(const brief_rays_desc *desc, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                    int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits, void *acc, void *stream)
{
    brief_view_desc v;
    ViewChunk ch;
    if (int rc = check_rays_chunk(desc, k0, off, s0, s1, r0, r1, lanes, &v, &ch)) return rc;
    if (!vals || !hits || !acc) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    if (elem_kind != BRIEF_OUT_U8 && elem_kind != BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "rays: elem_kind must be BRIEF_OUT_U8 (1) or BRIEF_OUT_U16 (2)");
    if (channels < 1 || channels > 4) return fail(BRIEF_ERR_INVALID, "rays: channels must be 1..4");
    if (mode == BRIEF_VIEW_SLICE) return fail(BRIEF_ERR_INVALID, "rays: BRIEF_VIEW_SLICE is not a mode of a ray view (a slice through a camera is out of scope); mode must be BRIEF_VIEW_MAX, _MIN or _MEAN");
    if (mode < BRIEF_VIEW_MAX || mode > BRIEF_VIEW_MEAN) return fail(BRIEF_ERR_INVALID, "rays: mode must be BRIEF_VIEW_MAX, _MIN or _MEAN");
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define RAYS_FOLD(T, M) hipLaunchKernelGGL((k_rays_fold<T, M>), grid, block, 0, st, ch, off, (const T *)vals, (int)channels, hits, acc)
    if (elem_kind == BRIEF_OUT_U8) {
        if (mode == 0) RAYS_FOLD(uint8_t, 0); else if (mode == 1) RAYS_FOLD(uint8_t, 1); else RAYS_FOLD(uint8_t, 2);
    } else {
        if (mode == 0) RAYS_FOLD(uint16_t, 0); else if (mode == 1) RAYS_FOLD(uint16_t, 1); else RAYS_FOLD(uint16_t, 2);
    }
#undef RAYS_FOLD
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_rays_surface_fold(const brief_rays_desc *desc, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                            int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                            int32_t *hits, int32_t *first, void *stream)
{
    brief_view_desc v;
    ViewChunk ch;
    SurfaceTest t;
    if (int rc = check_rays_chunk(desc, k0, off, s0, s1, r0, r1, lanes, &v, &ch)) return rc;
    if (!vals || !hits || !first) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    if (int rc = check_surface_test(elem_kind, channels, channel, level, side, &t)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_kind == BRIEF_OUT_U8) hipLaunchKernelGGL((k_rays_surface_fold<uint8_t>), grid, block, 0, st, ch, k0, off, (const uint8_t *)vals, (int)channels, t, hits, first);
    else hipLaunchKernelGGL((k_rays_surface_fold<uint16_t>), grid, block, 0, st, ch, k0, off, (const uint16_t *)vals, (int)channels, t, hits, first);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_rays_surface_coords(const brief_rays_desc *desc, const float *rays, const float *t_lo, const float *t_hi, int32_t midpoint, float *coords,
                              float *pos, void *stream)
{
    brief_view_desc v;
    int64_t n;
    if (int rc = check_rays(desc, &v, &n)) return rc;
    if (!rays || !t_lo || !t_hi || !coords) return fail(BRIEF_ERR_INVALID, "rays: null buffer (pos alone may be NULL)");
    if (midpoint != 0 && midpoint != 1) return fail(BRIEF_ERR_INVALID, "rays: midpoint must be 0 (the hit, t_hi) or 1 (the bracket's midpoint)");
    SurfaceVec step;
    for (int a = 0; a < 3; ++a) step.v[a] = brief_view_step(v, a);
    hipLaunchKernelGGL(k_rays_surface_coords, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, v, step, (int)midpoint, rays, t_lo, t_hi, coords, pos);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_rays_surface_shade(const brief_rays_desc *desc, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                             const float *gscale, const float *light, float *normal, float *shade, void *stream)
{
    brief_view_desc v;
    int64_t n;
    SurfaceTest test;
    if (int rc = check_rays(desc, &v, &n)) return rc;
    if (!t || !jac || !gscale || !light || !normal || !shade) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    if (int rc = check_surface_test(BRIEF_OUT_U16, channels, channel, 0, side, &test)) return rc;
    SurfaceVec g;
    for (int a = 0; a < 3; ++a) {
        g.v[a] = gscale[a];
        if (g.v[a] - g.v[a] != 0.f) return fail(BRIEF_ERR_INVALID, "rays: gscale must be finite");
    }
    hipLaunchKernelGGL(k_rays_surface_shade, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, t, jac, (int)channels, test, g, light, normal, shade);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same header on the host CPU: every buffer, the table included, is host memory; no GPU call
int brief_rays_sample_host(const brief_rays_desc *desc, const float *rays, const int32_t *row, const int32_t *col, const int32_t *k, int64_t n,
                           float *pos, float *coord, uint8_t *inside)
{
    brief_view_desc v;
    if (int rc = check_rays(desc, &v, nullptr)) return rc;
    if (!rays || !row || !col || !k || n < 0) return fail(BRIEF_ERR_INVALID, "rays: null table or index buffer, or a negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_step(v, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= v.rows || col[i] < 0 || col[i] >= v.cols || k[i] < 0 || k[i] >= v.depth)
            return fail(BRIEF_ERR_INVALID, "rays: a sample index outside rows x cols x depth");
        const int64_t r = (int64_t)row[i] * v.cols + col[i];
        if (int rc = check_rays_table(rays, r)) return rc;
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = brief_rays_at(rays + r * 6, a, k[i]);
        if (pos) { pos[3 * i] = p[0]; pos[3 * i + 1] = p[1]; pos[3 * i + 2] = p[2]; }
        if (coord)
            for (int a = 0; a < 3; ++a) coord[3 * i + a] = brief_view_coord(v, a, step[a], p[a]);
        if (inside) inside[i] = brief_view_inside(v, p[0], p[1], p[2]) ? 1 : 0;
    }
    return 0;
}

int brief_rays_sample_t_host(const brief_rays_desc *desc, const float *rays, const int32_t *row, const int32_t *col, const float *t, int64_t n,
                             float *pos, float *coord, uint8_t *inside)
{
    brief_view_desc v;
    if (int rc = check_rays(desc, &v, nullptr)) return rc;
    if (!rays || !row || !col || !t || n < 0) return fail(BRIEF_ERR_INVALID, "rays: null table or index buffer, or a negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_step(v, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= v.rows || col[i] < 0 || col[i] >= v.cols || !(t[i] >= 0.f && t[i] <= (float)(v.depth - 1)))
            return fail(BRIEF_ERR_INVALID, "rays: a sample outside rows x cols x [0, depth - 1]");
        const int64_t r = (int64_t)row[i] * v.cols + col[i];
        if (int rc = check_rays_table(rays, r)) return rc;
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = brief_rays_at_t(rays + r * 6, a, t[i]);
        if (pos) { pos[3 * i] = p[0]; pos[3 * i + 1] = p[1]; pos[3 * i + 2] = p[2]; }
        if (coord)
            for (int a = 0; a < 3; ++a) coord[3 * i + a] = brief_view_coord(v, a, step[a], p[a]);
        if (inside) inside[i] = brief_view_inside(v, p[0], p[1], p[2]) ? 1 : 0;
    }
    return 0;
}

int brief_rays_clip_host(const brief_rays_desc *desc, const float *rays, int32_t *k0, int32_t *cnt)
{
    brief_view_desc v;
    int64_t n;
    if (int rc = check_rays(desc, &v, &n)) return rc;
    if (!rays || !k0 || !cnt) return fail(BRIEF_ERR_INVALID, "rays: null buffer");
    for (int64_t r = 0; r < n; ++r)
        if (int rc = check_rays_table(rays, r)) return rc;
    for (int64_t r = 0; r < n; ++r) brief_rays_ray_range(v, rays + r * 6, k0[r], cnt[r]);
    return 0;
}

}   // extern "C"
