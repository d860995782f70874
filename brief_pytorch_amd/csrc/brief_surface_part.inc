// brief_surface_part.inc — the surface view of a PARTITION (a DivideTask artefact, one net per block): hits are routed across blocks
// (part of the single translation unit brief_hip.hip, included at its very end: kernels and host code of a feature that touches no other
// kernel).  The rules are csrc/brief_view.h "the surface view of a PARTITION"; view.render_surface_partition drives them; DESIGN.md
// "Surface view of a partition" has the reasoning.
//   k_surface_part_fold    k_view_part_fold's walk (window rays, the exact clip-box-and-cell test on every sample) with k_surface_fold's
//                          fold: first = the smallest owned inside k whose value passes the side test, a butterfly min within the ray's
//                          group of G = 2^lg lanes (64-wide waves: a group never spans two), and lane 0 does one plain read-modify-write
//                          of the IMAGE pixel's hits and first.  A min and a sum of integers: the blocks fold in any order.
//   k_surface_part_route   one thread per image ray: the block whose cell holds the ray's point at the round's depth (the midpoint of
//                          its bracket, or the hit t_hi), an O(nparts) loop over the device table of blocks; an unowned midpoint moves
//                          t_lo (the gap rule `empty`).
//   (caller)               buckets the rays by owner: per block a LIST of image rays.
//   k_surface_part_coords  block-local coordinates of a list's points, coords[i] for ray rays[i] (and the global position of the ray).
//   (caller)               the owner's forward entry on them, the block's own integer epilogue.
//   k_surface_part_step    k_surface_step on a list: vals[i] moves the bracket of ray rays[i].
//   k_surface_part_shade   k_surface_shade on a list: jac[i] gives the normal and the Lambert term of ray rays[i].
// A ray is in at most ONE list of a round (it has one owner), and the launches of a round follow each other on one stream: no atomics.
// Every decision compares decoded integers or floats computed per ray alone: first, t_lo, t_hi and owner do not depend on the order
// of the blocks, on chunking, on the bucketing or on the run.  Lists are int64 image-ray indices.

template <typename T>
__global__ __launch_bounds__(256) void k_surface_part_fold(brief_view_desc v, brief_view_part pt, ViewChunk ch, const int32_t *__restrict__ k0,
                                                           const int64_t *__restrict__ off, const T *__restrict__ vals, int C, SurfaceTest test,
                                                           int32_t *__restrict__ hits, int32_t *__restrict__ first)
{
    const int G = 1 << ch.lg, sub = threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> ch.lg, nr = ch.r1 - ch.r0;
    const int64_t iters = (nr + groups - 1) / groups;               // the same for every lane: the butterfly below needs the whole group
    int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> ch.lg;
    for (int64_t it = 0; it < iters; ++it, g += groups) {
        const ViewPartRay w = view_part_ray(v, pt, ch, off, g);     // (a group beyond the last ray walks an empty range of ray r0)
        const ViewRay &q = w.q;
        const int32_t kb = k0[q.r];
        int n = 0;
        int32_t f = INT32_MAX;
        for (int64_t s = q.lo + sub; s < q.hi; s += G) {
            const int32_t k = kb + (int32_t)(s - q.a);
            const float p0 = brief_view_at(v, 0, q.base[0], k), p1 = brief_view_at(v, 1, q.base[1], k), p2 = brief_view_at(v, 2, q.base[2], k);
            if (!(brief_view_inside(v, p0, p1, p2) && brief_view_part_owned(pt, p0, p1, p2))) continue;
            ++n;
            if (k < f && surface_pass(test, (int32_t)vals[(s - ch.s0) * C + test.channel])) f = k;      // (a lane's k ascend: its first pass)
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {                      // (G is the launch's: every group of the wave takes the same steps)
            n += __shfl_xor(n, o);
            const int32_t y = __shfl_xor(f, o);
            f = y < f ? y : f;
        }
        if (sub == 0 && n > 0) {                                     // the pixel's owner in this launch
            hits[w.pixel] += n;
            if (f < first[w.pixel]) first[w.pixel] = f;
        }
    }
}

__global__ __launch_bounds__(256) void k_surface_part_route(brief_view_desc v, const brief_view_part *__restrict__ parts, int32_t nparts, int mid,
                                                            float *__restrict__ t_lo, const float *__restrict__ t_hi, int32_t *__restrict__ owner)
{
    const int64_t rays = (int64_t)v.rows * v.cols;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rays; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = (int32_t)(r / v.cols), col = (int32_t)(r - (int64_t)row * v.cols);
        const float lo = t_lo[r];
        float moved = lo;
        const int32_t o = brief_view_part_route(v, parts, nparts, row, col, moved, t_hi[r], mid != 0);
        if (moved > lo) t_lo[r] = moved;                             // (written only where the gap rule moves it)
        owner[r] = o;
    }
}

__global__ __launch_bounds__(256) void k_surface_part_coords(brief_view_desc v, brief_view_part pt, SurfaceVec step, int mid, const float *__restrict__ t_lo,
                                                             const float *__restrict__ t_hi, const int64_t *__restrict__ list, int64_t n,
                                                             float *__restrict__ coords, float *__restrict__ pos)
{
    const int64_t rays = (int64_t)v.rows * v.cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = list[i];
        const bool in_image = r >= 0 && r < rays;                    // an entry outside the image reads and writes nothing of the image
        const float t = in_image ? brief_view_surface_t(t_lo[r], t_hi[r], mid != 0) : __builtin_nanf("");
        const bool hit = t == t;
        const int32_t row = in_image ? (int32_t)(r / v.cols) : 0, col = in_image ? (int32_t)(r - (int64_t)row * v.cols) : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // a ray without a point gets the clip box's corner: a valid position whose value nobody reads
            const float p = hit ? brief_view_at_t(v, a, brief_view_base(v, a, row, col), t) : v.box_lo[a];
            coords[i * 3 + a] = brief_view_part_coord(v, pt, a, step.v[a], brief_view_part_local(pt, a, p));
            if (pos && in_image) pos[r * 3 + a] = hit ? p : t;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_surface_part_step(const int64_t *__restrict__ list, int64_t n, const T *__restrict__ vals, int C, SurfaceTest test,
                                                           float *__restrict__ t_lo, float *__restrict__ t_hi)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = list[i];
        if (r < 0) continue;
        const float lo = t_lo[r], hi = t_hi[r];
        if (!(lo < hi)) continue;                                    // cut, or no hit: never refined
        const float t = brief_view_mid(lo, hi);
        if (surface_pass(test, (int32_t)vals[i * C + test.channel])) t_hi[r] = t; else t_lo[r] = t;
    }
}

// k_surface_shade's arithmetic, operation for operation, on jac[i] for ray list[i]
__global__ __launch_bounds__(256) void k_surface_part_shade(const int64_t *__restrict__ list, int64_t n, const float *__restrict__ t,
                                                            const float *__restrict__ jac, int C, SurfaceTest test, SurfaceVec gscale, SurfaceVec light,
                                                            float *__restrict__ normal, float *__restrict__ shade)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = list[i];
        if (r < 0) continue;
        float nn[3] = {0.f, 0.f, 0.f}, s = 0.f;
        if (t[r] == t[r]) {
            const float *j = jac + (i * C + test.channel) * 3;
            const float g0 = j[0] * gscale.v[0], g1 = j[1] * gscale.v[1], g2 = j[2] * gscale.v[2];
            const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
            if (len > 0.f && len - len == 0.f) {
                const float sign = test.below ? 1.f : -1.f;
                nn[0] = sign * g0 / len; nn[1] = sign * g1 / len; nn[2] = sign * g2 / len;
                const float d = -(nn[0] * light.v[0] + nn[1] * light.v[1] + nn[2] * light.v[2]);
                s = d > 0.f ? d : 0.f;
            }
        }
        normal[r * 3] = nn[0]; normal[r * 3 + 1] = nn[1]; normal[r * 3 + 2] = nn[2];
        shade[r] = s;
    }
}

// ---- host side
static const int64_t kSurfacePartMaxBlocks = ((int64_t)1 << 31) - 1;

// check_view_part for an entry of the route's table: the window plays no part in the routing, so an EMPTY one (wrows == wcols == 0: a
// block the clip box misses, view.make_part) is allowed there
static int check_route_part(const brief_view_desc *v, const brief_view_part *pt)
{
    if (!pt) return fail(BRIEF_ERR_INVALID, "view: null block descriptor");
    brief_view_part p = *pt;
    if (p.wrows == 0 && p.wcols == 0) { p.row0 = p.col0 = 0; p.wrows = p.wcols = 1; }
    return check_view_part(v, &p);
}

static int check_surface_list(const void *list, int64_t n)
{
    if (!list) return fail(BRIEF_ERR_INVALID, "surface: null buffer (the list of rays)");
    if (n < 1) return fail(BRIEF_ERR_INVALID, "surface: a list of rays needs n >= 1 entries");
    return 0;
}

static int check_route(const brief_view_desc *view, const brief_view_part *parts, int32_t nparts, const float *t_lo, const float *t_hi, int32_t midpoint,
                       const int32_t *owner, int64_t *rays)
{
    if (int rc = check_surface_rays(view, rays)) return rc;
    for (int a = 0; a < 3; ++a)
        if (view->dims[a] >= kViewPartMaxDim)
            return fail(BRIEF_ERR_INVALID, "view: a partition needs every axis of the volume below 2^23 (the cell bounds s - 0.5 and e + 0.5 must be exact floats)");
    if (nparts < 1 || (int64_t)nparts > kSurfacePartMaxBlocks) return fail(BRIEF_ERR_INVALID, "surface: nparts must be 1 .. 2^31 - 1 blocks");
    if (!parts || !t_lo || !t_hi || !owner) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (midpoint != 0 && midpoint != 1) return fail(BRIEF_ERR_INVALID, "surface: midpoint must be 0 (the hit, t_hi) or 1 (the bracket's midpoint)");
    return 0;
}

extern "C" {

int brief_surface_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                            int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level,
                            int32_t side, int32_t *hits, int32_t *first, void *stream)
{
    ViewChunk ch;
    SurfaceTest t;
    if (int rc = check_view_part_chunk(view, part, k0, off, s0, s1, r0, r1, lanes, &ch)) return rc;
    if (!vals || !hits || !first) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(elem_kind, channels, channel, level, side, &t)) return rc;
    const dim3 grid(view_blocks((r1 - r0) << ch.lg)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_kind == BRIEF_OUT_U8)
        hipLaunchKernelGGL((k_surface_part_fold<uint8_t>), grid, block, 0, st, *view, *part, ch, k0, off, (const uint8_t *)vals, (int)channels, t, hits, first);
    else
        hipLaunchKernelGGL((k_surface_part_fold<uint16_t>), grid, block, 0, st, *view, *part, ch, k0, off, (const uint16_t *)vals, (int)channels, t, hits, first);
    HIP_TRY(hipGetLastError());
    return 0;
}

// parts is DEVICE memory: it cannot be read before the launch, so its entries are trusted (the kernel only compares floats against
// them: a malformed entry gives a wrong owner, never an access out of bounds).  brief_surface_part_route_host checks entry by entry.
int brief_surface_part_route(const brief_view_desc *view, const brief_view_part *parts, int32_t nparts, float *t_lo, const float *t_hi, int32_t midpoint,
                             int32_t *owner, void *stream)
{
    int64_t rays;
    if (int rc = check_route(view, parts, nparts, t_lo, t_hi, midpoint, owner, &rays)) return rc;
    hipLaunchKernelGGL(k_surface_part_route, dim3(view_blocks(rays)), dim3(256), 0, (hipStream_t)stream, *view, parts, nparts, (int)midpoint, t_lo, t_hi, owner);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_part_coords(const brief_view_desc *view, const brief_view_part *part, const float *t_lo, const float *t_hi, int32_t midpoint,
                              const int64_t *rays, int64_t n, float *coords, float *pos, void *stream)
{
    int64_t image;
    if (int rc = check_view_part(view, part)) return rc;
    if (int rc = check_surface_rays(view, &image)) return rc;
    if (int rc = check_surface_list(rays, n)) return rc;
    if (!t_lo || !t_hi || !coords) return fail(BRIEF_ERR_INVALID, "surface: null buffer (pos alone may be NULL)");
    if (midpoint != 0 && midpoint != 1) return fail(BRIEF_ERR_INVALID, "surface: midpoint must be 0 (the hit, t_hi) or 1 (the bracket's midpoint)");
    SurfaceVec step;
    for (int a = 0; a < 3; ++a) step.v[a] = brief_view_part_step(*view, *part, a);
    hipLaunchKernelGGL(k_surface_part_coords, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, *view, *part, step, (int)midpoint, t_lo, t_hi, rays, n,
                       coords, pos);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_part_step(const int64_t *rays, int64_t n, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                            float *t_lo, float *t_hi, void *stream)
{
    SurfaceTest t;
    if (int rc = check_surface_list(rays, n)) return rc;
    if (!vals || !t_lo || !t_hi) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(elem_kind, channels, channel, level, side, &t)) return rc;
    const dim3 grid(view_blocks(n)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_kind == BRIEF_OUT_U8) hipLaunchKernelGGL((k_surface_part_step<uint8_t>), grid, block, 0, st, rays, n, (const uint8_t *)vals, (int)channels, t, t_lo, t_hi);
    else hipLaunchKernelGGL((k_surface_part_step<uint16_t>), grid, block, 0, st, rays, n, (const uint16_t *)vals, (int)channels, t, t_lo, t_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_surface_part_shade(const int64_t *rays, int64_t n, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                             const float *gscale, const float *light, float *normal, float *shade, void *stream)
{
    SurfaceTest test;
    if (int rc = check_surface_list(rays, n)) return rc;
    if (!t || !jac || !gscale || !light || !normal || !shade) return fail(BRIEF_ERR_INVALID, "surface: null buffer");
    if (int rc = check_surface_test(BRIEF_OUT_U16, channels, channel, 0, side, &test)) return rc;
    SurfaceVec g, l;
    for (int a = 0; a < 3; ++a) {
        g.v[a] = gscale[a]; l.v[a] = light[a];
        if (g.v[a] - g.v[a] != 0.f || l.v[a] - l.v[a] != 0.f) return fail(BRIEF_ERR_INVALID, "surface: gscale and light must be finite");
    }
    hipLaunchKernelGGL(k_surface_part_shade, dim3(view_blocks(n)), dim3(256), 0, (hipStream_t)stream, rays, n, t, jac, (int)channels, test, g, l, normal, shade);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same header on the host CPU: no GPU call.  Every buffer is host memory; t_lo is updated in place, as the kernel updates it.
int brief_surface_part_route_host(const brief_view_desc *view, const brief_view_part *parts, int32_t nparts, float *t_lo, const float *t_hi,
                                  int32_t midpoint, int32_t *owner)
{
    int64_t rays;
    if (int rc = check_route(view, parts, nparts, t_lo, t_hi, midpoint, owner, &rays)) return rc;
    for (int32_t b = 0; b < nparts; ++b)
        if (int rc = check_route_part(view, parts + b)) return rc;
    for (int32_t row = 0; row < view->rows; ++row)
        for (int32_t col = 0; col < view->cols; ++col) {
            const int64_t r = (int64_t)row * view->cols + col;
            owner[r] = brief_view_part_route(*view, parts, nparts, row, col, t_lo[r], t_hi[r], midpoint != 0);
        }
    return 0;
}

// brief_view_part_sample_host at a real depth t, 0 <= t <= depth - 1: the points the refinement evaluates for the block
int brief_view_part_sample_t_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *row, const int32_t *col, const float *t,
                                  int64_t n, float *pos, float *local, float *coord, uint8_t *inside, uint8_t *owned)
{
    if (int rc = check_view_part(view, part)) return rc;
    if (!row || !col || !t || n < 0) return fail(BRIEF_ERR_INVALID, "view: null index buffer or negative count");
    float step[3];
    for (int a = 0; a < 3; ++a) step[a] = brief_view_part_step(*view, *part, a);
    for (int64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= view->rows || col[i] < 0 || col[i] >= view->cols || !(t[i] >= 0.f && t[i] <= (float)(view->depth - 1)))
            return fail(BRIEF_ERR_INVALID, "view: a sample outside rows x cols x [0, depth - 1]");
        float p[3], q[3];
        for (int a = 0; a < 3; ++a) {
            p[a] = brief_view_at_t(*view, a, brief_view_base(*view, a, row[i], col[i]), t[i]);
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
