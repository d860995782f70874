// brief_rays.h — the geometry of the RAY VIEW (brief_pytorch_amd/view.py make_camera / render_rays, csrc/brief_rays.inc), defined once: the
// scalar functions the gfx950 kernels call, compiled on the host too (brief_rays_sample_host / _sample_t_host / _clip_host,
// tests/test_camera_host.py).
//
// A ray view is rows x cols rays of `depth` samples each; ray r = row * cols + col is six floats of a table,
//     ray[0 .. 3) = base (z, y, x), ray[3 .. 6) = dd (z, y, x)                                              VOXEL-INDEX units of the fitted grid
// so a ray bundle may fan out from a point (a perspective camera) or be any set of rays a caller fills in.  Per ray it is the
// orthographic view's arithmetic (csrc/brief_view.h) with a foot and a step of its own; every fp32 operation rounds on its own:
//     position    p_a(r, k) = fl(base_a[r] + fl((float)k * dd_a[r]))          (brief_view_at; k < 2^24: an exact float)
//     real depth  p_a(r, t) = fl(base_a[r] + fl(t * dd_a[r]))                 (brief_view_at_t)
//     inside      brief_view_inside, coordinate brief_view_coord / brief_view_step: the very functions, called on the brief_view_desc
//                 brief_rays_view() makes of the descriptor (dims, lo / hi, rows, cols, depth, the clip box; origin and steps zero).
// A table filled from an orthographic view (base = that view's sample (row, col, 0), dd = its ddepth) therefore gives that view's
// positions, coordinates and inside flags bit for bit.
//
// Ray range.  Along a ray every p_a is monotone in k whatever the ray's direction, so the inside samples are ONE interval of k, found
// by brief_view_first's bisection on the ray's own position function; the direction is per ray, rising = !(dd_a < 0), and a zero
// component is legal (the position is constant on that axis: the bisection gives 0 or depth).  Whatever the table holds, NaN
// included, the bisection runs ceil(log2(depth + 1)) steps and 0 <= k0 <= k0 + cnt <= depth: a bad table may give a wrong image, never
// an index outside a buffer or an unbounded loop.
#pragma once
#include "brief_view.h"

// the orthographic descriptor that carries what is not per ray: what brief_view_inside / _coord / _step, brief_view_finish,
// brief_surface_bracket and brief_surface_step read
BRIEF_HD brief_view_desc brief_rays_view(const brief_rays_desc &d)
{
    brief_view_desc v;
    for (int a = 0; a < 3; ++a) {
        v.dims[a] = d.dims[a];
        v.origin[a] = v.drow[a] = v.dcol[a] = v.ddepth[a] = 0.f;
        v.box_lo[a] = d.box_lo[a];
        v.box_hi[a] = d.box_hi[a];
    }
    v.lo = d.lo; v.hi = d.hi;
    v.rows = d.rows; v.cols = d.cols; v.depth = d.depth; v.reserved = 0;
    return v;
}

BRIEF_HD float brief_rays_at(const float *ray, int a, int32_t k)
{
    BRIEF_VIEW_NO_CONTRACT
    const float d = (float)k * ray[3 + a];
    return ray[a] + d;
}

BRIEF_HD float brief_rays_at_t(const float *ray, int a, float t)
{
    BRIEF_VIEW_NO_CONTRACT
    const float d = t * ray[3 + a];
    return ray[a] + d;
}

// brief_view_first on the ray's own position: the first k in [0, depth] at which the predicate holds, depth if it never does
BRIEF_HD int32_t brief_rays_first(int32_t depth, const float *ray, int a, float bound, bool rising, bool strict)
{
    int32_t lo = 0, hi = depth;                      // the predicate is false below lo and true from hi on
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const float p = brief_rays_at(ray, a, mid);
        const bool t = rising ? (strict ? p > bound : p >= bound) : (strict ? p < bound : p <= bound);
        if (t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the inside samples of the ray are exactly k0 <= k < k0 + cnt (cnt == 0: the ray misses the box; k0 is 0 then)
BRIEF_HD void brief_rays_ray_range(const brief_view_desc &v, const float *ray, int32_t &k0, int32_t &cnt)
{
    int32_t b = 0, e = v.depth;
    for (int a = 0; a < 3; ++a) {
        const bool rising = !(ray[3 + a] < 0.f);
        const int32_t first = brief_rays_first(v.depth, ray, a, rising ? v.box_lo[a] : v.box_hi[a], rising, false);
        const int32_t end = brief_rays_first(v.depth, ray, a, rising ? v.box_hi[a] : v.box_lo[a], rising, true);
        b = first > b ? first : b;
        e = end < e ? end : e;
    }
    cnt = e > b ? e - b : 0;
    k0 = cnt ? b : 0;
}
