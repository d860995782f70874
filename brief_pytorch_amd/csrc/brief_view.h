// brief_view.h — the geometry of the orthographic view decode (brief_pytorch_amd/view.py, csrc/brief_view.inc), defined once: the scalar
// functions the gfx950 kernels call, compiled on the host too (brief_view_sample_host / brief_view_clip_host, tests/test_view_host.py).
//
// A view is a lattice of samples (row, col, k), row < rows, col < cols, k < depth, in VOXEL-INDEX space of the fitted grid `dims`.
// Every fp32 operation rounds on its own; nothing is contracted into an fma except where an fma is written:
//     position    p_a = fl(fl(fl(origin_a + fl(row * drow_a)) + fl(col * dcol_a)) + fl(k * ddepth_a))       (row, col, k < 2^24: exact floats)
//     inside      box_lo_a <= p_a <= box_hi_a on every axis
//     coordinate  step_a = fl(fl(hi - lo) / (float)(n_a - 1))                                               (fill_grid of brief_hip.hip)
//                 x_a = p_a < (float)(n_a / 2) ? fma(step_a, p_a, lo) : fma(-step_a, (float)(n_a - 1) - p_a, hi)
// The coordinate is lin_coord's two-sided form (brief_device.inc) taken at a real position: at an integer position it is the grid's
// own coordinate of that voxel, bit for bit, so an axis-aligned view of unit spacing reproduces the grid decode.
//
// Ray range.  With row and col fixed, every p_a is a monotone function of k (k -> fl(k * d) is monotone, and so is x -> fl(b + x)),
// so the inside samples of a ray are ONE interval of k.  brief_view_ray_range finds it by bisection on the position function itself:
// the range it returns holds every inside sample of the ray and nothing else, whatever the roundings do at a face the ray skims.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#ifndef BRIEF_HD
#define BRIEF_HD __host__ __device__ __forceinline__
#endif
#else
#include <cmath>
#ifndef BRIEF_HD
#define BRIEF_HD static inline
#endif
#endif

#if defined(__clang__)
#define BRIEF_VIEW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BRIEF_VIEW_NO_CONTRACT      /* g++: built with -ffp-contract=off */
#endif

// the ray's foot: the position of sample (row, col, 0) on axis a
BRIEF_HD float brief_view_base(const brief_view_desc &v, int a, int32_t row, int32_t col)
{
    BRIEF_VIEW_NO_CONTRACT
    const float r = (float)row * v.drow[a];
    const float c = (float)col * v.dcol[a];
    const float t = v.origin[a] + r;
    return t + c;
}

BRIEF_HD float brief_view_at(const brief_view_desc &v, int a, float base, int32_t k)
{
    BRIEF_VIEW_NO_CONTRACT
    const float d = (float)k * v.ddepth[a];
    return base + d;
}

// the same at a real depth t (the surface view's refinement): p_a = fl(base_a + fl(t * ddepth_a)).  (float)k is exact for k < 2^24, so
// at an integer t this is brief_view_at, bit for bit; and t -> p_a is monotone, as k -> p_a is.
BRIEF_HD float brief_view_at_t(const brief_view_desc &v, int a, float base, float t)
{
    BRIEF_VIEW_NO_CONTRACT
    const float d = t * v.ddepth[a];
    return base + d;
}

// the midpoint of a bracket, t_mid = fl(t_lo + fl(0.5f * fl(t_hi - t_lo))): never outside [t_lo, t_hi]
BRIEF_HD float brief_view_mid(float t_lo, float t_hi)
{
    BRIEF_VIEW_NO_CONTRACT
    const float w = t_hi - t_lo;
    const float h = 0.5f * w;
    return t_lo + h;
}

BRIEF_HD float brief_view_pos(const brief_view_desc &v, int a, int32_t row, int32_t col, int32_t k)
{
    return brief_view_at(v, a, brief_view_base(v, a, row, col), k);
}

BRIEF_HD bool brief_view_inside(const brief_view_desc &v, float p0, float p1, float p2)
{
    return v.box_lo[0] <= p0 && p0 <= v.box_hi[0] && v.box_lo[1] <= p1 && p1 <= v.box_hi[1] && v.box_lo[2] <= p2 && p2 <= v.box_hi[2];
}

BRIEF_HD float brief_view_step(const brief_view_desc &v, int a)
{
    BRIEF_VIEW_NO_CONTRACT
    const float spread = v.hi - v.lo;
    return v.dims[a] > 1 ? spread / (float)(v.dims[a] - 1) : 0.f;
}

BRIEF_HD float brief_view_coord(const brief_view_desc &v, int a, float step, float p)
{
    BRIEF_VIEW_NO_CONTRACT
    const int64_t nn = v.dims[a];
    if (p < (float)(nn / 2)) return fmaf(step, p, v.lo);
    const float back = (float)(nn - 1) - p;
    return fmaf(-step, back, v.hi);
}

// the first k in [0, depth] at which `p_a(k) >= bound` (ge) or `p_a(k) > bound` (!ge) holds, for a position that does not decrease with k
// (rising) or does not increase (then the first k at which `<=` / `<` holds); depth if it never does
BRIEF_HD int32_t brief_view_first(const brief_view_desc &v, int a, float base, float bound, bool rising, bool strict)
{
    int32_t lo = 0, hi = v.depth;                    // the predicate is false below lo and true from hi on
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const float p = brief_view_at(v, a, base, mid);
        const bool t = rising ? (strict ? p > bound : p >= bound) : (strict ? p < bound : p <= bound);
        if (t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the inside samples of ray (row, col) are exactly k0 <= k < k0 + cnt (cnt == 0: the ray misses the box; k0 is 0 then)
BRIEF_HD void brief_view_ray_range(const brief_view_desc &v, int32_t row, int32_t col, int32_t &k0, int32_t &cnt)
{
    int32_t b = 0, e = v.depth;
    for (int a = 0; a < 3; ++a) {
        const float base = brief_view_base(v, a, row, col);
        const bool rising = !(v.ddepth[a] < 0.f);
        // rising: inside from the first p >= box_lo up to the first p > box_hi; falling: from the first p <= box_hi up to the first p < box_lo
        const int32_t first = brief_view_first(v, a, base, rising ? v.box_lo[a] : v.box_hi[a], rising, false);
        const int32_t end = brief_view_first(v, a, base, rising ? v.box_hi[a] : v.box_lo[a], rising, true);
        b = first > b ? first : b;
        e = end < e ? end : e;
    }
    cnt = e > b ? e - b : 0;
    k0 = cnt ? b : 0;
}

// ---- a view of a PARTITION (a DivideTask artefact: one net per block): the nearest block owns a sample.
// The lattice stays the view's, in the voxel-index space of the WHOLE volume: p_a is brief_view_pos, unchanged.  A block with the
// inclusive index range [s_a, e_a], n_a = e_a - s_a + 1, owns the half-open CELL
//     owned       (float)s_a - 0.5f <= p_a < (float)(s_a + n_a) - 0.5f on every axis      (exact floats: every axis is below 2^23)
// and a sample is evaluated for the block iff it is inside the clip box (brief_view_inside) AND owned.  Both tests read the global
// float p_a, and the cells of a tiling partition are disjoint and cover [-0.5, N - 0.5): a sample inside the clip box has exactly ONE
// owner, whatever the roundings do at a face a ray skims; a sample in a gap no block covers has none.
//     local       q_a = fl(p_a - (float)s_a)
//     coordinate  brief_view_coord's two-sided form on the block's own grid: step_a = fl(fl(hi - lo) / (float)(n_a - 1)),
//                 x_a = q_a < (float)(n_a / 2) ? fma(step_a, q_a, lo) : fma(-step_a, (float)(n_a - 1) - q_a, hi)
// At an integer position q_a is exact and x_a is the block grid's own coordinate, bit for bit.  For q_a in [-0.5, 0) or
// (n_a - 1, n_a - 0.5) the block's net is evaluated up to half a voxel OUTSIDE its grid: that is what "nearest" means.
// Ray range: p_a(k) is monotone, so "inside the clip box and owned" is still one interval of k, the intersection of
// brief_view_ray_range's with the cell's; the cell's ends are found by the same bisection (brief_view_first).
// Only the rays of the block's WINDOW, [row0, row0 + wrows) x [col0, col0 + wcols) of the image, are clipped and walked: the host
// computes it so that every ray outside it misses the block (view.make_part).  The view's origin is NOT moved into the window: that
// would change the roundings of p and break single ownership.
BRIEF_HD float brief_view_part_cell_lo(const brief_view_part &pt, int a) { return (float)pt.start[a] - 0.5f; }
BRIEF_HD float brief_view_part_cell_hi(const brief_view_part &pt, int a) { return (float)(pt.start[a] + pt.dims[a]) - 0.5f; }

BRIEF_HD bool brief_view_part_owned(const brief_view_part &pt, float p0, float p1, float p2)
{
    return brief_view_part_cell_lo(pt, 0) <= p0 && p0 < brief_view_part_cell_hi(pt, 0) && brief_view_part_cell_lo(pt, 1) <= p1 &&
           p1 < brief_view_part_cell_hi(pt, 1) && brief_view_part_cell_lo(pt, 2) <= p2 && p2 < brief_view_part_cell_hi(pt, 2);
}

BRIEF_HD float brief_view_part_step(const brief_view_desc &v, const brief_view_part &pt, int a)
{
    BRIEF_VIEW_NO_CONTRACT
    const float spread = v.hi - v.lo;
    return pt.dims[a] > 1 ? spread / (float)(pt.dims[a] - 1) : 0.f;
}

BRIEF_HD float brief_view_part_local(const brief_view_part &pt, int a, float p)
{
    BRIEF_VIEW_NO_CONTRACT
    return p - (float)pt.start[a];
}

BRIEF_HD float brief_view_part_coord(const brief_view_desc &v, const brief_view_part &pt, int a, float step, float q)
{
    BRIEF_VIEW_NO_CONTRACT
    const int64_t nn = pt.dims[a];
    if (q < (float)(nn / 2)) return fmaf(step, q, v.lo);
    const float back = (float)(nn - 1) - q;
    return fmaf(-step, back, v.hi);
}

// the samples of ray (row, col) the block evaluates are exactly k0 <= k < k0 + cnt (cnt == 0: none; k0 is 0 then)
BRIEF_HD void brief_view_part_ray_range(const brief_view_desc &v, const brief_view_part &pt, int32_t row, int32_t col, int32_t &k0, int32_t &cnt)
{
    int32_t b = 0, e = v.depth;
    for (int a = 0; a < 3; ++a) {
        const float base = brief_view_base(v, a, row, col);
        const bool rising = !(v.ddepth[a] < 0.f);
        const float c_lo = brief_view_part_cell_lo(pt, a), c_hi = brief_view_part_cell_hi(pt, a);
        // the clip box, closed: brief_view_ray_range's two bounds
        int32_t first = brief_view_first(v, a, base, rising ? v.box_lo[a] : v.box_hi[a], rising, false);
        int32_t end = brief_view_first(v, a, base, rising ? v.box_hi[a] : v.box_lo[a], rising, true);
        b = first > b ? first : b;
        e = end < e ? end : e;
        // the cell, half-open.  rising: from the first p >= s - 0.5 up to the first p >= e + 0.5; falling: from the first p < e + 0.5 up
        // to the first p < s - 0.5
        first = brief_view_first(v, a, base, rising ? c_lo : c_hi, rising, !rising);
        end = brief_view_first(v, a, base, rising ? c_hi : c_lo, rising, !rising);
        b = first > b ? first : b;
        e = end < e ? end : e;
    }
    cnt = e > b ? e - b : 0;
    k0 = cnt ? b : 0;
}

// ---- the surface view of a PARTITION: every point the refinement evaluates, and the hit itself, is ROUTED to the block that owns it.
// The depth a round evaluates is the surface view's: the midpoint of a bracket (brief_view_mid) where t_lo < t_hi and the round asks for
// it, else t_hi (the hit; NaN without one).  The point's owner is found by the same half-open cell test on the same global float
// p_a = brief_view_at_t(...) that gives a sample its owner (brief_view_part_owned): a point exactly on a face s - 0.5 belongs to the
// UPPER block, and a point no block's cell holds (a pruned block's gap) has no owner, -1.  The gap rule `empty`: such a point holds
// nothing, it fails the side test on either side, so an unowned midpoint becomes the new t_lo.
BRIEF_HD float brief_view_surface_t(float t_lo, float t_hi, bool mid) { return mid && t_lo < t_hi ? brief_view_mid(t_lo, t_hi) : t_hi; }

// the index of the block among parts[0 .. nparts) whose cell holds p, -1 if none does (the first one, should cells overlap)
BRIEF_HD int32_t brief_view_part_owner(const brief_view_part *parts, int32_t nparts, float p0, float p1, float p2)
{
    for (int32_t b = 0; b < nparts; ++b)
        if (brief_view_part_owned(parts[b], p0, p1, p2)) return b;
    return -1;
}

// one ray's routing: the owner of its point at brief_view_surface_t(t_lo, t_hi, mid), -1 where the ray has nothing to evaluate (NaN;
// with mid, not t_lo < t_hi; with mid, a point in a gap, and then t_lo becomes the midpoint)
BRIEF_HD int32_t brief_view_part_route(const brief_view_desc &v, const brief_view_part *parts, int32_t nparts, int32_t row, int32_t col, float &t_lo,
                                       float t_hi, bool mid)
{
    if (mid && !(t_lo < t_hi)) return -1;
    const float t = brief_view_surface_t(t_lo, t_hi, mid);
    if (!(t == t)) return -1;
    const int32_t o = brief_view_part_owner(parts, nparts, brief_view_at_t(v, 0, brief_view_base(v, 0, row, col), t),
                                            brief_view_at_t(v, 1, brief_view_base(v, 1, row, col), t),
                                            brief_view_at_t(v, 2, brief_view_base(v, 2, row, col), t));
    if (mid && o < 0) t_lo = t;
    return o;
}
