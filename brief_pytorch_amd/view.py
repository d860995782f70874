"""Oblique slices and projections of a stored artefact along any direction: an orthographic view decode.  A view is a lattice of
rows x cols parallel rays with `depth` samples each, anywhere in the volume and at any orientation.  Only the samples inside the clip
box are evaluated, by the net's own forward entry on explicit coordinates, chunk by chunk; each chunk is folded into per-pixel
accumulators on the device (max | min | mean along the ray, or a single plane: slice) and dropped.  The volume is never decoded.
(csrc/brief_view.h has the geometry, csrc/brief_view.inc the kernels, DESIGN.md "View decode" the reasoning.)

The surface view (render_surface, decompress_surface) folds the same march to the FIRST sample of every ray at which a channel
crosses a level, refines that hit by bisection and shades it with the net's analytic normal (DESIGN.md "Surface view").

A view of a DivideTask artefact (render_partition, decompress_divide_view) is the same lattice over the whole volume with one net per
block: the nearest block owns a sample (DESIGN.md "View decode of a partition").  Its march, _march_partition, also serves the composite
of a partition (composite.render_composite_partition) and its surface view (render_surface_partition, decompress_divide_surface: every
refinement point and the hit are routed to the block that owns them; DESIGN.md "Surface view of a partition").

A ray view (make_camera, rays_from_view, render_rays, render_surface_rays, decompress_camera, decompress_camera_surface) takes its
rays from a table instead of a lattice, six floats per ray: a perspective camera at a point, inside the volume or outside it, through
the same march and folds (csrc/brief_rays.h, csrc/brief_rays.inc, DESIGN.md "Camera view").

make_view, make_camera, part_window and make_part are host arithmetic; brief_rays_sample_host / _sample_t_host / _clip_host and brief_view_sample_host / brief_view_sample_t_host / brief_view_clip_host,
brief_view_part_clip_host / brief_view_part_sample_host / brief_view_part_sample_t_host and brief_surface_part_route_host restate the
device's geometry on the CPU; everything else needs a ROCm GPU
(there is no CPU fallback)."""
import ctypes as C
import math
import os

import numpy as np

from . import _lib, artefact
from . import region as region_mod

MODES = ("max", "min", "mean", "slice")
MAX_COUNT = 1 << 24          # rows, cols and depth travel as floats
OWNERS = ("nearest",)
DIVIDE_REFUSAL = ("view decode of a DivideTask artefact is refused unless the ownership rule is named: every block has its own net and "
                  "coordinate grid, and a sample between two blocks needs an owner; ask for --view-owner nearest "
                  "(decompress_divide_view: the nearest block owns a sample; nothing is blended across a face, that is a follow-up).  "
                  "The surface view of a partition also asks for its gap rule, --view-surface-gap empty (decompress_divide_surface)")
PART_MAX_DIM = 1 << 23       # a block's cell bounds s - 0.5 and e + 0.5 are exact floats below it


def _vec3(v, what):
    try:
        out = np.array([float(x) for x in v], np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be three numbers in (z, y, x) order (got %r)" % (what, v)) from None
    if out.shape != (3,) or not np.isfinite(out).all():
        raise ValueError("%s must be three finite numbers in (z, y, x) order (got %r)" % (what, v))
    return out


def _positive(v, what):
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise ValueError("%s must be a positive finite number (got %r)" % (what, v))
    return v


def _count(span, spacing, what):
    n = int(math.floor(span / spacing + 1e-9)) + 1
    if n >= MAX_COUNT:
        raise ValueError("%s = %d is refused: sizes of 2^24 and above are not exact in a float" % (what, n))
    return max(n, 1)


def frame(direction, up=None):
    """the orthonormal PHYSICAL frame (row_dir, col_dir, direction) of a view, float64, each in (z, y, x) order.  `direction` is
    normalised; the rows of the image run along `up` made orthogonal to it (default: the grid axis the direction has least of, the
    first of them on a tie); col_dir = direction x row_dir with (z, y, x) as the three components, so (direction, row_dir, col_dir)
    is a proper rotation of (z, y, x) and a turning direction never mirrors the image.  Looking along +z gives rows = y, cols = x,
    along +x rows = z, cols = y, along -y rows = z, cols = x: the orientations of mip_ops' three images."""
    d = _vec3(direction, "direction")
    if not np.linalg.norm(d) > 0:
        raise ValueError("direction must not be the zero vector")
    d = d / np.linalg.norm(d)
    if up is None:
        u = np.zeros(3)
        u[int(np.argmin(np.abs(d)))] = 1.0
    else:
        u = _vec3(up, "up")
        if not np.linalg.norm(u) > 0:
            raise ValueError("up must not be the zero vector")
    r = u - np.dot(u, d) * d
    if not np.linalg.norm(r) > 1e-9 * np.linalg.norm(u):
        raise ValueError("up %r is parallel to direction %r: the image's rows have no direction" % (tuple(u), tuple(d)))
    r = r / np.linalg.norm(r)
    c = np.cross(d, r)
    return r, c / np.linalg.norm(c), d


def make_view(dims, direction, up=None, centre=None, spacing=1.0, depth_spacing=1.0, size=None, depth=None, voxel_size=(1, 1, 1), region=None):
    """the descriptor (_lib.ViewDesc = brief_view_desc) of an orthographic view of the grid `dims` (3 spatial axes, (z, y, x)).
    direction, up: see frame(); they are PHYSICAL directions, voxel_size (sz, sy, sx) being a voxel's physical extent per axis
                   (every step is divided by it per axis to give voxel-index units).
    centre:        the voxel-index position the view is centred on (default: the volume's centre, (n - 1) / 2 per axis).
    spacing, depth_spacing: distance between neighbouring pixels / between samples of a ray, in physical units (voxels for the
                   default voxel_size).
    region:        the clip box (numpy slice semantics per axis, step 1 only; default the whole grid): samples outside it are
                   never evaluated and never folded.
    size:          (rows, cols), centred on `centre`; default: the smallest image that covers the clip box's projection.
    depth:         (t0, t1), the range along `direction` relative to `centre` in physical units, sampled at t0, t0 + depth_spacing,
                   ... <= t1; a single number t is the one plane (t, t); default: the range that covers the clip box.
    Everything is computed in float64 and rounded to fp32 once.  lo / hi of the descriptor are set by render()."""
    dims = [int(v) for v in dims]
    if len(dims) != 3:
        raise ValueError("a view is defined for 3-D data only (got a %d-D grid)" % len(dims))
    if any(n < 2 for n in dims):
        raise ValueError("a view needs every axis of the grid to be at least 2 voxels long (got %s): an axis of length 1 has no coordinate "
                         "range to sample" % (dims,))
    vs = _vec3(voxel_size, "voxel_size")
    if (vs <= 0).any():
        raise ValueError("voxel_size must be positive on every axis (got %r)" % (tuple(voxel_size),))
    spacing, depth_spacing = _positive(spacing, "spacing"), _positive(depth_spacing, "depth_spacing")
    row_dir, col_dir, d = frame(direction, up)
    start, stop, step = region_mod.normalize_region(dims, region if region is not None else (slice(None),) * 3, 1)
    if any(s != 1 for s in step):
        raise ValueError("the clip box of a view is a box, not a lattice: region steps other than 1 are refused (got %s)" % (step,))
    box_lo, box_hi = np.array(start, np.float64), np.array(stop, np.float64) - 1.0
    c = (np.array(dims, np.float64) - 1.0) / 2.0 if centre is None else _vec3(centre, "centre")
    corners = np.array([[(box_lo, box_hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
    rel = (corners - c) * vs                                     # physical offsets of the clip box's corners from the centre
    pu, pv, pw = rel @ row_dir, rel @ col_dir, rel @ d
    if size is None:
        u0, v0 = float(pu.min()), float(pv.min())
        rows, cols = _count(float(pu.max()) - u0, spacing, "rows"), _count(float(pv.max()) - v0, spacing, "cols")
    else:
        try:
            rows, cols = (int(x) for x in size)
        except (TypeError, ValueError):
            raise ValueError("size must be (rows, cols) (got %r)" % (size,)) from None
        if rows < 1 or cols < 1:
            raise ValueError("size must be at least 1 x 1 (got %r)" % (size,))
        if rows >= MAX_COUNT or cols >= MAX_COUNT:
            raise ValueError("size %r is refused: sizes of 2^24 and above are not exact in a float" % (size,))
        u0, v0 = -(rows - 1) / 2.0 * spacing, -(cols - 1) / 2.0 * spacing
    if depth is None:
        w0 = float(pw.min())
        nk = _count(float(pw.max()) - w0, depth_spacing, "depth")
    else:
        t0, t1 = (float(depth), float(depth)) if np.isscalar(depth) else (float(x) for x in depth)
        if not (math.isfinite(t0) and math.isfinite(t1) and t1 >= t0):
            raise ValueError("depth must be a finite range (t0, t1) with t1 >= t0 (got %r)" % (depth,))
        w0, nk = t0, _count(t1 - t0, depth_spacing, "depth")
    v = _lib.ViewDesc()
    origin = c + (u0 * row_dir + v0 * col_dir + w0 * d) / vs
    for a in range(3):
        v.dims[a] = dims[a]
        v.origin[a] = origin[a]
        v.drow[a], v.dcol[a], v.ddepth[a] = spacing * row_dir[a] / vs[a], spacing * col_dir[a] / vs[a], depth_spacing * d[a] / vs[a]
        v.box_lo[a], v.box_hi[a] = box_lo[a], box_hi[a]
    v.lo, v.hi = -1.0, 1.0
    v.rows, v.cols, v.depth = rows, cols, nk
    return v


def _with_range(view, lo, hi):
    v = _lib.ViewDesc.from_buffer_copy(view)
    v.lo, v.hi = float(lo), float(hi)
    return v


def sample_host(view, row, col, k):
    """(pos [n, 3] float32, coord [n, 3] float32, inside [n] bool) of the samples (row, col, k) as the device computes them: the same
    header on the host CPU (brief_view_sample_host), no GPU call"""
    row, col, k = (np.ascontiguousarray(x, np.int32).ravel() for x in (row, col, k))
    n = len(row)
    if len(col) != n or len(k) != n:
        raise ValueError("row, col and k must have one entry per sample")
    pos, coord, inside = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_view_sample_host(C.byref(view), p(row), p(col), p(k), n, p(pos), p(coord), p(inside)))
    return pos, coord, inside.astype(bool)


def clip_host(view):
    """(k0 [rows, cols], cnt [rows, cols]) int32: the inside samples of every ray, k0 <= k < k0 + cnt, on the host CPU"""
    k0, cnt = np.empty((view.rows, view.cols), np.int32), np.empty((view.rows, view.cols), np.int32)
    _lib.check(_lib.lib().brief_view_clip_host(C.byref(view), k0.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
    return k0, cnt


def sample_t_host(view, row, col, t):
    """sample_host at real depths t (float32, 0 <= t <= depth - 1): position p_a = fl(base_a + fl(t * ddepth_a)), the positions the
    surface view's refinement evaluates (brief_view_sample_t_host); at an integer t it is sample_host's sample k = t, bit for bit"""
    row, col = (np.ascontiguousarray(x, np.int32).ravel() for x in (row, col))
    t = np.ascontiguousarray(t, np.float32).ravel()
    n = len(row)
    if len(col) != n or len(t) != n:
        raise ValueError("row, col and t must have one entry per sample")
    pos, coord, inside = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_view_sample_t_host(C.byref(view), p(row), p(col), p(t), n, p(pos), p(coord), p(inside)))
    return pos, coord, inside.astype(bool)


def _lanes(mean_count):
    """adjacent lanes that share a ray: the power of two at or above the mean samples per hit ray, 1 .. 64"""
    g = 1
    while g < 64 and g < mean_count:
        g *= 2
    return g


class _Lattice:
    """the geometry of an orthographic view as the shared march and renderers call it: the descriptor (lo / hi set) and the entries
    that read it.  _Bundle is the same for a ray view; everything else of a render is shared."""
    slice_ok = True

    def __init__(self, v):
        self.desc = self.flat = v               # flat: the brief_view_desc that finish, bracket and step read rows x cols of
        self.rows, self.cols, self.depth = v.rows, v.cols, v.depth

    def clip(self, k0, cnt):
        _lib.check(_lib.lib().brief_view_clip(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(cnt), _lib.stream_ptr()))

    def coords(self, k0, off, s0, s1, r0, r1, lanes, coords):
        _lib.check(_lib.lib().brief_view_coords(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(coords), _lib.stream_ptr()))

    def fold(self, k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, m, hits, acc):
        _lib.check(_lib.lib().brief_view_fold(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch, m,
                                              _lib.ptr(hits), _lib.ptr(acc), _lib.stream_ptr()))

    def surface_fold(self, k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, channel, level, sd, hits, first):
        _lib.check(_lib.lib().brief_surface_fold(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch, channel,
                                                 level, sd, _lib.ptr(hits), _lib.ptr(first), _lib.stream_ptr()))

    def surface_coords(self, t_lo, t_hi, mid, coords, pos):
        _lib.check(_lib.lib().brief_surface_coords(C.byref(self.desc), _lib.ptr(t_lo), _lib.ptr(t_hi), mid, _lib.ptr(coords), _lib.ptr(pos),
                                                   _lib.stream_ptr()))

    def surface_shade(self, t, jac, ch, channel, sd, g, light, normal, shade):
        f3 = C.c_float * 3
        l = _unit3(light if light is not None else list(self.desc.ddepth), "light")
        _lib.check(_lib.lib().brief_surface_shade(C.byref(self.desc), _lib.ptr(t), _lib.ptr(jac), ch, channel, sd, f3(*g), f3(*l), _lib.ptr(normal),
                                                  _lib.ptr(shade), _lib.stream_ptr()))


class _Bundle(_Lattice):
    """the geometry of a ray view (a RayView with lo / hi set, its table and headlight on the device): brief_rays_*"""
    slice_ok = False

    def __init__(self, desc, table, light):
        self.desc, self.flat = desc, _flat_view(desc)
        self.rows, self.cols, self.depth = desc.rows, desc.cols, desc.depth
        self.table, self.light = table, light

    def clip(self, k0, cnt):
        _lib.check(_lib.lib().brief_rays_clip(C.byref(self.desc), _lib.ptr(self.table), _lib.ptr(k0), _lib.ptr(cnt), _lib.stream_ptr()))

    def coords(self, k0, off, s0, s1, r0, r1, lanes, coords):
        _lib.check(_lib.lib().brief_rays_coords(C.byref(self.desc), _lib.ptr(self.table), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes,
                                                _lib.ptr(coords), _lib.stream_ptr()))

    def fold(self, k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, m, hits, acc):
        _lib.check(_lib.lib().brief_rays_fold(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch, m,
                                              _lib.ptr(hits), _lib.ptr(acc), _lib.stream_ptr()))

    def surface_fold(self, k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, channel, level, sd, hits, first):
        _lib.check(_lib.lib().brief_rays_surface_fold(C.byref(self.desc), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch,
                                                      channel, level, sd, _lib.ptr(hits), _lib.ptr(first), _lib.stream_ptr()))

    def surface_coords(self, t_lo, t_hi, mid, coords, pos):
        _lib.check(_lib.lib().brief_rays_surface_coords(C.byref(self.desc), _lib.ptr(self.table), _lib.ptr(t_lo), _lib.ptr(t_hi), mid, _lib.ptr(coords),
                                                        _lib.ptr(pos), _lib.stream_ptr()))

    def surface_shade(self, t, jac, ch, channel, sd, g, light, normal, shade):
        import torch
        table = self.light                       # the per-ray headlight; a given light is one direction for every ray
        if light is not None:
            l = torch.from_numpy(_unit3(light, "light").astype(np.float32)).to(self.table.device)
            table = l.expand(self.rows * self.cols, 3).contiguous()
        f3 = C.c_float * 3
        _lib.check(_lib.lib().brief_rays_surface_shade(C.byref(self.desc), _lib.ptr(t), _lib.ptr(jac), ch, channel, sd, f3(*g), _lib.ptr(table),
                                                       _lib.ptr(normal), _lib.ptr(shade), _lib.stream_ptr()))


def _march(phi, v, kind, dt, scale, vrange, chunk, fold, with_coords=False):
    """the part every view shares: clip the rays of `v` (a descriptor with lo / hi set, or a _Lattice / _Bundle: the two geometries
    differ in the clip and the coords calls only), scan, and evaluate the compacted sample list chunk by chunk with
    the net's own forward entry, handing each chunk to fold(k0, off, s0, s1, r0, r1, lanes, vals); with_coords: the chunk's
    coordinates [n, 3] too, as the keyword `coords` (the shaded composite picks the samples it lights from them).
    Returns (k0, total, rays_hit)."""
    import torch
    geo = v if isinstance(v, _Lattice) else _Lattice(v)
    dev, ch = phi.params.device, int(phi.data_channel)
    rays = geo.rows * geo.cols
    k0, cnt = torch.empty(rays, dtype=torch.int32, device=dev), torch.empty(rays, dtype=torch.int32, device=dev)
    geo.clip(k0, cnt)
    off = torch.zeros(rays + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, dtype=torch.int64, out=off[1:])
    total, rays_hit = int(off[-1].item()), int((cnt > 0).sum().item())
    if total > 0:
        phi.sync_packed()
        lanes = _lanes(total / rays_hit)
        cuts = torch.tensor(list(range(0, total, chunk)) + [total], dtype=torch.int64, device=dev)
        r0s = torch.searchsorted(off[1:], cuts[:-1], right=True).cpu().tolist()       # the first ray that ends behind s0
        r1s = torch.searchsorted(off[:-1], cuts[1:], right=False).cpu().tolist()      # the first ray that starts at or behind s1
        cuts = cuts.cpu().tolist()
        coords = torch.empty((min(chunk, total), 3), dtype=torch.float32, device=dev)
        vals = torch.empty((min(chunk, total), ch), dtype=dt, device=dev)
        for s0, s1, r0, r1 in zip(cuts[:-1], cuts[1:], r0s, r1s):
            n = s1 - s0
            geo.coords(k0, off, s0, s1, r0, r1, lanes, coords)
            b = _lib.BatchDesc(coords.data_ptr(), None, None, None, 0, n, 0, 0, 0)
            _lib.check(phi._abi_forward(None, b, vals, kind, scale, vrange, n))
            if with_coords:
                fold(k0, off, s0, s1, r0, r1, lanes, vals, coords=coords)
            else:
                fold(k0, off, s0, s1, r0, r1, lanes, vals)
    return k0, total, rays_hit


def render(phi, view, mode, lo, hi, out_kind, scale, vrange, chunk=None):
    """the view of the net `phi` (any net kind and precision its forward entry serves) on the linspace grid view.dims over [lo, hi]:
    (image [rows, cols, channels], hits [rows, cols] int32, stats) as device tensors.  mode 'max' | 'min' | 'mean' folds the inside
    samples of every ray; 'slice' needs a view of depth 1 and gives that plane.  out_kind 'u8' | 'u16' with scale / vrange: the
    fused integer epilogue of decode_box; max / min / slice images are of that dtype, a mean is float32 (float)((double)sum / hits).
    Pixels whose ray has no inside sample (hits == 0) are 0.  Samples are evaluated in chunks of at most `chunk` (default
    mip.DEFAULT_CHUNK): the memory is one chunk of coordinates and values plus the accumulators, whatever the volume's size.
    stats = {rays, rays_hit, samples_inside, samples_evaluated}."""
    if mode not in MODES:
        raise ValueError("view mode %r is not one of %s" % (mode, " | ".join(MODES)))
    if out_kind not in ("u8", "u16"):
        raise ValueError("render folds the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    if mode == "slice" and view.depth != 1:
        raise ValueError("mode 'slice' needs a view of one plane (depth 1); this one has %d samples per ray" % view.depth)
    return _render(phi, lambda: _Lattice(_with_range(view, lo, hi)), mode, out_kind, scale, vrange, chunk)


def _render(phi, geometry, mode, out_kind, scale, vrange, chunk):
    """render and render_rays behind their own checks: geometry() makes the _Lattice / _Bundle once the net is known to be on a GPU"""
    import torch
    from . import mip
    if int(phi.coords_channel) != 3:
        raise ValueError("a view is defined for 3-D data only (the net takes %d coordinates)" % phi.coords_channel)
    phi._require_gpu()
    chunk = int(chunk or mip.DEFAULT_CHUNK)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    L, st = _lib.lib(), _lib.stream_ptr
    geo = geometry()
    dev, ch = phi.params.device, int(phi.data_channel)
    rays = geo.rows * geo.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if out_kind == "u8" else (_lib.OUT_U16, torch.uint16)
    m = _lib.VIEW_MODE[mode]
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    if mode == "mean":
        acc = torch.zeros((rays, ch), dtype=torch.int64, device=dev)
    else:
        acc = torch.full((rays, ch), 0x7FFFFFFF if mode == "min" else 0, dtype=torch.int32, device=dev)

    def fold(k0, off, s0, s1, r0, r1, lanes, vals):
        geo.fold(k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, m, hits, acc)
    _, total, rays_hit = _march(phi, geo, kind, dt, scale, vrange, chunk, fold)
    image = torch.empty((geo.rows, geo.cols, ch), dtype=torch.float32 if mode == "mean" else dt, device=dev)
    _lib.check(L.brief_view_finish(C.byref(geo.flat), kind, ch, m, _lib.ptr(hits), _lib.ptr(acc), _lib.ptr(image), st()))
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": int(hits.sum(dtype=torch.int64).item()), "samples_evaluated": total}
    return image, hits.view(geo.rows, geo.cols), stats


# ---- a view of a partition: the nearest block owns a sample (csrc/brief_view.h "a view of a PARTITION") -------------------------------
def part_window(view, start, dims):
    """(row0, col0, wrows, wcols): a rectangle of image rays that holds every ray which can meet the block's cell
    [start - 0.5, start + dims - 0.5] intersected with the clip box; (0, 0, 0, 0) where that intersection is empty.  Float64: the box's
    corners are taken through the inverse of (drow, dcol, ddepth); their (row, col) bounding rectangle is the box's shadow along the
    rays.  It is padded by one pixel plus a bound on what the fp32 roundings of a position (three products, three sums, each half an
    ulp of at most the largest position) can move a sample across the image, so every ray outside it misses the block exactly."""
    return tuple(int(x) for x in _windows(view, [start], [dims])[0])


def _windows(view, starts, dims):
    """part_window of many blocks at once: int64 [blocks, 4]"""
    f = lambda a: np.array(list(a), np.float64)
    starts, dims = np.asarray(starts, np.float64).reshape(-1, 3), np.asarray(dims, np.float64).reshape(-1, 3)
    lo, hi = np.maximum(f(view.box_lo), starts - 0.5), np.minimum(f(view.box_hi), starts + dims - 0.5)
    m = np.stack([f(view.drow), f(view.dcol), f(view.ddepth)], 1)
    inv = np.linalg.inv(m)
    upper = np.array([[(i >> a) & 1 for a in range(3)] for i in range(8)], bool)
    corners = np.where(upper[None], hi[:, None, :], lo[:, None, :])
    t = (corners - f(view.origin)) @ inv.T
    reach = np.abs(f(view.origin)) + view.rows * np.abs(m[:, 0]) + view.cols * np.abs(m[:, 1]) + view.depth * np.abs(m[:, 2])
    pad = 1.0 + np.abs(inv[:2]) @ (8.0 * 2.0 ** -24 * reach)
    r0, r1 = np.maximum(np.floor(t[..., 0].min(1) - pad[0]), 0), np.minimum(np.ceil(t[..., 0].max(1) + pad[0]), view.rows - 1)
    c0, c1 = np.maximum(np.floor(t[..., 1].min(1) - pad[1]), 0), np.minimum(np.ceil(t[..., 1].max(1) + pad[1]), view.cols - 1)
    out = np.stack([r0, c0, r1 - r0 + 1, c1 - c0 + 1], 1)
    out[(lo > hi).any(1) | (r1 < r0) | (c1 < c0)] = 0
    return out.astype(np.int64)


def make_part(view, start, dims, window=None):
    """the block descriptor (_lib.ViewPart = brief_view_part) of the block whose first voxel is `start` and whose own grid is `dims`, in
    the volume view.dims.  window: (row0, col0, wrows, wcols), default part_window's; 'image' is the whole image.  An empty window has
    wrows == wcols == 0 and is never handed to the library."""
    start, dims, whole = [int(x) for x in start], [int(x) for x in dims], [int(x) for x in view.dims]
    if len(start) != 3 or len(dims) != 3:
        raise ValueError("a block of a view is 3-D: start and dims need three entries (got %r, %r)" % (start, dims))
    if any(n >= PART_MAX_DIM for n in whole):
        raise ValueError("a view of a partition is refused for a volume of %s: an axis of 2^23 or more does not keep the cell bounds "
                         "s - 0.5 and e + 0.5 exact in a float" % (whole,))
    if any(n < 2 for n in dims):
        raise ValueError(ENVELOPE["min_axis"][1] % (dims,))
    if any(s < 0 or s + n > w for s, n, w in zip(start, dims, whole)):
        raise ValueError("the block at %s of dims %s does not lie inside the volume %s" % (start, dims, whole))
    pt = _lib.ViewPart()
    for a in range(3):
        pt.start[a], pt.dims[a] = start[a], dims[a]
    if window is None:
        window = part_window(view, start, dims)
    elif isinstance(window, str) and window == "image":
        window = (0, 0, view.rows, view.cols)
    pt.row0, pt.col0, pt.wrows, pt.wcols = (int(x) for x in window)
    return pt


def part_clip_host(view, part):
    """(k0 [wrows, wcols], cnt [wrows, wcols]) int32: the samples of every ray of the block's window that the block evaluates (inside
    the clip box and owned), k0 <= k < k0 + cnt, on the host CPU (brief_view_part_clip_host)"""
    shape = (part.wrows, part.wcols)
    k0, cnt = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    if k0.size:
        _lib.check(_lib.lib().brief_view_part_clip_host(C.byref(view), C.byref(part), k0.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
    return k0, cnt


def part_sample_host(view, part, row, col, k):
    """(pos [n, 3], local [n, 3], coord [n, 3] float32, inside [n], owned [n] bool) of the samples (row, col, k) as the device computes
    them for the block: the global position, the block-local position q = fl(p - start), the block-local coordinate, the clip box's
    closed test and the cell's half-open test (brief_view_part_sample_host; the window plays no part)"""
    row, col, k = (np.ascontiguousarray(x, np.int32).ravel() for x in (row, col, k))
    n = len(row)
    if len(col) != n or len(k) != n:
        raise ValueError("row, col and k must have one entry per sample")
    pos, local, coord = (np.empty((n, 3), np.float32) for _ in range(3))
    inside, owned = np.empty(n, np.uint8), np.empty(n, np.uint8)
    if part.wrows < 1 or part.wcols < 1:
        part = make_part(view, list(part.start), list(part.dims), "image")
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_view_part_sample_host(C.byref(view), C.byref(part), p(row), p(col), p(k), n, p(pos), p(local), p(coord), p(inside),
                                                      p(owned)))
    return pos, local, coord, inside.astype(bool), owned.astype(bool)


def _at_ray(t, base):
    """a block's slice of a window-ray array: the pointer to entry `base` of the tensor t"""
    return C.c_void_p(t.data_ptr() + t.element_size() * t.stride(0) * base)


def _plan_partition(parts, view, chunk, who):
    """the checks every view of a partition shares, before any GPU call: (parts, channels, chunk, block descriptors, per-block view
    descriptors with the block's lo / hi)"""
    from . import mip
    parts = list(parts)
    if not parts:
        raise ValueError("%s needs at least one block" % who)
    ch = int(parts[0][0].data_channel)
    for phi, *_ in parts:
        if int(phi.coords_channel) != 3:
            raise ValueError("a view is defined for 3-D data only (the net takes %d coordinates)" % phi.coords_channel)
        if int(phi.data_channel) != ch:
            raise ValueError("the blocks of a view must agree in their channel count (got %d and %d)" % (ch, phi.data_channel))
    chunk = int(chunk or mip.DEFAULT_CHUNK)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    first = np.array([[int(x) for x in p[1]] for p in parts], np.int64).reshape(len(parts), -1)
    size = np.array([[int(x) for x in p[2]] for p in parts], np.int64).reshape(len(parts), -1)
    for i in range(len(parts) - 1):
        meet = ((first[i] < first[i + 1:] + size[i + 1:]) & (first[i + 1:] < first[i] + size[i])).all(1)
        if meet.any():
            raise ValueError("the blocks at %s and %s overlap: a sample there would have two owners"
                             % (first[i].tolist(), first[i + 1 + int(np.argmax(meet))].tolist()))
    pts = [make_part(view, s, n, w) for s, n, w in zip(first.tolist(), size.tolist(), _windows(view, first, size).tolist())]
    for phi, *_ in parts:
        phi._require_gpu()
    vs = [_with_range(view, lo, hi) for _, _, _, lo, hi, _, _ in parts]
    return parts, ch, chunk, pts, vs


def _march_partition(parts, vs, pts, kind, dt, chunk, fold, clipped=None, counts=None):
    """the part every view of a partition shares, as _march is for the single-net views.  All blocks are clipped, each over its own
    window, into one block-major array (or `clipped` = (k0, cnt) of an earlier march is taken as it is); ONE scan of the counts (and of
    the hit flags, for the lanes per ray) and ONE read of the per-block totals follow; then block by block and chunk by chunk the
    block-local coordinates, the net's own forward entry with the block's integer epilogue, and
    fold(i, v, pt, base, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals): block i's descriptors, the base of its slice of the window-ray
    arrays, its slices of k0 and off, the chunk [s0, s1) in off's numbering and its window rays [r0, r1) within the slice.
    counts: int32 [window_rays], taken instead of the clip's counts (each either the clip's own or 0): the march of a later pass over
    a subset of the window rays.  Returns a dict: k0, cnt (None without a window ray), edges (the slices' bounds), window_rays,
    evaluated, blocks_hit, segments (window rays that hold a sample)."""
    import torch
    L, stream = _lib.lib(), _lib.stream_ptr()
    dev, ch = parts[0][0].params.device, int(parts[0][0].data_channel)
    sizes = [pt.wrows * pt.wcols for pt in pts]
    edges = [0]
    for n in sizes:
        edges.append(edges[-1] + n)
    window_rays = edges[-1]
    out = dict(k0=None, cnt=None, edges=edges, window_rays=window_rays, evaluated=0, blocks_hit=0, segments=0)
    if window_rays == 0:
        return out
    if clipped is None:
        k0, cnt = torch.empty(window_rays, dtype=torch.int32, device=dev), torch.empty(window_rays, dtype=torch.int32, device=dev)
        for v, pt, base, n in zip(vs, pts, edges, sizes):            # the clip needs no net
            if n:
                _lib.check(L.brief_view_part_clip(C.byref(v), C.byref(pt), _at_ray(k0, base), _at_ray(cnt, base), stream))
    else:
        k0, cnt = clipped
    out["k0"], out["cnt"] = k0, cnt
    n_w = cnt if counts is None else counts
    # ONE scan of the counts (and of the hit flags, for the lanes per ray) and ONE read of the per-block totals
    off = torch.zeros((2, window_rays + 1), dtype=torch.int64, device=dev)
    torch.cumsum(n_w, 0, dtype=torch.int64, out=off[0, 1:])
    torch.cumsum(n_w > 0, 0, dtype=torch.int64, out=off[1, 1:])
    at = off[:, torch.tensor(edges, dtype=torch.int64, device=dev)].cpu().tolist()
    off = off[0]
    totals = [b - a for a, b in zip(at[0][:-1], at[0][1:])]
    hit_rays = [b - a for a, b in zip(at[1][:-1], at[1][1:])]
    evaluated = at[0][-1]
    out["evaluated"], out["blocks_hit"], out["segments"] = evaluated, sum(1 for t in totals if t > 0), at[1][-1]
    if evaluated > 0:
        # the chunks of every block's span, and the window rays that may hold a sample of each, in ONE search and read
        plan = [(i, s0, min(s0 + chunk, at[0][i + 1])) for i, t in enumerate(totals) if t > 0 for s0 in range(at[0][i], at[0][i + 1], chunk)]
        cuts = torch.tensor([[p[1] for p in plan], [p[2] for p in plan]], dtype=torch.int64, device=dev)
        r0s, r1s = torch.stack([torch.searchsorted(off[1:], cuts[0], right=True),      # the first ray that ends behind s0
                                torch.searchsorted(off[:-1], cuts[1], right=False)]).cpu().tolist()      # ... that starts at or behind s1
        room = min(chunk, max(totals))
        coords = torch.empty((room, 3), dtype=torch.float32, device=dev)
        vals = torch.empty((room, ch), dtype=dt, device=dev)
        p_coords, p_vals = _lib.ptr(coords), _lib.ptr(vals)
        block = -1
        for (i, s0, s1), r0, r1 in zip(plan, r0s, r1s):
            if i != block:                                       # the block's net, descriptors and slices, once per block
                block, phi, base = i, parts[i][0], edges[i]
                phi.sync_packed()
                v, pt, k0_b, off_b = C.byref(vs[i]), C.byref(pts[i]), _at_ray(k0, base), _at_ray(off, base)
                lanes = _lanes(totals[i] / hit_rays[i])
            n = s1 - s0
            _lib.check(L.brief_view_part_coords(v, pt, k0_b, off_b, s0, s1, r0 - base, r1 - base, lanes, p_coords, stream))
            b = _lib.BatchDesc(coords.data_ptr(), None, None, None, 0, n, 0, 0, 0)
            _lib.check(phi._abi_forward(None, b, vals, kind, parts[i][5], parts[i][6], n))
            fold(i, v, pt, base, k0_b, off_b, s0, s1, r0 - base, r1 - base, lanes, p_vals)
    return out


def render_partition(parts, view, mode, out_kind, chunk=None):
    """render for a PARTITION of the grid view.dims: parts is a list of blocks (phi, start, dims, lo, hi, scale, vrange), one net per
    block on its own linspace grid `dims` over [lo, hi] whose first voxel is `start` in the whole volume, with its own integer
    epilogue (scale, vrange).  The nearest block owns a sample: a block evaluates exactly the samples inside the clip box whose
    global position lies in its half-open cell start - 0.5 <= p < start + dims - 0.5, on block-local coordinates (up to half a voxel
    outside its own grid).  Blocks must not overlap; a sample in a gap no block covers is neither evaluated nor folded.  Returns
    render's (image, hits, stats); every fold is an integer fold, so the order of the blocks and the chunking change no bit.

    All blocks are clipped first, each over its own WINDOW of rays (part_window), into one block-major array; one scan and one read of
    the per-block totals follow, then block by block the net's own forward entry on chunks of the block's span (a chunk never spans
    two blocks) and the fold.  A block whose window or total is empty launches nothing after the clip.  The nets may be of different
    kinds; their channel count must agree.  Memory: one chunk, the window arrays and the accumulators (and the nets themselves).
    stats: render's keys over the whole image, plus blocks, blocks_hit (blocks that own a sample) and rays_clipped (the windows' sum)."""
    import torch
    if mode not in MODES:
        raise ValueError("view mode %r is not one of %s" % (mode, " | ".join(MODES)))
    if out_kind not in ("u8", "u16"):
        raise ValueError("render_partition folds the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    if mode == "slice" and view.depth != 1:
        raise ValueError("mode 'slice' needs a view of one plane (depth 1); this one has %d samples per ray" % view.depth)
    parts, ch, chunk, pts, vs = _plan_partition(parts, view, chunk, "render_partition")
    L, stream = _lib.lib(), _lib.stream_ptr()
    dev = parts[0][0].params.device
    rays = view.rows * view.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if out_kind == "u8" else (_lib.OUT_U16, torch.uint16)
    m = _lib.VIEW_MODE[mode]
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    if mode == "mean":
        acc = torch.zeros((rays, ch), dtype=torch.int64, device=dev)
    else:
        acc = torch.full((rays, ch), 0x7FFFFFFF if mode == "min" else 0, dtype=torch.int32, device=dev)
    p_hits, p_acc = _lib.ptr(hits), _lib.ptr(acc)

    def fold(i, v, pt, base, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals):
        _lib.check(L.brief_view_part_fold(v, pt, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals, kind, ch, m, p_hits, p_acc, stream))
    march = _march_partition(parts, vs, pts, kind, dt, chunk, fold)
    window_rays, evaluated, blocks_hit = march["window_rays"], march["evaluated"], march["blocks_hit"]
    image = torch.empty((view.rows, view.cols, ch), dtype=torch.float32 if mode == "mean" else dt, device=dev)
    _lib.check(L.brief_view_finish(C.byref(vs[0]), kind, ch, m, _lib.ptr(hits), _lib.ptr(acc), _lib.ptr(image), stream))
    rays_hit, inside = torch.stack([(hits > 0).sum(), hits.sum(dtype=torch.int64)]).cpu().tolist()      # (a ray's range is exact: hit <=> hits > 0)
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": inside, "samples_evaluated": evaluated, "blocks": len(parts),
             "blocks_hit": blocks_hit, "rays_clipped": window_rays}
    return image, hits.view(view.rows, view.cols), stats


# ---- surface view: first-hit depth, refined, and shaded normals ---------------------------------------------------------------------
SIDES = ("above", "below")
MAX_REFINE = 16
NO_HIT = 0x7FFFFFFF          # the fold's identity of `first`


def check_surface(level, channel, side, refine, channels, out_kind):
    """the surface view's own arguments, refused by name: (level, channel, refine) as ints"""
    top = 255 if out_kind in ("u8", "uint8") else 65535
    try:
        lv = int(level)
        whole = float(level) == lv
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError("level must be an integer grey level of the integer decode (got %r)" % (level,))
    if not 0 <= lv <= top:
        raise ValueError("level %d lies outside the range of the integer decode, 0 .. %d" % (lv, top))
    if int(channel) != channel or not 0 <= int(channel) < int(channels):
        raise ValueError("channel %r does not exist: the net has the channels 0 .. %d" % (channel, int(channels) - 1))
    if side not in SIDES:
        raise ValueError("side %r is not one of %s" % (side, " | ".join(SIDES)))
    if int(refine) != refine or not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError("refine must be 0 .. %d rounds of bisection (got %r)" % (MAX_REFINE, refine))
    return lv, int(channel), int(refine)


def _unit3(v, what):
    v = _vec3(v, what)
    if not np.linalg.norm(v) > 0:
        raise ValueError("%s must not be the zero vector" % what)
    return v / np.linalg.norm(v)


def render_surface(phi, view, level, lo, hi, out_kind, scale, vrange, channel=0, side="above", refine=8, shading=True, light=None,
                   gscale=None, chunk=None):
    """the isosurface view of the net `phi`: for every ray of `view` the first inside sample at which channel `channel` of the integer
    decode (out_kind, scale, vrange: render's) passes the side test, value >= level ('above') or value <= level ('below'), refined
    by `refine` rounds of bisection between that sample and the one before it, and shaded.  A dict of device tensors:
        first     int32 [rows, cols]: the sample index k of the first hit, -1 without one
        t_lo, t_hi, t  float32 [rows, cols]: the final bracket in sample units (the test fails at t_lo and passes at t_hi) and the
                  hit t = t_hi; NaN without a hit.  A CUT ray (first is the ray's first inside sample: the clip box slices the object
                  open) has no bracket: t_lo == t_hi == first, never refined.  refine=0: t == first.
        position  float32 [rows, cols, 3]: the hit in voxel-index units, NaN without a hit
        normal    float32 [rows, cols, 3], shade float32 [rows, cols] (None with shading=False): the unit normal -g / |g| ('above': out
                  of a bright object) or +g / |g| ('below') of g_a = d(channel) / d(coordinate a) * gscale_a at the hit, from the
                  analytic Jacobian (fp32 SIREN up to 1024 features; anything else is refused BEFORE any decode), and the Lambert term
                  max(0, -(normal . light)).  gscale: grey levels per physical unit and coordinate unit, default gradient.voxel_scale
                  (voxels of extent 1); light: the direction the light travels, in the normal's frame, default the view's own
                  direction ddepth (a headlight; decompress_surface passes the physical one).  0 without a hit.
        hits      int32 [rows, cols]: inside samples per ray
        stats     render's keys, rays_surface (rays with a hit), rays_cut, refine_points (points the refinement evaluated)
    The march evaluates exactly what render evaluates, in chunks of `chunk`; a refinement round is one dense pass over rows * cols
    points (1 / depth of the march).  Every decision compares decoded integers: first, t_lo, t_hi do not depend on chunking or run."""
    return _render_surface(phi, lambda: _Lattice(_with_range(view, lo, hi)), "render_surface", list(view.dims), level, lo, hi, out_kind, scale, vrange,
                           channel, side, refine, shading, light, gscale, chunk)


def _render_surface(phi, geometry, who, dims, level, lo, hi, out_kind, scale, vrange, channel, side, refine, shading, light, gscale, chunk):
    """render_surface and render_surface_rays: geometry() makes the _Lattice / _Bundle once every refusal has passed"""
    import torch
    from . import gradient, mip
    if out_kind not in ("u8", "u16"):
        raise ValueError("%s tests the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (who, out_kind))
    if int(phi.coords_channel) != 3:
        raise ValueError("a view is defined for 3-D data only (the net takes %d coordinates)" % phi.coords_channel)
    ch = int(phi.data_channel)
    level, channel, refine = check_surface(level, channel, side, refine, ch, out_kind)
    if shading:
        why = gradient.refusal(getattr(type(phi), "kind", "SIREN"), phi.precision, phi.features)
        if why is not None:
            raise ValueError("normals and shading need the analytic Jacobian: %s; ask for shading=False" % why)
    phi._require_gpu()
    chunk = int(chunk or mip.DEFAULT_CHUNK)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    L, st = _lib.lib(), _lib.stream_ptr
    geo = geometry()
    v = geo.flat
    dev, rays = phi.params.device, geo.rows * geo.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if out_kind == "u8" else (_lib.OUT_U16, torch.uint16)
    sd = _lib.SURFACE_SIDE[side]
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    first = torch.full((rays,), NO_HIT, dtype=torch.int32, device=dev)

    def fold(k0, off, s0, s1, r0, r1, lanes, vals):
        geo.surface_fold(k0, off, s0, s1, r0, r1, lanes, vals, kind, ch, channel, level, sd, hits, first)
    k0, total, rays_hit = _march(phi, geo, kind, dt, scale, vrange, chunk, fold)
    t_lo, t_hi = torch.empty(rays, dtype=torch.float32, device=dev), torch.empty(rays, dtype=torch.float32, device=dev)
    _lib.check(L.brief_surface_bracket(C.byref(v), _lib.ptr(k0), _lib.ptr(first), _lib.ptr(t_lo), _lib.ptr(t_hi), st()))
    hit = first != NO_HIT
    rays_surface, rays_cut = int(hit.sum().item()), int((hit & (first == k0)).sum().item())
    coords = torch.empty((rays, 3), dtype=torch.float32, device=dev)
    pos = torch.empty((rays, 3), dtype=torch.float32, device=dev)
    refine_points = 0
    if refine and rays_surface > rays_cut:
        vals = torch.empty((rays, ch), dtype=dt, device=dev)
        for _ in range(refine):
            geo.surface_coords(t_lo, t_hi, 1, coords, None)
            for o in range(0, rays, mip.DEFAULT_CHUNK):            # (dense: rows * cols points, whatever `chunk` bounds the march to)
                n = min(mip.DEFAULT_CHUNK, rays - o)
                b = _lib.BatchDesc(coords[o:o + n].data_ptr(), None, None, None, 0, n, 0, 0, 0)
                _lib.check(phi._abi_forward(None, b, vals[o:o + n], kind, scale, vrange, n))
            _lib.check(L.brief_surface_step(C.byref(v), _lib.ptr(vals), kind, ch, channel, level, sd, _lib.ptr(t_lo), _lib.ptr(t_hi), st()))
        refine_points = refine * rays
    geo.surface_coords(t_lo, t_hi, 0, coords, pos)
    normal = shade = None
    if shading:
        g = np.asarray(gscale if gscale is not None else gradient.voxel_scale(dims, lo, hi, scale, vrange[0], vrange[1]), np.float64)
        if g.shape != (3,) or not np.isfinite(g).all():
            raise ValueError("gscale must be three finite numbers in (z, y, x) order (got %r)" % (gscale,))
        _, jac = phi.spatial_gradient(coords, want_value=False)
        normal = torch.empty((geo.rows, geo.cols, 3), dtype=torch.float32, device=dev)
        shade = torch.empty((geo.rows, geo.cols), dtype=torch.float32, device=dev)
        geo.surface_shade(t_hi, jac, ch, channel, sd, g, light, normal, shade)
    shape = (geo.rows, geo.cols)
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": int(hits.sum(dtype=torch.int64).item()), "samples_evaluated": total,
             "rays_surface": rays_surface, "rays_cut": rays_cut, "refine_points": refine_points}
    return {"first": torch.where(hit, first, torch.full_like(first, -1)).view(shape), "t_lo": t_lo.view(shape), "t_hi": t_hi.view(shape),
            "t": t_hi.view(shape), "position": pos.view(*shape, 3), "normal": normal, "shade": shade, "hits": hits.view(shape), "stats": stats}


# ---- surface view of a partition: hits are routed across blocks (csrc/brief_view.h "the surface view of a PARTITION") ----------------
GAPS = ("empty",)


def _check_gap(gap):
    if gap not in GAPS:
        raise ValueError("gap %r is not a gap rule of the surface view of a partition (%s): 'empty' is the only one, a point no block "
                         "owns holds nothing and fails the side test on either side" % (gap, " | ".join(GAPS)))


def _part_array(pts):
    """a ctypes array of brief_view_part from a list of descriptors (empty windows allowed: the route does not read them)"""
    arr = (_lib.ViewPart * len(pts))()
    for i, pt in enumerate(pts):
        arr[i] = pt
    return arr


def part_sample_t_host(view, part, row, col, t):
    """part_sample_host at real depths t (float32, 0 <= t <= depth - 1): (pos, local, coord [n, 3] float32, inside, owned [n] bool) of
    the points the refinement of a surface evaluates for the block (brief_view_part_sample_t_host); at an integer t it is
    part_sample_host's sample k = t, bit for bit"""
    row, col = (np.ascontiguousarray(x, np.int32).ravel() for x in (row, col))
    t = np.ascontiguousarray(t, np.float32).ravel()
    n = len(row)
    if len(col) != n or len(t) != n:
        raise ValueError("row, col and t must have one entry per sample")
    pos, local, coord = (np.empty((n, 3), np.float32) for _ in range(3))
    inside, owned = np.empty(n, np.uint8), np.empty(n, np.uint8)
    if part.wrows < 1 or part.wcols < 1:
        part = make_part(view, list(part.start), list(part.dims), "image")
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_view_part_sample_t_host(C.byref(view), C.byref(part), p(row), p(col), p(t), n, p(pos), p(local), p(coord), p(inside),
                                                        p(owned)))
    return pos, local, coord, inside.astype(bool), owned.astype(bool)


def route_host(view, pts, t_lo, t_hi, midpoint):
    """(owner int32 [rows, cols], t_lo float32 [rows, cols]) of one routing round on the host CPU (brief_surface_part_route_host): the
    index in `pts` (block descriptors) of the block that owns every ray's point at the bracket's midpoint (midpoint=True) or at t_hi,
    -1 where the ray has nothing to evaluate, and t_lo moved to the midpoint where that point lies in a gap"""
    shape = (view.rows, view.cols)
    lo = np.array(t_lo, np.float32).reshape(shape).copy()
    hi = np.ascontiguousarray(np.array(t_hi, np.float32).reshape(shape))
    owner = np.empty(shape, np.int32)
    arr = _part_array(pts)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_surface_part_route_host(C.byref(view), C.cast(arr, C.c_void_p), len(pts), p(lo), p(hi), int(bool(midpoint)), p(owner)))
    return owner, lo


def render_surface_partition(parts, view, level, out_kind, channel=0, side="above", refine=8, shading=True, light=None, voxel_size=(1, 1, 1),
                             gap="empty", chunk=None):
    """render_surface for a PARTITION of the grid view.dims (parts: render_partition's blocks (phi, start, dims, lo, hi, scale, vrange)).
    The march is render_partition's: the nearest block owns a sample, and first is the smallest owned inside k whose value passes the
    side test, a min over all blocks.  The bracket is (first - 1, first) where first is behind the ray's first sample inside the clip
    box, whether sample first - 1 is owned or lies in a gap; a CUT ray (first is that first sample) has none.  A bracket can straddle
    a face, so every refinement point, and the hit itself, is ROUTED: its owner is the block whose half-open cell holds its global
    position (a point exactly on a face belongs to the upper block), evaluated on that block's local coordinates with its own integer
    epilogue.  gap 'empty' (the only rule): a point no block owns holds nothing, it fails the test on either side.  Returns
    render_surface's dict, and
        owner     int32 [rows, cols]: the index in `parts` of the block that owns the hit, -1 without one
        normal, shade  from the OWNER's analytic Jacobian at the hit, scaled by the owner's own gradient.voxel_scale(block dims, lo, hi,
                  scale, vrange) / voxel_size; refused by name before any decode if any block's net has no Jacobian kernel
                  (shading=False then serves blocks of mixed kinds).  light: default the view's own direction ddepth
        stats     render_surface's keys (refine_points: the points the refinement evaluated) plus blocks, blocks_hit, rays_clipped,
                  rays_straddle (rays whose initial bracket's two ends have different owners, or an unowned lower end) and
                  refine_launch_blocks (the sum over the rounds of the blocks that received a point)
    A round is one route launch, one bucketing of the rays by owner (a stable sort and a count, ONE host read), and per block that
    received points coords -> the net's forward entry -> step, in lists of at most mip.DEFAULT_CHUNK; a block without points launches
    nothing.  Every decision compares decoded integers: first, t_lo, t_hi and owner do not depend on the order of the blocks, on
    chunking or on the run."""
    import torch
    from . import gradient, mip
    _check_gap(gap)
    if out_kind not in ("u8", "u16"):
        raise ValueError("render_surface_partition tests the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    parts = list(parts)
    if not parts:
        raise ValueError("render_surface_partition needs at least one block")
    level, channel, refine = check_surface(level, channel, side, refine, int(parts[0][0].data_channel), out_kind)
    if shading:
        for phi, start, *_ in parts:
            why = gradient.refusal(getattr(type(phi), "kind", "SIREN"), phi.precision, phi.features)
            if why is not None:
                raise ValueError("normals and shading need the analytic Jacobian of every block's net, and the block at %s has none: %s; ask "
                                 "for shading=False" % ([int(x) for x in start], why))
    vs3 = _vec3(voxel_size, "voxel_size")
    if (vs3 <= 0).any():
        raise ValueError("voxel_size must be positive on every axis (got %r)" % (tuple(voxel_size),))
    parts, ch, chunk, pts, vs = _plan_partition(parts, view, chunk, "render_surface_partition")
    L, stream = _lib.lib(), _lib.stream_ptr()
    dev, rays, nb = parts[0][0].params.device, view.rows * view.cols, len(parts)
    kind, dt = (_lib.OUT_U8, torch.uint8) if out_kind == "u8" else (_lib.OUT_U16, torch.uint16)
    sd = _lib.SURFACE_SIDE[side]
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    first = torch.full((rays,), NO_HIT, dtype=torch.int32, device=dev)
    p_hits, p_first = _lib.ptr(hits), _lib.ptr(first)

    def fold(i, v, pt, base, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals):
        _lib.check(L.brief_surface_part_fold(v, pt, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals, kind, ch, channel, level, sd, p_hits, p_first, stream))
    march = _march_partition(parts, vs, pts, kind, dt, chunk, fold)
    # the bracket: the clip of the WHOLE view (no net), then brief_surface_bracket as for a single net
    v0 = C.byref(vs[0])
    k0, cnt = torch.empty(rays, dtype=torch.int32, device=dev), torch.empty(rays, dtype=torch.int32, device=dev)
    _lib.check(L.brief_view_clip(v0, _lib.ptr(k0), _lib.ptr(cnt), stream))
    t_lo, t_hi = torch.empty(rays, dtype=torch.float32, device=dev), torch.empty(rays, dtype=torch.float32, device=dev)
    _lib.check(L.brief_surface_bracket(v0, _lib.ptr(k0), p_first, _lib.ptr(t_lo), _lib.ptr(t_hi), stream))
    table = torch.frombuffer(bytearray(bytes(_part_array(pts))), dtype=torch.uint8).to(dev)      # the route's table of blocks
    owner, owner_lo = torch.empty(rays, dtype=torch.int32, device=dev), torch.empty(rays, dtype=torch.int32, device=dev)
    p_lo, p_hi, p_table = _lib.ptr(t_lo), _lib.ptr(t_hi), _lib.ptr(table)

    def route(mid):
        _lib.check(L.brief_surface_part_route(v0, p_table, nb, p_lo, p_hi, mid, _lib.ptr(owner), stream))
    # the ends of the initial bracket: the owner of t_lo (the route at t_hi of the bracket (t_lo, t_lo)) against the owner of t_hi
    _lib.check(L.brief_surface_part_route(v0, p_table, nb, p_lo, p_lo, 0, _lib.ptr(owner_lo), stream))
    route(0)
    hit = first != NO_HIT
    bracketed = hit & (first != k0)
    rays_surface, rays_cut, rays_hit, inside, straddle = torch.stack([
        hit.sum(), (hit & (first == k0)).sum(), (hits > 0).sum(), hits.sum(dtype=torch.int64), (bracketed & (owner_lo != owner)).sum()]).cpu().tolist()
    # the window of a block whose cell the clip box misses is empty: the list entries take the whole image then (the window plays no part)
    full = [pt if pt.wrows > 0 and pt.wcols > 0 else make_part(view, list(pt.start), list(pt.dims), "image") for pt in pts]
    room = mip.DEFAULT_CHUNK

    def buckets():
        """the rays grouped by owner, one stable sort and ONE host read of the per-block counts: (order, [(block, offset, count)])"""
        order = torch.argsort(owner, stable=True)
        counts = torch.bincount((owner + 1).to(torch.int64), minlength=nb + 1).cpu().tolist()
        out, at = [], counts[0]                                     # (the rays without an owner come first)
        for i in range(nb):
            if counts[i + 1]:
                out.append((i, at, counts[i + 1]))
            at += counts[i + 1]
        return order, out

    def lists(order, found):
        """(block, pointer to the list, entries) per list of at most `room` rays"""
        for i, at, n in found:
            for o in range(0, n, room):
                yield i, _at_ray(order, at + o), min(room, n - o)
    refine_points = launch_blocks = 0
    coords = vals = None
    if refine and rays_surface > rays_cut:
        for _ in range(refine):
            route(1)
            order, found = buckets()
            launch_blocks += len(found)
            if found and coords is None:
                most = min(room, rays)
                coords = torch.empty((most, 3), dtype=torch.float32, device=dev)
                vals = torch.empty((most, ch), dtype=dt, device=dev)
            block = -1
            for i, p_list, n in lists(order, found):
                if i != block:
                    block = i
                    parts[i][0].sync_packed()
                _lib.check(L.brief_surface_part_coords(C.byref(vs[i]), C.byref(full[i]), p_lo, p_hi, 1, p_list, n, _lib.ptr(coords), None, stream))
                b = _lib.BatchDesc(coords.data_ptr(), None, None, None, 0, n, 0, 0, 0)
                _lib.check(parts[i][0]._abi_forward(None, b, vals, kind, parts[i][5], parts[i][6], n))
                _lib.check(L.brief_surface_part_step(p_list, n, _lib.ptr(vals), kind, ch, channel, level, sd, p_lo, p_hi, stream))
                refine_points += n
    # the hit is t_hi, always an evaluated point: it has an owner
    route(0)
    pos = torch.full((rays, 3), float("nan"), dtype=torch.float32, device=dev)
    normal = shade = None
    if shading:
        normal = torch.zeros((view.rows, view.cols, 3), dtype=torch.float32, device=dev)
        shade = torch.zeros((view.rows, view.cols), dtype=torch.float32, device=dev)
        l = _unit3(light if light is not None else list(view.ddepth), "light")
        f3 = C.c_float * 3
    if rays_surface:
        order, found = buckets()
        if coords is None:
            coords = torch.empty((min(room, rays), 3), dtype=torch.float32, device=dev)
        for i, p_list, n in lists(order, found):
            phi, _, dims, lo, hi, scale, vrange = parts[i]
            _lib.check(L.brief_surface_part_coords(C.byref(vs[i]), C.byref(full[i]), p_lo, p_hi, 0, p_list, n, _lib.ptr(coords), _lib.ptr(pos), stream))
            if shading:
                g = gradient.voxel_scale([int(x) for x in dims], lo, hi, scale, vrange[0], vrange[1]) / vs3
                _, jac = phi.spatial_gradient(coords[:n], want_value=False)
                _lib.check(L.brief_surface_part_shade(p_list, n, p_hi, _lib.ptr(jac), ch, channel, sd, f3(*g), f3(*l), _lib.ptr(normal), _lib.ptr(shade),
                                                      stream))
    shape = (view.rows, view.cols)
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": inside, "samples_evaluated": march["evaluated"], "rays_surface": rays_surface,
             "rays_cut": rays_cut, "refine_points": refine_points, "blocks": nb, "blocks_hit": march["blocks_hit"],
             "rays_clipped": march["window_rays"], "rays_straddle": straddle, "refine_launch_blocks": launch_blocks}
    return {"first": torch.where(hit, first, torch.full_like(first, -1)).view(shape), "t_lo": t_lo.view(shape), "t_hi": t_hi.view(shape),
            "t": t_hi.view(shape), "position": pos.view(*shape, 3), "normal": normal, "shade": shade, "hits": hits.view(shape),
            "owner": owner.view(shape), "stats": stats}


# ---- ray view: a perspective camera, or any table of rays (csrc/brief_rays.h, csrc/brief_rays.inc; DESIGN.md "Camera view") -----------
CAMERA_MODES = ("max", "min", "mean")
CAMERA_SCOPE = ("a camera renders the projections max | min | mean and the surface view: %s through a camera is out of scope (a follow-up; "
                "every ray of a camera is sampled at one uniform spacing so that a composite needs no opacity correction later)")


class RayView:
    """a ray view: desc (_lib.RaysDesc: dims, lo / hi, rows, cols, depth, the clip box), rays float32 [rows, cols, 6] = (base z, y, x,
    step z, y, x) per ray in voxel-index units, light float32 [rows, cols, 3] (the unit physical direction of every ray: a point light
    at a camera's eye), and near / depth_spacing, the fp32 numbers that turn a depth t in samples into a physical distance along the
    ray, distance = fl(near + fl(t * depth_spacing))"""

    def __init__(self, desc, rays, light, near, depth_spacing):
        self.desc, self.near, self.depth_spacing = desc, float(np.float32(near)), float(np.float32(depth_spacing))
        self.rays = np.ascontiguousarray(rays, np.float32).reshape(desc.rows, desc.cols, 6)
        self.light = np.ascontiguousarray(light, np.float32).reshape(desc.rows, desc.cols, 3)

    rows, cols, depth = (property(lambda self, n=n: getattr(self.desc, n)) for n in ("rows", "cols", "depth"))


def _rays_desc(dims, box_lo, box_hi, rows, cols, depth, lo=-1.0, hi=1.0):
    d = _lib.RaysDesc()
    for a in range(3):
        d.dims[a], d.box_lo[a], d.box_hi[a] = int(dims[a]), box_lo[a], box_hi[a]
    d.lo, d.hi = float(lo), float(hi)
    d.rows, d.cols, d.depth = int(rows), int(cols), int(depth)
    return d


def _flat_view(desc):
    """the brief_view_desc that carries a ray view's dims, lo / hi, box, rows, cols and depth, with zero steps: what brief_view_finish,
    brief_surface_bracket and brief_surface_step read (brief_rays_view of csrc/brief_rays.h)"""
    v = _lib.ViewDesc()
    for a in range(3):
        v.dims[a], v.box_lo[a], v.box_hi[a] = desc.dims[a], desc.box_lo[a], desc.box_hi[a]
    v.lo, v.hi = desc.lo, desc.hi
    v.rows, v.cols, v.depth = desc.rows, desc.cols, desc.depth
    return v


def make_camera(dims, eye, direction, up=None, fov=60.0, size=(256, 256), near=0.0, far=None, depth_spacing=1.0, voxel_size=(1, 1, 1), region=None):
    """the RayView of a perspective camera at `eye` looking along `direction`, over the grid `dims` (3 spatial axes, (z, y, x)).
    eye:           a voxel-index position, as make_view's centre; it may lie inside the volume (a fly-through).
    direction, up: see frame(); PHYSICAL directions, voxel_size being a voxel's physical extent per axis.
    fov:           the full opening angle over the rows, degrees, 0 < fov < 180; pixels are square.
    size:          (rows, cols).  Pixel (i, j) looks along w = direction + u_i * row_dir + v_j * col_dir with u_i = (i - (rows - 1) / 2) * s,
                   v_j = (j - (cols - 1) / 2) * s, s = 2 tan(fov / 2) / rows (the pixel pitch on the image plane at unit distance).
    near, far, depth_spacing: physical distances from the eye.  Sample k of EVERY ray lies at near + k * depth_spacing along the ray's
                   unit direction w / |w|: base = eye + near * unit / voxel_size, step = depth_spacing * unit / voxel_size.  far
                   defaults to the largest distance from the eye to a corner of the clip box; depth = floor((far - near) /
                   depth_spacing + 1e-9) + 1.
    region:        the clip box (make_view's).
    Everything is computed in float64 and rounded to fp32 once.  lo / hi of the descriptor are set by render_rays()."""
    dims = [int(v) for v in dims]
    if len(dims) != 3:
        raise ValueError("a view is defined for 3-D data only (got a %d-D grid)" % len(dims))
    if any(n < 2 for n in dims):
        raise ValueError(ENVELOPE["min_axis"][1] % (dims,))
    vs = _vec3(voxel_size, "voxel_size")
    if (vs <= 0).any():
        raise ValueError("voxel_size must be positive on every axis (got %r)" % (tuple(voxel_size),))
    depth_spacing = _positive(depth_spacing, "depth_spacing")
    e = _vec3(eye, "eye")
    fov = float(fov)
    if not 0.0 < fov < 180.0:
        raise ValueError("fov must lie strictly between 0 and 180 degrees (got %r): it is the full opening angle over the rows" % (fov,))
    near = float(near)
    if not (math.isfinite(near) and near >= 0):
        raise ValueError("near must be a finite distance >= 0 from the eye (got %r)" % (near,))
    try:
        rows, cols = (int(x) for x in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (rows, cols) (got %r)" % (size,)) from None
    if rows < 1 or cols < 1:
        raise ValueError("size must be at least 1 x 1 (got %r)" % (size,))
    if rows >= MAX_COUNT or cols >= MAX_COUNT:
        raise ValueError("size %r is refused: sizes of 2^24 and above are not exact in a float" % (size,))
    row_dir, col_dir, d = frame(direction, up)
    start, stop, step = region_mod.normalize_region(dims, region if region is not None else (slice(None),) * 3, 1)
    if any(s != 1 for s in step):
        raise ValueError("the clip box of a view is a box, not a lattice: region steps other than 1 are refused (got %s)" % (step,))
    box_lo, box_hi = np.array(start, np.float64), np.array(stop, np.float64) - 1.0
    if far is None:
        corners = np.array([[(box_lo, box_hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
        far = max(float(np.linalg.norm((corners - e) * vs, axis=1).max()), near)
    else:
        far = float(far)
        if not (math.isfinite(far) and far >= near):
            raise ValueError("far must be a finite distance >= near = %r from the eye (got %r)" % (near, far))
    depth = _count(far - near, depth_spacing, "depth")
    s = 2.0 * math.tan(math.radians(fov) / 2.0) / rows
    u = (np.arange(rows, dtype=np.float64) - (rows - 1) / 2.0) * s
    w = (np.arange(cols, dtype=np.float64) - (cols - 1) / 2.0) * s
    ray = d[None, None, :] + u[:, None, None] * row_dir[None, None, :] + w[None, :, None] * col_dir[None, None, :]
    unit = ray / np.linalg.norm(ray, axis=2, keepdims=True)
    table = np.concatenate([e + near * unit / vs, depth_spacing * unit / vs], axis=2)
    return RayView(_rays_desc(dims, box_lo, box_hi, rows, cols, depth), table, unit, near, depth_spacing)


def rays_from_view(view):
    """the RayView of an orthographic view (a _lib.ViewDesc): base = the fp32 position of its sample (row, col, 0) as the device computes
    it (sample_host), step = view.ddepth on every ray, light = ddepth normalised.  Through brief_rays_* it gives the orthographic
    renderers' results bit for bit; it is also the pattern for a caller's own rays.  near = 0 and depth_spacing = 1: the distance of a
    surface is its depth in samples."""
    row, col = np.meshgrid(np.arange(view.rows), np.arange(view.cols), indexing="ij")
    base = sample_host(view, row, col, np.zeros_like(row))[0]
    dd = np.array(list(view.ddepth), np.float32)
    table = np.concatenate([base, np.broadcast_to(dd, base.shape)], axis=1)
    light = np.broadcast_to(_unit3(list(view.ddepth), "ddepth"), base.shape)
    desc = _rays_desc(list(view.dims), list(view.box_lo), list(view.box_hi), view.rows, view.cols, view.depth, view.lo, view.hi)
    return RayView(desc, table, light, 0.0, 1.0)


def _rays_host(cam, row, col, third, dtype, entry):
    row, col = (np.ascontiguousarray(x, np.int32).ravel() for x in (row, col))
    third = np.ascontiguousarray(third, dtype).ravel()
    n = len(row)
    if len(col) != n or len(third) != n:
        raise ValueError("row, col and the depth must have one entry per sample")
    pos, coord, inside = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(entry(C.byref(cam.desc), p(cam.rays), p(row), p(col), p(third), n, p(pos), p(coord), p(inside)))
    return pos, coord, inside.astype(bool)


def rays_sample_host(cam, row, col, k):
    """sample_host for a RayView: (pos [n, 3], coord [n, 3] float32, inside [n] bool) of the samples (row, col, k) as the device computes
    them, p_a = fl(base_a + fl(k * step_a)) (brief_rays_sample_host: the same header on the host CPU, no GPU call)"""
    return _rays_host(cam, row, col, k, np.int32, _lib.lib().brief_rays_sample_host)


def rays_sample_t_host(cam, row, col, t):
    """rays_sample_host at real depths t (float32, 0 <= t <= depth - 1): the points the refinement of a surface evaluates
    (brief_rays_sample_t_host); at an integer t it is rays_sample_host's sample k = t, bit for bit"""
    return _rays_host(cam, row, col, t, np.float32, _lib.lib().brief_rays_sample_t_host)


def rays_clip_host(cam):
    """clip_host for a RayView: (k0 [rows, cols], cnt [rows, cols]) int32, the inside samples of every ray, on the host CPU"""
    k0, cnt = np.empty((cam.rows, cam.cols), np.int32), np.empty((cam.rows, cam.cols), np.int32)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    _lib.check(_lib.lib().brief_rays_clip_host(C.byref(cam.desc), p(cam.rays), p(k0), p(cnt)))
    return k0, cnt


def _bundle(cam, lo, hi, device):
    import torch
    desc = _lib.RaysDesc.from_buffer_copy(cam.desc)
    desc.lo, desc.hi = float(lo), float(hi)
    return _Bundle(desc, torch.from_numpy(cam.rays).to(device), torch.from_numpy(cam.light).to(device))


def render_rays(phi, cam, mode, lo, hi, out_kind, scale, vrange, chunk=None):
    """render through a RayView (make_camera, rays_from_view, or a caller's own table): the same contract, result and stats, behind
    any net and precision the forward entry serves.  mode 'max' | 'min' | 'mean'; a slice is refused.  The march, the chunking and
    the integer folds are render's; only the clip and the coordinates read the ray table, and the fold tests no sample again (the
    clip's list is exact), so samples_evaluated == samples_inside."""
    if mode not in CAMERA_MODES:
        if mode == "slice":
            raise ValueError(CAMERA_SCOPE % "mode 'slice'")
        raise ValueError("view mode %r is not one of %s" % (mode, " | ".join(CAMERA_MODES)))
    if out_kind not in ("u8", "u16"):
        raise ValueError("render_rays folds the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    return _render(phi, lambda: _bundle(cam, lo, hi, phi.params.device), mode, out_kind, scale, vrange, chunk)


def render_surface_rays(phi, cam, level, lo, hi, out_kind, scale, vrange, channel=0, side="above", refine=8, shading=True, light=None,
                        gscale=None, chunk=None):
    """render_surface through a RayView: its dict (first, t_lo, t_hi, t in samples along each ray, position, normal, shade, hits, stats)
    plus distance float32 [rows, cols] = fl(near + fl(t * depth_spacing)), the physical distance of the hit from the eye along its
    ray, NaN without a hit.  light=None is the per-ray headlight cam.light (a point light at the eye); a given light is one constant
    direction for every ray.  Shading has render_surface's envelope, refused before any decode."""
    out = _render_surface(phi, lambda: _bundle(cam, lo, hi, phi.params.device), "render_surface_rays", list(cam.desc.dims), level, lo, hi, out_kind,
                          scale, vrange, channel, side, refine, shading, light, gscale, chunk)
    out["distance"] = out["t"] * cam.depth_spacing + cam.near     # (two fp32 operations, each rounded on its own)
    return out


# ---- artefacts ------------------------------------------------------------------------------------------------------------------
ENVELOPE = dict(
    no_error_bound="a view of an error-bounded artefact is refused: its corrections (error_bound %s) exist on the points of the "
                   "fitted grid %s only, and a view samples between them",
    need_3d="a view is defined for 3-D data only: this artefact holds %d-D data of shape %s",
    need_integer="the view decode supports uint8 / uint16 data only (the fused integer decode); this artefact holds %s",
    need_minmaxany="the view decode supports the 'minmaxany_a_b' normalisations only (the fused integer decode), not Normalize.name=%s",
    local_postprocess=True,
    min_axis=(2, "a view needs every axis of the grid to be at least 2 voxels long (got %s): an axis of length 1 has no coordinate "
                 "range to sample"))


CAMERA_DIVIDE_REFUSAL = ("a camera view of a DivideTask artefact is refused: a camera view of a partition is a follow-up (every block has its own "
                         "net, and the rays of a camera are not parallel, so a block's window of rays is not a shadow of its cell); render an "
                         "orthographic view with --view-owner nearest, or fit the volume as a SingleTask")


def open_single(opt, module_path, sideinfos, refusal=DIVIDE_REFUSAL):
    """artefact.open_artefact for the view decodes, which exist for SingleTask artefacts only: the side info of a whole DivideTask job
    (it describes no net, so it cannot be opened) and blocks beside the module directory are refused by name"""
    from .io import load_yaml
    if isinstance(sideinfos, str):
        sideinfos = load_yaml(sideinfos)
    if "phi_features" not in sideinfos or os.path.isdir(os.path.join(os.path.dirname(str(module_path)), "sideinfos")):
        raise ValueError(refusal)
    return artefact.open_artefact(opt, module_path, sideinfos)


def check_envelope(art, mode):
    """what the view decode supports, checked on the opened artefact before any decode: a SingleTask artefact (open_single) without
    stored corrections, 3-D uint8 / uint16 data with no axis of length 1 under a 'minmaxany_a_b' normalisation (the fused integer
    epilogue), and a Decompress.postprocess that is local to a voxel (for a mean: the identity)"""
    from .misc import preprocess_is_identity
    if mode not in MODES:
        raise ValueError("view mode %r is not one of %s" % (mode, " | ".join(MODES)))
    artefact.check_envelope(art, **ENVELOPE)
    pp = art.postprocess
    if mode == "mean" and not preprocess_is_identity(np.zeros(1, np.dtype(art.dtype)), pp.denoise.level, pp.denoise.close, pp.clip):
        raise ValueError("a mean view with a Decompress.postprocess that changes values is refused: a threshold or a clip does not "
                         "commute with a mean (denoise.level %s, clip %s); use an identity postprocess" % (pp.denoise.level, list(pp.clip)))


def _plane_depth(mode, depth, offset):
    """make_view's `depth` of a decode: a slice takes its plane's `offset`, every other mode a `depth` range"""
    if mode == "slice":
        if depth is not None:
            raise ValueError("mode 'slice' takes the plane's `offset`, not a `depth` range")
        return 0.0 if offset is None else float(offset)
    if offset is not None:
        raise ValueError("`offset` names the plane of mode 'slice'; mode %r takes a `depth` range" % mode)
    return depth


def decompress_view(art, direction, up=None, mode="max", region=None, centre=None, spacing=1.0, depth_spacing=1.0,
                    size=None, depth=None, offset=None, voxel_size=(1, 1, 1), device="cuda", chunk=None, return_hits=False):
    """an orthographic view of a stored SingleTask artefact (art: open_single's) as a numpy image [rows, cols, channels], without
    decoding the volume.
    mode 'max' | 'min' (source dtype) or 'mean' (float32) folds every ray over the clip box `region` (None: the whole grid);
    'slice' (source dtype) is the one plane at `offset` along `direction` from `centre` (default 0: through the centre).  The
    geometry arguments are make_view's.  Decompress.postprocess is applied to the IMAGE for max, min and slice: on unsigned data the
    threshold (x <= level -> 0) and the clip are monotone non-decreasing maps, which commute with max and min (the argument of
    mip.decompress_mip), and on a slice they act per pixel as they would per voxel.  They do not commute with a mean: a mean with a
    postprocess other than the identity is refused.  Refused by name before any decode: DivideTask and error-bounded artefacts, 2-D
    data, dtypes other than uint8 / uint16, normalisations other than 'minmaxany_a_b', a denoise through a binary opening, an axis
    of length 1.  return_hits: (image, hits [rows, cols] int32, stats) instead of the image."""
    check_envelope(art, mode)
    depth = _plane_depth(mode, depth, offset)
    view = make_view(art.dims, direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    image, hits, stats = render(art.load_phi(device), view, mode, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange, chunk=chunk)
    img = image.cpu().numpy()
    if mode != "mean":
        img = np.array(art.postprocess_local(img), copy=True)
        img[hits.cpu().numpy() == 0] = 0                            # (a ray without a sample stays 0 whatever the clip's floor is)
    return (img, hits.cpu().numpy(), stats) if return_hits else img


def decompress_divide_view(opt, orig_sideinfos, module_dir, sideinfos_dir, direction, up=None, mode="max", region=None, centre=None, spacing=1.0,
                           depth_spacing=1.0, size=None, depth=None, offset=None, voxel_size=(1, 1, 1), device="cuda", chunk=None, return_hits=False):
    """decompress_view for a stored DivideTask artefact (orig_sideinfos: the job's side info, dict or path; module_dir / sideinfos_dir:
    the blocks' trees), without decoding the volume or any block: the view is a view of the WHOLE volume, `region` and `centre` index
    it, and the nearest block owns a sample (render_partition: a sample belongs to the block whose half-open cell, half a voxel
    around its index range, holds it; the block's net is evaluated up to half a voxel outside its own grid there; nothing is blended
    across a face).  An axis-aligned view of unit spacing samples voxels only and equals decompress_divide_mip's image / a plane of
    decompress_divide_region bit for bit.  A sample in a gap no block covers is not evaluated: a ray that meets no block is 0.
    Decompress.postprocess acts on the image as in decompress_view.  Refused by name before any net is opened: per block everything
    check_envelope refuses (error-bounded blocks, dtype, normalisation, postprocess, an axis of length 1), blocks of different
    dtypes or channel counts, overlapping blocks, 2-D data, an axis of 2^23 or more."""
    data_shape, _, arts, starts = _divide_plan(opt, orig_sideinfos, module_dir, sideinfos_dir, mode)
    depth = _plane_depth(mode, depth, offset)
    view = make_view(data_shape[:-1], direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    make_part(view, starts[0], arts[0].dims, "image")             # (the 2^23 rule, before any net is opened)
    parts = [(art.load_phi(device), s, art.dims, art.lo, art.hi, art.norm_range, art.vrange) for art, s in zip(arts, starts)]
    image, hits, stats = render_partition(parts, view, mode, arts[0].out_kind, chunk=chunk)
    img = image.cpu().numpy()
    if mode != "mean":
        img = np.array(arts[0].postprocess_local(img), copy=True)
        img[hits.cpu().numpy() == 0] = 0                            # (a ray without a sample stays 0 whatever the clip's floor is)
    return (img, hits.cpu().numpy(), stats) if return_hits else img


def _divide_plan(opt, orig_sideinfos, module_dir, sideinfos_dir, mode):
    """decompress_divide_view's envelope and refusals, before any net is opened: (data_shape, arts, starts)"""
    from . import config
    if isinstance(opt, str):
        opt = config.load(opt)
    data_shape, blocks = artefact.divide_blocks(orig_sideinfos, module_dir, sideinfos_dir, one_dtype="the view decode")
    if len(data_shape) != 4:
        raise ValueError(ENVELOPE["need_3d"] % (len(data_shape) - 1, data_shape))
    arts = [artefact.open_artefact(opt, b.module_path, b.side) for b in blocks]
    for art in arts:
        check_envelope(art, mode)
    pair = artefact.first_overlap(blocks, "dhw")
    if pair is not None:
        raise ValueError("the blocks %s and %s overlap: merge_divided_data adds overlapping blocks, and a sample of a view has one owner; "
                         "decode the region and resample it" % (pair[0].name, pair[1].name))
    starts = [[b.ranges[a][0] for a in "dhw"] for b in blocks]
    for b, art, s in zip(blocks, arts, starts):
        if art.cout != data_shape[-1] or art.dims != [b.ranges[a][1] - b.ranges[a][0] + 1 for a in "dhw"]:
            raise ValueError("the block %s holds data of shape %s: not its index range of a volume with %d channels" % (b.name, art.data_shape, data_shape[-1]))
    return data_shape, blocks, arts, starts


def decompress_divide_surface(opt, orig_sideinfos, module_dir, sideinfos_dir, direction, level, up=None, region=None, centre=None, spacing=1.0,
                              depth_spacing=1.0, size=None, depth=None, voxel_size=(1, 1, 1), channel=0, side="above", refine=8, shading=True,
                              light=None, device="cuda", chunk=None, gap="empty"):
    """decompress_surface for a stored DivideTask artefact (orig_sideinfos, module_dir, sideinfos_dir: decompress_divide_view's), without
    decoding the volume or any block: render_surface_partition's dict as numpy arrays (first, t_lo, t_hi, t, position, normal, shade,
    hits, owner: the index of the hit's block in the artefact's block order, stats) plus depth = t * depth_spacing.  The view is a view
    of the WHOLE volume; the nearest block owns a sample, every refinement point and the hit are routed to the block that owns them,
    and a point in a gap no block covers holds nothing (gap 'empty', the only rule).  `level` is a grey level of the blocks' shared
    integer dtype, compared before Decompress.postprocess.  Normals are physical, each from its owner's net and its owner's own scale.
    Refused by name before any net is opened: everything decompress_divide_view refuses (error-bounded or overlapping blocks, blocks
    of different dtypes or channel counts, 2-D data, an axis of 2^23 or more or of length 1), everything check_surface refuses, a gap
    rule other than 'empty', and shading where any block's net has no Jacobian kernel (ask for shading=False)."""
    from . import gradient
    _check_gap(gap)
    data_shape, blocks, arts, starts = _divide_plan(opt, orig_sideinfos, module_dir, sideinfos_dir, "max")
    check_surface(level, channel, side, refine, data_shape[-1], arts[0].dtype)
    if shading:
        for b, art in zip(blocks, arts):
            why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
            if why is not None:
                raise ValueError("normals and shading need the analytic Jacobian of every block's net, and the block %s has none: %s; ask for "
                                 "shading=False" % (b.name, why))
    view = make_view(data_shape[:-1], direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    make_part(view, starts[0], arts[0].dims, "image")             # (the 2^23 rule, before any net is opened)
    physical = frame(direction, up)[2] if light is None else _unit3(light, "light")
    parts = [(art.load_phi(device), s, art.dims, art.lo, art.hi, art.norm_range, art.vrange) for art, s in zip(arts, starts)]
    out = render_surface_partition(parts, view, level, arts[0].out_kind, channel=channel, side=side, refine=refine, shading=shading, light=physical,
                                   voxel_size=voxel_size, gap=gap, chunk=chunk)
    res = {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}
    res["depth"] = res["t"] * np.float32(depth_spacing)
    return res


def physical_shading(art, direction, up, light, voxel_size):
    """(light, gscale) of a shaded view of a stored artefact, both physical: the unit direction the light travels, (z, y, x), default
    the view's own `direction` (a headlight), and per axis the factor between the net's Jacobian and grey levels per physical unit,
    gradient.voxel_scale / voxel_size.  The surface view's and the shaded composite's."""
    from . import gradient
    physical = frame(direction, up)[2] if light is None else _unit3(light, "light")
    gscale = gradient.voxel_scale(art.dims, art.lo, art.hi, art.norm_range, art.vrange[0], art.vrange[1]) / _vec3(voxel_size, "voxel_size")
    return physical, gscale


def decompress_surface(art, direction, level, up=None, region=None, centre=None, spacing=1.0, depth_spacing=1.0,
                       size=None, depth=None, voxel_size=(1, 1, 1), channel=0, side="above", refine=8, shading=True, light=None, device="cuda",
                       chunk=None):
    """the isosurface view of a stored SingleTask artefact (art: open_single's), without decoding the volume: a dict of numpy arrays, render_surface's
    first, t_lo, t_hi, t, position, normal, shade, hits and stats, plus depth = t * depth_spacing (float32, physical units along the
    ray from the view's first sample plane; NaN without a hit).  The geometry arguments are make_view's; `region` is the clip box.

    `level` is a grey level of the artefact's INTEGER DECODE (uint8 / uint16 after the fused de-normalisation), compared BEFORE
    Decompress.postprocess: a threshold or a clip of the postprocess does not move the surface.  side 'above': the first sample with
    value >= level (the surface of a bright object); 'below': value <= level.  Normals are physical: the stored net's analytic
    gradient in grey levels per physical unit (gradient.voxel_scale / voxel_size per axis), and `light` is the physical direction
    the light travels, default `direction` (a headlight).  Refused by name before any decode: everything view.check_envelope
    refuses, a level outside the dtype's range, a channel that does not exist, a side other than 'above' | 'below', refine outside
    0 .. 16, and shading behind a net without the Jacobian kernel (anything but an fp32 SIREN of at most 1024 features; ask for
    shading=False to get first, depth and position)."""
    from . import gradient
    check_envelope(art, "max")
    check_surface(level, channel, side, refine, art.cout, art.dtype)
    if shading:
        why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
        if why is not None:
            raise ValueError("normals and shading need the analytic Jacobian: %s; ask for shading=False" % why)
    view = make_view(art.dims, direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    physical, gscale = physical_shading(art, direction, up, light, voxel_size)
    out = render_surface(art.load_phi(device), view, level, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange,
                         channel=channel, side=side, refine=refine, shading=shading, light=physical, gscale=gscale, chunk=chunk)
    res = {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}
    res["depth"] = res["t"] * np.float32(depth_spacing)
    return res


# ---- a camera on a stored artefact ------------------------------------------------------------------------------------------------------
def open_single_camera(opt, module_path, sideinfos):
    """open_single for the camera decodes: a DivideTask artefact is refused with the camera's own message"""
    return open_single(opt, module_path, sideinfos, CAMERA_DIVIDE_REFUSAL)


def decompress_camera(art, eye, direction, up=None, mode="max", fov=60.0, size=(256, 256), near=0.0, far=None, depth_spacing=1.0,
                      voxel_size=(1, 1, 1), region=None, device="cuda", chunk=None, return_hits=False):
    """a perspective view of a stored SingleTask artefact (art: open_single_camera's) as a numpy image [rows, cols, channels], without
    decoding the volume: mode 'max' | 'min' (source dtype) or 'mean' (float32) folds every ray of the camera (make_camera's arguments)
    over the clip box `region`.  The envelope and the handling of Decompress.postprocess are decompress_view's: a threshold and a clip
    commute with max and min and act on the image; a mean with a postprocess other than the identity is refused.  A slice and a
    composite through a camera are out of scope and refused by name.  return_hits: (image, hits [rows, cols] int32, stats)."""
    if mode not in CAMERA_MODES:
        if mode == "slice":
            raise ValueError(CAMERA_SCOPE % "mode 'slice'")
        raise ValueError("view mode %r is not one of %s" % (mode, " | ".join(CAMERA_MODES)))
    check_envelope(art, mode)
    cam = make_camera(art.dims, eye, direction, up, fov, size, near, far, depth_spacing, voxel_size, region)
    image, hits, stats = render_rays(art.load_phi(device), cam, mode, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange, chunk=chunk)
    img = image.cpu().numpy()
    if mode != "mean":
        img = np.array(art.postprocess_local(img), copy=True)
        img[hits.cpu().numpy() == 0] = 0                            # (a ray without a sample stays 0 whatever the clip's floor is)
    return (img, hits.cpu().numpy(), stats) if return_hits else img


def decompress_camera_surface(art, eye, direction, level, up=None, fov=60.0, size=(256, 256), near=0.0, far=None, depth_spacing=1.0,
                              voxel_size=(1, 1, 1), region=None, channel=0, side="above", refine=8, shading=True, light=None, device="cuda",
                              chunk=None):
    """the isosurface of a stored SingleTask artefact seen through a perspective camera (make_camera's arguments): a dict of numpy
    arrays, render_surface_rays' first, t_lo, t_hi, t, position, normal, shade, hits, stats and distance (float32, the physical
    distance of the hit from the eye along its ray; NaN without a hit).  `level`, `side`, `refine` and the refusals are
    decompress_surface's.  Normals are physical; light=None is a point light at the eye (every ray is lit along its own direction),
    a given light is one physical direction the light travels."""
    from . import gradient
    check_envelope(art, "max")
    check_surface(level, channel, side, refine, art.cout, art.dtype)
    if shading:
        why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
        if why is not None:
            raise ValueError("normals and shading need the analytic Jacobian: %s; ask for shading=False" % why)
    cam = make_camera(art.dims, eye, direction, up, fov, size, near, far, depth_spacing, voxel_size, region)
    gscale = gradient.voxel_scale(art.dims, art.lo, art.hi, art.norm_range, art.vrange[0], art.vrange[1]) / _vec3(voxel_size, "voxel_size")
    out = render_surface_rays(art.load_phi(device), cam, level, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange, channel=channel, side=side,
                              refine=refine, shading=shading, light=None if light is None else _unit3(light, "light"), gscale=gscale, chunk=chunk)
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}
