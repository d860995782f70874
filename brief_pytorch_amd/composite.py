"""Composite view of a stored artefact: direct volume rendering through a transfer function, front-to-back emission-absorption
compositing along the rays of an orthographic view (view.make_view).  The march is the view's: clip, scan, the net's own forward entry
on the compacted sample list chunk by chunk (view._march); each chunk is folded into per-pixel integer state on the device and
dropped.  The volume is never decoded.

Compositing is order-dependent, so it is taken to the log domain and to integers (csrc/brief_composite.h; DESIGN.md "Composite view"):
a sample's optical depth tau and premultiplied emission come from a table, the prefix of tau along the ray is an integer sum, the
transmittance W of that prefix a pure integer function, and a pixel the uint64 sum of W * emission.  The image does not depend on the
chunking, on the lanes per ray or on the run, bit for bit.

The composite of a DivideTask artefact (render_composite_partition, decompress_divide_composite) is the same image over the whole
volume with one net per block, the nearest block owning a sample: the blocks are marched in separate passes, so the optical depth in
front of a block's part of a ray is carried across the blocks, and only the parts behind something partly opaque are marched a
second time (DESIGN.md "Composite view of a partition").

The shaded composite (render_composite with shade=(KA, KD)) lights every sample's emission by the net's analytic gradient, a
two-sided Lambert term in Q8; the Jacobian is evaluated only at the samples that emit and are not hidden, which the integer prefix
names exactly (DESIGN.md "Shaded composite").

parse_transfer, make_transfer, check_transfer and shade_quant are host arithmetic; composite_host, composite_shade_host, shade_q_host,
part_fold_host, part_carry_host and part_gather_host restate the device's folds on the CPU (brief_view_composite_host,
brief_view_composite_shade_host, brief_view_composite_part_*_host); everything else needs a ROCm GPU (there is no CPU fallback)."""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from . import view as view_mod

TAU_SAT = 32 << 16           # BRIEF_COMPOSITE_TAU_SAT: opaque, in units of 2^-16 octaves
E_MAX = 65280                # BRIEF_COMPOSITE_E_MAX: 256 * 255
DEFAULT_BITS = {"u8": 8, "u16": 12}
DIVIDE_REFUSAL = ("a composite view of a DivideTask artefact is refused: every block has its own net and is evaluated in a pass of its "
                  "own, and a sample's weight is the transmittance of everything in front of it, a prefix that crosses the blocks of a "
                  "ray; it needs a second pass over the blocks (a follow-up).  Decode the region and render it, or use --view with "
                  "--view-owner nearest for a projection.  That second pass exists where the ownership rule is named: --view-composite with "
                  "--view-owner nearest (decompress_divide_composite) renders the composite of the partition")

DIVIDE_SHADE_REFUSAL = ("a shaded composite of a DivideTask artefact is refused: the partition composite marches the blocks behind something "
                        "partly opaque a second time, and that second pass would have to carry every block's gradients too (a follow-up).  "
                        "Leave --view-composite-shade out for the plain composite of the partition")


def _kind(out_kind):
    """('u8' | 'u16', bits of the dtype)"""
    k = {"u8": "u8", "uint8": "u8", "u16": "u16", "uint16": "u16"}.get(str(out_kind))
    if k is None:
        raise ValueError("a composite classifies the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    return k, 8 if k == "u8" else 16


def parse_transfer(text, out_kind=None):
    """the control points of a transfer function, [(level, r, g, b, a), ...], from `level:r,g,b,a;level:r,g,b,a;...` or from `@file`
    holding the same, one point per line or separated by `;`.  level: an integer grey level of the integer decode, strictly ascending
    (with out_kind: inside that dtype's range, else inside uint16's); r, g, b: 0 .. 255; a in [0, 1]: the opacity accumulated over one
    physical unit of length."""
    text = str(text)
    if text.startswith("@"):
        path = text[1:]
        if not os.path.isfile(path):
            raise ValueError("transfer function file %r does not exist" % path)
        with open(path) as f:
            text = f.read()
    top = 65535 if out_kind is None else (1 << _kind(out_kind)[1]) - 1
    points = []
    for part in text.replace("\n", ";").split(";"):
        part = part.strip()
        if not part:
            continue
        try:
            level, rest = part.split(":")
            level = int(level.strip())
            r, g, b, a = (float(x) for x in rest.split(","))
        except ValueError:
            raise ValueError("transfer point %r is not of the form level:r,g,b,a (an integer level, three colours 0 .. 255, an opacity 0 .. 1)"
                             % part) from None
        if not 0 <= level <= top:
            raise ValueError("transfer point %r: level %d lies outside the range of the integer decode, 0 .. %d" % (part, level, top))
        if points and level <= points[-1][0]:
            raise ValueError("transfer point %r: levels must be strictly ascending (%d follows %d)" % (part, level, points[-1][0]))
        if not all(0 <= c <= 255 for c in (r, g, b)):
            raise ValueError("transfer point %r: a colour must lie in 0 .. 255" % part)
        if not 0 <= a <= 1:
            raise ValueError("transfer point %r: the opacity must lie in [0, 1]" % part)
        points.append((level, r, g, b, a))
    if not points:
        raise ValueError("a transfer function needs at least one point level:r,g,b,a")
    return points


def check_transfer(tf, out_kind):
    """a host-visible table as the kernels expect it: (int32 [2^bits, 4] C-contiguous, bits), every entry in range"""
    _, width = _kind(out_kind)
    t = np.ascontiguousarray(tf)
    if t.dtype != np.int32 or t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("a transfer table is int32 [2^bits, 4] = (tau, eR, eG, eB) (got %s %s)" % (t.dtype, t.shape))
    bits = int(t.shape[0]).bit_length() - 1
    if t.shape[0] != 1 << bits or not 1 <= bits <= width:
        raise ValueError("a transfer table of %d rows is refused: the rows must be 2^bits, bits 1 .. %d for %s data" % (t.shape[0], width, out_kind))
    if t[:, 0].min() < 0 or t[:, 0].max() > TAU_SAT:
        raise ValueError("a transfer table's tau must lie in 0 .. TAU_SAT = %d (got %d .. %d)" % (TAU_SAT, t[:, 0].min(), t[:, 0].max()))
    if t[:, 1:].min() < 0 or t[:, 1:].max() > E_MAX:
        raise ValueError("a transfer table's emission must lie in 0 .. %d (got %d .. %d)" % (E_MAX, t[:, 1:].min(), t[:, 1:].max()))
    return t, bits


def make_transfer(points, out_kind, depth_spacing, bits=None):
    """the table int32 [2^bits, 4] = (tau, eR, eG, eB) of the control points [(level, r, g, b, a), ...] (parse_transfer's) for rays
    sampled every `depth_spacing` physical units.  Entry i stands for the values i * 2^s .. (i + 1) * 2^s - 1, s = bits of the dtype -
    bits, and is taken at their middle, i * 2^s + (2^s - 1) / 2.  Colour and opacity are interpolated linearly between the points and
    constant outside them, in float64.  a is the opacity over one physical unit, so over a sample's step the transmittance is
    (1 - a)^depth_spacing: tau = rint(-log2(1 - a) * depth_spacing * 65536) clamped to TAU_SAT, a = 1 being TAU_SAT.  The opacity
    correction for the sample spacing happens here; the kernel stays integer.  e_c = rint(256 * colour_c * (1 - 2^(-tau / 65536))),
    from the already quantised tau.  bits: default 8 for uint8, 12 for uint16."""
    kind, width = _kind(out_kind)
    bits = DEFAULT_BITS[kind] if bits is None else int(bits)
    if not 1 <= bits <= width:
        raise ValueError("bits = %d is refused: a transfer table of %s data has 2^bits rows, bits 1 .. %d" % (bits, kind, width))
    depth_spacing = float(depth_spacing)
    if not (math.isfinite(depth_spacing) and depth_spacing > 0):
        raise ValueError("depth_spacing must be a positive finite number (got %r)" % (depth_spacing,))
    pts = [tuple(p) for p in points]
    if not pts or any(len(p) != 5 for p in pts):
        raise ValueError("a transfer function needs at least one point (level, r, g, b, a)")
    p = np.array(pts, np.float64)
    top = (1 << width) - 1
    if (p[:, 0] != np.rint(p[:, 0])).any() or (p[:, 0] < 0).any() or (p[:, 0] > top).any() or (np.diff(p[:, 0]) <= 0).any():
        raise ValueError("the levels of a transfer function must be integers of the integer decode, 0 .. %d, strictly ascending (got %s)"
                         % (top, [q[0] for q in pts]))
    if (p[:, 1:4] < 0).any() or (p[:, 1:4] > 255).any() or (p[:, 4] < 0).any() or (p[:, 4] > 1).any() or not np.isfinite(p).all():
        raise ValueError("a transfer point's colours must lie in 0 .. 255 and its opacity in [0, 1]")
    shift = width - bits
    x = np.arange(1 << bits, dtype=np.float64) * (1 << shift) + ((1 << shift) - 1) / 2.0
    colour = np.stack([np.interp(x, p[:, 0], p[:, 1 + c]) for c in range(3)], 1)
    a = np.clip(np.interp(x, p[:, 0], p[:, 4]), 0.0, 1.0)
    with np.errstate(divide="ignore"):
        octaves = -np.log2(1.0 - a) * depth_spacing              # (a = 1: inf, clamped below)
    tau = np.rint(np.minimum(octaves * 65536.0, float(TAU_SAT))).astype(np.int64)
    alpha = -np.expm1(-tau.astype(np.float64) / 65536.0 * math.log(2.0))
    tf = np.empty((1 << bits, 4), np.int32)
    tf[:, 0] = tau
    tf[:, 1:] = np.rint(256.0 * colour * alpha[:, None])
    return check_transfer(tf, kind)[0]


def composite_host(view, k0, off, vals, tf, channel=0, background=(0, 0, 0)):
    """the composite of given samples on the host CPU (brief_view_composite_host), no GPU call: (image uint8 [rows, cols, 4], hits int32
    [rows, cols], tau_run int32 [rows, cols], acc uint64 [rows, cols, 3]).  k0 [rays] int32 and off [rays + 1] int64 are the compacted
    list (off[0] == 0), vals [off[-1], channels] uint8 | uint16 its values, tf a table of check_transfer's form."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype not in (np.uint8, np.uint16) or vals.ndim != 2:
        raise ValueError("vals must be uint8 or uint16 [samples, channels] (got %s %s)" % (vals.dtype, vals.shape))
    kind = "u8" if vals.dtype == np.uint8 else "u16"
    tf, bits = check_transfer(tf, kind)
    rays = view.rows * view.cols
    k0, off = np.ascontiguousarray(k0, np.int32).ravel(), np.ascontiguousarray(off, np.int64).ravel()
    if len(k0) != rays or len(off) != rays + 1:
        raise ValueError("k0 needs one entry per ray and off one more (%d rays; got %d and %d)" % (rays, len(k0), len(off)))
    if len(vals) != int(off[-1]):
        raise ValueError("vals holds %d samples, off names %d" % (len(vals), int(off[-1])))
    hits, tau_run = np.empty(rays, np.int32), np.empty(rays, np.int32)
    acc, out = np.empty((rays, 3), np.uint64), np.empty((rays, 4), np.uint8)
    p = (lambda a: a.ctypes.data_as(C.c_void_p))
    bg = (C.c_int32 * 3)(*[int(b) for b in background])
    _lib.check(_lib.lib().brief_view_composite_host(C.byref(view), p(k0), p(off), p(vals), _lib.OUT_U8 if kind == "u8" else _lib.OUT_U16,
                                                    vals.shape[1], int(channel), p(tf), bits, bg, p(hits), p(tau_run), p(acc), p(out)))
    shape = (view.rows, view.cols)
    return out.reshape(*shape, 4), hits.reshape(shape), tau_run.reshape(shape), acc.reshape(*shape, 3)


def shade_quant(shade):
    """(ka_q, kd_q) = (round(256 * KA), round(256 * KD)), integers 0 .. 256, of shade = (KA, KD): the ambient and the diffuse weight of
    the shaded composite, each in [0, 1]"""
    try:
        ka, kd = (float(x) for x in shade)
    except (TypeError, ValueError):
        raise ValueError("shade must be two numbers KA,KD, the ambient and the diffuse weight, each in [0, 1] (got %r)" % (shade,)) from None
    if not (0.0 <= ka <= 1.0 and 0.0 <= kd <= 1.0):        # (a NaN fails both comparisons)
        raise ValueError("shade KA,KD = %r is refused: the ambient and the diffuse weight must each lie in [0, 1]" % (tuple(shade),))
    return int(math.floor(256.0 * ka + 0.5)), int(math.floor(256.0 * kd + 0.5))


def _shade_desc(gscale, light, ka_q, kd_q):
    """the brief_composite_shade of gscale and light (three finite numbers each, (z, y, x)) and the quantised weights"""
    g, l = view_mod._vec3(gscale, "gscale"), view_mod._vec3(light, "light")
    sh = _lib.CompositeShade()
    for a in range(3):
        sh.gscale[a], sh.light[a] = g[a], l[a]
    sh.ka_q, sh.kd_q = int(ka_q), int(kd_q)
    return sh


def shade_q_host(jac, gscale, light, ka_q, kd_q):
    """s_q int32 [n], the factor of a sample's emission in Q8, of the Jacobian rows jac [n, 3] float32 on the host CPU
    (brief_composite_shade_q_host: the header the kernels run); ka_q = 0, kd_q = 256 gives c_q = round(256 * |cos|) itself"""
    jac = np.ascontiguousarray(jac, np.float32)
    if jac.ndim != 2 or jac.shape[1] != 3 or not len(jac):
        raise ValueError("jac must be float32 [n, 3], n >= 1 (got %s)" % (jac.shape,))
    out = np.empty(len(jac), np.int32)
    sh = _shade_desc(gscale, light, ka_q, kd_q)
    _lib.check(_lib.lib().brief_composite_shade_q_host(jac.ctypes.data_as(C.c_void_p), len(jac), C.byref(sh), out.ctypes.data_as(C.c_void_p)))
    return out


def composite_shade_host(view, k0, off, vals, tf, jac, gscale, light, ka_q, kd_q, channel=0, background=(0, 0, 0)):
    """composite_host with every emission lit (brief_view_composite_shade_host), no GPU call: (image, hits, tau_run, acc, need int32
    [off[-1]]: the samples that need a gradient).  jac [off[-1], channels, 3] float32 is the dense Jacobian, one row per sample."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype not in (np.uint8, np.uint16) or vals.ndim != 2:
        raise ValueError("vals must be uint8 or uint16 [samples, channels] (got %s %s)" % (vals.dtype, vals.shape))
    kind = "u8" if vals.dtype == np.uint8 else "u16"
    tf, bits = check_transfer(tf, kind)
    rays = view.rows * view.cols
    k0, off = np.ascontiguousarray(k0, np.int32).ravel(), np.ascontiguousarray(off, np.int64).ravel()
    if len(k0) != rays or len(off) != rays + 1:
        raise ValueError("k0 needs one entry per ray and off one more (%d rays; got %d and %d)" % (rays, len(k0), len(off)))
    if len(vals) != int(off[-1]):
        raise ValueError("vals holds %d samples, off names %d" % (len(vals), int(off[-1])))
    jac = np.ascontiguousarray(jac, np.float32)
    if jac.shape != (len(vals), vals.shape[1], 3):
        raise ValueError("jac must be float32 [samples, channels, 3] = %s (got %s)" % ((len(vals), vals.shape[1], 3), jac.shape))
    sh = _shade_desc(gscale, light, ka_q, kd_q)
    hits, tau_run, need = np.empty(rays, np.int32), np.empty(rays, np.int32), np.zeros(len(vals), np.int32)
    acc, out = np.empty((rays, 3), np.uint64), np.empty((rays, 4), np.uint8)
    bg = (C.c_int32 * 3)(*[int(b) for b in background])
    _lib.check(_lib.lib().brief_view_composite_shade_host(C.byref(view), _hp(k0), _hp(off), _hp(vals), _lib.OUT_U8 if kind == "u8" else _lib.OUT_U16,
                                                          vals.shape[1], int(channel), _hp(tf), bits, bg, _hp(jac), C.byref(sh), _hp(need),
                                                          _hp(hits), _hp(tau_run), _hp(acc), _hp(out)))
    shape = (view.rows, view.cols)
    return out.reshape(*shape, 4), hits.reshape(shape), tau_run.reshape(shape), acc.reshape(*shape, 3), need


def _background(background):
    try:
        bg = [int(b) for b in background]
        whole = all(float(b) == int(b) for b in background)
    except (TypeError, ValueError):
        bg, whole = [], False
    if len(bg) != 3 or not whole or not all(0 <= b <= 255 for b in bg):
        raise ValueError("background must be three integers r, g, b in 0 .. 255 (got %r)" % (background,))
    return bg


def _device_table(tf, kind_name, width, dev):
    """(the table on the device, its bits): a numpy array is checked (check_transfer), an int32 device tensor of the same form is taken
    as it is"""
    import torch
    if isinstance(tf, torch.Tensor):
        bits = int(tf.shape[0]).bit_length() - 1 if tf.dim() == 2 else 0
        if tf.dtype != torch.int32 or tf.dim() != 2 or tf.shape[1] != 4 or tf.shape[0] != 1 << bits or not 1 <= bits <= width or not tf.is_contiguous():
            raise ValueError("a transfer table is a contiguous int32 [2^bits, 4], bits 1 .. %d for %s data (got %s %s)"
                             % (width, kind_name, tf.dtype, tuple(tf.shape)))
        return tf.to(dev), bits
    t, bits = check_transfer(tf, kind_name)
    return torch.from_numpy(t).to(dev), bits


def render_composite(phi, view, tf, lo, hi, out_kind, scale, vrange, channel=0, background=(0, 0, 0), chunk=None, shade=None, light=None,
                     gscale=None, compact=True):
    """the composite view of the net `phi` (any net kind and precision its forward entry serves) on the linspace grid view.dims over
    [lo, hi]: (image uint8 [rows, cols, 4] = R, G, B, A, hits [rows, cols] int32, stats) as device tensors.  Channel `channel` of the
    integer decode (out_kind 'u8' | 'u16' with scale / vrange: view.render's) is classified by the table `tf` (make_transfer's: a numpy
    array, checked here, or an int32 device tensor of the same form, taken as it is) and composited front to back along every ray, in
    ascending k; RGB is already composited over `background` (0 .. 255 per channel), A is the ray's opacity.  A ray without an inside
    sample shows the background with A = 0.  Samples are evaluated in chunks of at most `chunk` (default mip.DEFAULT_CHUNK) in the
    list's order; the image does not depend on it.  stats: view.render's keys.

    shade=(KA, KD), each in [0, 1]: the SHADED composite (csrc/brief_composite.h; DESIGN.md "Shaded composite").  Opacity, hits and A
    stay the plain composite's; a sample's emission is scaled by KA + KD * |n . l| in Q8, n the direction of the channel's analytic
    gradient times `gscale` (default gradient.voxel_scale: voxels of extent 1) and l the unit direction `light` travels (default the
    view's own direction ddepth; decompress_composite passes the physical ones).  The Jacobian is evaluated only at the samples that
    emit and are not hidden behind a saturated prefix; stats gains samples_shaded, their count.  compact=False evaluates it at every
    sample instead (the reference path: the same image).  A net without the Jacobian kernel (anything but an fp32 SIREN of at most
    1024 features) is refused before any decode.  shade=None is the plain composite; light, gscale or compact=False without shade
    are refused."""
    import torch
    from . import mip
    if shade is None:
        for name, given in (("light", light is not None), ("gscale", gscale is not None), ("compact=False", not compact)):
            if given:
                raise ValueError("%s describes the shaded composite: give its weights with shade=(KA, KD)" % name)
    else:
        return _render_composite_shaded(phi, view, tf, lo, hi, out_kind, scale, vrange, channel, background, chunk, shade, light, gscale, compact)
    kind_name, width = _kind(out_kind)
    if int(phi.coords_channel) != 3:
        raise ValueError("a view is defined for 3-D data only (the net takes %d coordinates)" % phi.coords_channel)
    ch = int(phi.data_channel)
    if int(channel) != channel or not 0 <= int(channel) < ch:
        raise ValueError("channel %r does not exist: the net has the channels 0 .. %d" % (channel, ch - 1))
    bg = (C.c_int32 * 3)(*_background(background))
    phi._require_gpu()
    dev = phi.params.device
    table, bits = _device_table(tf, kind_name, width, dev)
    chunk = int(chunk or mip.DEFAULT_CHUNK)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    L, st = _lib.lib(), _lib.stream_ptr
    v = view_mod._with_range(view, lo, hi)
    rays = v.rows * v.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if kind_name == "u8" else (_lib.OUT_U16, torch.uint16)
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    tau_run = torch.zeros(rays, dtype=torch.int32, device=dev)
    acc = torch.zeros((rays, 3), dtype=torch.int64, device=dev)         # (uint64 on the device; below 2^50 under a table of make_transfer)

    def fold(k0, off, s0, s1, r0, r1, lanes, vals):
        _lib.check(L.brief_view_composite_fold(C.byref(v), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch, int(channel),
                                               _lib.ptr(table), bits, _lib.ptr(hits), _lib.ptr(tau_run), _lib.ptr(acc), st()))
    _, total, rays_hit = view_mod._march(phi, v, kind, dt, scale, vrange, chunk, fold)
    image = torch.empty((v.rows, v.cols, 4), dtype=torch.uint8, device=dev)
    _lib.check(L.brief_view_composite_finish(C.byref(v), bg, _lib.ptr(hits), _lib.ptr(tau_run), _lib.ptr(acc), _lib.ptr(image), st()))
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": int(hits.sum(dtype=torch.int64).item()), "samples_evaluated": total}
    return image, hits.view(v.rows, v.cols), stats


def _render_composite_shaded(phi, view, tf, lo, hi, out_kind, scale, vrange, channel, background, chunk, shade, light, gscale, compact):
    """render_composite with shade: per chunk select (which samples need a gradient), scan, pick, the Jacobian on the picked samples
    and the shaded fold; a chunk that lights nothing is folded by the plain fold (every one of its samples adds 0)"""
    import torch
    from . import gradient, mip
    kind_name, width = _kind(out_kind)
    ka_q, kd_q = shade_quant(shade)
    if int(phi.coords_channel) != 3:
        raise ValueError("a view is defined for 3-D data only (the net takes %d coordinates)" % phi.coords_channel)
    ch = int(phi.data_channel)
    if int(channel) != channel or not 0 <= int(channel) < ch:
        raise ValueError("channel %r does not exist: the net has the channels 0 .. %d" % (channel, ch - 1))
    why = gradient.refusal(getattr(type(phi), "kind", "SIREN"), phi.precision, phi.features)
    if why is not None:
        raise ValueError("a shaded composite needs the analytic Jacobian: %s" % why)
    g = gscale if gscale is not None else gradient.voxel_scale(list(view.dims), lo, hi, scale, vrange[0], vrange[1])
    sh = _shade_desc(g, view_mod._unit3(light if light is not None else list(view.ddepth), "light"), ka_q, kd_q)
    bg = (C.c_int32 * 3)(*_background(background))
    phi._require_gpu()
    dev = phi.params.device
    table, bits = _device_table(tf, kind_name, width, dev)
    chunk = int(chunk or mip.DEFAULT_CHUNK)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    L, st = _lib.lib(), _lib.stream_ptr
    v = view_mod._with_range(view, lo, hi)
    rays = v.rows * v.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if kind_name == "u8" else (_lib.OUT_U16, torch.uint16)
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    tau_run = torch.zeros(rays, dtype=torch.int32, device=dev)
    acc = torch.zeros((rays, 3), dtype=torch.int64, device=dev)         # (uint64 on the device)
    buf = {}
    shaded = [0]

    def fold(k0, off, s0, s1, r0, r1, lanes, vals, coords):
        n = s1 - s0
        if not buf:                                                  # (the march's own chunk size: min(chunk, total))
            buf["need"] = torch.empty(len(vals), dtype=torch.int32, device=dev)
            buf["slot"] = torch.empty(len(vals), dtype=torch.int64, device=dev)
            buf["sel"] = torch.empty((len(vals), 3), dtype=torch.float32, device=dev) if compact else None
        need, slot = buf["need"], buf["slot"]
        head = (C.byref(v), _lib.ptr(k0), _lib.ptr(off), s0, s1, r0, r1, lanes, _lib.ptr(vals), kind, ch, int(channel), _lib.ptr(table), bits)
        _lib.check(L.brief_view_composite_select(*head, _lib.ptr(tau_run), _lib.ptr(need), st()))
        torch.cumsum(need[:n], 0, dtype=torch.int64, out=slot[:n])  # inclusive: the last entry is m
        m = int(slot[n - 1].item())                                  # the chunk's one host read
        shaded[0] += m
        if m == 0:
            _lib.check(L.brief_view_composite_fold(*head, _lib.ptr(hits), _lib.ptr(tau_run), _lib.ptr(acc), st()))
            return
        if compact:
            slot[:n] -= need[:n]                                     # exclusive
            _lib.check(L.brief_view_composite_pick(_lib.ptr(need), _lib.ptr(slot), _lib.ptr(coords), n, _lib.ptr(buf["sel"]), st()))
            _, jac = phi.spatial_gradient(buf["sel"][:m], want_value=False)
            p_slot = _lib.ptr(slot)
        else:
            _, jac = phi.spatial_gradient(coords[:n], want_value=False)
            p_slot = None
        _lib.check(L.brief_view_composite_shade_fold(*head, _lib.ptr(need), p_slot, _lib.ptr(jac), C.byref(sh), _lib.ptr(hits), _lib.ptr(tau_run),
                                                     _lib.ptr(acc), st()))
    _, total, rays_hit = view_mod._march(phi, v, kind, dt, scale, vrange, chunk, fold, with_coords=True)
    image = torch.empty((v.rows, v.cols, 4), dtype=torch.uint8, device=dev)
    _lib.check(L.brief_view_composite_finish(C.byref(v), bg, _lib.ptr(hits), _lib.ptr(tau_run), _lib.ptr(acc), _lib.ptr(image), st()))
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": int(hits.sum(dtype=torch.int64).item()), "samples_evaluated": total,
             "samples_shaded": shaded[0]}
    return image, hits.view(v.rows, v.cols), stats


# ---- the composite of a partition: the prefix is carried across blocks (csrc/brief_composite.h "the composite of a PARTITION") --------
def windows_table(pts):
    """(the table of brief_composite_window of the block descriptors `pts` (view.make_part's) as a ctypes array, window_rays): block b's
    slice of the block-major window-ray arrays starts at base[b]; an empty window is 0 x 0"""
    wins = (_lib.CompositeWindow * len(pts))()
    at = 0
    for w, pt in zip(wins, pts):
        n = int(pt.wrows) * int(pt.wcols)
        w.base = at
        w.row0, w.col0, w.wrows, w.wcols = (pt.row0, pt.col0, pt.wrows, pt.wcols) if n else (0, 0, 0, 0)
        at += n
    return wins, at


_hp = (lambda a: a.ctypes.data_as(C.c_void_p))


def part_fold_host(view, part, k0, off, vals, tf, hits_w, tau_w, acc_w, channel=0):
    """k_composite_part_fold on the host CPU (brief_view_composite_part_fold_host), no GPU call: folds the block's whole list (k0 [wrays]
    int32, off [wrays + 1] int64 in any numbering, vals [off[-1] - off[0], channels] uint8 | uint16) into the window rays' state
    hits_w int32 [wrays] (or None), tau_w int32 [wrays] (carry-in, then carry-out) and acc_w uint64 [wrays, 3], IN PLACE"""
    vals = np.ascontiguousarray(vals)
    if vals.dtype not in (np.uint8, np.uint16) or vals.ndim != 2:
        raise ValueError("vals must be uint8 or uint16 [samples, channels] (got %s %s)" % (vals.dtype, vals.shape))
    kind = "u8" if vals.dtype == np.uint8 else "u16"
    tf, bits = check_transfer(tf, kind)
    wrays = int(part.wrows) * int(part.wcols)
    k0, off = np.ascontiguousarray(k0, np.int32).ravel(), np.ascontiguousarray(off, np.int64).ravel()
    if len(k0) != wrays or len(off) != wrays + 1:
        raise ValueError("k0 needs one entry per window ray and off one more (%d window rays; got %d and %d)" % (wrays, len(k0), len(off)))
    if len(vals) != int(off[-1] - off[0]):
        raise ValueError("vals holds %d samples, off names %d" % (len(vals), int(off[-1] - off[0])))
    for a, dt, n in ((hits_w, np.int32, wrays), (tau_w, np.int32, wrays), (acc_w, np.uint64, wrays * 3)):
        if a is not None and (a.dtype != dt or a.size != n or not a.flags.c_contiguous):
            raise ValueError("the state of a block is hits_w int32 [wrays], tau_w int32 [wrays], acc_w uint64 [wrays, 3], C-contiguous")
    if wrays:
        _lib.check(_lib.lib().brief_view_composite_part_fold_host(
            C.byref(view), C.byref(part), _hp(k0), _hp(off), _hp(vals), _lib.OUT_U8 if kind == "u8" else _lib.OUT_U16, vals.shape[1], int(channel),
            _hp(tf), bits, _hp(hits_w) if hits_w is not None else None, _hp(tau_w), _hp(acc_w)))


def part_carry_host(view, wins, window_rays, k0, cnt, tau_w):
    """(carry, cnt2) int32 [window_rays] on the host CPU (brief_view_composite_part_carry_host): per segment the saturated sum of the
    totals tau_w of the same pixel's segments with a smaller k0, and cnt where 0 < carry < TAU_SAT, else 0"""
    k0, cnt, tau_w = (np.ascontiguousarray(a, np.int32).ravel() for a in (k0, cnt, tau_w))
    if not len(k0) == len(cnt) == len(tau_w) == window_rays:
        raise ValueError("k0, cnt and tau_w need one entry per window ray (%d)" % window_rays)
    carry, cnt2 = np.zeros(window_rays, np.int32), np.zeros(window_rays, np.int32)
    _lib.check(_lib.lib().brief_view_composite_part_carry_host(C.byref(view), wins, len(wins), window_rays, _hp(k0), _hp(cnt), _hp(tau_w),
                                                               _hp(carry), _hp(cnt2)))
    return carry, cnt2


def part_gather_host(view, wins, window_rays, hits_w, tau_w, acc_w, carry, acc_w2):
    """(hits int32 [rows, cols], tau_run int32 [rows, cols], acc uint64 [rows, cols, 3]) of the image from the window rays' state on the
    host CPU (brief_view_composite_part_gather_host)"""
    hits_w, tau_w, carry = (np.ascontiguousarray(a, np.int32).ravel() for a in (hits_w, tau_w, carry))
    acc_w, acc_w2 = (np.ascontiguousarray(a, np.uint64).ravel() for a in (acc_w, acc_w2))
    if not len(hits_w) == len(tau_w) == len(carry) == window_rays or not len(acc_w) == len(acc_w2) == 3 * window_rays:
        raise ValueError("the window rays' state needs one entry per window ray (%d), acc_w and acc_w2 three" % window_rays)
    rays = view.rows * view.cols
    hits, tau_run, acc = np.zeros(rays, np.int32), np.zeros(rays, np.int32), np.zeros((rays, 3), np.uint64)
    _lib.check(_lib.lib().brief_view_composite_part_gather_host(C.byref(view), wins, len(wins), window_rays, _hp(hits_w), _hp(tau_w), _hp(acc_w),
                                                                _hp(carry), _hp(acc_w2), _hp(hits), _hp(tau_run), _hp(acc)))
    shape = (view.rows, view.cols)
    return hits.reshape(shape), tau_run.reshape(shape), acc.reshape(*shape, 3)


def render_composite_partition(parts, view, tf, out_kind, channel=0, background=(0, 0, 0), chunk=None):
    """render_composite for a PARTITION of the grid view.dims: parts is view.render_partition's list of blocks (phi, start, dims, lo, hi,
    scale, vrange), and the nearest block owns a sample, exactly as there.  Returns (image uint8 [rows, cols, 4] = R, G, B, A, hits
    [rows, cols] int32, stats) as device tensors: the composite of every pixel's owned samples in ascending k, whichever block owns
    them, bit for bit what render_composite's fold gives on that list.  A sample in a gap no block covers contributes nothing; a ray
    that meets no block shows the background with A = 0.

    The blocks are evaluated in separate passes, in no depth order, and a sample's weight is the transmittance of everything in front
    of it.  Per pixel and block the owned samples are one interval of k, a SEGMENT.  PASS A marches all blocks (view._march_partition)
    and folds every segment on its own, under carry-in 0, into per-window-ray state: its total T and its colour sums.  The CARRY
    kernel gives every segment C = min(sum of T over the pixel's segments with a smaller k0, TAU_SAT).  C == 0 (nothing, or only
    transparent segments, in front): pass A's sums are final.  C == TAU_SAT: the segment is hidden.  PASS B marches only the other
    segments again, with carry-in C.  The GATHER kernel sums a pixel's segments, and the finish is render_composite's.  All sums are
    integer sums and the saturation commutes with them, so the order of the blocks, the chunking and the run change no bit.  Memory:
    one chunk, the per-window-ray state and the image; nothing grows with the samples.
    stats: view.render_partition's keys, samples_evaluated counting both passes, plus samples_second_pass and segments (non-empty
    intervals over all pixels and blocks)."""
    import torch
    kind_name, width = _kind(out_kind)
    parts, ch, chunk, pts, vs = view_mod._plan_partition(parts, view, chunk, "render_composite_partition")
    if int(channel) != channel or not 0 <= int(channel) < ch:
        raise ValueError("channel %r does not exist: the nets have the channels 0 .. %d" % (channel, ch - 1))
    channel = int(channel)
    bg = (C.c_int32 * 3)(*_background(background))
    dev = parts[0][0].params.device
    table, bits = _device_table(tf, kind_name, width, dev)
    L, stream, at_ray = _lib.lib(), _lib.stream_ptr(), view_mod._at_ray
    rays = view.rows * view.cols
    kind, dt = (_lib.OUT_U8, torch.uint8) if kind_name == "u8" else (_lib.OUT_U16, torch.uint16)
    wins, window_rays = windows_table(pts)
    hits = torch.zeros(rays, dtype=torch.int32, device=dev)
    tau_run = torch.zeros(rays, dtype=torch.int32, device=dev)
    acc = torch.zeros((rays, 3), dtype=torch.int64, device=dev)         # (uint64 on the device)
    p_table = _lib.ptr(table)
    evaluated = second = blocks_hit = segments = 0
    if window_rays > 0:
        hits_w = torch.zeros(window_rays, dtype=torch.int32, device=dev)
        tau_w = torch.zeros(window_rays, dtype=torch.int32, device=dev)
        acc_w = torch.zeros((window_rays, 3), dtype=torch.int64, device=dev)

        def fold_into(h, t, a):
            def fold(i, v, pt, base, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals):
                _lib.check(L.brief_view_composite_part_fold(v, pt, k0_b, off_b, s0, s1, r0, r1, lanes, p_vals, kind, ch, channel, p_table, bits,
                                                            at_ray(h, base) if h is not None else None, at_ray(t, base), at_ray(a, base), stream))
            return fold
        first = view_mod._march_partition(parts, vs, pts, kind, dt, chunk, fold_into(hits_w, tau_w, acc_w))
        evaluated, blocks_hit, segments = first["evaluated"], first["blocks_hit"], first["segments"]
        if evaluated > 0:
            k0, cnt = first["k0"], first["cnt"]
            d_wins = torch.frombuffer(bytearray(bytes(wins)), dtype=torch.uint8).to(dev)
            carry = torch.empty(window_rays, dtype=torch.int32, device=dev)
            cnt2 = torch.empty(window_rays, dtype=torch.int32, device=dev)
            v0 = C.byref(vs[0])
            _lib.check(L.brief_view_composite_part_carry(v0, _lib.ptr(d_wins), len(pts), window_rays, _lib.ptr(k0), _lib.ptr(cnt), _lib.ptr(tau_w),
                                                         _lib.ptr(carry), _lib.ptr(cnt2), stream))
            tau_w2 = carry.clone()
            acc_w2 = torch.zeros((window_rays, 3), dtype=torch.int64, device=dev)
            second = view_mod._march_partition(parts, vs, pts, kind, dt, chunk, fold_into(None, tau_w2, acc_w2), clipped=(k0, cnt),
                                               counts=cnt2)["evaluated"]
            _lib.check(L.brief_view_composite_part_gather(v0, _lib.ptr(d_wins), len(pts), window_rays, _lib.ptr(hits_w), _lib.ptr(tau_w),
                                                          _lib.ptr(acc_w), _lib.ptr(carry), _lib.ptr(acc_w2), _lib.ptr(hits), _lib.ptr(tau_run),
                                                          _lib.ptr(acc), stream))
    image = torch.empty((view.rows, view.cols, 4), dtype=torch.uint8, device=dev)
    _lib.check(L.brief_view_composite_finish(C.byref(vs[0]), bg, _lib.ptr(hits), _lib.ptr(tau_run), _lib.ptr(acc), _lib.ptr(image), stream))
    rays_hit, inside = torch.stack([(hits > 0).sum(), hits.sum(dtype=torch.int64)]).cpu().tolist()      # (a ray's range is exact: hit <=> hits > 0)
    stats = {"rays": rays, "rays_hit": rays_hit, "samples_inside": inside, "samples_evaluated": evaluated + second, "blocks": len(parts),
             "blocks_hit": blocks_hit, "rays_clipped": window_rays, "samples_second_pass": second, "segments": segments}
    return image, hits.view(view.rows, view.cols), stats


def open_single(opt, module_path, sideinfos):
    """view.open_single for the composite: a DivideTask artefact is refused in the composite's own words before any net is opened"""
    from .io import load_yaml
    if isinstance(sideinfos, str):
        sideinfos = load_yaml(sideinfos)
    if "phi_features" not in sideinfos or os.path.isdir(os.path.join(os.path.dirname(str(module_path)), "sideinfos")):
        raise ValueError(DIVIDE_REFUSAL)
    return view_mod.open_single(opt, module_path, sideinfos)


def decompress_composite(art, direction, transfer, up=None, region=None, centre=None, spacing=1.0, depth_spacing=1.0, size=None, depth=None,
                         voxel_size=(1, 1, 1), channel=0, background=(0, 0, 0), bits=None, device="cuda", chunk=None, return_hits=False,
                         shade=None, light=None):
    """the composite view of a stored SingleTask artefact (art: open_single's) as a numpy image uint8 [rows, cols, 4] = R, G, B, A, without
    decoding the volume.  The geometry arguments are view.make_view's; `region` is the clip box.

    transfer: the transfer function, as text (parse_transfer: 'level:r,g,b,a;...' or '@file') or as a list of points (level, r, g, b,
    a).  Its levels are grey levels of the artefact's INTEGER DECODE (uint8 / uint16 after the fused de-normalisation), BEFORE
    Decompress.postprocess, as for the surface view; a is the opacity over one physical unit, corrected for depth_spacing in
    make_transfer (bits: the table's size, default 8 for uint8, 12 for uint16).  A Decompress.postprocess that changes values is
    refused: a threshold or a clip would have to act on every sample before its classification, and the samples are never held.
    Refused by name before any decode: everything view.check_envelope refuses (error-bounded artefacts, 2-D data, dtype,
    normalisation, an axis of length 1), a non-identity postprocess, a channel that does not exist, a background outside 0 .. 255, a
    malformed transfer function; DivideTask artefacts by open_single.  return_hits: (image, hits [rows, cols] int32, stats).

    shade=(KA, KD): the shaded composite (render_composite).  The gradient is physical, the stored net's analytic Jacobian in grey
    levels per physical unit, and `light` is the physical direction the light travels, default `direction` (a headlight): both as
    decompress_surface derives them (view.physical_shading).  Refused by name before any decode too: KA or KD outside [0, 1], light
    without shade, a zero light, and a net without the Jacobian kernel (anything but an fp32 SIREN of at most 1024 features;
    quantised artefacts load as one)."""
    view_mod.check_envelope(art, "max")
    _check_postprocess(art)
    shading = {}
    if shade is None:
        if light is not None:
            raise ValueError("light describes the shaded composite: give its weights with shade=(KA, KD)")
    else:
        from . import gradient
        shade_quant(shade)
        why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
        if why is not None:
            raise ValueError("a shaded composite needs the analytic Jacobian: %s" % why)
        physical, gscale = view_mod.physical_shading(art, direction, up, light, voxel_size)
        shading = dict(shade=shade, light=physical, gscale=gscale)
    if int(channel) != channel or not 0 <= int(channel) < int(art.cout):
        raise ValueError("channel %r does not exist: the artefact has the channels 0 .. %d" % (channel, int(art.cout) - 1))
    _background(background)
    points = parse_transfer(transfer, art.out_kind) if isinstance(transfer, str) else transfer
    tf = make_transfer(points, art.out_kind, depth_spacing, bits)
    view = view_mod.make_view(art.dims, direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    image, hits, stats = render_composite(art.load_phi(device), view, tf, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange,
                                          channel=int(channel), background=background, chunk=chunk, **shading)
    img = image.cpu().numpy()
    return (img, hits.cpu().numpy(), stats) if return_hits else img


def _check_postprocess(art):
    from .misc import preprocess_is_identity
    pp = art.postprocess
    if not preprocess_is_identity(np.zeros(1, np.dtype(art.dtype)), pp.denoise.level, pp.denoise.close, pp.clip):
        raise ValueError("a composite view with a Decompress.postprocess that changes values is refused: the transfer function classifies "
                         "the integer decode of every sample, and a threshold or a clip (denoise.level %s, clip %s) does not commute with "
                         "the compositing; use an identity postprocess and put the threshold into the transfer function"
                         % (pp.denoise.level, list(pp.clip)))


def decompress_divide_composite(opt, orig_sideinfos, module_dir, sideinfos_dir, direction, transfer, up=None, region=None, centre=None, spacing=1.0,
                                depth_spacing=1.0, size=None, depth=None, voxel_size=(1, 1, 1), channel=0, background=(0, 0, 0), bits=None,
                                device="cuda", chunk=None, return_hits=False, shade=None, light=None):
    """decompress_composite for a stored DivideTask artefact (orig_sideinfos: the job's side info, dict or path; module_dir /
    sideinfos_dir: the blocks' trees), without decoding the volume or any block: the view is a view of the WHOLE volume, `region` and
    `centre` index it, the nearest block owns a sample (view.decompress_divide_view's rule; nothing is blended across a face), and the
    prefix of a ray's optical depth is carried across the blocks (render_composite_partition).  transfer, channel, background and bits
    are decompress_composite's.  Refused by name before any net is opened: per block everything view.check_envelope refuses
    (error-bounded blocks, dtype, normalisation, an axis of length 1), a Decompress.postprocess that changes values, blocks of
    different dtypes or channel counts, overlapping blocks, 2-D data, an axis of 2^23 or more, a channel that does not exist, a
    background outside 0 .. 255, a malformed transfer function; shade or light (the shaded composite of a partition is a follow-up).
    return_hits: (image, hits [rows, cols] int32, stats)."""
    from . import artefact, config
    if shade is not None or light is not None:
        raise ValueError(DIVIDE_SHADE_REFUSAL)
    if isinstance(opt, str):
        opt = config.load(opt)
    data_shape, blocks = artefact.divide_blocks(orig_sideinfos, module_dir, sideinfos_dir, one_dtype="the composite view")
    if len(data_shape) != 4:
        raise ValueError(view_mod.ENVELOPE["need_3d"] % (len(data_shape) - 1, data_shape))
    arts = [artefact.open_artefact(opt, b.module_path, b.side) for b in blocks]
    for art in arts:
        view_mod.check_envelope(art, "max")
        _check_postprocess(art)
    pair = artefact.first_overlap(blocks, "dhw")
    if pair is not None:
        raise ValueError("the blocks %s and %s overlap: merge_divided_data adds overlapping blocks, and a sample of a view has one owner; "
                         "decode the region and render it" % (pair[0].name, pair[1].name))
    starts = [[b.ranges[a][0] for a in "dhw"] for b in blocks]
    for b, art in zip(blocks, arts):
        if art.cout != data_shape[-1] or art.dims != [b.ranges[a][1] - b.ranges[a][0] + 1 for a in "dhw"]:
            raise ValueError("the block %s holds data of shape %s: not its index range of a volume with %d channels" % (b.name, art.data_shape, data_shape[-1]))
    if int(channel) != channel or not 0 <= int(channel) < int(data_shape[-1]):
        raise ValueError("channel %r does not exist: the artefact has the channels 0 .. %d" % (channel, int(data_shape[-1]) - 1))
    _background(background)
    out_kind = arts[0].out_kind
    points = parse_transfer(transfer, out_kind) if isinstance(transfer, str) else transfer
    tf = make_transfer(points, out_kind, depth_spacing, bits)
    view = view_mod.make_view(data_shape[:-1], direction, up, centre, spacing, depth_spacing, size, depth, voxel_size, region)
    view_mod.make_part(view, starts[0], arts[0].dims, "image")    # (the 2^23 rule, before any net is opened)
    parts = [(art.load_phi(device), s, art.dims, art.lo, art.hi, art.norm_range, art.vrange) for art, s in zip(arts, starts)]
    image, hits, stats = render_composite_partition(parts, view, tf, out_kind, channel=int(channel), background=background, chunk=chunk)
    img = image.cpu().numpy()
    return (img, hits.cpu().numpy(), stats) if return_hits else img
