"""Second-order feature maps straight from a stored artefact: the analytic Hessian of the fitted SIREN with respect to the voxel
position, in grey levels per voxel step squared, evaluated on the HIP path (csrc/brief_hess.inc through SIREN.decode_hessian_box) with
decode_box's region semantics: a region equals the slice of the whole, results do not depend on how a region is cut into calls, and the
same call gives the same bits.  The derived maps (laplacian, eigenvalues, vesselness) are elementwise torch ops on the device, per chunk
of the result.  (DESIGN.md "Hessian decode".)

Component order of the last axis (the upper triangle, row by row): (00, 01, 02, 11, 12, 22) for three axes, (00, 01, 11) for two.

voxel_scale, refusal, supported, and laplacian / eigenvalues / vesselness on CPU tensors are host arithmetic; everything else needs a ROCm
GPU (there is no CPU fallback)."""
import functools
import math

import numpy as np

from . import derivative
from .derivative import MAX_FEATURES, NETS, PRECISIONS      # noqa: F401 (the envelope is the two derivative decodes')

NOUN = derivative.Noun("spatial Hessians", "Hessian", "Hessian decode")
MODES = ("components", "laplacian", "eigenvalues", "vesselness")
PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}      # axes of component h
DERIVED_CHUNK = 1 << 22            # rows of the result a derived map is computed on at a time (its float64 temporaries)


def ndim_of(nh):
    """the number of axes of a Hessian with nh stored components (3 -> 2, 6 -> 3)"""
    if nh not in (3, 6):
        raise ValueError("a Hessian has 3 (two axes) or 6 (three axes) stored components, not %d" % nh)
    return 2 if nh == 3 else 3


def voxel_scale(dims, lo, hi, norm_range, vmin, vmax):
    """per component (a, b): step_a * step_b * (vmax - vmin) / (hi_n - lo_n), in float64 [nh]; step_a = (hi - lo) / (dims[a] - 1), 0 for an
    axis of length 1.

    The factor between d2(net output) / d(coordinate a) d(coordinate b) and grey levels per voxel step squared: the second derivative
    of the unclipped, untruncated invnormalize_data('minmaxany_a_b') of the net's output (affine: (y - lo_n) / (hi_n - lo_n) * (vmax -
    vmin) + vmin, norm_range = (lo_n, hi_n)), per step of one voxel of the linspace grid `dims` over [lo, hi] along each of the two
    axes.  With a stride it is still per voxel of that grid; with a resampled view (shape) `dims` is the resampled grid."""
    step = derivative.steps(dims, lo, hi)
    grey = derivative.grey(norm_range, vmin, vmax)
    return np.array([step[i] * step[j] * grey for i, j in PAIRS[len(dims)]], dtype=np.float64)


def refusal(phi_name, precision, features):
    """None where spatial Hessians exist, else the refusal text (pure: no GPU, no library)"""
    return derivative.refusal(NOUN, phi_name, precision, features)


def supported(phi_name, precision, features):
    """whether spatial Hessians exist for a net of this class, precision and width (refusal() has the text)"""
    return refusal(phi_name, precision, features) is None


def check_artefact(art):
    """what decompress_hessian supports, checked on the opened artefact before any decode"""
    derivative.check_artefact(art, NOUN)


def check_mode(mode):
    if mode not in MODES:
        raise ValueError("unknown Hessian mode %r (%s)" % (mode, ", ".join(MODES)))


# ---- derived maps: elementwise torch ops on whatever device the components are on

def full(h):
    """[..., nh] -> the symmetric matrices [..., n, n]"""
    import torch
    n = ndim_of(h.shape[-1])
    out = torch.empty((*h.shape[:-1], n, n), dtype=h.dtype, device=h.device)
    for k, (i, j) in enumerate(PAIRS[n]):
        out[..., i, j] = h[..., k]
        out[..., j, i] = h[..., k]
    return out


def laplacian(h):
    """the trace: [..., nh] -> [...]  (float32 sums in the order 00 + 11 (+ 22))"""
    n = ndim_of(h.shape[-1])
    if n == 2:
        return h[..., 0] + h[..., 2]
    return h[..., 0] + h[..., 3] + h[..., 5]


def frobenius(h):
    """the Frobenius norm of the symmetric matrix (off-diagonal components count twice): [..., nh] -> [...]"""
    n = ndim_of(h.shape[-1])
    if n == 2:
        return (h[..., 0] ** 2 + h[..., 2] ** 2 + 2 * h[..., 1] ** 2).sqrt()
    return (h[..., 0] ** 2 + h[..., 3] ** 2 + h[..., 5] ** 2 + 2 * (h[..., 1] ** 2 + h[..., 2] ** 2 + h[..., 4] ** 2)).sqrt()


def _eig64(h):
    """the eigenvalues in float64, ascending by value: [..., nh] -> [..., n]; closed forms, elementwise"""
    import torch
    n = ndim_of(h.shape[-1])
    h = h.to(torch.float64)
    if n == 2:
        a, b, d = h[..., 0], h[..., 1], h[..., 2]
        m = 0.5 * (a + d)
        r = torch.sqrt((0.5 * (a - d)) ** 2 + b * b)
        return torch.stack((m - r, m + r), dim=-1)
    a, b, c, d, e, f = (h[..., k] for k in range(6))
    # A = q I + p B with B traceless, tr B^2 = 6: the eigenvalues of B are 2 cos(phi + 2 pi k / 3), cos 3 phi = det B / 2
    q = (a + d + f) / 3.0
    aq, dq, fq = a - q, d - q, f - q
    p2 = (aq * aq + dq * dq + fq * fq + 2.0 * (b * b + c * c + e * e)) / 6.0
    p = torch.sqrt(p2)
    det = aq * (dq * fq - e * e) - b * (b * fq - e * c) + c * (b * e - dq * c)
    safe = p > 0
    r = torch.where(safe, det / torch.where(safe, 2.0 * p2 * p, torch.ones_like(p)), torch.zeros_like(p)).clamp(-1.0, 1.0)
    phi = torch.acos(r) / 3.0
    e_hi = q + 2.0 * p * torch.cos(phi)
    e_lo = q + 2.0 * p * torch.cos(phi + 2.0 * math.pi / 3.0)
    e_mid = 3.0 * q - e_hi - e_lo
    return torch.stack((e_lo, e_mid, e_hi), dim=-1)


def _by_abs(ev):
    import torch
    order = torch.argsort(ev.abs(), dim=-1, stable=True)
    return torch.gather(ev, -1, order)


def eigenvalues(h):
    """The eigenvalues of the symmetric matrices: [..., nh] -> float32 [..., n], sorted by increasing absolute value (|l1| <= |l2| <=
    |l3|, Frangi's order).  The closed-form trigonometric solution (3 x 3) / the quadratic (2 x 2), evaluated elementwise in float64
    and rounded to float32 at the end; no torch.linalg."""
    import torch
    return _by_abs(_eig64(h)).to(torch.float32)


def vesselness(h, alpha=0.5, beta=0.5, c=None, bright=True):
    """Frangi's single-scale vesselness on eigenvalues(h): [..., nh] -> float32 [...].

    three axes (|l1| <= |l2| <= |l3|):  Ra = |l2| / |l3|, Rb = |l1| / sqrt(|l2 l3|), S = sqrt(l1^2 + l2^2 + l3^2),
        V = (1 - exp(-Ra^2 / 2 alpha^2)) exp(-Rb^2 / 2 beta^2) (1 - exp(-S^2 / 2 c^2)),   0 unless l2 and l3 are both negative (bright
        tubes on a dark ground; bright=False: both positive)
    two axes (|l1| <= |l2|):  Rb = |l1| / |l2|, S = sqrt(l1^2 + l2^2),
        V = exp(-Rb^2 / 2 beta^2) (1 - exp(-S^2 / 2 c^2)),   0 unless l2 is negative (bright=False: positive)
    c=None: half the largest Frobenius norm of the map `h` (Frangi's choice); a map of zeros scores 0."""
    import torch
    n = ndim_of(h.shape[-1])
    if c is None:
        c = 0.5 * float(frobenius(h.to(torch.float64)).max()) if h.numel() else 0.0
    ev = _by_abs(_eig64(h))
    s2 = (ev * ev).sum(dim=-1)
    tiny = torch.finfo(torch.float64).tiny
    structure = 1.0 - torch.exp(-s2 / (2.0 * c * c)) if c > 0 else torch.zeros_like(s2)
    if n == 2:
        l1, l2 = ev[..., 0], ev[..., 1]
        rb2 = (l1 / l2.abs().clamp_min(tiny)) ** 2
        v = torch.exp(-rb2 / (2.0 * beta * beta)) * structure
        ok = (l2 < 0) if bright else (l2 > 0)
    else:
        l1, l2, l3 = ev[..., 0], ev[..., 1], ev[..., 2]
        ra2 = (l2 / l3.abs().clamp_min(tiny)) ** 2
        rb2 = l1 * l1 / (l2 * l3).abs().clamp_min(tiny)
        v = (1.0 - torch.exp(-ra2 / (2.0 * alpha * alpha))) * torch.exp(-rb2 / (2.0 * beta * beta)) * structure
        ok = ((l2 < 0) & (l3 < 0)) if bright else ((l2 > 0) & (l3 > 0))
    return torch.where(ok, v, torch.zeros_like(v)).to(torch.float32)


def derive(h, mode, chunk=DERIVED_CHUNK, **kw):
    """the map `mode` of the components h [*extent, cout, nh], computed where h lives, `chunk` rows at a time: components -> h itself,
    laplacian / vesselness -> [*extent, cout], eigenvalues -> [*extent, cout, n].  vesselness with c=None takes c from the WHOLE map."""
    import torch
    check_mode(mode)
    if mode == "components":
        return h
    if mode == "laplacian":
        return laplacian(h)
    nh = h.shape[-1]
    flat = h.reshape(-1, nh)
    if mode == "vesselness" and kw.get("c") is None:
        kw = dict(kw, c=0.5 * max([float(frobenius(flat[o:o + chunk].to(torch.float64)).max()) for o in range(0, flat.shape[0], chunk)], default=0.0))
    fn = eigenvalues if mode == "eigenvalues" else (lambda t: vesselness(t, **kw))
    parts = [fn(flat[o:o + chunk]) for o in range(0, flat.shape[0], chunk)]
    out = torch.cat(parts, dim=0) if parts else fn(flat)
    return out.reshape(*h.shape[:-1], *out.shape[1:])


# ---- artefact walks (derivative.py's)

def _block_hessian(art, dims, start, stop, step, device, chunk=None):
    """the scaled components [*extent, cout, nh] (device, float32) of one stored net over the box start:stop:step of the grid `dims`"""
    import torch
    phi = art.load_phi(device)
    hess = phi.decode_hessian_box(dims, start, stop, step, art.lo, art.hi, chunk=chunk)
    scale = voxel_scale(dims, art.lo, art.hi, art.norm_range, art.vrange[0], art.vrange[1])
    return hess * torch.tensor(scale, dtype=torch.float32, device=hess.device)


def decompress_hessian_device(opt, module_path, sideinfos, region=None, step=1, shape=None, mode="components", device="cuda", chunk=None, **kw):
    """decompress_hessian's result as a device tensor"""
    check_mode(mode)
    h = derivative.single(opt, module_path, sideinfos, region, step, shape, device, functools.partial(_block_hessian, chunk=chunk), NOUN)
    return derive(h, mode, **kw)


def decompress_hessian(opt, module_path, sideinfos, region=None, step=1, shape=None, mode="components", device="cuda", chunk=None, **kw):
    """The Hessian of a stored SingleTask artefact over `region` (None: the whole grid; NFGR.decompress_region's region, step and shape
    semantics), as numpy float32:
        mode="components"   [*extent, cout, nh]  entry [..., c, h] = d2(channel c) / d(axis a) d(axis b), (a, b) = PAIRS[ndim][h], in GREY
                            LEVELS PER VOXEL STEP SQUARED of the grid being evaluated (the fitted one; with `shape`, the resampled one; a
                            stride does not change the unit)
        mode="laplacian"    [*extent, cout]      the trace
        mode="eigenvalues"  [*extent, cout, n]   sorted by increasing absolute value
        mode="vesselness"   [*extent, cout]      Frangi's single-scale measure (alpha, beta, c, bright as keywords; c=None: half the
                            largest Frobenius norm of THIS result)
    It is voxel_scale x the analytic Hessian of the stored net at the voxel centres: the second derivative of the unclipped,
    untruncated de-normalised output.  Defined for 'minmaxany_a_b' artefacts of any dtype; other normalisations are refused by name.
    Quantised artefacts work unchanged (load_model dequantises).  For an error-bounded artefact the result is the Hessian of the net
    ALONE: the stored corrections are integer repairs of single voxels and have no derivative.  Decompress.postprocess is NOT applied.
    Nets other than an fp32 SIREN of at most 1024 features are refused before any decode."""
    return decompress_hessian_device(opt, module_path, sideinfos, region, step, shape, mode, device, chunk, **kw).cpu().numpy()


def decompress_divide_hessian_device(opt, orig_sideinfos, module_dir, sideinfos_dir, region=None, step=1, mode="components", device="cuda",
                                     chunk=None, **kw):
    """decompress_divide_hessian's result as a device tensor"""
    check_mode(mode)
    h = derivative.divide(opt, orig_sideinfos, module_dir, sideinfos_dir, region, step, device, functools.partial(_block_hessian, chunk=chunk),
                          lambda nd: len(PAIRS[nd]), NOUN)
    return derive(h, mode, **kw)


def decompress_divide_hessian(opt, orig_sideinfos, module_dir, sideinfos_dir, region=None, step=1, mode="components", device="cuda",
                              chunk=None, **kw):
    """The Hessian of a stored DivideTask artefact over `region` (decompress_divide_region's region semantics; decompress_hessian's
    modes and units).  Only the blocks that meet the region are evaluated; each on its OWN grid and with its OWN voxel_scale (its dims,
    its min and max), placed at its output offset; voxels no block covers are 0.  The field is each block's own net up to the block's
    faces and is DISCONTINUOUS there: no derivative is taken across a face.  Blocks whose ranges overlap are refused (merge_divided_data
    adds and clips there); there is no `shape` (every block has its own linspace grid).  The derived maps are taken of the assembled
    components (vesselness with c=None: half the largest Frobenius norm over the whole region)."""
    return decompress_divide_hessian_device(opt, orig_sideinfos, module_dir, sideinfos_dir, region, step, mode, device, chunk, **kw).cpu().numpy()
