"""Spatial gradients straight from a stored artefact: the analytic Jacobian of the fitted SIREN with respect to the voxel position,
in grey levels per voxel step, evaluated on the HIP path (csrc/brief_jac.inc through SIREN.decode_gradient_box) with decode_box's
region semantics: a region equals the slice of the whole, results do not depend on how a region is cut into calls, and the same
call gives the same bits.  (DESIGN.md "Spatial-gradient decode".)

voxel_scale, refusal and supported are host arithmetic; everything else needs a ROCm GPU (there is no CPU fallback)."""
import functools

from . import derivative
from .derivative import MAX_FEATURES, NETS, PRECISIONS      # noqa: F401 (the envelope is the two derivative decodes')

NOUN = derivative.Noun("spatial gradients", "gradient", "spatial-gradient decode")


def voxel_scale(dims, lo, hi, norm_range, vmin, vmax):
    """per axis (hi - lo) / (dims[a] - 1) * (vmax - vmin) / (b - a), in float64; 0 for an axis of length 1.

    The factor between d(net output) / d(coordinate) and grey levels per voxel step: the derivative of the unclipped, untruncated
    invnormalize_data('minmaxany_a_b') of the net's output ((y - a) / (b - a) * (vmax - vmin) + vmin, norm_range = (a, b)), per step
    of one voxel of the linspace grid `dims` over [lo, hi] that is being evaluated.  With a stride it is still per voxel of that grid;
    with a resampled view (shape) `dims` is the resampled grid, so it is per voxel of that one."""
    return derivative.steps(dims, lo, hi) * derivative.grey(norm_range, vmin, vmax)


def refusal(phi_name, precision, features):
    """None where spatial gradients exist, else the refusal text (pure: no GPU, no library)"""
    return derivative.refusal(NOUN, phi_name, precision, features)


def supported(phi_name, precision, features):
    """whether spatial gradients exist for a net of this class, precision and width (refusal() has the text)"""
    return refusal(phi_name, precision, features) is None


def check_artefact(art):
    """what decompress_gradient supports, checked on the opened artefact before any decode"""
    derivative.check_artefact(art, NOUN)


def _block_gradient(art, dims, start, stop, step, device, chunk=None):
    """the scaled Jacobian [*extent, cout, cin] (device, float32) of one stored net over the box start:stop:step of the grid `dims`"""
    import torch
    phi = art.load_phi(device)
    jac, _ = phi.decode_gradient_box(dims, start, stop, step, art.lo, art.hi, chunk=chunk, want_value=False)
    scale = voxel_scale(dims, art.lo, art.hi, art.norm_range, art.vrange[0], art.vrange[1])
    return jac * torch.tensor(scale, dtype=torch.float32, device=jac.device)


def decompress_gradient_device(opt, module_path, sideinfos, region=None, step=1, shape=None, device="cuda", chunk=None):
    """decompress_gradient's result as a device tensor (what the magnitude of decompress.py is taken of)"""
    return derivative.single(opt, module_path, sideinfos, region, step, shape, device, functools.partial(_block_gradient, chunk=chunk), NOUN)


def decompress_gradient(opt, module_path, sideinfos, region=None, step=1, shape=None, device="cuda", chunk=None):
    """The spatial gradient of a stored SingleTask artefact over `region` (None: the whole grid; NFGR.decompress_region's region,
    step and shape semantics): numpy float32 [*extent, cout, cin], entry [..., c, a] = d(channel c) / d(axis a) in GREY LEVELS PER
    VOXEL STEP of the grid being evaluated (the fitted one; with `shape`, the resampled one; a stride does not change the unit).

    It is voxel_scale x the analytic Jacobian of the stored net at the voxel centres: the derivative of the unclipped, untruncated
    de-normalised output.  Defined for 'minmaxany_a_b' artefacts of any dtype; other normalisations are refused by name.  Quantised
    artefacts work unchanged (load_model dequantises: the gradient is that of the dequantised weights).  For an error-bounded
    artefact the result is the gradient of the net ALONE: the stored corrections are integer repairs of single voxels and have no
    derivative.  Decompress.postprocess (threshold, clip) is NOT applied: it acts on grey values, not on their derivative.
    Nets other than an fp32 SIREN of at most 1024 features are refused before any decode."""
    return decompress_gradient_device(opt, module_path, sideinfos, region, step, shape, device, chunk).cpu().numpy()


def decompress_divide_gradient_device(opt, orig_sideinfos, module_dir, sideinfos_dir, region=None, step=1, device="cuda", chunk=None):
    """decompress_divide_gradient's result as a device tensor"""
    return derivative.divide(opt, orig_sideinfos, module_dir, sideinfos_dir, region, step, device, functools.partial(_block_gradient, chunk=chunk),
                             lambda nd: nd, NOUN)


def decompress_divide_gradient(opt, orig_sideinfos, module_dir, sideinfos_dir, region=None, step=1, device="cuda", chunk=None):
    """The spatial gradient of a stored DivideTask artefact over `region` (decompress_divide_region's region semantics): numpy float32
    [*extent, cout, cin] in grey levels per voxel step.  Only the blocks that meet the region are evaluated; each on its OWN grid and
    with its OWN voxel_scale (its dims, its min and max), placed at its output offset; voxels no block covers are 0.  The field is
    each block's own net up to the block's faces and is DISCONTINUOUS there: no derivative is taken across a face.  Blocks whose
    ranges overlap are refused (merge_divided_data adds and clips there).  decompress_gradient's notes on corrections, quantised
    weights and Decompress.postprocess hold per block."""
    return decompress_divide_gradient_device(opt, orig_sideinfos, module_dir, sideinfos_dir, region, step, device, chunk).cpu().numpy()


def magnitude(grad):
    """sqrt(sum over the axes of g^2): [*extent, cout, cin] -> [*extent, cout] (a torch tensor in, the same device out)"""
    return (grad * grad).sum(dim=-1).sqrt()
