"""What the spatial-gradient decode (gradient.py) and the Hessian decode (hessian.py) have in common: the float64 factors between
coordinate units and grey levels per voxel step, the refusals, and the one walk over a stored artefact (single) or over the blocks of
a DivideTask artefact (divide).  A decode is a Noun (its three wordings) and a block function; a further derivative map (a curvature,
a divergence) is another pair of those, not another copy of the walk.  (DESIGN.md "Derivative decodes: the shared pieces".)

steps, grey, refusal and check_artefact are host arithmetic; the walks need a ROCm GPU (there is no CPU fallback)."""
import collections

import numpy as np

from . import artefact, config
from . import region as region_mod

MAX_FEATURES = 1024
NETS = ("SIREN",)                  # the net classes brief_siren_jac_* / brief_siren_hess_* evaluate
PRECISIONS = ("fp32", "f32")

# a decode's wordings: `plural` exist for some nets ("spatial gradients"), no merged block has a `single` ("gradient"), the `decode`
# refuses by name ("spatial-gradient decode")
Noun = collections.namedtuple("Noun", "plural single decode")


def steps(dims, lo, hi):
    """per axis (hi - lo) / (dims[a] - 1) in float64, the step of one voxel of the linspace grid `dims` over [lo, hi]; 0 for an axis of
    length 1"""
    out = np.zeros(len(dims), dtype=np.float64)
    for ax, n in enumerate(dims):
        if int(n) > 1:
            out[ax] = (np.float64(hi) - np.float64(lo)) / np.float64(int(n) - 1)
    return out


def grey(norm_range, vmin, vmax):
    """(vmax - vmin) / (b - a) in float64: grey levels per unit of the net's output under invnormalize_data('minmaxany_a_b'),
    norm_range = (a, b)"""
    a, b = (np.float64(v) for v in norm_range)
    return (np.float64(vmax) - np.float64(vmin)) / (b - a)


def refusal(noun, phi_name, precision, features):
    """None where the decode exists, else the refusal text (pure: no GPU, no library)"""
    if str(phi_name) not in NETS or str(precision) not in PRECISIONS or not 1 <= int(features) <= MAX_FEATURES:
        return "%s exist for fp32 SIREN up to %d features (this net is %s, %s, %d features)" % (
            noun.plural, MAX_FEATURES, phi_name, precision, int(features))
    return None


def check_artefact(art, noun):
    """what the decode supports, checked on the opened artefact before any decode"""
    why = refusal(noun, art.phi_name, art.precision, art.phi_features)
    if why is not None:
        raise ValueError(why)
    artefact.check_envelope(art, need_minmaxany="the " + noun.decode + " supports the 'minmaxany_a_b' normalisations only (their inverse "
                                                "is affine in the net's output), not Normalize.name=%s")


def single(opt, module_path, sideinfos, region, step, shape, device, block_fn, noun):
    """block_fn(art, dims, start, stop, step, device) over `region` of a stored SingleTask artefact (None: the whole grid;
    NFGR.decompress_region's region, step and shape semantics)"""
    art = artefact.open_artefact(opt, module_path, sideinfos)
    check_artefact(art, noun)
    dims = artefact.view_dims(art.dims, shape)
    start, stop, stp = region_mod.normalize_region(dims, region if region is not None else (slice(None),) * len(dims), step)
    return block_fn(art, dims, start, stop, stp, device)


def divide(opt, orig_sideinfos, module_dir, sideinfos_dir, region, step, device, block_fn, last_axis, noun):
    """float32 [*extent, cout, last_axis(number of axes)] on `device`: block_fn of every block of a stored DivideTask artefact that meets
    `region`, each on its own grid, placed at its output offset; voxels no block covers are 0.  Every block is opened and every refusal
    made before any decode; blocks whose ranges overlap are refused."""
    import torch
    if isinstance(opt, str):
        opt = config.load(opt)
    data_shape, blocks = artefact.divide_blocks(orig_sideinfos, module_dir, sideinfos_dir)
    dims, cout = data_shape[:-1], data_shape[-1]
    start, stop, stp = region_mod.normalize_region(dims, region if region is not None else (slice(None),) * len(dims), step)
    ext = region_mod.extents(start, stop, stp)
    arts = {b.name: artefact.open_artefact(opt, b.module_path, b.side) for b in blocks}
    for art in arts.values():
        check_artefact(art, noun)
    pair = artefact.first_overlap(blocks, "dhw" if len(dims) == 3 else "hw")
    if pair is not None:
        raise ValueError("the blocks %s and %s overlap: merge_divided_data adds overlapping blocks and clips the sum, which has "
                         "no single net's %s; the %s needs a partition without overlap" % (pair[0].name, pair[1].name, noun.single, noun.decode))
    out = torch.zeros((*ext, cout, last_axis(len(dims))), dtype=torch.float32, device=device)
    for b, o_lo, o_hi, l_start, l_stop in artefact.meeting(blocks, start, stp, ext):
        art = arts[b.name]
        out[tuple(slice(lo, hi) for lo, hi in zip(o_lo, o_hi))] = block_fn(art, art.dims, l_start, l_stop, stp, device)
    return out
