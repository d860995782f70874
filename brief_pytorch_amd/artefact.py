"""Reading a stored artefact: what is stored under a `compressed` directory and how it is evaluated.  open_artefact turns (options,
module path, side info) into one Artefact that every decode path starts from; check_envelope is the one list of "what this decode
supports" refusals; divide_blocks / first_overlap / meeting walk the blocks of a DivideTask artefact.  (DESIGN.md "Reading an
artefact".)

Host code: nothing here imports torch or the HIP library until load_phi, so refusals stay GPU-free."""
import collections
import copy
import os

import numpy as np

from . import config, corrections
from . import region as region_mod


# ---- the three helpers every decoder needs -----------------------------------------------------------------------------------------
def _coords_range(mode):
    if mode == "n11":
        return -1.0, 1.0
    if mode == "0p1":
        return 0.0, 1.0
    lo, hi = mode.split(",")
    return float(lo), float(hi)


def check_error_bound(cf, dtype):
    """the error-bounded mode acts on the integers of the fused decode epilogue: uint8 / uint16 data under a 'minmaxany_a_b'
    normalisation, and nothing may change values behind it (Decompress.postprocess must be the identity).  Anything else is
    refused by name: the bound could not be promised."""
    from .io import minmaxany_range
    from .misc import preprocess_is_identity
    dtype = np.dtype(dtype)
    if dtype.name not in ("uint8", "uint16"):
        raise ValueError("Compress.error_bound supports uint8 / uint16 data only: a bound in grey levels cannot be promised for %s data" % dtype.name)
    if minmaxany_range(cf.Normalize.name) is None:
        raise ValueError("Compress.error_bound supports the 'minmaxany_a_b' normalisations only (the fused integer decode): the bound "
                         "cannot be promised under Normalize.name=%s" % cf.Normalize.name)
    pp = cf.Decompress.postprocess
    if not preprocess_is_identity(np.zeros(1, dtype), pp.denoise.level, pp.denoise.close, pp.clip):
        raise ValueError("Compress.error_bound needs an identity Decompress.postprocess (denoise.level <= 0, a clip that covers the %s range): "
                         "the bound cannot be promised behind postprocess denoise.level=%s clip=%s" % (dtype.name, pp.denoise.level, list(pp.clip)))


def _load_corrections(cf, module_path, sideinfos):
    """None for an artefact without `error_bound` in its side info; else (idx, q, header) of its corrections file.  A decoder never
    hands back an unbounded volume silently: a missing or foreign file, or decode options the bound does not hold under, raise."""
    if "error_bound" not in sideinfos:
        return None
    check_error_bound(cf, sideinfos["dtype"])
    path = corrections.path_for(module_path)
    if not os.path.isfile(path):
        raise corrections.CorrectionsError("the side info promises error_bound=%s but %s is missing: refusing to decode an unbounded volume"
                                           % (sideinfos["error_bound"], path))
    idx, q, head = corrections.read(path)
    n = int(np.prod(sideinfos["data_shape"]))
    if head["bound"] != int(sideinfos["error_bound"]) or head["n"] != n or head["dtype"] != sideinfos["dtype"]:
        raise corrections.CorrectionsError("%s (bound %d, %d %s elements) does not belong to this artefact (error_bound %s, %d %s elements)"
                                           % (path, head["bound"], head["n"], head["dtype"], sideinfos["error_bound"], n, sideinfos["dtype"]))
    return idx, q, head


def _region_postprocess_check(dtype, pp):
    """a region equals the slice of the whole decode only where Decompress.postprocess is local to a voxel: the clip and a plain
    threshold are; a denoise through a binary opening (denoise.close) of a non-zero level is not.  (At level <= 0 the opening
    only zeroes voxels the clip, whose floor is >= 0, sends to the same value, so a threshold gives the same result.)"""
    from .io import range_limit
    if pp.denoise.level > 0 and pp.denoise.close is not False:
        raise ValueError("Decompress.postprocess.denoise (level %s through a binary opening) is not local to a voxel: a region "
                         "cannot equal the slice of the whole decode; decode the whole volume instead" % pp.denoise.level)
    range_limit(np.zeros(1, dtype), pp.clip)      # the clip's own checks, before any decode


# ---- one stored net ------------------------------------------------------------------------------------------------------------
class Artefact:
    """One stored net (a SingleTask artefact, or one block of a DivideTask one) as its decoders see it.  Plain attributes, all set
    by open_artefact from the options and the side info alone: nothing under `module_path` is touched before load_phi / corrections.

    cf            a private copy of the CompressFramework options, Module.phi patched to the stored net (features, name)
    side, module_path
    data_shape, dims, cout, dtype      the stored grid [*dims, cout] and the source dtype's name
    precision, phi_name, phi_features  the arithmetic and the net the weights were fitted in
    lo, hi        the coordinate range of Compress.coords_mode
    norm_range    (a, b) of Normalize 'minmaxany_a_b', else None;  vrange: (min, max) of the source data
    integer       uint8 / uint16 data under 'minmaxany_a_b': the fused integer epilogue decodes it (decompress's fused branch)
    out_kind      'u8' | 'u16' where `integer`, else None
    postprocess   Decompress.postprocess"""

    def __init__(self, cf, side, module_path, default_precision=None, default_name=None):
        from .io import minmaxany_range
        self.cf, self.side, self.module_path = cf, side, module_path
        self.data_shape = [int(v) for v in side["data_shape"]]
        self.dims, self.cout = self.data_shape[:-1], self.data_shape[-1]
        self.dtype = side["dtype"]
        self.phi_features = side["phi_features"]
        self.phi_name = side["phi_name"] if default_name is None else side.get("phi_name", default_name)
        # the arithmetic the net was fitted in: the side info records it when it is not fp32
        self.precision = str(side.get("phi_precision", default_precision or cf.Compress.get("precision", "fp32")))
        cf.Module.phi.features, cf.Module.phi.name = self.phi_features, self.phi_name
        self.lo, self.hi = _coords_range(cf.Compress.coords_mode)
        self.norm_range = minmaxany_range(cf.Normalize.name)
        self.vrange = (side["min"], side["max"])
        self.integer = self.norm_range is not None and self.dtype in ("uint8", "uint16")
        self.out_kind = ("u8" if self.dtype == "uint8" else "u16") if self.integer else None
        self.postprocess = cf.Decompress.postprocess

    def __eq__(self, other):
        return isinstance(other, Artefact) and vars(self) == vars(other)

    def load_phi(self, device):
        """the stored net on `device`, in the precision it was fitted in: the one place a decoder builds its net"""
        from .modelsave import load_model
        from .networks import init_phi
        phi = init_phi({**dict(self.cf.Module.phi), "precision": self.precision})
        load_model(phi, self.module_path, "cpu")
        phi.to(device)
        return phi

    def corrections(self):
        """None, or (idx, q, header) of the corrections file an error-bounded artefact promises (raises where it cannot be honoured)"""
        return _load_corrections(self.cf, self.module_path, self.side)

    def postprocess_local(self, data):
        """the part of Decompress.postprocess that is local to a voxel (threshold, clip), what regions and images get; the binary
        opening is refused beforehand by _region_postprocess_check"""
        from .misc import preprocess
        return preprocess(data, self.postprocess.denoise.level, False, self.postprocess.clip)


def open_artefact(opt, module_path, sideinfos, *, default_precision=None, default_name=None):
    """The Artefact of one stored net.  opt: the whole option tree, its path, or the CompressFramework tree alone (what NFGR
    holds); sideinfos: the side-info dict or its path.  The caller's trees are not modified.  Reads the two YAML files at most.
    default_precision / default_name: what to assume where the side info does not say (`phi_precision` / `phi_name`); without
    them the precision falls back to Compress.precision, then fp32, and a missing `phi_name` is a KeyError."""
    from .io import load_yaml
    if isinstance(opt, str):
        opt = config.load(opt)
    if isinstance(sideinfos, str):
        sideinfos = load_yaml(sideinfos)
    cf = opt.CompressFramework if "CompressFramework" in opt else opt      # the one place the two forms of `opt` are told apart
    return Artefact(copy.deepcopy(cf), sideinfos, module_path, default_precision, default_name)


def view_dims(dims, shape):
    """the grid a decode evaluates: the fitted `dims`, or with `shape` the resampled view of that spatial shape (one length >= 1 per axis)"""
    if shape is None:
        return dims
    shape = [int(v) for v in shape]
    if len(shape) != len(dims) or any(v < 1 for v in shape):
        raise ValueError("shape %s does not fit the %d spatial axes of the artefact" % (shape, len(dims)))
    return shape


def check_envelope(art, *, no_error_bound=None, need_3d=None, need_integer=None, need_minmaxany=None, local_postprocess=False, min_axis=None):
    """What a decode mode supports, refused on options and side info before any decode, in this order.  A condition is checked where
    its argument is given; the argument is the mode's own wording of the refusal (a % template), so each mode keeps its text.
    no_error_bound (error_bound, dims): no stored corrections;  need_3d (axes, data_shape): 3-D data;  need_integer (dtype): uint8 /
    uint16 data;  need_minmaxany (Normalize.name): a 'minmaxany_a_b' normalisation;  local_postprocess: a Decompress.postprocess
    local to a voxel (_region_postprocess_check's text);  min_axis (n, template of dims): every spatial axis at least n long."""
    if no_error_bound is not None and "error_bound" in art.side:
        raise ValueError(no_error_bound % (art.side["error_bound"], art.dims))
    if need_3d is not None and len(art.data_shape) != 4:
        raise ValueError(need_3d % (len(art.dims), art.data_shape))
    if need_integer is not None and art.dtype not in ("uint8", "uint16"):
        raise ValueError(need_integer % art.dtype)
    if need_minmaxany is not None and art.norm_range is None:
        raise ValueError(need_minmaxany % art.cf.Normalize.name)
    if local_postprocess:
        _region_postprocess_check(np.dtype(art.dtype), art.postprocess)
    if min_axis is not None and any(n < min_axis[0] for n in art.dims):
        raise ValueError(min_axis[1] % (art.dims,))


# ---- the blocks of a DivideTask artefact ---------------------------------------------------------------------------------------
Block = collections.namedtuple("Block", "name side ranges module_path")      # ranges: parse_chunk_name's inclusive index ranges per axis letter


def block_paths(module_dir, sideinfos_dir, name):
    """(module path, side-info path) of the block `name` in the tree compress_divide writes"""
    return os.path.join(module_dir, name, "module"), os.path.join(sideinfos_dir, name, "sideinfos.yaml")


def divide_blocks(orig_sideinfos, module_dir, sideinfos_dir, one_dtype=None):
    """(data_shape of the whole volume, its blocks in sorted-name order) of a stored DivideTask artefact; orig_sideinfos: the job's
    side info (dict or path).  one_dtype: the decode's name where it needs one dtype for all blocks (refused otherwise)."""
    from .io import load_yaml
    from .misc import parse_chunk_name
    orig = load_yaml(orig_sideinfos) if isinstance(orig_sideinfos, str) else orig_sideinfos
    names = sorted(os.listdir(module_dir))
    if not names:
        raise ValueError("no blocks under %s" % module_dir)
    blocks = []
    for name in names:
        module_path, side_path = block_paths(module_dir, sideinfos_dir, name)
        blocks.append(Block(name, load_yaml(side_path), parse_chunk_name(name), module_path))
        first, side = blocks[0], blocks[-1].side
        if one_dtype is not None and side["dtype"] != first.side["dtype"]:
            raise ValueError("%s needs one dtype for all blocks (%s is %s, %s is %s)" % (one_dtype, first.name, first.side["dtype"], name, side["dtype"]))
    return [int(v) for v in orig["data_shape"]], blocks


def _axes(nd):
    return "dhw" if nd == 3 else "hw"


def _ranges_overlap(a, b, axes):
    return all(a[k][0] <= b[k][1] and b[k][0] <= a[k][1] for k in axes)


def first_overlap(blocks, axes):
    """the first pair of blocks (in order) whose inclusive ranges share a voxel on every axis of `axes` ('dhw' | 'hw'), or None"""
    for i, a in enumerate(blocks):
        for b in blocks[i + 1:]:
            if _ranges_overlap(a.ranges, b.ranges, axes):
                return a, b
    return None


def meeting(blocks, start, step, extent):
    """(block, out_lo, out_hi, local_start, local_stop) for every block the strided region (start, step, extent) meets:
    region.block_intersection's result per block, the blocks that miss the region left out"""
    axes = _axes(len(start))
    for b in blocks:
        hit = region_mod.block_intersection(start, step, extent, [b.ranges[a][0] for a in axes], [b.ranges[a][1] for a in axes])
        if hit is not None:
            yield (b, *hit)
