"""Max-intensity projections straight from a stored artefact: the three images misc.mip_ops takes from a decoded volume, without ever
holding that volume.  A region is decoded chunk by chunk on the device (decode_box into one reused buffer, the stored corrections of
an error-bounded artefact added back), each chunk is folded into three small images by brief_mip_accumulate (csrc/brief_mip.inc) and
forgotten.  (DESIGN.md "Projection decode".)

plan_chunks is host arithmetic; everything else needs a ROCm GPU (there is no CPU fallback)."""
import numpy as np

from . import _lib, artefact, config, corrections
from . import region as region_mod

DEFAULT_CHUNK = 1 << 24          # voxels decoded per step: 32 MiB of uint16, against 2 GiB for a whole 1024^3 volume
SHAPE_REFUSAL = ("max-intensity projections of a resampled view (shape) are refused: the projection decode runs on the fitted grid only; "
                 "decode the view with decompress_region and take mip_ops of it")


def plan_chunks(extent, limit):
    """the sub-boxes (lo, hi), hi exclusive, that tile the box of shape `extent` exactly, in z-major order, each of at most `limit`
    voxels: runs of whole z-slices where a slice fits, else runs of whole rows of one slice, else pieces of one row."""
    ext = [int(v) for v in extent]
    limit = int(limit)
    if len(ext) != 3 or any(v < 1 for v in ext):
        raise ValueError("plan_chunks needs a 3-D extent with every axis >= 1 (got %r)" % (extent,))
    if limit < 1:
        raise ValueError("plan_chunks needs a limit of at least one voxel (got %r)" % (limit,))
    e0, e1, e2 = ext
    if e1 * e2 <= limit:
        nz = limit // (e1 * e2)
        return [((z, 0, 0), (min(z + nz, e0), e1, e2)) for z in range(0, e0, nz)]
    if e2 <= limit:
        ny = limit // e2
        return [((z, y, 0), (z + 1, min(y + ny, e1), e2)) for z in range(e0) for y in range(0, e1, ny)]
    return [((z, y, x), (z + 1, y + 1, min(x + limit, e2))) for z in range(e0) for y in range(e1) for x in range(0, e2, limit)]


def accumulate(box, images, origin=(0, 0, 0)):
    """fold the dense device tensor box [e0, e1, e2, C] (uint8 | uint16) into images = (mip_d [I1, I2, C], mip_h [I0, I2, C],
    mip_w [I0, I1, C]) by elementwise max, the box sitting at `origin` of the frame the images span (brief_mip_accumulate)"""
    import ctypes as C
    import torch
    mip_d, mip_h, mip_w = images
    if box.dim() != 4 or not box.is_contiguous() or box.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("mip.accumulate needs a contiguous uint8 / uint16 tensor [e0, e1, e2, channels]")
    ch = box.shape[3]
    frame = (mip_h.shape[0], mip_d.shape[0], mip_d.shape[1])
    want = ((frame[1], frame[2], ch), (frame[0], frame[2], ch), (frame[0], frame[1], ch))
    for img, shape in zip(images, want):
        if tuple(img.shape) != shape or img.dtype != box.dtype or not img.is_contiguous() or img.device != box.device:
            raise ValueError("mip.accumulate: the images must be contiguous %s tensors of shapes %s on the box's device" % (box.dtype, want))
    if not box.is_cuda:
        raise _lib.BriefError("mip.accumulate runs on a ROCm GPU only; there is no CPU fallback")
    i3 = C.c_int64 * 3
    _lib.check(_lib.lib().brief_mip_accumulate(_lib.ptr(box), _lib.OUT_U8 if box.dtype == torch.uint8 else _lib.OUT_U16,
                                               i3(*[int(v) for v in box.shape[:3]]), int(ch), _lib.ptr(mip_d), _lib.ptr(mip_h), _lib.ptr(mip_w),
                                               i3(*[int(v) for v in origin]), i3(*[int(v) for v in frame]), _lib.stream_ptr()))
    return images


def decode_mips(phi, dims, start, stop, step, lo, hi, out_kind, scale, vrange, corr=None, data_shape=None, chunk=None, into=None, origin=None):
    """the three projections of the box start:stop:step (lists, one entry per axis, as region.normalize_region returns them) of the
    net `phi` on the linspace grid `dims`: equal to mip_ops of decode_box over the same box, but decoded in sub-boxes of at most
    `chunk` voxels (plan_chunks; default DEFAULT_CHUNK) into one reused device buffer, each folded into the images and dropped.
    out_kind 'u8' | 'u16' with scale / vrange: the fused integer epilogue of decode_box.  corr = (idx, q, header) of the artefact's
    corrections file (flat indices into data_shape = dims + [channels]): those that fall on a sub-box are added to it before the
    fold (corrections.select / apply, as decompress_region does).  Returns device tensors (mip_d, mip_h, mip_w) of the box's
    shape; with `into` = three images of a larger frame the box is folded into them at `origin` instead (and they are returned)."""
    import torch
    if out_kind not in ("u8", "u16"):
        raise ValueError("decode_mips folds the integer decode only: out_kind must be 'u8' or 'u16' (got %r)" % (out_kind,))
    dims = [int(v) for v in dims]
    if len(dims) != 3:
        raise ValueError("max-intensity projections are defined for 3-D data only (got a %d-D grid)" % len(dims))
    start, stop, step = region_mod.normalize_region(dims, tuple(slice(b, e) for b, e in zip(start, stop)), step)
    ext = region_mod.extents(start, stop, step)
    ch = int(phi.data_channel)
    dt = torch.uint8 if out_kind == "u8" else torch.uint16
    dev = phi.params.device
    if into is None:
        into = (torch.zeros((ext[1], ext[2], ch), dtype=dt, device=dev), torch.zeros((ext[0], ext[2], ch), dtype=dt, device=dev),
                torch.zeros((ext[0], ext[1], ch), dtype=dt, device=dev))
        origin = (0, 0, 0)
    elif origin is None:
        origin = (0, 0, 0)
    data_shape = [int(v) for v in (data_shape if data_shape is not None else dims + [ch])]
    chunk = int(chunk or DEFAULT_CHUNK)
    pieces = plan_chunks(ext, chunk)
    buf = torch.empty(max(int(np.prod([h - l for l, h in zip(*p)])) for p in pieces) * ch, dtype=dt, device=dev)
    for p_lo, p_hi in pieces:
        sub = [h - l for l, h in zip(p_lo, p_hi)]
        s_start = [b + s * l for b, s, l in zip(start, step, p_lo)]
        s_stop = [b + s * (h - 1) + 1 for b, s, h in zip(start, step, p_hi)]
        box = buf[:int(np.prod(sub)) * ch].view(*sub, ch)
        phi.decode_box(dims, s_start, s_stop, step, lo, hi, out_kind=out_kind, scale=scale, vrange=vrange, out=box)
        if corr is not None:
            bi, bq = corrections.select(corr[0], corr[1], data_shape, s_start + [0], s_stop + [ch], step + [1])
            corrections.apply(box, bi, bq, corr[2]["bound"])
        accumulate(box, into, [o + l for o, l in zip(origin, p_lo)])
    return into


# ---- artefacts ------------------------------------------------------------------------------------------------------------------
ENVELOPE = dict(
    need_3d="max-intensity projections are defined for 3-D data only (mip_ops needs ndim == 4): this artefact holds %d-D data of shape %s",
    need_integer="the projection decode supports uint8 / uint16 data only (the fused integer decode); this artefact holds %s: "
                 "decode it and take mip_ops",
    need_minmaxany="the projection decode supports the 'minmaxany_a_b' normalisations only (the fused integer decode), not "
                   "Normalize.name=%s: decode the volume and take mip_ops",
    local_postprocess=True)


def check_envelope(art, shape=None):
    """what the projection decode supports, checked on the opened artefact before any decode: 3-D uint8 / uint16 data under a
    'minmaxany_a_b' normalisation (the fused integer epilogue), a Decompress.postprocess that is local to a voxel, the fitted grid"""
    if shape is not None:
        raise ValueError(SHAPE_REFUSAL)
    artefact.check_envelope(art, **ENVELOPE)


def _load_phi(cf, module_path, sideinfos, device):
    """the stored net on `device` (artefact.Artefact.load_phi); the name the GPU tests load an artefact's net by.  No module of the
    package uses it."""
    return artefact.open_artefact(cf, module_path, sideinfos).load_phi(device)


def _fold_artefact(art, start, stop, step, device, chunk, into=None, origin=None):
    """decode_mips of one stored net (a SingleTask artefact, or one block of a partition)"""
    corr = art.corrections()         # raises when a promised bound cannot be honoured
    phi = art.load_phi(device)
    return decode_mips(phi, art.dims, start, stop, step, art.lo, art.hi, art.out_kind, art.norm_range, art.vrange, corr=corr,
                       data_shape=art.data_shape, chunk=chunk, into=into, origin=origin)


def decompress_mip(opt, module_path, sideinfos, region=None, step=1, device="cuda", shape=None, chunk=None):
    """mip_ops(NFGR.decompress_region(opt, module_path, sideinfos, region, step)) bit for bit, as numpy (mip_d, mip_h, mip_w) in the
    source dtype, without the volume: the region (None: the whole grid) is decoded in chunks that are folded on the device.
    Decompress.postprocess is applied to the three IMAGES, not to the voxels: on unsigned data the threshold (x <= level -> 0) and
    the clip are monotone non-decreasing maps, and a monotone map commutes with max, so the result is the same.  Supported: 3-D
    uint8 / uint16 data under 'minmaxany_a_b'; 2-D data, other dtypes or normalisations, a denoise through a binary opening and a
    resampled view (shape) are refused before any decode.  Error-bounded artefacts get their corrections per chunk."""
    art = artefact.open_artefact(opt, module_path, sideinfos)
    check_envelope(art, shape)
    start, stop, stp = region_mod.normalize_region(art.dims, region if region is not None else (slice(None),) * 3, step)
    images = _fold_artefact(art, start, stop, stp, device, chunk)
    return tuple(art.postprocess_local(img.cpu().numpy()) for img in images)


def decompress_divide_mip(opt, orig_sideinfos, module_dir, sideinfos_dir, region=None, step=1, device="cuda", shape=None, chunk=None):
    """mip_ops(decompress_divide_region(opt, ..., region, step)) bit for bit for a stored DivideTask artefact: only the blocks that
    meet the region are decoded, each folded straight into the three full images at its output offset.  Voxels no block covers count
    as 0, as in merge_divided_data; a ray no block meets at all is 0 in its image.  Decompress.postprocess acts on the images (see
    decompress_mip).  Blocks whose ranges overlap are refused: merge_divided_data ADDS there, and a max of sums is not a sum of
    maxima."""
    import torch
    if isinstance(opt, str):
        opt = config.load(opt)
    if shape is not None:
        raise ValueError(SHAPE_REFUSAL)
    data_shape, blocks = artefact.divide_blocks(orig_sideinfos, module_dir, sideinfos_dir, one_dtype="the projection decode")
    if len(data_shape) != 4:
        raise ValueError(ENVELOPE["need_3d"] % (len(data_shape) - 1, data_shape))
    start, stop, stp = region_mod.normalize_region(data_shape[:-1], region if region is not None else (slice(None),) * 3, step)
    ext = region_mod.extents(start, stop, stp)
    # every refusal before any decode
    arts = {b.name: artefact.open_artefact(opt, b.module_path, b.side) for b in blocks}
    for art in arts.values():
        check_envelope(art)
    pair = artefact.first_overlap(blocks, "dhw")
    if pair is not None:
        raise ValueError("the blocks %s and %s overlap: merge_divided_data adds overlapping blocks, and a max-intensity projection "
                         "of a sum is not the max of the blocks' projections; decode the region and take mip_ops" % (pair[0].name, pair[1].name))
    first, cout = arts[blocks[0].name], data_shape[-1]
    dt = torch.uint8 if first.dtype == "uint8" else torch.uint16
    images = (torch.zeros((ext[1], ext[2], cout), dtype=dt, device=device), torch.zeros((ext[0], ext[2], cout), dtype=dt, device=device),
              torch.zeros((ext[0], ext[1], cout), dtype=dt, device=device))
    covered = (np.zeros((ext[1], ext[2]), bool), np.zeros((ext[0], ext[2]), bool), np.zeros((ext[0], ext[1]), bool))
    for b, o_lo, o_hi, l_start, l_stop in artefact.meeting(blocks, start, stp, ext):
        _fold_artefact(arts[b.name], l_start, l_stop, stp, device, chunk, into=images, origin=o_lo)
        z, y, x = (slice(lo, hi) for lo, hi in zip(o_lo, o_hi))
        covered[0][y, x] = True
        covered[1][z, x] = True
        covered[2][z, y] = True
    out = []
    for img, cov in zip(images, covered):
        a = np.array(first.postprocess_local(img.cpu().numpy()), copy=True)
        a[~cov] = 0                                              # (the postprocess of a ray of uncovered zeros is never applied: they stay 0)
        out.append(a)
    return tuple(out)
