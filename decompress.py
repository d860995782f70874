#!/usr/bin/env python3
"""Decode a region of a stored BRIEF artefact without decoding the whole volume:

    python decompress.py -p <run yaml> -c <outputs/.../steps{k}/compressed> --region z0:z1,y0:y1,x0:x1 [--step s] [--shape D,H,W] -o roi.tif|roi.npy

The artefact kind is read from the directory: a `sideinfos/` directory of blocks is a DivideTask artefact, a single
`sideinfos.yaml` beside `module` a SingleTask one.  2-D data takes `--region y0:y1,x0:x1`.  A part of the region may be
`a:b`, `a:`, `:b`, `:` or `a:b:s` (numpy slice semantics; out-of-range bounds are refused, not clipped).  `--shape`
(SingleTask only) evaluates the net on a linspace grid of that spatial shape, and the region indexes that grid.

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --mip -o out.tif

`--mip` writes the three max-intensity projections of the region (out_mip_d.tif, out_mip_h.tif, out_mip_w.tif) instead of the
region itself: it is decoded chunk by chunk on the GPU and folded into the three images, the volume is never held (3-D uint8 /
uint16 artefacts; not with `--shape`).

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --gradient components -o grad.npy

`--gradient components` writes the analytic spatial gradient of the stored net over the region, float32 [*extent, channels, axes] in
grey levels per voxel step; `--gradient magnitude` writes its Euclidean norm over the axes, float32 [*extent, channels] (fp32 SIREN
artefacts up to 1024 features under a `minmaxany_a_b` normalisation; `.npy` output only; not with `--mip`; `--shape` on SingleTask only).

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --hessian components|laplacian|eigenvalues|vesselness -o hess.npy

`--hessian components` writes the analytic Hessian of the stored net over the region, float32 [*extent, channels, 6] in the order
(zz, zy, zx, yy, yx, xx) ([..., 3] = (yy, yx, xx) for 2-D data), in grey levels per voxel step squared; `laplacian` its trace
[*extent, channels], `eigenvalues` its eigenvalues by increasing absolute value [*extent, channels, axes], `vesselness` Frangi's
single-scale measure [*extent, channels] (the envelope of `--gradient`; `.npy` output only; not with `--mip`, `--gradient`, `--view` or
`--view-surface`; `--step` keeps the unit, `--shape` (SingleTask only) uses the resampled grid's spacing).

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --view dz,dy,dx [--view-up uz,uy,ux]
        [--view-mode max|min|mean|slice] [--view-spacing s] [--view-depth-spacing t] [--view-size R,C] [--view-offset t]
        [--voxel-size sz,sy,sx] -o out.tif|out.npy|out.png

`--view` writes ONE image: the orthographic view of the artefact along the direction (dz, dy, dx), with `--region` as the clip box.
`max` (default), `min` and `mean` fold every ray over the clip box (a rotating-MIP frame, a thick-slab mean); `slice` is the plane
through the volume's centre, `--view-offset` voxels along the direction, at any orientation (an oblique reslice).  Only samples inside
the clip box are evaluated; the volume is never decoded (SingleTask 3-D uint8 / uint16 artefacts; `mean` writes float32 `.npy` only;
not with `--mip`, `--gradient`, `--shape` or a `--step` other than 1).

    python decompress.py -p <run yaml> -c <.../compressed of a DivideTask job> --region :,:,: --view dz,dy,dx --view-owner nearest ... -o out.tif

A DivideTask artefact has one net per block, so a sample between two blocks needs an owner: `--view-owner nearest` names the rule (the
block whose cell, half a voxel around its index range, holds the sample evaluates it; nothing is blended across a face).  The view is
a view of the whole volume.  Without the option a DivideTask artefact is refused; the option on a SingleTask artefact, without
`--view`, or with `--view-surface` but without `--view-surface-gap` is refused by name.

    python decompress.py -p <run yaml> -c <.../compressed of a DivideTask job> --region :,:,: --view dz,dy,dx --view-owner nearest
        --view-surface LEVEL --view-surface-gap empty [--view-surface-side ...] [--view-refine N] ... -o out.png|out.tif|out.npy

`--view-surface LEVEL --view-surface-gap empty` with `--view-owner nearest` renders the isosurface of a DivideTask artefact: the march is
the view's, and every point of the bisection, and the hit itself, is routed to the block whose cell holds it, so a bracket may straddle a
face; the normal is the owning block's.  `--view-surface-gap empty` names what a point no block owns holds: nothing, it fails the level
test on either side.  The outputs are those of `--view-surface` below.  The option without `--view-surface`, on a SingleTask artefact or
with another value is refused by name.

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --view dz,dy,dx --view-surface LEVEL
        [--view-surface-side above|below] [--view-refine N] [--view-channel C] [--view-light lz,ly,lx] -o out.png|out.tif|out.npy

`--view-surface LEVEL` renders an ISOSURFACE instead of a projection: per ray the first sample at which channel C of the integer decode
is >= LEVEL (`above`, default) or <= LEVEL (`below`), refined by N rounds of bisection (default 8, 0 .. 16), and Lambert-shaded with the
stored net's own analytic normal, lit along `--view-light` (default: the view direction, a headlight).  LEVEL is a grey level of the
integer decode, before `Decompress.postprocess`.  `.png` / `.tif` hold the shaded image as uint8, floor(255 * shade + 0.5); `.npy` holds
float32 [rows, cols, 5] = depth, normal (z, y, x), shade, with NaN depth where no ray hits.  Artefacts other than an fp32 SIREN up to
1024 features have no analytic normal: `.npy` then holds the depth alone, [rows, cols], and an image output is refused by name (the
view options that shape the geometry apply; not with `--view-mode` or `--view-offset`).

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --view dz,dy,dx --view-composite 'L:r,g,b,a;L:r,g,b,a;...'|@file
        [--view-composite-channel C] [--view-background r,g,b] [--view-composite-bits B]
        [--view-composite-shade KA,KD [--view-composite-light lz,ly,lx]] -o out.png|out.npy

`--view-composite SPEC` renders the view through a TRANSFER FUNCTION instead: every sample of a ray is classified by channel C of the
integer decode (control points `level:r,g,b,a`, levels strictly ascending and before `Decompress.postprocess`, colours 0 .. 255, `a` the
opacity over one voxel of depth; linear between the points, constant outside) and composited front to back over `--view-background`,
in integers: the image does not depend on the chunking or the run.  `.png` holds R,G,B, `.npy` uint8 [rows, cols, 4] = R,G,B,A
(artefacts with an identity postprocess; the view options that shape the geometry apply; not with `--view-mode`,
`--view-offset`, `--view-surface...`, `--mip`, `--gradient`, `--hessian`, `--shape` or `--step`).
`--view-composite-shade KA,KD` lights every sample's emission by the stored net's own analytic gradient: the emission is scaled by
KA + KD * |n . l| (KA, KD in [0, 1]; two-sided, a density has no outside), n the direction of the physical gradient (`--voxel-size`)
and l the physical direction `--view-composite-light` travels (default: the view direction, a headlight).  Opacity and the A channel
do not change, and the gradient is evaluated only at samples that emit and are not hidden.  fp32 SIREN artefacts up to 1024 features
(quantised ones included); a DivideTask artefact with `--view-composite-shade` is refused (a follow-up).

    python decompress.py -p <run yaml> -c <.../compressed of a DivideTask job> --region :,:,: --view dz,dy,dx --view-composite SPEC --view-owner nearest ... -o out.png|out.npy

`--view-composite SPEC --view-owner nearest` renders the composite of a DivideTask artefact: the nearest block owns a sample, as for
`--view`, and the optical depth in front of a sample is carried across the blocks of its ray, so the image is the composite of the
whole volume's samples in depth order, bit for bit independent of the order of the blocks.  Blocks behind something partly opaque are
evaluated a second time.  Without `--view-owner` a DivideTask artefact is refused; `--view-owner` on a SingleTask artefact is refused.

    python decompress.py -p <run yaml> -c <.../compressed> --region :,:,: --view dz,dy,dx --view-eye z,y,x [--view-fov DEG] [--view-near T]
        [--view-far T] [--view-size R,C] [--view-depth-spacing S] [--view-up uz,uy,ux] [--voxel-size sz,sy,sx]
        [--view-mode max|min|mean | --view-surface LEVEL ...] -o out.tif|out.png|out.npy

`--view-eye z,y,x` turns the view into a PERSPECTIVE CAMERA at that voxel-index position, looking along `--view`; the eye may lie inside
the volume (a fly-through); a position whose first number is negative is attached with `=`, `--view-eye=-20,4,52`.  `--view-fov` is the full opening angle over the rows in degrees (default 60), `--view-size` the image
(default 256,256), and every ray is sampled at the distances `--view-near` + k * `--view-depth-spacing` from the eye up to `--view-far`
(default: the clip box's farthest corner).  `--view-mode max|min|mean` writes a projection, `--view-surface LEVEL` the isosurface with a
point light at the eye (or along `--view-light`); the outputs are those of the orthographic forms, and the `.npy` of a surface holds the
DISTANCE of the hit from the eye in the depth slot.  SingleTask artefacts; refused by name: a DivideTask or an error-bounded artefact,
`--view-eye` without `--view`, `--view-fov` / `--view-near` / `--view-far` without `--view-eye`, and `--view-eye` with `--view-spacing`,
`--view-offset`, `--view-mode slice`, `--view-composite...`, `--view-owner`, `--mip`, `--gradient`, `--hessian`, `--shape` or `--step`.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _paths(c):
    """(module, sideinfos.yaml, sideinfos) under the artefact directory `c`.  SingleTask: the net and its side info, no `sideinfos`
    directory.  DivideTask: the job's side info is sideinfos.yaml, the blocks are listed under module/ and sideinfos/"""
    return os.path.join(c, "module"), os.path.join(c, "sideinfos.yaml"), os.path.join(c, "sideinfos")


def main(argv=None):
    ap = argparse.ArgumentParser(description="decode a region of a BRIEF artefact (MI355X fused path)")
    ap.add_argument("-p", required=True, help="the run's yaml file")
    ap.add_argument("-c", required=True, help="the artefact directory: outputs/.../steps{k}/compressed")
    ap.add_argument("--region", required=True, help="z0:z1,y0:y1,x0:x1 (3-D) or y0:y1,x0:x1 (2-D)")
    ap.add_argument("--step", type=int, default=1, help="stride of every axis whose part has none (default 1)")
    ap.add_argument("--shape", default=None, help="D,H,W: decode a resampled view on a grid of this shape (SingleTask)")
    ap.add_argument("--mip", action="store_true", help="write the region's three max-intensity projections <out>_mip_{d,h,w}<ext> instead of the region")
    ap.add_argument("--gradient", default=None, metavar="{components,magnitude}",
                    help="write the region's analytic spatial gradient (grey levels per voxel step) or its magnitude instead of the region (.npy)")
    ap.add_argument("--hessian", default=None, metavar="{components,laplacian,eigenvalues,vesselness}",
                    help="write the region's analytic Hessian (grey levels per voxel step squared) or a map derived from it instead of the region (.npy)")
    ap.add_argument("--view", default=None, metavar="dz,dy,dx", help="write the orthographic view along this direction instead of the region (--region is the clip box)")
    ap.add_argument("--view-up", default=None, metavar="uz,uy,ux", help="the direction the image's rows run along (default: the grid axis the view direction has least of)")
    ap.add_argument("--view-mode", default="max", help="max | min | mean | slice (default max)")
    ap.add_argument("--view-spacing", type=float, default=1.0, help="distance between pixels, in voxels (default 1)")
    ap.add_argument("--view-depth-spacing", type=float, default=1.0, help="distance between the samples of a ray, in voxels (default 1)")
    ap.add_argument("--view-size", default=None, metavar="R,C", help="image size (default: the smallest image that covers the clip box)")
    ap.add_argument("--view-offset", type=float, default=None, help="slice: the plane's offset from the volume's centre along the direction (default 0)")
    ap.add_argument("--view-owner", default=None, metavar="{nearest}",
                    help="the rule that gives every sample of a --view (or of a --view --view-composite) of a DivideTask artefact its block: nearest (the block whose cell, half a voxel "
                         "around its index range, holds the sample); without it a DivideTask artefact is refused")
    ap.add_argument("--view-surface", type=int, default=None, metavar="LEVEL", help="render the isosurface of this grey level of the integer decode: first-hit depth and shaded normals")
    ap.add_argument("--view-surface-side", default=None, help="above (value >= LEVEL, default) | below (value <= LEVEL)")
    ap.add_argument("--view-refine", type=int, default=None, metavar="N", help="rounds of bisection of the hit, 0 .. 16 (default 8)")
    ap.add_argument("--view-channel", type=int, default=None, metavar="C", help="the channel the level is tested on (default 0)")
    ap.add_argument("--view-light", default=None, metavar="lz,ly,lx", help="the physical direction the light travels (default: the view direction)")
    ap.add_argument("--view-surface-gap", default=None, metavar="{empty}",
                    help="the rule that says what a point no block owns holds in the --view-surface of a DivideTask artefact (with --view-owner nearest): "
                         "empty (nothing: it fails the level test on either side); without it the isosurface of a DivideTask artefact is refused")
    ap.add_argument("--view-composite", default=None, metavar="SPEC",
                    help="render the view through a transfer function, level:r,g,b,a;level:r,g,b,a;... or @file: front-to-back emission-absorption compositing "
                         "(a DivideTask artefact with --view-owner nearest)")
    ap.add_argument("--view-composite-channel", type=int, default=None, metavar="C", help="the channel the transfer function classifies (default 0)")
    ap.add_argument("--view-background", default=None, metavar="r,g,b", help="the colour behind the composite, 0 .. 255 each (default 0,0,0)")
    ap.add_argument("--view-composite-bits", type=int, default=None, metavar="B", help="the transfer table has 2^B rows (default 8 for uint8, 12 for uint16)")
    ap.add_argument("--view-composite-shade", default=None, metavar="KA,KD",
                    help="light the composite by the net's analytic gradient: emission x (KA + KD |n . l|), the ambient and the diffuse weight each in [0, 1]")
    ap.add_argument("--view-composite-light", default=None, metavar="lz,ly,lx",
                    help="the physical direction the light of --view-composite-shade travels (default: the view direction)")
    ap.add_argument("--view-eye", default=None, metavar="z,y,x",
                    help="a perspective camera at this voxel-index position looking along --view (it may lie inside the volume): --view-mode max|min|mean or --view-surface")
    ap.add_argument("--view-fov", type=float, default=None, metavar="DEG", help="the camera's full opening angle over the rows, degrees (default 60)")
    ap.add_argument("--view-near", type=float, default=None, metavar="T", help="the distance from the eye of every ray's first sample (default 0)")
    ap.add_argument("--view-far", type=float, default=None, metavar="T", help="the distance from the eye of every ray's last sample (default: the clip box's farthest corner)")
    ap.add_argument("--voxel-size", default=None, metavar="sz,sy,sx", help="physical extent of a voxel per axis (default 1,1,1)")
    ap.add_argument("-o", required=True, help="output file (.tif / .tiff / .npy / .png / .jpg)")
    args = ap.parse_args(argv)
    if any(v is not None for v in (args.view_eye, args.view_fov, args.view_near, args.view_far)):
        _camera_refusals(args)        # every refusal by name, before the GPU path is imported
    if any(v is not None for v in (args.view_composite, args.view_composite_channel, args.view_background, args.view_composite_bits,
                                   args.view_composite_shade, args.view_composite_light)):
        _composite_refusals(args)     # every refusal by name, before the GPU path is imported
    if args.hessian is not None:
        why = "each writes a result of its own; ask for one of them"
        _derivative_refusals(args, "--hessian", args.hessian, ("components", "laplacian", "eigenvalues", "vesselness"), "Hessian",
                             (("--mip", args.mip, why), ("--gradient", args.gradient is not None, why),
                              ("--view-surface", args.view_surface is not None, why), ("--view", args.view is not None, why)))
    if args.view is not None:
        _view_refusals(args)          # every refusal by name, before the GPU path is imported
    elif args.view_owner is not None:
        raise SystemExit("--view-owner names the rule that gives the samples of a --view of a DivideTask artefact their blocks: give the "
                         "view's direction with --view dz,dy,dx")
    elif args.view_surface is not None or any(v is not None for v in (args.view_surface_side, args.view_refine, args.view_channel, args.view_light,
                                                                      args.view_surface_gap)):
        raise SystemExit("--view-surface / --view-surface-side / --view-surface-gap / --view-refine / --view-channel / --view-light describe the "
                         "isosurface of a --view: give its direction with --view dz,dy,dx")
    elif any(v is not None for v in (args.view_up, args.view_size, args.view_offset, args.voxel_size)) or args.view_mode != "max" \
            or args.view_spacing != 1.0 or args.view_depth_spacing != 1.0:
        raise SystemExit("--view-up / --view-mode / --view-spacing / --view-depth-spacing / --view-size / --view-offset / --voxel-size "
                         "describe a --view: give its direction with --view dz,dy,dx")
    if args.gradient is not None:
        _derivative_refusals(args, "--gradient", args.gradient, ("components", "magnitude"), "gradient",
                             (("--mip", args.mip, "a projection of a gradient is not defined here; ask for one of them"),))
    if args.mip and args.shape:
        from brief_pytorch_amd.mip import SHAPE_REFUSAL
        raise SystemExit("--mip --shape: " + SHAPE_REFUSAL)

    import torch
    from brief_pytorch_amd import config
    from brief_pytorch_amd.framework import NFGR, decompress_divide_region
    from brief_pytorch_amd.region import parse_region, parse_shape
    from brief_pytorch_amd.tool import save_img

    opt = config.load(args.p)
    region = parse_region(args.region)
    shape = parse_shape(args.shape) if args.shape else None
    module, side_path, blocks_dir = _paths(args.c)
    divide = os.path.isdir(blocks_dir)
    if args.view is not None:
        return _view(args, opt, region, divide)
    if args.mip:
        return _mip(args, opt, region, divide)
    if args.gradient is not None:
        from brief_pytorch_amd import gradient
        return _derivative(args, opt, region, shape, divide, "--gradient", args.gradient, "spatial gradient (%s, grey levels per voxel)",
                           gradient.decompress_gradient_device, gradient.decompress_divide_gradient_device,
                           gradient.magnitude if args.gradient == "magnitude" else None)
    if args.hessian is not None:
        import functools
        from brief_pytorch_amd import hessian
        return _derivative(args, opt, region, shape, divide, "--hessian", args.hessian, "Hessian (%s, grey levels per voxel squared)",
                           functools.partial(hessian.decompress_hessian_device, mode=args.hessian),
                           functools.partial(hessian.decompress_divide_hessian_device, mode=args.hessian))
    t0 = time.perf_counter()
    if divide:
        if shape is not None:
            raise SystemExit("--shape: resampling is not defined for a DivideTask artefact (every block has its own linspace grid)")
        data = decompress_divide_region(opt, side_path, module, blocks_dir, region, args.step)
    else:
        data = NFGR.decompress_region(opt, module, side_path, region, args.step, shape=shape)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    save_img(args.o, data)
    print("%s region %s: shape %s, dtype %s, decoded in %.3f s -> %s" % ("DivideTask" if divide else "SingleTask", args.region,
                                                                          tuple(data.shape), data.dtype, dt, args.o))
    return 0


def _mip(args, opt, region, divide):
    import torch
    from brief_pytorch_amd.framework import NFGR, decompress_divide_mip
    from brief_pytorch_amd.misc import save_mips
    module, side_path, blocks_dir = _paths(args.c)
    t0 = time.perf_counter()
    try:
        if divide:
            mips = decompress_divide_mip(opt, side_path, module, blocks_dir, region, args.step)
        else:
            mips = NFGR.decompress_mip(opt, module, side_path, region, args.step)
    except ValueError as e:                                       # a refusal (2-D data, dtype, normalisation, postprocess, region)
        raise SystemExit("--mip: %s" % e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stem, ext = os.path.splitext(os.path.basename(args.o))
    save_mips(mips, os.path.dirname(args.o) or ".", stem, ext)
    print("%s region %s: max-intensity projections d %s, h %s, w %s, dtype %s, decoded in %.3f s -> %s_mip_{d,h,w}%s" % (
        "DivideTask" if divide else "SingleTask", args.region, tuple(mips[0].shape), tuple(mips[1].shape), tuple(mips[2].shape), mips[0].dtype,
        dt, os.path.splitext(args.o)[0], ext))
    return 0


def _floats(text, n, what):
    try:
        out = [float(x) for x in text.split(",")]
    except ValueError:
        out = []
    if len(out) != n:
        raise SystemExit("%s %s: expected %d comma-separated numbers" % (what, text, n))
    return out


def _view_refusals(args):
    for flag, on in (("--mip", args.mip), ("--gradient", args.gradient is not None), ("--shape", args.shape is not None),
                     ("--step %d" % args.step, args.step != 1)):
        if on:
            raise SystemExit("--view with %s: a view is one image of the fitted grid along its own direction (its sampling is set by "
                             "--view-spacing and --view-depth-spacing); ask for one of them" % flag)
    from brief_pytorch_amd.view import DIVIDE_REFUSAL, GAPS, MODES, OWNERS
    if args.view_surface_gap is not None and args.view_surface is not None:
        if args.view_surface_gap not in GAPS:
            raise SystemExit("--view-surface-gap %s: unknown rule (%s)" % (args.view_surface_gap, ", ".join(GAPS)))
        if not os.path.isdir(_paths(args.c)[2]):
            raise SystemExit("--view-surface-gap %s: the rule says what a point between the blocks of a DivideTask artefact holds, and %s is a "
                             "SingleTask artefact (one net covers the volume); leave the option out" % (args.view_surface_gap, args.c))
    if args.view_surface is None:
        for flag, v in (("--view-surface-side", args.view_surface_side), ("--view-refine", args.view_refine), ("--view-channel", args.view_channel),
                        ("--view-light", args.view_light), ("--view-surface-gap", args.view_surface_gap)):
            if v is not None:
                raise SystemExit("%s describes an isosurface: give its level with --view-surface LEVEL" % flag)
    else:
        from brief_pytorch_amd.view import MAX_REFINE, SIDES
        if args.view_mode != "max":
            raise SystemExit("--view-surface with --view-mode %s: an isosurface is a view of its own (the first crossing of a level along "
                             "every ray); ask for one of them" % args.view_mode)
        if args.view_offset is not None:
            raise SystemExit("--view-surface with --view-offset: the offset names the plane of --view-mode slice")
        if args.view_surface_side is not None and args.view_surface_side not in SIDES:
            raise SystemExit("--view-surface-side %s: unknown side (%s)" % (args.view_surface_side, ", ".join(SIDES)))
        if args.view_refine is not None and not 0 <= args.view_refine <= MAX_REFINE:
            raise SystemExit("--view-refine %d: the rounds of bisection must be 0 .. %d" % (args.view_refine, MAX_REFINE))
        if args.view_channel is not None and args.view_channel < 0:
            raise SystemExit("--view-channel %d: a channel is 0 or above" % args.view_channel)
        if args.view_surface < 0 or args.view_surface > 65535:
            raise SystemExit("--view-surface %d: the level must be a grey level of the integer decode, 0 .. 65535" % args.view_surface)
        if args.view_light is not None:
            _floats(args.view_light, 3, "--view-light")
    if args.view_mode not in MODES:
        raise SystemExit("--view-mode %s: unknown mode (%s)" % (args.view_mode, ", ".join(MODES)))
    ext = os.path.splitext(args.o)[1].lower()
    if args.view_mode == "mean" and ext != ".npy":
        raise SystemExit("--view-mode mean writes a float32 image as .npy only (got %s): float output in image formats is not supported"
                         % (ext or "no extension"))
    if args.view_mode != "slice" and args.view_offset is not None:
        raise SystemExit("--view-offset names the plane of --view-mode slice (got --view-mode %s)" % args.view_mode)
    _floats(args.view, 3, "--view")
    if args.view_up is not None:
        _floats(args.view_up, 3, "--view-up")
    if args.voxel_size is not None:
        _floats(args.voxel_size, 3, "--voxel-size")
    if args.view_size is not None:
        _floats(args.view_size, 2, "--view-size")
    divide = os.path.isdir(_paths(args.c)[2])
    if args.view_owner is not None:
        if args.view_owner not in OWNERS:
            raise SystemExit("--view-owner %s: unknown rule (%s)" % (args.view_owner, ", ".join(OWNERS)))
        if args.view_surface is not None and args.view_surface_gap is None:
            raise SystemExit("--view-surface with --view-owner: the isosurface of a DivideTask artefact is refused unless its gap rule is named: "
                             "the refinement of a hit and its normal need per-point routing between blocks (a bracket can straddle a face, or "
                             "end in a gap no block covers); ask for --view-surface-gap empty (a point no block owns holds nothing)")
        if not divide:
            raise SystemExit("--view-owner %s: the rule chooses among the blocks of a DivideTask artefact, and %s is a SingleTask artefact (one "
                             "net owns every sample); leave the option out" % (args.view_owner, args.c))
    elif divide:
        raise SystemExit("--view: " + DIVIDE_REFUSAL)


def _camera_refusals(args):
    if args.view_eye is None:
        raise SystemExit("--view-fov / --view-near / --view-far describe the camera of a --view-eye: give the eye's position with --view-eye z,y,x")
    if args.view is None:
        raise SystemExit("--view-eye %s places a camera, and a camera looks along a direction: give it with --view dz,dy,dx" % args.view_eye)
    lattice = "a camera has no pixel lattice in the volume (its image is set by --view-fov and --view-size)"
    scope = "through a camera it is out of scope, a follow-up; ask for --view-mode max|min|mean or --view-surface LEVEL"
    each = "each writes a result of its own; ask for one of them"
    composite = any(v is not None for v in (args.view_composite, args.view_composite_channel, args.view_background, args.view_composite_bits,
                                            args.view_composite_shade, args.view_composite_light))
    for flag, on, why in (("--view-spacing", args.view_spacing != 1.0, lattice), ("--view-offset", args.view_offset is not None, lattice),
                          ("--view-mode slice", args.view_mode == "slice", "a slice is a plane of parallel rays; " + scope),
                          ("--view-composite", composite, "a composite is defined for the orthographic view; " + scope),
                          ("--view-owner", args.view_owner is not None, "a camera view of a partition is a follow-up"),
                          ("--mip", args.mip, each), ("--gradient", args.gradient is not None, each), ("--hessian", args.hessian is not None, each),
                          ("--shape", args.shape is not None, "a camera samples the fitted grid along its own rays"),
                          ("--step %d" % args.step, args.step != 1, "a camera samples the fitted grid along its own rays")):
        if on:
            raise SystemExit("--view-eye with %s: %s" % (flag, why))
    _floats(args.view_eye, 3, "--view-eye")
    if os.path.isdir(_paths(args.c)[2]):
        from brief_pytorch_amd.view import CAMERA_DIVIDE_REFUSAL
        raise SystemExit("--view-eye: " + CAMERA_DIVIDE_REFUSAL)


def _camera(args, opt, region):
    """--view dz,dy,dx --view-eye z,y,x: a projection (--view-mode max|min|mean) or the isosurface (--view-surface LEVEL) through a camera"""
    import numpy as np
    import torch
    from brief_pytorch_amd import gradient, view
    from brief_pytorch_amd.tool import save_img
    module, side_path, _ = _paths(args.c)
    npy = os.path.splitext(args.o)[1].lower() == ".npy"
    kw = dict(up=_floats(args.view_up, 3, "--view-up") if args.view_up is not None else None, region=region,
              fov=60.0 if args.view_fov is None else args.view_fov, near=0.0 if args.view_near is None else args.view_near, far=args.view_far,
              depth_spacing=args.view_depth_spacing,
              size=[int(x) for x in _floats(args.view_size, 2, "--view-size")] if args.view_size is not None else (256, 256),
              voxel_size=_floats(args.voxel_size, 3, "--voxel-size") if args.voxel_size is not None else (1, 1, 1))
    eye, direction = _floats(args.view_eye, 3, "--view-eye"), _floats(args.view, 3, "--view")
    t0 = time.perf_counter()
    try:
        art = view.open_single_camera(opt, module, side_path)
        if args.view_surface is None:
            data, hits, stats = view.decompress_camera(art, eye, direction, mode=args.view_mode, return_hits=True, **kw)
        else:
            why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
            if why is not None and not npy:
                raise ValueError("a shaded image needs the analytic Jacobian: %s; write the distance with -o <file>.npy" % why)
            res = view.decompress_camera_surface(
                art, eye, direction, args.view_surface, channel=args.view_channel or 0, side=args.view_surface_side or "above",
                refine=8 if args.view_refine is None else args.view_refine, shading=why is None,
                light=_floats(args.view_light, 3, "--view-light") if args.view_light is not None else None, **kw)
            stats = res["stats"]
    except ValueError as e:                                       # a refusal (artefact kind, dtype, normalisation, level, net, geometry, region)
        raise SystemExit("--view-eye: %s" % e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.view_surface is None:
        what = "view (%s)" % args.view_mode
    else:
        what = "surface view (level %d, %s: %d rays hit the surface, %d cut by the clip box, %d refinement points)" % (
            args.view_surface, args.view_surface_side or "above", stats["rays_surface"], stats["rays_cut"], stats["refine_points"])
        if not npy:
            data = np.floor(255.0 * res["shade"].astype(np.float64) + 0.5).astype(np.uint8)[..., None]
        elif res["shade"] is None:
            data = res["distance"]
        else:                                                     # (the orthographic layout, the distance from the eye in the depth slot)
            data = np.concatenate([res["distance"][..., None], res["normal"], res["shade"][..., None]], axis=-1).astype(np.float32)
    if npy:
        np.save(args.o, data)
    else:
        save_img(args.o, data)
    print("SingleTask camera %s at eye %s along %s of region %s: %s, dtype %s, %d of %d rays hit, %d samples evaluated, decoded in %.3f s -> %s" % (
        what, args.view_eye, args.view, args.region, tuple(data.shape), data.dtype, stats["rays_hit"], stats["rays"], stats["samples_evaluated"], dt, args.o))
    return 0


def _view(args, opt, region, divide):
    import numpy as np
    import torch
    from brief_pytorch_amd.framework import NFGR, decompress_divide_view
    from brief_pytorch_amd.tool import save_img
    if args.view_eye is not None:
        return _camera(args, opt, region)
    if args.view_surface is not None:
        return _surface(args, opt, region, divide)
    if args.view_composite is not None:
        return _composite(args, opt, region, divide)
    module, side_path, blocks_dir = _paths(args.c)
    t0 = time.perf_counter()
    kw = dict(up=_floats(args.view_up, 3, "--view-up") if args.view_up is not None else None, mode=args.view_mode, region=region,
              spacing=args.view_spacing, depth_spacing=args.view_depth_spacing,
              size=[int(x) for x in _floats(args.view_size, 2, "--view-size")] if args.view_size is not None else None,
              offset=args.view_offset, voxel_size=_floats(args.voxel_size, 3, "--voxel-size") if args.voxel_size is not None else (1, 1, 1),
              return_hits=True)
    try:
        if divide:                                                # (--view-owner nearest: _view_refusals refused everything else)
            img, hits, stats = decompress_divide_view(opt, side_path, module, blocks_dir, _floats(args.view, 3, "--view"), **kw)
        else:
            img, hits, stats = NFGR.decompress_view(opt, module, side_path, _floats(args.view, 3, "--view"), **kw)
    except ValueError as e:                                       # a refusal (artefact kind, dtype, normalisation, postprocess, geometry, region)
        raise SystemExit("--view: %s" % e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if os.path.splitext(args.o)[1].lower() == ".npy":
        np.save(args.o, img)
    else:
        save_img(args.o, img)
    print("%s view %s (%s) of region %s: image %s, dtype %s, %d of %d rays hit, %d samples evaluated, decoded in %.3f s -> %s" % (
        "DivideTask (%d of %d blocks hit, owner %s)" % (stats["blocks_hit"], stats["blocks"], args.view_owner) if divide else "SingleTask",
        args.view, args.view_mode, args.region, tuple(img.shape), img.dtype, stats["rays_hit"], stats["rays"], stats["samples_evaluated"], dt, args.o))
    return 0


def _surface(args, opt, region, divide):
    import numpy as np
    import torch
    from brief_pytorch_amd import artefact, gradient, view
    from brief_pytorch_amd.tool import save_img
    module, side_path, blocks_dir = _paths(args.c)
    npy = os.path.splitext(args.o)[1].lower() == ".npy"
    t0 = time.perf_counter()
    try:
        if divide:                                                # (--view-owner nearest --view-surface-gap empty: _view_refusals refused everything else)
            arts = [artefact.open_artefact(opt, b.module_path, b.side)      # (opening reads the side info only, no net)
                    for b in artefact.divide_blocks(side_path, module, blocks_dir, one_dtype="the view decode")[1]]
            why = next((w for w in (gradient.refusal(a.phi_name, a.precision, a.phi_features) for a in arts) if w is not None), None)
            render = lambda *a, **kw: view.decompress_divide_surface(opt, side_path, module, blocks_dir, *a, gap=args.view_surface_gap, **kw)
        else:
            art = view.open_single(opt, module, side_path)
            why = gradient.refusal(art.phi_name, art.precision, art.phi_features)
            render = lambda *a, **kw: view.decompress_surface(art, *a, **kw)
        if why is not None and not npy:
            raise ValueError("a shaded image needs the analytic Jacobian: %s; write the depth with -o <file>.npy" % why)
        res = render(
            _floats(args.view, 3, "--view"), args.view_surface,
            up=_floats(args.view_up, 3, "--view-up") if args.view_up is not None else None, region=region,
            spacing=args.view_spacing, depth_spacing=args.view_depth_spacing,
            size=[int(x) for x in _floats(args.view_size, 2, "--view-size")] if args.view_size is not None else None,
            voxel_size=_floats(args.voxel_size, 3, "--voxel-size") if args.voxel_size is not None else (1, 1, 1),
            channel=args.view_channel or 0, side=args.view_surface_side or "above", refine=8 if args.view_refine is None else args.view_refine,
            shading=why is None, light=_floats(args.view_light, 3, "--view-light") if args.view_light is not None else None)
    except ValueError as e:                                       # a refusal (artefact kind, dtype, normalisation, level, channel, net, geometry)
        raise SystemExit("--view-surface: %s" % e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not npy:
        data = np.floor(255.0 * res["shade"].astype(np.float64) + 0.5).astype(np.uint8)[..., None]
        save_img(args.o, data)
    elif res["shade"] is None:
        data = res["depth"]
        np.save(args.o, data)
    else:
        data = np.concatenate([res["depth"][..., None], res["normal"], res["shade"][..., None]], axis=-1).astype(np.float32)
        np.save(args.o, data)
    stats = res["stats"]
    print("%s surface view %s (level %d, %s) of region %s: %s %s, dtype %s, %d of %d rays hit the surface (%d cut by the clip box), "
          "%d samples evaluated, %d refinement points, decoded in %.3f s -> %s" % (
              "DivideTask (%d of %d blocks hit, owner %s, gap %s, %d brackets straddle a face)" % (
                  stats["blocks_hit"], stats["blocks"], args.view_owner, args.view_surface_gap, stats["rays_straddle"]) if divide else "SingleTask",
              args.view, args.view_surface, args.view_surface_side or "above", args.region, "image" if not npy else "array", tuple(data.shape),
              data.dtype, stats["rays_surface"], stats["rays"], stats["rays_cut"], stats["samples_evaluated"], stats["refine_points"], dt, args.o))
    return 0


def _composite_refusals(args):
    if args.view_composite is None:
        raise SystemExit("--view-composite-channel / --view-background / --view-composite-bits / --view-composite-shade / --view-composite-light "
                         "describe a composite: give its transfer function with --view-composite SPEC")
    if args.view is None:
        raise SystemExit("--view-composite renders a --view through a transfer function: give the view's direction with --view dz,dy,dx")
    from brief_pytorch_amd.view import OWNERS
    divide = os.path.isdir(_paths(args.c)[2])
    if args.view_owner is not None and divide and args.view_owner not in OWNERS:
        raise SystemExit("--view-owner %s: unknown rule (%s)" % (args.view_owner, ", ".join(OWNERS)))
    for flag, on in (("--view-mode %s" % args.view_mode, args.view_mode != "max"), ("--view-offset", args.view_offset is not None),
                     ("--view-surface", args.view_surface is not None), ("--view-surface-side", args.view_surface_side is not None),
                     ("--view-surface-gap", args.view_surface_gap is not None),
                     ("--view-refine", args.view_refine is not None), ("--view-channel", args.view_channel is not None),
                     ("--view-light", args.view_light is not None),
                     ("--view-owner", args.view_owner is not None and not (args.view_owner in OWNERS and divide)), ("--mip", args.mip),
                     ("--gradient", args.gradient is not None), ("--hessian", args.hessian is not None), ("--shape", args.shape is not None),
                     ("--step %d" % args.step, args.step != 1)):
        if on:
            raise SystemExit("--view-composite with %s: a composite is a view of its own (every sample of a ray, classified by the transfer "
                             "function and composited front to back; its channel is --view-composite-channel); ask for one of them" % flag)
    ext = os.path.splitext(args.o)[1].lower()
    if ext not in (".png", ".npy"):
        raise SystemExit("--view-composite writes an RGB image as .png or the RGBA array as .npy (got %s): the .tif writer holds one channel "
                         "per page, and no other format is supported" % (ext or "no extension"))
    from brief_pytorch_amd import composite
    from brief_pytorch_amd import view as view_mod
    try:
        composite.parse_transfer(args.view_composite)
        if args.view_background is not None:
            composite._background(_floats(args.view_background, 3, "--view-background"))
    except ValueError as e:
        raise SystemExit("--view-composite: %s" % e)
    if args.view_composite_channel is not None and args.view_composite_channel < 0:
        raise SystemExit("--view-composite-channel %d: a channel is 0 or above" % args.view_composite_channel)
    if args.view_composite_bits is not None and not 1 <= args.view_composite_bits <= 16:
        raise SystemExit("--view-composite-bits %d: the transfer table has 2^B rows, B 1 .. 8 for uint8 and 1 .. 16 for uint16" % args.view_composite_bits)
    if args.view_composite_light is not None and args.view_composite_shade is None:
        raise SystemExit("--view-composite-light names the direction the light of a shaded composite travels: give the weights of the shading "
                         "with --view-composite-shade KA,KD")
    if args.view_composite_shade is not None:
        try:
            composite.shade_quant(_floats(args.view_composite_shade, 2, "--view-composite-shade"))
            if args.view_composite_light is not None:
                view_mod._unit3(_floats(args.view_composite_light, 3, "--view-composite-light"), "--view-composite-light")
        except ValueError as e:
            raise SystemExit("--view-composite-shade: %s" % e)
    if divide and args.view_owner is None:
        raise SystemExit("--view-composite: " + composite.DIVIDE_REFUSAL)
    if divide and args.view_composite_shade is not None:
        raise SystemExit("--view-composite-shade: " + composite.DIVIDE_SHADE_REFUSAL)


def _write_rgb_png(path, rgb):
    """uint8 [rows, cols, 3] = R, G, B into a PNG whose bytes are R, G, B: tool.write_png takes cv2's B, G, R (and read_png hands it back)"""
    from brief_pytorch_amd.tool import write_png
    write_png(path, rgb[..., ::-1])


def _composite(args, opt, region, divide):
    import numpy as np
    import torch
    from brief_pytorch_amd.framework import NFGR, decompress_divide_composite
    module, side_path, blocks_dir = _paths(args.c)
    t0 = time.perf_counter()
    try:
        if divide:                                                # (--view-owner nearest: _composite_refusals refused everything else)
            render = lambda *a, **kw: decompress_divide_composite(opt, side_path, module, blocks_dir, *a, **kw)
        else:
            render = lambda *a, **kw: NFGR.decompress_composite(opt, module, side_path, *a, **kw)
        shading = {}
        if args.view_composite_shade is not None:                 # (a SingleTask artefact: _composite_refusals refused a DivideTask one)
            shading = dict(shade=_floats(args.view_composite_shade, 2, "--view-composite-shade"),
                           light=_floats(args.view_composite_light, 3, "--view-composite-light") if args.view_composite_light is not None else None)
        img, hits, stats = render(
            _floats(args.view, 3, "--view"), args.view_composite,
            up=_floats(args.view_up, 3, "--view-up") if args.view_up is not None else None, region=region,
            spacing=args.view_spacing, depth_spacing=args.view_depth_spacing,
            size=[int(x) for x in _floats(args.view_size, 2, "--view-size")] if args.view_size is not None else None,
            voxel_size=_floats(args.voxel_size, 3, "--voxel-size") if args.voxel_size is not None else (1, 1, 1),
            channel=args.view_composite_channel or 0,
            background=_floats(args.view_background, 3, "--view-background") if args.view_background is not None else (0, 0, 0),
            bits=args.view_composite_bits, return_hits=True, **shading)
    except ValueError as e:                                       # a refusal (artefact kind, dtype, normalisation, postprocess, transfer, geometry, net)
        raise SystemExit("--view-composite: %s" % e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if os.path.splitext(args.o)[1].lower() == ".npy":
        data = img
        np.save(args.o, data)
    else:
        data = np.ascontiguousarray(img[..., :3])
        _write_rgb_png(args.o, data)
    print("%s composite view %s of region %s: image %s, dtype %s, %d of %d rays hit, %d samples evaluated%s, decoded in %.3f s -> %s" % (
        "DivideTask (%d of %d blocks hit, owner %s, %d samples in the second pass)" % (
            stats["blocks_hit"], stats["blocks"], args.view_owner, stats["samples_second_pass"]) if divide else "SingleTask",
        args.view, args.region, tuple(data.shape), data.dtype, stats["rays_hit"], stats["rays"], stats["samples_evaluated"],
        ", %d of them shaded (%s)" % (stats["samples_shaded"], args.view_composite_shade) if "samples_shaded" in stats else "", dt, args.o))
    return 0


def _derivative_refusals(args, flag, mode, modes, noun, clashes):
    """every refusal of --gradient / --hessian by name, before the GPU path is imported; clashes: (other flag, given, why not both)"""
    if mode not in modes:
        raise SystemExit("%s %s: unknown mode (%s or %s)" % (flag, mode, ", ".join(modes[:-1]), modes[-1]))
    for other, on, why in clashes:
        if on:
            raise SystemExit("%s with %s: %s" % (flag, other, why))
    if os.path.splitext(args.o)[1].lower() != ".npy":
        raise SystemExit("%s writes float32 arrays as .npy only (got %s): %s output in image formats is not supported"
                         % (flag, os.path.splitext(args.o)[1] or "no extension", noun))
    if args.shape and os.path.isdir(_paths(args.c)[2]):
        raise SystemExit("%s --shape: resampling is not defined for a DivideTask artefact (every block has its own linspace grid)" % flag)


def _derivative(args, opt, region, shape, divide, flag, mode, what, single, divided, finish=None):
    """--gradient / --hessian: single / divided are the decode's *_device functions, finish a map of the result on the device"""
    import numpy as np
    import torch
    module, side_path, blocks_dir = _paths(args.c)
    t0 = time.perf_counter()
    try:
        if divide:
            r = divided(opt, side_path, module, blocks_dir, region, args.step)
        else:
            r = single(opt, module, side_path, region, args.step, shape=shape)
    except ValueError as e:                                       # a refusal (net class, precision, width, normalisation, overlap, region)
        raise SystemExit("%s: %s" % (flag, e))
    if finish is not None:
        r = finish(r)                                             # on the device
    data = r.cpu().numpy()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    np.save(args.o, data)
    print("%s region %s: %s, shape %s, dtype %s, decoded in %.3f s -> %s" % (
        "DivideTask" if divide else "SingleTask", args.region, what % mode, tuple(data.shape), data.dtype, dt, args.o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
