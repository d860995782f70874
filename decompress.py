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
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


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
    ap.add_argument("-o", required=True, help="output file (.tif / .tiff / .npy / .png / .jpg)")
    args = ap.parse_args(argv)
    if args.gradient is not None:
        # every refusal by name, before the GPU path is imported
        if args.gradient not in ("components", "magnitude"):
            raise SystemExit("--gradient %s: unknown mode (components or magnitude)" % args.gradient)
        if args.mip:
            raise SystemExit("--gradient with --mip: a projection of a gradient is not defined here; ask for one of them")
        if os.path.splitext(args.o)[1].lower() != ".npy":
            raise SystemExit("--gradient writes float32 arrays as .npy only (got %s): gradient output in image formats is not supported"
                             % (os.path.splitext(args.o)[1] or "no extension"))
        if args.shape and os.path.isdir(os.path.join(args.c, "sideinfos")):
            raise SystemExit("--gradient --shape: resampling is not defined for a DivideTask artefact (every block has its own linspace grid)")
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
    divide = os.path.isdir(os.path.join(args.c, "sideinfos"))
    if args.mip:
        return _mip(args, opt, region, divide)
    if args.gradient is not None:
        return _gradient(args, opt, region, shape, divide)
    t0 = time.perf_counter()
    if divide:
        if shape is not None:
            raise SystemExit("--shape: resampling is not defined for a DivideTask artefact (every block has its own linspace grid)")
        data = decompress_divide_region(opt, os.path.join(args.c, "sideinfos.yaml"), os.path.join(args.c, "module"),
                                        os.path.join(args.c, "sideinfos"), region, args.step)
    else:
        data = NFGR.decompress_region(opt, os.path.join(args.c, "module"), os.path.join(args.c, "sideinfos.yaml"), region, args.step,
                                      shape=shape)
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
    t0 = time.perf_counter()
    try:
        if divide:
            mips = decompress_divide_mip(opt, os.path.join(args.c, "sideinfos.yaml"), os.path.join(args.c, "module"),
                                         os.path.join(args.c, "sideinfos"), region, args.step)
        else:
            mips = NFGR.decompress_mip(opt, os.path.join(args.c, "module"), os.path.join(args.c, "sideinfos.yaml"), region, args.step)
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


def _gradient(args, opt, region, shape, divide):
    import numpy as np
    import torch
    from brief_pytorch_amd import gradient
    t0 = time.perf_counter()
    try:
        if divide:
            g = gradient.decompress_divide_gradient_device(opt, os.path.join(args.c, "sideinfos.yaml"), os.path.join(args.c, "module"),
                                                           os.path.join(args.c, "sideinfos"), region, args.step)
        else:
            g = gradient.decompress_gradient_device(opt, os.path.join(args.c, "module"), os.path.join(args.c, "sideinfos.yaml"), region, args.step,
                                                    shape=shape)
    except ValueError as e:                                       # a refusal (net class, precision, width, normalisation, overlap, region)
        raise SystemExit("--gradient: %s" % e)
    if args.gradient == "magnitude":
        g = gradient.magnitude(g)                                 # on the device
    data = g.cpu().numpy()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    np.save(args.o, data)
    print("%s region %s: spatial gradient (%s, grey levels per voxel), shape %s, dtype %s, decoded in %.3f s -> %s" % (
        "DivideTask" if divide else "SingleTask", args.region, args.gradient, tuple(data.shape), data.dtype, dt, args.o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
