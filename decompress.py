#!/usr/bin/env python3
"""Decode a region of a stored BRIEF artefact without decoding the whole volume:

    python decompress.py -p <run yaml> -c <outputs/.../steps{k}/compressed> --region z0:z1,y0:y1,x0:x1 [--step s] [--shape D,H,W] -o roi.tif|roi.npy

The artefact kind is read from the directory: a `sideinfos/` directory of blocks is a DivideTask artefact, a single
`sideinfos.yaml` beside `module` a SingleTask one.  2-D data takes `--region y0:y1,x0:x1`.  A part of the region may be
`a:b`, `a:`, `:b`, `:` or `a:b:s` (numpy slice semantics; out-of-range bounds are refused, not clipped).  `--shape`
(SingleTask only) evaluates the net on a linspace grid of that spatial shape, and the region indexes that grid.
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
    ap.add_argument("-o", required=True, help="output file (.tif / .tiff / .npy / .png / .jpg)")
    args = ap.parse_args(argv)

    import torch
    from brief_pytorch_amd import config
    from brief_pytorch_amd.framework import NFGR, decompress_divide_region
    from brief_pytorch_amd.region import parse_region, parse_shape
    from brief_pytorch_amd.tool import save_img

    opt = config.load(args.p)
    region = parse_region(args.region)
    shape = parse_shape(args.shape) if args.shape else None
    divide = os.path.isdir(os.path.join(args.c, "sideinfos"))
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


if __name__ == "__main__":
    sys.exit(main())
