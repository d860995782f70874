"""Max-intensity projections of a stored artefact: the existing path (decode the region, copy it to the host, numpy max along three
axes) against the projection decode (NFGR.decompress_mip: decode a chunk, fold it on the device, drop it), and the fold kernels on
their own against a device-to-device copy of the same bytes.

    python tools/mip_timing.py [--reps 3] [--workdir DIR] [--json out.json]

Three artefacts, written from random-init nets (the time does not depend on the weights): a 512^3 uint16 volume behind a 4x256
SIREN, the default.yaml net (4x22) on 64^3, and a DivideTask artefact (256^3 in 2x2x2 blocks, 4x64 each).  Each once whole and once
for a slab of 64 slices (of 16 on the 64^3 volume).  Per case:
  (a) decompress_region (decompress_divide_region) + mip_ops      wall time, the yardstick
  (b) decompress_mip (decompress_divide_mip)                      wall time
  (c) brief_mip_accumulate on one decoded chunk of that case      device events; GB/s = the chunk's bytes / time (the two kernels
                                                                   read them once each), beside torch's copy of the same bytes
Every call is warmed once; the median of --reps is printed."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brief_pytorch_amd import config, mip  # noqa: E402
from brief_pytorch_amd.framework import NFGR, decompress_divide_mip, decompress_divide_region  # noqa: E402
from brief_pytorch_amd.misc import chunk_name, mip_ops  # noqa: E402
from brief_pytorch_amd.modelsave import save_model  # noqa: E402
from brief_pytorch_amd.networks import SIREN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _side(shape, features):
    return {"dtype": "uint16", "min": 0.0, "max": 65535.0, "data_shape": list(shape) + [1], "phi_features": features, "phi_name": "SIREN"}


def _write_net(path, features, seed):
    torch.manual_seed(seed)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save_model(SIREN(coords_channel=3, data_channel=1, features=features, layers=5, w0=20), path)


def _single(workdir, tag, edge, features):
    d = os.path.join(workdir, tag)
    _write_net(os.path.join(d, "module"), features, 0)
    with open(os.path.join(d, "sideinfos.yaml"), "w") as f:
        yaml.safe_dump(_side((edge,) * 3, features), f)
    return d


def _divide(workdir, tag, edge, features):
    d = os.path.join(workdir, tag)
    half = edge // 2
    for i, (z, y, x) in enumerate(np.ndindex(2, 2, 2)):
        name = chunk_name({"d": [z * half, (z + 1) * half - 1], "h": [y * half, (y + 1) * half - 1], "w": [x * half, (x + 1) * half - 1]})
        _write_net(os.path.join(d, "module", name, "module"), features, i)
        os.makedirs(os.path.join(d, "sideinfos", name))
        with open(os.path.join(d, "sideinfos", name, "sideinfos.yaml"), "w") as f:
            yaml.safe_dump(_side((half,) * 3, features), f)
    with open(os.path.join(d, "sideinfos.yaml"), "w") as f:
        yaml.safe_dump({"data_shape": [edge] * 3 + [1]}, f)
    return d


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    workdir = args.workdir or tempfile.mkdtemp(prefix="mip_timing_")
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cases = [("SIREN 4x256, 512^3 u16", "single", _single(workdir, "s512", 512, 256), 512, 64),
             ("SIREN 4x22, 64^3 u16", "single", _single(workdir, "s64", 64, 22), 64, 16),
             ("DivideTask 2x2x2 of 4x64, 256^3 u16", "divide", _divide(workdir, "d256", 256, 64), 256, 64)]
    rows = []
    for label, kind, d, edge, slab in cases:
        z0 = (edge - slab) // 2
        for what, region in (("whole", (slice(None),) * 3), ("%d-slice slab" % slab, (slice(z0, z0 + slab), slice(None), slice(None)))):
            if kind == "single":
                mod, side = os.path.join(d, "module"), os.path.join(d, "sideinfos.yaml")
                old = lambda: mip_ops(NFGR.decompress_region(opt, mod, side, region))                      # noqa: E731
                new = lambda: NFGR.decompress_mip(opt, mod, side, region)                                   # noqa: E731
            else:
                a = (os.path.join(d, "sideinfos.yaml"), os.path.join(d, "module"), os.path.join(d, "sideinfos"))
                old = lambda: mip_ops(decompress_divide_region(opt, *a, region))                            # noqa: E731
                new = lambda: decompress_divide_mip(opt, *a, region)                                        # noqa: E731
            ms_old, want = _wall(old, args.reps)
            ms_new, got = _wall(new, args.reps)
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            # the fold alone, on one chunk as decode_mips plans it for this case (a block of the partition for the DivideTask)
            e = edge if kind == "single" else edge // 2
            ext = [min(slab if what != "whole" else e, e), e, e]
            p_lo, p_hi = mip.plan_chunks(ext, mip.DEFAULT_CHUNK)[0]
            shape = [h - l for l, h in zip(p_lo, p_hi)] + [1]
            box = torch.randint(0, 65536, shape, dtype=torch.int32, device="cuda").to(torch.uint16)
            imgs = tuple(torch.zeros(s + [1], dtype=torch.uint16, device="cuda") for s in ([shape[1], shape[2]], [shape[0], shape[2]], [shape[0], shape[1]]))
            dst = torch.empty_like(box)
            ms_k = _events(lambda: mip.accumulate(box, imgs), max(args.reps, 5))
            ms_c = _events(lambda: dst.copy_(box), max(args.reps, 5))
            nbytes = box.numel() * 2
            r = {"case": label, "region": what, "path_a_ms": ms_old, "path_b_ms": ms_new, "a_over_b": ms_old / ms_new, "bit_identical": same,
                 "chunk_shape": shape[:3], "chunk_bytes": nbytes, "k_mip_ms": ms_k, "k_mip_gbps": nbytes / ms_k / 1e6, "copy_ms": ms_c,
                 "copy_gbps": nbytes / ms_c / 1e6, "k_mip_over_copy": ms_k / ms_c}
            rows.append(r)
            print("%-38s %-14s (a) region + mip_ops %9.1f ms  (b) decompress_mip %9.1f ms  a/b %6.2f  identical %s | k_mip on %s: %.3f ms, "
                  "%.0f GB/s; copy %.3f ms, %.0f GB/s; k_mip/copy %.2f" % (label, what, ms_old, ms_new, r["a_over_b"], same,
                                                                           "x".join(map(str, shape[:3])), ms_k, r["k_mip_gbps"], ms_c, r["copy_gbps"],
                                                                           r["k_mip_over_copy"]), flush=True)
            del box, imgs, dst
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"reps": args.reps, "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
