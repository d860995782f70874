"""What the error-bounded mode (Compress.error_bound) costs on one synthetic uint16 volume, over a list of bounds:

    python tools/error_bound_sweep.py --size 512 --steps 2000 --features 256 --eps 655 --sigmas 2 3 4 6 --timing --out eb.md
    python tools/error_bound_sweep.py --size 512 --detail 64 ...          (the textured volume of tools/rate_distortion.py)

A SIREN is fitted through the fused path, decoded with the fused uint16 epilogue, and for every bound eps the corrections are found
on the device (corrections.find), packed (corrections.encode, with both standard-library codecs) and applied.  Printed per eps:
K, the corrections' bytes (lzma | zlib), total bits per voxel (fp32 weights + corrections), PSNR before and after, the maximum
error after (which must be <= eps).  --sigmas adds bounds at multiples of the fit's RMSE.  --timing: device-event times of the
count + emit pass and of the apply pass against the whole-grid decode of the same volume, alternated in one process behind a
warm-up, and the bytes per second the passes reach.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brief_pytorch_amd import _lib, corrections              # noqa: E402
from brief_pytorch_amd.fit import Fitter                     # noqa: E402
from brief_pytorch_amd.networks import SIREN                 # noqa: E402
from brief_pytorch_amd.synthetic import make_volume_torch    # noqa: E402

HBM_PEAK = 6.3e12       # bytes / s a streaming kernel reaches on an MI355X (8 TB/s nominal)


def psnr_u16(a, b):
    sse = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().brief_sse_u16(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(sse), _lib.stream_ptr()))
    s = sse.item()
    return float("inf") if s == 0 else -10.0 * np.log10(s / a.numel() / 65535.0 ** 2)


def timed(fn, reps):
    """median / min of `reps` device-event timings of fn() in ms"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--detail", type=int, default=0, help="1/f texture components of the synthetic field (0 = the bench volume)")
    ap.add_argument("--eps", type=int, nargs="*", default=[655])
    ap.add_argument("--sigmas", type=float, nargs="*", default=[2, 3, 4, 6], help="further bounds at these multiples of the fit's RMSE")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    n = a.size
    dims, vox = (n, n, n), n ** 3
    vol = make_volume_torch(dims, seed=42, detail=a.detail).reshape(-1)
    vf = vol.to(torch.int32).to(torch.float32)
    vmin, vmax = float(vf.min()), float(vf.max())
    tv = ((vf - vmin) / (vmax - vmin) * 100.0).reshape(vox, 1).contiguous()
    del vf
    torch.manual_seed(42)
    m = SIREN(coords_channel=3, data_channel=1, features=a.features, layers=a.layers, w0=20.0).to("cuda")
    Fitter(m, tv, dims, sampler="randompoint", sample_size=100000, seed=42).run(a.steps)
    torch.cuda.synchronize()

    def decode():
        return m.decode_grid(dims, out_kind="u16", scale=(0.0, 100.0), vrange=(vmin, vmax))
    dec = decode().reshape(-1)
    before = psnr_u16(vol, dec)
    rmse = 65535.0 * 10.0 ** (-before / 20.0)
    net_bits = 32.0 * m.param_count / vox
    eps_list = sorted(set(int(e) for e in a.eps) | set(max(0, int(round(s * rmse))) for s in a.sigmas))
    lines = ["%d^3 uint16 volume (detail %d), SIREN %dx%d after %d steps: PSNR %.2f dB (RMSE %.1f grey levels), net %.4f bits/voxel, max error %d"
             % (n, a.detail, a.layers - 1, a.features, a.steps, before, rmse, net_bits, corrections.max_abs_diff(vol, dec)), "",
             "| eps | K | K / voxels | lzma bytes | zlib bytes | bits/voxel (net + lzma) | PSNR before dB | PSNR after dB | max error after | pack s (lzma / zlib) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    for eps in eps_list:
        idx, q = corrections.find(dec, vol, eps)
        fixed = corrections.apply(dec.clone(), idx, q, eps)
        worst = corrections.max_abs_diff(vol, fixed)
        assert worst <= eps, (eps, worst)
        after = psnr_u16(vol, fixed)
        hi, hq = idx.cpu().numpy(), q.cpu().numpy()
        size, secs = {}, {}
        for codec in ("lzma", "zlib"):
            t0 = time.perf_counter()
            size[codec] = len(corrections.encode(hi, hq, eps, vox, np.uint16, codec=codec))
            secs[codec] = time.perf_counter() - t0
        row = "| %d | %d | %.5f | %d | %d | %.4f | %.2f | %.2f | %d | %.1f / %.1f |" % (
            eps, idx.numel(), idx.numel() / vox, size["lzma"], size["zlib"], net_bits + 8.0 * size["lzma"] / vox, before, after, worst,
            secs["lzma"], secs["zlib"])
        print(row, flush=True)
        lines.append(row)
        del idx, q, fixed
    if a.timing:
        L = _lib.lib()
        eps = eps_list[len(eps_list) // 2]
        per = int(L.brief_correct_chunk_elems(2))
        counts = torch.empty((vox + per - 1) // per, dtype=torch.int32, device="cuda")
        st = _lib.stream_ptr()

        def count():
            _lib.check(L.brief_correct_count(_lib.ptr(dec), _lib.ptr(vol), 2, vox, eps, 0, _lib.ptr(counts), st))
        count()
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        offsets, total = incl - counts, int(incl[-1].item())
        idx = torch.empty(total, dtype=torch.int64, device="cuda")
        q = torch.empty(total, dtype=torch.int32, device="cuda")
        work = dec.clone()

        def emit():
            _lib.check(L.brief_correct_emit(_lib.ptr(dec), _lib.ptr(vol), 2, vox, eps, 0, _lib.ptr(offsets), total, _lib.ptr(idx), _lib.ptr(q), st))

        def both():
            count()
            o = torch.cumsum(counts, 0, dtype=torch.int64) - counts
            _lib.check(L.brief_correct_emit(_lib.ptr(dec), _lib.ptr(vol), 2, vox, eps, 0, _lib.ptr(o), total, _lib.ptr(idx), _lib.ptr(q), st))

        def apply():
            _lib.check(L.brief_correct_apply(_lib.ptr(work), 2, vox, _lib.ptr(idx), _lib.ptr(q), total, eps, 0, st))
        # warm-up from idle clocks: a second of decodes, then every timed shape once
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:
            decode()
            torch.cuda.synchronize()
        for fn in (count, emit, both, apply):
            fn()
        res = {"decode": [], "count": [], "emit": [], "count + scan + emit": [], "apply": []}
        for _ in range(a.reps):                                  # alternated: one timing of each per round
            for name, fn in (("decode", decode), ("count", count), ("emit", emit), ("count + scan + emit", both), ("apply", apply)):
                res[name].append(timed(fn, 1)[0])
        t_dec = float(np.median(res["decode"]))
        vol_bytes = 2.0 * vox
        moved = {"count": 2 * vol_bytes, "emit": 2 * vol_bytes + 12.0 * total, "count + scan + emit": 4 * vol_bytes + 12.0 * total,
                 "apply": 12.0 * total + 2 * 2.0 * total}
        lines += ["", "Timing at eps = %d (K = %d, %.3f %% of the voxels), median of %d alternated rounds behind a 1 s warm-up:" % (eps, total, 100.0 * total / vox, a.reps), "",
                  "| pass | ms (median) | ms (min) | share of the decode | bytes moved | TB/s | share of %.1f TB/s |" % (HBM_PEAK / 1e12), "|---|---|---|---|---|---|---|"]
        for name in ("decode", "count", "emit", "count + scan + emit", "apply"):
            med, mn = float(np.median(res[name])), float(np.min(res[name]))
            if name == "decode":
                lines.append("| decode (whole grid, fused uint16 epilogue) | %.3f | %.3f | 1 | %.3g | | |" % (med, mn, vol_bytes))
            else:
                rate = moved[name] / (med * 1e-3)
                lines.append("| %s | %.3f | %.3f | %.4f | %.3g | %.2f | %.2f |" % (name, med, mn, med / t_dec, moved[name], rate / 1e12, rate / HBM_PEAK))
        print("\n".join(lines[-(len(res) + 4):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
