"""Projection decode on the GPU: brief_mip_accumulate against numpy, decode_mips against mip_ops of decode_box, and
NFGR.decompress_mip / decompress_divide_mip / decompress.py --mip against mip_ops of the existing decodes.  Every comparison is
bitwise: a max of integers has one right answer."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from brief_pytorch_amd import _lib, config, corrections, mip
from brief_pytorch_amd.framework import NFGR, MyLogger, decompress_divide_mip, decompress_divide_region
from brief_pytorch_amd.misc import mip_ops
from brief_pytorch_amd.modelsave import save_model
from brief_pytorch_amd.networks import SIREN
from brief_pytorch_amd.synthetic import make_volume
from brief_pytorch_amd.tool import read_img, save_img

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = dict(scale=(-0.5, 0.5), vrange=(3.0, 60000.0))
EXTENTS = [(1, 1, 1), (5, 7, 9), (3, 300, 5), (70, 45, 133), (257, 2, 64), (2, 3, 1031)]


def _random(rng, shape, dtype):
    """skewed towards small values, so that the maxima along a ray are not all the type's maximum"""
    return (rng.random(shape) ** 4 * np.iinfo(dtype).max).astype(dtype)


def _fold(box, images, origin):
    out = mip.accumulate(torch.from_numpy(box).to(DEV), tuple(torch.from_numpy(i).to(DEV) for i in images), origin)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_kernel_against_numpy(dtype, channels):
    rng = np.random.default_rng(100 * channels + np.dtype(dtype).itemsize)
    for ext in EXTENTS:
        box = _random(rng, ext + (channels,), dtype)
        # into zero images of the box's own frame
        zero = [np.zeros(s + (channels,), dtype) for s in ((ext[1], ext[2]), (ext[0], ext[2]), (ext[0], ext[1]))]
        got = _fold(box, zero, (0, 0, 0))
        for g, ax in zip(got, range(3)):
            assert g.dtype == dtype and np.array_equal(g, box.max(ax)), (ext, ax)
        again = _fold(box, zero, (0, 0, 0))
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), ext
        # a second box into NON-zero images, at a non-zero origin of a larger frame: max with what is there, nothing else touched
        org = (2, 3, 5)
        frame = tuple(e + o + p for e, o, p in zip(ext, org, (1, 4, 3)))
        imgs = [_random(rng, s + (channels,), dtype) for s in ((frame[1], frame[2]), (frame[0], frame[2]), (frame[0], frame[1]))]
        want = [i.copy() for i in imgs]
        z, y, x = (slice(o, o + e) for o, e in zip(org, ext))
        want[0][y, x] = np.maximum(want[0][y, x], box.max(0))
        want[1][z, x] = np.maximum(want[1][z, x], box.max(1))
        want[2][z, y] = np.maximum(want[2][z, y], box.max(2))
        got = _fold(box, imgs, org)
        for g, w_, ax in zip(got, want, range(3)):
            assert np.array_equal(g, w_), (ext, ax)
        again = _fold(box, imgs, org)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), ext


def test_kernel_grid_stride_and_misaligned_source():
    """more rows (k_mip_rows) and more (z, segment) pieces (k_mip_cols) than the grid's cap of 256 workgroups per compute unit, so
    that workgroups take a second turn; and a box that starts one element into an allocation (not 16-byte aligned: element loads
    although the rows are whole vectors)"""
    rng = np.random.default_rng(7)
    cap = 256 * _lib.lib().brief_cu_count()
    for ext in ((1, cap + 4001, 3), (cap + 4001, 1, 3)):
        box = _random(rng, ext + (1,), np.uint8)
        zero = [np.zeros(s + (1,), np.uint8) for s in ((ext[1], ext[2]), (ext[0], ext[2]), (ext[0], ext[1]))]
        for g, ax in zip(_fold(box, zero, (0, 0, 0)), range(3)):
            assert np.array_equal(g, box.max(ax)), (ext, ax)
    for dtype, ext, ch in ((np.uint16, (9, 5, 64), 1), (np.uint8, (6, 7, 32), 4)):
        box = _random(rng, ext + (ch,), dtype)
        buf = torch.zeros(box.size + 1, dtype=torch.from_numpy(box).dtype, device=DEV)
        view = buf[1:].view(*box.shape)
        view.copy_(torch.from_numpy(box).to(DEV))
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        imgs = tuple(torch.zeros(s + (ch,), dtype=buf.dtype, device=DEV) for s in ((ext[1], ext[2]), (ext[0], ext[2]), (ext[0], ext[1])))
        for g, ax in zip(mip.accumulate(view, imgs), range(3)):
            assert np.array_equal(g.cpu().numpy(), box.max(ax)), (ext, ax)


def test_accumulate_refusals():
    import ctypes as C
    L = _lib.lib()
    i3 = C.c_int64 * 3
    box = torch.zeros((4, 5, 6, 1), dtype=torch.uint16, device=DEV)
    d, h, w = (torch.zeros(s, dtype=torch.uint16, device=DEV) for s in ((5, 6, 1), (4, 6, 1), (4, 5, 1)))
    p, st = _lib.ptr, _lib.stream_ptr()
    good = dict(src=p(box), kind=_lib.OUT_U16, ext=(4, 5, 6), ch=1, d=p(d), h=p(h), w=p(w), org=(0, 0, 0), frame=(4, 5, 6))
    for change, what in [(dict(src=None), "null"), (dict(h=None), "null"), (dict(kind=_lib.OUT_F32), "elem_kind"), (dict(kind=3), "elem_kind"),
                         (dict(ch=0), "channels"), (dict(ch=5), "channels"), (dict(ext=(4, 0, 6)), ">= 1"), (dict(frame=(4, 5, 0)), ">= 1"),
                         (dict(org=(0, 1, 0)), "inside the frame"), (dict(org=(-1, 0, 0)), "inside the frame"),
                         (dict(ext=(4, 5, 7)), "inside the frame"), (dict(frame=(1 << 31, 5, 6)), "2^31")]:
        a = dict(good, **change)
        rc = L.brief_mip_accumulate(a["src"], a["kind"], i3(*a["ext"]), a["ch"], a["d"], a["h"], a["w"], i3(*a["org"]), i3(*a["frame"]), st)
        assert rc == -1 and what in L.brief_last_error().decode(), (change, L.brief_last_error())
    torch.cuda.synchronize()
    assert not any(t.cpu().numpy().any() for t in (d, h, w))


def _mips_of(t):
    return mip_ops(t.cpu().numpy())


def test_chunk_invariance():
    torch.manual_seed(3)
    for cout, kind in ((1, "u16"), (3, "u8")):
        m = SIREN(coords_channel=3, data_channel=cout, features=22, layers=4, w0=20).to(DEV)
        dims = [19, 23, 29]
        for start, stop, step in (([0, 0, 0], dims, [1, 1, 1]), ([1, 2, 0], [19, 22, 29], [2, 1, 3])):
            want = _mips_of(m.decode_box(dims, start, stop, step, -1.0, 1.0, out_kind=kind, **EPI))
            ext = [(e - b + s - 1) // s for b, e, s in zip(start, stop, step)]
            for chunk in (1000, ext[1] * ext[2], None, 5):
                got = mip.decode_mips(m, dims, start, stop, step, -1.0, 1.0, kind, EPI["scale"], EPI["vrange"], chunk=chunk)
                for g, w_ in zip(got, want):
                    assert g.is_cuda and np.array_equal(g.cpu().numpy(), w_), (kind, start, chunk)


# ---- artefacts ------------------------------------------------------------------------------------------------------------------
def _single_opt(tmp_path, yaml, steps, given, eps=None):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", yaml))
    cf = opt.CompressFramework
    cf.Compress.max_steps = steps
    cf.Compress.checkpoints = "none"
    cf.Compress.param.filesize_ratio = 0
    cf.Compress.param.given_size = given
    cf.Compress.loss_log_freq = steps
    if eps is not None:
        cf.Compress.error_bound = eps
    cf.Decompress.mip = False
    cf.Decompress.ssim = False
    opt.Log.outputs_dir = str(tmp_path / "outputs")
    opt.Log.time = False
    return opt


def _fit_single(tmp_path, yaml, steps=2000, given=20000.0, eps=None, shape=(24, 40, 56), seed=11):
    """2000 steps: with Adamax at lr 1e-3 the output of these nets first rises as one level towards the volume's mean (a third of the
    normalised range, about 1000 steps: the decode is a constant until then, and projections of a constant test nothing); the
    structure comes after that"""
    vol = make_volume(shape, seed=seed)
    path = str(tmp_path / "vol.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, yaml, steps, given, eps)
    Log = MyLogger(**opt.Log)
    torch.manual_seed(1)
    NFGR(opt.CompressFramework, Log=Log).compress(path)
    cdir = os.path.join(Log.logdir, "steps%d" % steps, "compressed")
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    return opt, cdir, yml, vol


@pytest.fixture(scope="module")
def single_artefact(tmp_path_factory):
    return _fit_single(tmp_path_factory.mktemp("mip_single"), "default.yaml")


REGION = "3:20,5:33:2,1:50:3"
REGION_SLICES = (slice(3, 20), slice(5, 33, 2), slice(1, 50, 3))


def _check_single(opt, cdir):
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    whole = NFGR.decompress(opt, mod, side)
    assert whole.dtype == np.uint16 and whole.shape == (24, 40, 56, 1)
    for region, sl in ((None, (slice(None),) * 3), (REGION, REGION_SLICES)):
        got = NFGR.decompress_mip(opt, mod, side, region)
        want = mip_ops(whole[sl])
        for g, w_ in zip(got, want):
            assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g, w_), region
    return whole


@pytest.mark.parametrize("yaml", ["default.yaml", "mfn_fourier.yaml", "sirenps.yaml"])
def test_singletask_equals_mip_ops_of_decompress(yaml, single_artefact, tmp_path):
    opt, cdir = single_artefact[:2] if yaml == "default.yaml" else _fit_single(tmp_path, yaml)[:2]
    whole = _check_single(opt, cdir)
    # a threshold and a narrowing clip: the postprocess acts on the images there and on the voxels here
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    vmin, span = int(whole.min()), int(whole.max()) - int(whole.min())
    lo, level, hi = vmin + span // 8, vmin + span // 4, vmin + span // 2
    assert span >= 64 and 0 < lo < level < hi < whole.max(), "the fit is too short for a decode with structure"
    pp.denoise.level, pp.denoise.close, pp.clip = level, False, [lo, hi]
    whole2 = _check_single(o2, cdir)
    assert not np.array_equal(whole2, whole)


def test_error_bounded_artefact(tmp_path):
    eps = 50
    opt, cdir, _, vol = _fit_single(tmp_path, "default.yaml", eps=eps)
    mod, side = os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml")
    idx, q, head = corrections.read(os.path.join(cdir, "corrections.bin"))
    assert head["count"] > 0 and idx.size == head["count"]
    dec = NFGR.decompress(opt, mod, side)
    raw = NFGR._decode_integer(opt.CompressFramework, mod, config.load(side)).cpu().numpy().reshape(dec.shape)
    assert not np.array_equal(mip_ops(raw)[0], mip_ops(dec)[0]), "the corrections do not reach the projections: the case is vacuous"
    src = vol.reshape(dec.shape)
    for region, sl in ((None, (slice(None),) * 3), (REGION, REGION_SLICES)):
        got = NFGR.decompress_mip(opt, mod, side, region)
        for g, w_, s in zip(got, mip_ops(dec[sl]), mip_ops(src[sl])):
            assert np.array_equal(g, w_), region
            assert np.abs(g.astype(np.int64) - s.astype(np.int64)).max() <= eps
    # small chunks: the corrections of every sub-box
    got = mip.decompress_mip(opt, mod, side, REGION, chunk=97)
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, mip_ops(dec[REGION_SLICES])))
    os.rename(os.path.join(cdir, "corrections.bin"), os.path.join(cdir, "corrections.away"))
    with pytest.raises(corrections.CorrectionsError, match="corrections.bin"):
        NFGR.decompress_mip(opt, mod, side)


@pytest.fixture(scope="module")
def divide_artefact(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("mip_divide")
    vol = make_volume((32, 48, 64), seed=7)
    path = str(tmp_path / "d.tif")
    save_img(path, vol)
    opt = _single_opt(tmp_path, "default.yaml", 2000, 40000.0)
    cf = opt.CompressFramework
    cf.Compress.divide.divide_type = "total_2_2_2"
    cf.Compress.divide.param_alloc = "by_size"
    Log = MyLogger(**opt.Log)
    torch.manual_seed(42)
    fw = NFGR(cf, Log=Log)
    fw.compress_divide(path, opt)
    yml = str(tmp_path / "run.yaml")
    config.save(opt, yml)
    return fw, opt, os.path.join(Log.logdir, "steps2000", "compressed"), yml


def test_dividetask_equals_mip_ops_of_the_region_decode(divide_artefact):
    fw, opt, cdir, _ = divide_artefact
    args = (os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    assert len(os.listdir(args[1])) == 8
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 20000, False, [18000, 23000]      # (the volume: 17261 .. 26923, median 20317)
    for region in ((slice(None),) * 3, "5:30:2,10:40:3,7:60:5", "14:18,:,30:34", "0:16,0:24,0:32"):
        want = mip_ops(fw.decompress_divide_region(*args, region))
        got = fw.decompress_divide_mip(*args, region)
        for g, w_ in zip(got, want):
            assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g, w_), region
        want = mip_ops(decompress_divide_region(o2, *args, region))
        assert all(np.array_equal(g, w_) for g, w_ in zip(decompress_divide_mip(o2, *args, region), want)), region
    assert all(np.array_equal(g, w_) for g, w_ in zip(fw.decompress_divide_mip(*args), mip_ops(fw.decompress_divide(*args))))


def test_dividetask_with_a_gap_leaves_uncovered_rays_at_zero(divide_artefact, tmp_path):
    """a partition with a block missing (what adaptive blocking leaves where it prunes): inside 0:16 the rays along z through the
    missing block meet no block at all and stay 0, although the clip's floor would lift a 0 that went through the postprocess"""
    import shutil
    _, opt, cdir, _ = divide_artefact
    gap = str(tmp_path / "compressed")
    shutil.copytree(cdir, gap)
    for sub in ("module", "sideinfos"):
        shutil.rmtree(os.path.join(gap, sub, "d_0_15-h_0_23-w_0_31"))
    args = (os.path.join(gap, "sideinfos.yaml"), os.path.join(gap, "module"), os.path.join(gap, "sideinfos"))
    assert len(os.listdir(args[1])) == 7
    o2 = config.to_opt(config.to_plain(opt))
    pp = o2.CompressFramework.Decompress.postprocess
    pp.denoise.level, pp.denoise.close, pp.clip = 20000, False, [18000, 23000]
    for o in (opt, o2):
        for region in ("0:16,:,:", (slice(None),) * 3, "2:14:3,1:40:2,5:60:4"):
            want = mip_ops(decompress_divide_region(o, *args, region))
            got = decompress_divide_mip(o, *args, region)
            assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), region
    got = decompress_divide_mip(o2, *args, "0:16,:,:")
    assert (got[0][:24, :32] == 0).all() and (got[0][24:, 32:] >= 18000).all()


def test_memory_stays_bounded_by_the_chunk(tmp_path):
    torch.manual_seed(5)
    m = SIREN(coords_channel=3, data_channel=1, features=22, layers=5, w0=20)
    mod = str(tmp_path / "module")
    save_model(m, mod)
    side = {"dtype": "uint16", "min": 3.0, "max": 60000.0, "data_shape": [64, 256, 256, 1], "phi_features": 22, "phi_name": "SIREN"}
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    cf = opt.CompressFramework
    phi = mip._load_phi(cf, mod, side, DEV)
    volume_bytes = 64 * 256 * 256 * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = mip.decode_mips(phi, [64, 256, 256], [0, 0, 0], [64, 256, 256], [1, 1, 1], -1.0, 1.0, "u16", (0.0, 100.0), (3.0, 60000.0), chunk=1 << 18)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise %d bytes, decoded volume %d bytes" % (rise, volume_bytes))
    assert rise < volume_bytes // 4
    # the artefact-level call: the net (a few KiB) is loaded inside it
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    imgs = mip.decompress_mip(opt, mod, side, chunk=1 << 18)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < volume_bytes // 4
    want = mip_ops(NFGR.decompress(opt, mod, dict(side)))
    for g, i, w_ in zip(got, imgs, want):
        assert np.array_equal(g.cpu().numpy(), w_) and np.array_equal(i, w_)


def _cli(yml, cdir, region, out, step=1):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decompress.py"), "-p", yml, "-c", cdir, "--region", region, "--step", str(step), "--mip",
                        "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "max-intensity projections" in r.stdout and "uint16" in r.stdout
    stem, ext = os.path.splitext(out)
    assert not os.path.exists(out)
    return [read_img(stem + "_mip_%s%s" % (a, ext)) for a in "dhw"]


def test_cli_writes_the_three_projections(single_artefact, divide_artefact, tmp_path):
    opt, cdir, yml, _ = single_artefact
    want = NFGR.decompress_mip(opt, os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos.yaml"), "2:20,:,1:50", 2)
    got = _cli(yml, cdir, "2:20,:,1:50", str(tmp_path / "s.tif"), step=2)
    assert all(np.array_equal(g.reshape(w_.shape), w_) for g, w_ in zip(got, want))
    fw, opt, cdir, yml = divide_artefact
    want = fw.decompress_divide_mip(os.path.join(cdir, "sideinfos.yaml"), os.path.join(cdir, "module"), os.path.join(cdir, "sideinfos"))
    got = _cli(yml, cdir, ":,:,:", str(tmp_path / "d.npy"))
    assert all(np.array_equal(g.reshape(w_.shape), w_) for g, w_ in zip(got, want))
