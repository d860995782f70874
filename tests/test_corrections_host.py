"""Error-bounded mode, host side (brief_pytorch_amd/corrections.py and the refusals of the framework): the quantisation rule, the
corrections file, region selection — everything exact, nothing needs a GPU."""
import os

import numpy as np
import pytest

from brief_pytorch_amd import config, corrections
from brief_pytorch_amd.framework import NFGR, check_error_bound, error_bound_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("eps", [0, 1, 2, 7, 100, 65535])
def test_quantise_is_exact_for_every_difference(eps):
    """q == 0 <=> |d| <= eps and |d - q m| <= eps for EVERY difference two uint16 values can have"""
    d = np.arange(-65535, 65536, dtype=np.int64)
    q = corrections.quantise(d, eps)
    m = 2 * eps + 1
    assert np.array_equal(q == 0, np.abs(d) <= eps)
    assert (np.abs(d - q * m) <= eps).all()
    assert np.abs(q).max() <= 65535
    # floor division, not C's truncation: the first difference below -eps already gets q = -1
    assert corrections.quantise(-eps - 1, eps) == -1 and corrections.quantise(eps + 1, eps) == 1
    # the other input forms: narrow integer arrays must not overflow
    assert np.array_equal(corrections.quantise(d.astype(np.int32), eps), q)
    with pytest.raises(ValueError):
        corrections.quantise(d, -1)


def test_host_find_and_apply_restate_the_definition():
    rng = np.random.default_rng(0)
    for dtype, eps in ((np.uint8, 0), (np.uint8, 3), (np.uint16, 0), (np.uint16, 9), (np.uint16, 1000)):
        tmax = np.iinfo(dtype).max
        src = rng.integers(0, tmax + 1, 5000).astype(dtype)
        dec = np.clip(src.astype(np.int64) + rng.integers(-40, 41, src.size) * (rng.random(src.size) < 0.3), 0, tmax).astype(dtype)
        dec[:50], dec[50:100] = 0, tmax          # far off at both ends of the range
        idx, q = corrections.find_host(dec, src, eps, base=7)
        d = src.astype(np.int64) - dec.astype(np.int64)
        assert np.array_equal(idx - 7, np.flatnonzero(np.abs(d) > eps)) and idx.dtype == np.int64 and q.dtype == np.int32
        fixed = corrections.apply_host(dec, idx, q, eps, base=7)
        assert fixed.dtype == dec.dtype and np.abs(fixed.astype(np.int64) - src.astype(np.int64)).max() <= eps
        if eps == 0:
            assert np.array_equal(fixed, src)
    # saturation at both ends (corrections that do not belong to the array they are applied to)
    out = corrections.apply_host(np.array([3, 250, 100], np.uint8), [0, 1, 2], [-2, 2, 1], 2)
    assert out.tolist() == [0, 255, 105]


def _round_trip(tmp_path, idx, q, eps, n, dtype, codec):
    path = str(tmp_path / ("c_%s.bin" % codec))
    size = corrections.write(path, idx, q, eps, n, dtype, codec=codec)
    assert size == os.path.getsize(path)
    first = open(path, "rb").read()
    corrections.write(path, idx, q, eps, n, dtype, codec=codec)
    assert open(path, "rb").read() == first, "the file of a fixed input must be byte-identical when written twice"
    i2, q2, head = corrections.read(path)
    assert i2.dtype == np.int64 and q2.dtype == np.int32
    assert np.array_equal(i2, np.asarray(idx, np.int64)) and np.array_equal(q2, np.asarray(q, np.int32))
    assert head == {"version": 1, "dtype": np.dtype(dtype).name, "bound": eps, "n": n, "count": len(idx), "codec": codec, "bytes": size}
    return size


@pytest.mark.parametrize("codec", ["lzma", "zlib"])
def test_file_round_trip(tmp_path, codec):
    rng = np.random.default_rng(1)
    # K = 0
    _round_trip(tmp_path, np.zeros(0, np.int64), np.zeros(0, np.int32), 5, 1000, np.uint16, codec)
    _round_trip(tmp_path, np.zeros(0, np.int64), np.zeros(0, np.int32), 0, 0, np.uint8, codec)
    # K = n
    n = 4097
    q = rng.integers(1, 30, n).astype(np.int32) * rng.choice([-1, 1], n).astype(np.int32)
    _round_trip(tmp_path, np.arange(n), q, 3, n, np.uint8, codec)
    # random sparse sets
    for n, k in ((1, 1), (100000, 17), (1 << 22, 30000)):
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
        q = rng.integers(1, 4, k).astype(np.int32) * rng.choice([-1, 1], k).astype(np.int32)
        size = _round_trip(tmp_path, idx, q, 7, n, np.uint16, codec)
        assert size < 52 + 8 * k + 64      # gaps + values packed: far below the 12 bytes per entry of the raw arrays
    # eps = 0 with |q| up to 65535
    k = 20000
    idx = np.sort(rng.choice(1 << 20, k, replace=False)).astype(np.int64)
    q = rng.integers(-65535, 65536, k).astype(np.int32)
    q[q == 0] = 65535
    q[:2] = (-65535, 65535)
    _round_trip(tmp_path, idx, q, 0, 1 << 20, np.uint16, codec)
    # indices near 2^40: 64-bit gaps
    n = 1 << 40
    idx = np.concatenate([[5, (1 << 32) - 1, 1 << 32, (1 << 33) + 12345], n - 1 - np.arange(1000, 0, -1) * 3, [n - 1]]).astype(np.int64)
    q = rng.integers(1, 9, idx.size).astype(np.int32)
    _round_trip(tmp_path, idx, q, 2, n, np.uint16, codec)
    raw = open(str(tmp_path / ("c_%s.bin" % codec)), "rb").read()
    assert raw[:8] == b"BRIEFCOR" and raw[12] == 8          # the gap width of this file


def test_file_refuses_what_it_cannot_hold(tmp_path):
    p = str(tmp_path / "x.bin")
    with pytest.raises(corrections.CorrectionsError, match="ascending"):
        corrections.write(p, [5, 5], [1, 1], 0, 10, np.uint8)
    with pytest.raises(corrections.CorrectionsError, match="ascending"):
        corrections.write(p, [5, 10], [1, 1], 0, 10, np.uint8)
    with pytest.raises(corrections.CorrectionsError, match="non-zero"):
        corrections.write(p, [5], [0], 0, 10, np.uint8)
    with pytest.raises(corrections.CorrectionsError, match="uint8 / uint16"):
        corrections.write(p, [5], [1], 0, 10, np.float32)
    open(p, "wb").write(b"not a corrections file, whatever its length may be ........")
    with pytest.raises(corrections.CorrectionsError, match="not a corrections file"):
        corrections.read(p)
    corrections.write(p, [1, 2], [1, -1], 1, 10, np.uint8)
    blob = open(p, "rb").read()
    open(p, "wb").write(blob[:-1])
    with pytest.raises(corrections.CorrectionsError, match="damaged"):
        corrections.read(p)


def test_select_equals_brute_force_on_random_boxes():
    rng = np.random.default_rng(2)
    for dims in ((37, 53), (9, 14, 11), (6, 7, 8, 3), (5, 1, 9)):
        n = int(np.prod(dims))
        for density in (0.0, 0.05, 1.0):
            mask = rng.random(n) < density
            idx = np.flatnonzero(mask).astype(np.int64)
            q = rng.integers(1, 100, idx.size).astype(np.int32)
            full = np.zeros(n, np.int32)
            full[idx] = q
            full = full.reshape(dims)
            for _ in range(40):
                start = [int(rng.integers(0, d)) for d in dims]
                stop = [int(rng.integers(b + 1, d + 1)) for b, d in zip(start, dims)]
                step = [int(rng.integers(1, 5)) for _ in dims]
                box = full[tuple(slice(b, e, s) for b, e, s in zip(start, stop, step))]
                bi, bq = corrections.select(idx, q, dims, start, stop, step)
                want = np.flatnonzero(box.reshape(-1))
                assert np.array_equal(bi, want) and np.array_equal(bq, box.reshape(-1)[want]), (dims, start, stop, step)
            # the whole array and one element
            bi, bq = corrections.select(idx, q, dims, [0] * len(dims), list(dims), [1] * len(dims))
            assert np.array_equal(bi, idx) and np.array_equal(bq, q)
    idx = np.array([3, 10, 11, 40], np.int64)
    q = np.array([1, 2, 3, 4], np.int32)
    assert [a.tolist() for a in corrections.select_range(idx, q, 10, 40)] == [[10, 11], [2, 3]]
    with pytest.raises(ValueError):
        corrections.select(idx, q, (5, 10), [0], [5], [1])


def _cf(**over):
    opt = config.load(os.path.join(ROOT, "opt", "SingleTask", "error_bound.yaml"))
    return opt, opt.CompressFramework


def test_option_parsing_and_the_shipped_yaml():
    opt, cf = _cf()
    base = config.load(os.path.join(ROOT, "opt", "SingleTask", "default.yaml"))
    assert error_bound_of(base.CompressFramework) is None          # absent: off
    bound = error_bound_of(cf)
    assert isinstance(bound, int) and bound >= 0
    plain, want = config.to_plain(opt), config.to_plain(base)
    assert plain["CompressFramework"]["Compress"].pop("error_bound") == bound
    assert plain == want, "error_bound.yaml is default.yaml plus the one key"
    for off in (None, "none", "None", "null"):
        cf.Compress.error_bound = off
        assert error_bound_of(cf) is None
    for v in (0, 1, 65535):
        cf.Compress.error_bound = v
        assert error_bound_of(cf) == v
    for bad in (-1, 65536, 1.5, "3", True):
        cf.Compress.error_bound = bad
        with pytest.raises(ValueError, match="error_bound"):
            error_bound_of(cf)


def test_unsupported_configurations_are_refused_by_name():
    _, cf = _cf()
    check_error_bound(cf, np.uint16)
    cf8 = config.to_opt(config.to_plain(cf))
    cf8.Decompress.postprocess.clip = [0, 255]
    check_error_bound(cf8, np.uint8)
    with pytest.raises(ValueError, match="float32"):
        check_error_bound(cf, np.float32)
    with pytest.raises(ValueError, match="int16"):
        check_error_bound(cf, np.int16)
    other = config.to_opt(config.to_plain(cf))
    other.Normalize.name = "minmax01"
    with pytest.raises(ValueError, match="minmax01"):
        check_error_bound(other, np.uint16)
    clip = config.to_opt(config.to_plain(cf))
    clip.Decompress.postprocess.clip = [100, 30000]
    with pytest.raises(ValueError, match="postprocess"):
        check_error_bound(clip, np.uint16)
    den = config.to_opt(config.to_plain(cf))
    den.Decompress.postprocess.denoise.level = 500
    with pytest.raises(ValueError, match="postprocess"):
        check_error_bound(den, np.uint16)


def test_a_decoder_never_returns_an_unbounded_volume(tmp_path):
    """side info with error_bound and no (or a foreign) corrections file: every decoder raises, before a device is needed"""
    opt, cf = _cf()
    mod = str(tmp_path / "module")
    os.makedirs(mod)
    side = {"dtype": "uint16", "min": 0.0, "max": 60000.0, "normalized_min": 0.0, "normalized_max": 100.0, "data_shape": [4, 5, 6, 1],
            "phi_features": 16, "phi_name": "SIREN", "error_bound": 3}
    region = (slice(0, 2), slice(0, 5), slice(1, 6))
    with pytest.raises(corrections.CorrectionsError, match="corrections.bin"):
        NFGR.decompress(opt, mod, dict(side))
    with pytest.raises(corrections.CorrectionsError, match="corrections.bin"):
        NFGR.decompress_region(opt, mod, dict(side), region)
    # a file of another artefact (other bound / size / dtype)
    for eps, n, dt in ((4, 120, np.uint16), (3, 121, np.uint16), (3, 120, np.uint8)):
        corrections.write(corrections.path_for(mod), [1], [1], eps, n, dt)
        with pytest.raises(corrections.CorrectionsError, match="does not belong"):
            NFGR.decompress(opt, mod, dict(side))
    # a resampled view of a corrected artefact is refused by name
    corrections.write(corrections.path_for(mod), [1], [1], 3, 120, np.uint16)
    with pytest.raises(ValueError, match="resampled"):
        NFGR.decompress_region(opt, mod, dict(side), region, shape=(8, 10, 12))
    # decode options under which the bound does not hold
    o2 = config.to_opt(config.to_plain(opt))
    o2.CompressFramework.Decompress.postprocess.clip = [100, 30000]
    with pytest.raises(ValueError, match="postprocess"):
        NFGR.decompress(o2, mod, dict(side))
    assert corrections.path_for(os.path.join("a", "compressed", "module")) == os.path.join("a", "compressed", "corrections.bin")
