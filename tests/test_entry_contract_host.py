"""The arithmetic behind tests/test_gpu_entry_contract.py that needs no GPU.

1. The oracle's epilogue (oracle_invnormalize, the reference of every integer-decode comparison) equals a plain float32 restatement of the
   reference's invnormalize_data (utils/io.py:136-147) on 2^18 samples for four parameter sets.
2. The search for the inputs at which an epilogue goes wrong (tests/_variants.py: edge_values) finds what the GPU file feeds the kernels: the
   clip edges, and for both value ranges at least four inputs whose pre-truncation float is the largest float32 below an integer, next to
   the inputs that give the integer itself.
3. The parameter sets of the integer-decode comparison tell a right epilogue from the likely wrong ones.  With the u16 range (17261, 26923)
   a reciprocal multiply, a fused multiply-add, all-double arithmetic and round-to-nearest each change samples; with vmin = 0 or a
   power-of-two window some of them change nothing, which is why the ranges are what they are.  The u8 range (3, 250) has a span of 247
   against float32 steps of 2^-17 .. 2^-16 below 256: the first three variants move the pre-truncation float by at most one such step, which
   crosses an integer too rarely to count on; u8 is sensitive to the rounding MODE only (asserted), and the u16 case carries the others.
4. Every SIREN row of the variant list reaches the kernel its id states, by the restated dispatch of csrc/brief_hip.hip / brief_layout.h."""
import numpy as np
import pytest

from oracle import oracle as O

from . import _variants as V

N = 1 << 18


def _uniform(lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, size=N).astype(np.float32)


@pytest.mark.parametrize("kind,scale", [("u16", (0.0, 100.0)), ("u8", (0.0, 100.0)), ("u16", (-0.3712, 0.4189)), ("u8", (1.5, 97.25))])
def test_oracle_epilogue_is_the_references_float32_arithmetic(kind, scale):
    smin, smax = float(np.float32(scale[0])), float(np.float32(scale[1]))
    w = smax - smin
    y = _uniform(smin - w / 4, smax + w / 4, 11)
    y[:4] = [smin, smax, np.nextafter(np.float32(smin), np.float32(-np.inf)), np.nextafter(np.float32(smax), np.float32(np.inf))]
    ref = V.np_invnormalize(y, kind, smin, smax)
    assert np.array_equal(O.invnormalize(y, V.SIDE[kind], smin, smax), ref)
    vmin, vmax = V.VRANGE[kind]
    assert ref.min() == vmin and ref.max() == vmax and (ref == vmin).mean() > 0.1 and (ref == vmax).mean() > 0.1


@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_edge_value_search(kind):
    e = V.edge_values(kind)
    vmin, vmax = V.VRANGE[kind]
    side = V.SIDE[kind]
    assert len(e["below"]) >= 4 and len(e["at"]) == len(e["below"])
    u_below, u_at = V.np_epilogue_float(e["below"], kind, 0.0, 100.0), V.np_epilogue_float(e["at"], kind, 0.0, 100.0)
    k = O.invnormalize(e["at"], side).astype(np.int64)
    assert np.all(u_at == k) and np.all(vmin < k) and np.all(k < vmax) and len(set(k.tolist())) == len(k)
    assert np.all(u_below == np.nextafter(k.astype(np.float32), np.float32(0)))              # the largest float32 below k ...
    assert np.array_equal(O.invnormalize(e["below"], side).astype(np.int64), k - 1)        # ... truncates to k - 1 (rounding would give k)
    assert np.all(e["at"] == np.nextafter(e["below"], np.float32(np.inf)))
    assert np.all(O.invnormalize(e["clip_lo"], side) == vmin) and np.all(O.invnormalize(e["clip_hi"], side) == vmax)
    assert e["clip_lo"][0] == 0.0 and e["clip_lo"][1] < 0.0 and e["clip_lo"][2] < -1e5
    assert e["clip_hi"][0] == 100.0 and e["clip_hi"][1] > 100.0 and e["clip_hi"][2] > 1e5


def _wrong_epilogues(y, kind, smin, smax):
    """the likely wrong copies of the epilogue, each on float32 inputs -> integers"""
    vmin, vmax = V.VRANGE[kind]
    f32, f64 = np.float32, np.float64
    den, span, fmin = f32(f64(smax) - f64(smin)), f32(vmax - vmin), f32(vmin)
    clip = lambda t: np.clip(t, t.dtype.type(0), t.dtype.type(1))
    dt = V.NP_DTYPE[kind]
    t = clip((y - f32(smin)) / den)
    out = {}
    out["reciprocal"] = (clip((y - f32(smin)) * (f32(1) / den)) * span + fmin).astype(dt)
    out["fma"] = (t.astype(f64) * f64(span) + f64(fmin)).astype(f32).astype(dt)              # the product is exact in double: one rounding
    out["double"] = (clip((y.astype(f64) - smin) / (f64(smax) - f64(smin))) * (vmax - vmin) + vmin).astype(dt)
    out["round"] = np.rint(t * span + fmin).astype(dt)
    return out


def test_u16_parameters_tell_the_wrong_epilogues_apart():
    y = _uniform(-25.0, 125.0, 12)
    right = O.invnormalize(y, V.SIDE["u16"], 0.0, 100.0)
    changed = {k: int((v != right).sum()) for k, v in _wrong_epilogues(y, "u16", 0.0, 100.0).items()}
    print("u16 (0, 100) / (17261, 26923): samples of 2^18 changed by each wrong epilogue:", changed)
    for k, c in changed.items():
        assert c >= 10, (k, changed)


def test_u8_parameters_tell_the_rounding_mode_apart():
    y = _uniform(-25.0, 125.0, 13)
    right = O.invnormalize(y, V.SIDE["u8"], 0.0, 100.0)
    changed = {k: int((v != right).sum()) for k, v in _wrong_epilogues(y, "u8", 0.0, 100.0).items()}
    print("u8 (0, 100) / (3, 250): samples of 2^18 changed by each wrong epilogue:", changed)
    assert changed["round"] >= 10, changed


def test_every_siren_row_reaches_the_kernel_it_states():
    seen = set()
    for v in V.VARIANTS:
        assert v.id not in seen
        seen.add(v.id)
        if not v.siren:
            assert v.cls._abi == V.FAMILY_ABI[v.id]
            continue
        kw = v.kwargs
        assert V.siren_kernels(kw["features"], kw["layers"], kw.get("precision", "fp32"), kw["data_channel"]) == (v.decode_kernel, v.train_kernel), v.id
    # the restated rule at the thresholds between two kernels
    assert V.siren_kernels(64, 9)[1] == "k_small" and V.siren_kernels(64, 10)[1] == "k_fused<2>" and V.siren_kernels(65, 4)[1] == "k_lean"
    assert V.siren_kernels(1024, 3) == ("k_lean", "k_lean") and V.siren_kernels(1025, 3) == ("k_wide", "k_wide")
    assert V.siren_kernels(512, 3) == ("k_fused<16>", "k_lean") and V.siren_kernels(96, 4) == ("k_fused<3>", "k_lean")


def test_variant_modules_offer_their_whole_buffer_as_windows():
    """param_views() walks every window of a module: together they tile the canonical buffer, so zeroing them zeroes the net"""
    for v in V.VARIANTS:
        m = v.make()
        off = 0
        for name, pv in V.param_views(m):
            assert pv._off == off, (v.id, name)
            off += pv.numel()
        assert off == m.params.numel() == m.param_count, v.id
        hb = V.head_bias(m)
        assert hb.numel() == v.cout and m.data_channel == v.cout and m.coords_channel == v.cin and m.output_act == v.output_act
