"""The kernel variants behind the C-ABI entries, one row per kernel the library can reach, for the tests of what every kernel implements in
its own copy of the code: the integer epilogue, the sample sources and the external loss (tests/test_gpu_entry_contract.py on the GPU,
tests/test_entry_contract_host.py for the arithmetic that needs none).

A row builds its net through the public module classes and names the kernel it reaches for decode and for a train step.  For SIREN the
names are not taken on trust: siren_kernels() restates the dispatch of csrc/brief_hip.hip (launch_fused, use_small, launch_k16) and
csrc/brief_layout.h (brief_nt, brief_use_lean, brief_use_wide), and the host file asserts that every SIREN row reaches what it says.
The families have one forward kernel each (csrc/brief_family_host.inc), selected by the module class.

Also here, because both files need it: the float32 restatement of the reference's invnormalize_data and the search over the oracle's
epilogue for the inputs at which an epilogue can go wrong (edge_values)."""
import math

import numpy as np
import torch

from brief_pytorch_amd import networks as N
from oracle import oracle as O

# the value ranges of the integer decodes: neither starts at 0 and neither span is a power of two, so a reciprocal multiply, a fused
# multiply-add and double arithmetic all change results (tests/test_entry_contract_host.py measures how many)
VRANGE = {"u16": (17261.0, 26923.0), "u8": (3.0, 250.0)}
SIDE = {k: {"dtype": {"u16": "uint16", "u8": "uint8"}[k], "min": v[0], "max": v[1]} for k, v in VRANGE.items()}
NP_DTYPE = {"u16": np.uint16, "u8": np.uint8}

# forward bands of the project: fp32, bf16x3 and the families (header of tests/test_gpu_parity.py); bf16 (tests/test_gpu_bf16.py)
BAND_F32, BAND_BF16 = 2e-5, 3e-2


# ---- the SIREN dispatch, restated (csrc/brief_layout.h, csrc/brief_hip.hip)
def siren_nt(features, precision="fp32"):
    """brief_nt: 32-feature tiles of the padded width"""
    nt = (features + 31) // 32
    if precision == "bf16":
        return 8 if nt <= 8 else 16
    if precision == "bf16x3":
        return 8
    return nt


def siren_kernels(features, layers, precision="fp32", cout=1):
    """(decode kernel, train kernel) of a SIREN"""
    nt = siren_nt(features, precision)
    if precision == "bf16x3":
        return "k_fused_x3", "k_fused_x3"
    if precision == "bf16":
        k = "k16<%d,CO=%d>" % (nt, 1 if cout == 1 else 4)
        return k, k
    if nt > 32:                                                        # brief_use_wide
        return "k_wide", "k_wide"
    lean_train = (nt >= 5 and nt != 8) or nt == 3                      # brief_use_lean(d, true), BRIEF_LEAN3 = 1
    lean_decode = 5 <= nt <= 7 or (nt >= 9 and nt not in (12, 16))     # brief_use_lean(d, false)
    small = nt <= 2 and layers - 2 <= 7                                # use_small
    fused = "k_fused<%d>" % nt
    return ("k_lean" if lean_decode else fused), ("k_small" if small else ("k_lean" if lean_train else fused))


class Variant:
    """one row: `make()` builds the seeded net on the CPU (move it with .to)"""

    def __init__(self, vid, cls, decode_kernel, train_kernel, seed, band=BAND_F32, **kwargs):
        self.id, self.cls, self.decode_kernel, self.train_kernel = vid, cls, decode_kernel, train_kernel
        self.seed, self.band, self.kwargs = seed, band, kwargs
        self.cin, self.cout = kwargs["coords_channel"], kwargs["data_channel"]
        self.output_act = bool(kwargs.get("output_act", False))
        self.siren = cls is N.SIREN

    @property
    def label(self):
        """the pytest id: the row and the kernel(s) it reaches, decode then train (k_fused<1> is spelt k_fused_1)"""
        ks = [self.decode_kernel] + ([self.train_kernel] if self.train_kernel != self.decode_kernel else [])
        plain = lambda k: k.replace("<", "_").replace(">", "").replace(",", "_").replace("=", "")
        return "-".join([self.id] + [plain(k) for k in ks])

    def make(self, device=None):
        torch.manual_seed(self.seed)
        m = self.cls(**self.kwargs)
        return m if device is None else m.to(device)


def _siren(vid, seed, L, F, cin, cout, decode, train, band=BAND_F32, **kw):
    return Variant(vid, N.SIREN, decode, train, seed, band, coords_channel=cin, data_channel=cout, features=F, layers=L, w0=20, **kw)


VARIANTS = [
    _siren("s22", 1, 4, 22, 3, 1, "k_fused<1>", "k_small"),
    _siren("s100", 2, 4, 100, 2, 3, "k_fused<4>", "k_fused<4>"),
    _siren("s200", 3, 3, 200, 3, 2, "k_lean", "k_lean"),                                  # 7 tiles
    _siren("s256", 4, 4, 256, 3, 1, "k_fused<8>", "k_fused<8>", output_act=True),
    _siren("s300", 5, 3, 300, 3, 4, "k_lean", "k_lean"),                                  # 10 tiles: two left-over tiles shared along K
    _siren("s384", 6, 3, 384, 3, 1, "k_fused<12>", "k_lean"),
    _siren("s1100", 7, 3, 1100, 3, 1, "k_wide", "k_wide"),                                # scratch through the module
    _siren("b96", 8, 4, 96, 3, 3, "k16<8,CO=4>", "k16<8,CO=4>", band=BAND_BF16, precision="bf16"),
    _siren("x96", 9, 4, 96, 3, 1, "k_fused_x3", "k_fused_x3", precision="bf16x3"),
    Variant("ffn", N.FFN, "k_ffn_fwd", "k_ffn_fwd", 10, coords_channel=2, data_channel=3, features=70, embsize=40, layers=4),
    Variant("nerf", N.NeRF, "k_nerf_fwd", "k_nerf_fwd", 11, coords_channel=3, data_channel=2, features=48, frequencies=4, layers=5, skip=True),
    Variant("mfnf", N.MFNFourier, "k_mfn_fwd<Fourier>", "k_mfn_fwd<Fourier>", 12, coords_channel=3, data_channel=4, features=40, layers=4),
    Variant("mfng", N.MFNGabor, "k_mfn_fwd<Gabor>", "k_mfn_fwd<Gabor>", 13, coords_channel=3, data_channel=4, features=40, layers=4,
            output_act=True),
    Variant("pyr", N.SIREN_Pyramid, "k_taper_fwd", "k_taper_fwd", 14, coords_channel=3, data_channel=1, features=45, features_dis=7, layers=5,
            w0=20),
    Variant("ps", N.SIRENPS, "k_taper_fwd", "k_taper_fwd", 15, coords_channel=2, data_channel=3, features=14.2, ratio=1.5, layers=5, w0=20,
            output_act=True),
]
BY_ID = {v.id: v for v in VARIANTS}
FAMILY_ABI = {"ffn": "brief_ffn_", "nerf": "brief_nerf_", "mfnf": "brief_mfn_", "mfng": "brief_mfn_", "pyr": "brief_taper_", "ps": "brief_taper_"}


# ---- the modules' own parameter windows
def param_views(m):
    """[(name, _ParamView)] of every window a module offers into its canonical buffer, in buffer order"""
    out = []
    if hasattr(m, "fourierfeature_embedding"):
        out.append(("bvals", m.fourierfeature_embedding.bvals))
    if hasattr(m, "net"):
        for l, seq in enumerate(m.net):
            out += [("net.%d.weight" % l, seq[0].weight), ("net.%d.bias" % l, seq[0].bias)]
    else:      # the MFNs
        for i, lin in enumerate(m.linear):
            out += [("linear.%d.weight" % i, lin.weight), ("linear.%d.bias" % i, lin.bias)]
        out += [("output_linear.weight", m.output_linear.weight), ("output_linear.bias", m.output_linear.bias)]
        for i, f in enumerate(m.filters):
            if hasattr(f, "mu"):
                out += [("filters.%d.mu" % i, f.mu), ("filters.%d.gamma" % i, f.gamma)]
            out += [("filters.%d.linear.weight" % i, f.linear.weight), ("filters.%d.linear.bias" % i, f.linear.bias)]
    out.sort(key=lambda kv: kv[1]._off)
    return out


def head_bias(m):
    return m.net[-1][0].bias if hasattr(m, "net") else m.output_linear.bias


# ---- the reference's epilogue and the inputs at which a copy of it can go wrong
def np_epilogue_float(y, kind, scale_min, scale_max):
    """utils/io.py:136-147 of the reference on float32, as torch evaluates it, up to the cast: every python scalar becomes a float32 (the
    window's width is subtracted in double first) and every operation rounds once"""
    vmin, vmax = VRANGE[kind]
    t = np.asarray(y, np.float32) - np.float32(scale_min)
    t = t / np.float32(np.float64(scale_max) - np.float64(scale_min))
    t = np.clip(t, np.float32(0), np.float32(1))
    return t * np.float32(vmax - vmin) + np.float32(vmin)


def np_invnormalize(y, kind, scale_min, scale_max):
    """... and np.array(.., dtype) truncates"""
    return np_epilogue_float(y, kind, scale_min, scale_max).astype(NP_DTYPE[kind])


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _from_bits(b):
    return np.int32(b).view(np.float32)


def edge_values(kind, scale=(0.0, 100.0), want=4):
    """Inputs of the epilogue for `scale` and VRANGE[kind], found by bisection over the float32 bit patterns of the ORACLE's epilogue (it is
    monotone: every step rounds to nearest):
        "clip_lo" / "clip_hi"   scale_min / scale_max themselves, their float neighbours outside the window and one value far outside
        "below"                 `want` values whose pre-truncation float u is the largest float32 below an integer k (truncates to k - 1)
        "at"                    `want` values whose u is that integer k itself
    Returns {name: float32 array}; below[i] and at[i] are neighbouring floats around the same k."""
    smin, smax = np.float32(scale[0]), np.float32(scale[1])
    vmin, vmax = VRANGE[kind]
    assert 0 <= smin < smax, "the bisection walks positive float32 bit patterns"
    out = {"clip_lo": np.array([smin, np.nextafter(smin, np.float32(-np.inf)), smin - np.float32(1e6)], np.float32),
           "clip_hi": np.array([smax, np.nextafter(smax, np.float32(np.inf)), smax + np.float32(1e6)], np.float32)}
    code = O.invnormalize      # the oracle decides what an input truncates to
    below, at = [], []
    ks = np.linspace(vmin + 1, vmax - 1, 4 * want + 3).astype(np.int64)[1:-1]
    for k in ks:
        lo, hi = _bits(smin), _bits(smax)      # code(lo) = vmin < k <= vmax = code(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(code(np.array([_from_bits(mid)], np.float32), SIDE[kind], float(smin), float(smax))[0]) >= k:
                hi = mid
            else:
                lo = mid
        y_lo, y_hi = _from_bits(lo), _from_bits(hi)
        u_lo, u_hi = np_epilogue_float([y_lo], kind, smin, smax)[0], np_epilogue_float([y_hi], kind, smin, smax)[0]
        if u_lo == np.nextafter(np.float32(k), np.float32(0)) and u_hi == np.float32(k) and len(below) < want:
            below.append(y_lo)
            at.append(y_hi)
    out["below"], out["at"] = np.array(below, np.float32), np.array(at, np.float32)
    return out


def is_power_of_two(x):
    m, _ = math.frexp(float(x))
    return m == 0.5
