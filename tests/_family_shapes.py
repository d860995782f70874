"""The launch space of the four network families (FFN, NeRF, MFNFourier / MFNGabor, the tapered SIRENs), one row per shape, for the tests
that compare every path of it with a float64 reference (tests/test_gpu_family_shapes.py on the GPU, tests/test_family_shapes_host.py for
what needs none).

The families share one host driver, csrc/brief_family_host.inc.  What a shape reaches there is arithmetic, restated below and not taken
on trust: the forward instantiation k_<fam>_fwd<MTW, ..> (mtw), the dynamic LDS of that kernel (lds_bytes), the persistent grid
(family_grid), the split-K of the weight gradient (family_ksplit over the 64 x 64 wave jobs of the family's wgrad_block shapes) and
the number of k_<fam>_wgrad launches (wgrad_count over kWgradMax).  A row builds its net through the public module classes, seeded,
and names what it claims to reach; reach() evaluates the restated arithmetic for a CU count and unmet() checks the claims.  The
host file asserts every row's claims for 32, 64, 128 and 256 CUs, the GPU file for the device it runs on.

A new family adds its lds_bytes / wgrad_blocks below and its rows to ROWS.

The references are the torch restatements of tests/_family_ref.py; the bands are the ones the per-family files apply (no band is
defined here)."""
import numpy as np
import torch

from brief_pytorch_amd import networks as N
from tests import _family_ref as R

CU_COUNTS = (32, 64, 128, 256)
KWGRAD_MAX = {"ffn": 32, "nerf": 32, "mfn": 32, "taper": 16}      # FFN_WGRAD_LAYERS, NERF_WGRAD_BLOCKS, MFN_WGRAD_BLOCKS, BRIEF_TAPER_MAX_LAYERS
LDS_BUDGET = 160 * 1024
SPLIT_CAP = 64
LOSSES = [("datal2", False, 0.0), ("datasmoothl1", True, 0.0), ("datal2", True, 0.3)]      # the three settings of the per-family files
BETA = 0.05
# the tapered SIRENs' bands (tests/test_gpu_taper.py) and their widening cap (tests/_bands.py)
TAPER_FWD_TOL, TAPER_LOSS_TOL, TAPER_GRAD_TOL = 2e-5, 1e-4, 1e-4
MAX_WIDENED_FRACTION, MAX_BAND = 0.15, 1e-3


def _up(v, q):
    return (v + q - 1) // q * q


# ---- the driver's launch arithmetic, restated (csrc/brief_family_host.inc and the *_layout functions of the family files)
def family_of(m):
    if isinstance(m, N.FFN):
        return "ffn"
    if isinstance(m, N.NeRF):
        return "nerf"
    if isinstance(m, (N.MFNFourier, N.MFNGabor)):
        return "mfn"
    if isinstance(m, (N.SIREN_Pyramid, N.SIRENFT, N.SIRENPS)):
        return "taper"
    raise TypeError(type(m).__name__)


def tile_count(m):
    """nt of the family's layout: 32-feature tiles of the (widest) hidden width"""
    widest = max(m.widths) if family_of(m) == "taper" else m.features
    return (widest + 31) // 32


def mtw(nt):
    """feature tiles per wave: the MTW of k_<fam>_fwd<MTW, TRAIN, BOX>"""
    return (nt + 3) // 4


def lds_bytes(m):
    """dynamic LDS of k_<fam>_fwd: the register image of one 32-sample tile plus 32 x float4 of coordinates"""
    fam, FP = family_of(m), 32 * tile_count(m)
    if fam == "ffn":
        K0 = 2 * _up(m.embsize, 32)
        return 4 * (32 * max(K0, FP) + 128)
    if fam == "nerf":
        DP = _up(N.NeRF.encoding_width(m.coords_channel, m.frequencies), 8)
        return 4 * (32 * (DP + FP) + 128)
    if fam == "mfn":
        return 4 * (32 * FP + 128)
    return 4 * (1024 * tile_count(m) + 128)


def by_lds(lds):
    return LDS_BUDGET // lds


def family_grid(lds, n, cus):
    """persistent grid: up to two workgroups per CU, fewer when the LDS image does not fit twice"""
    tiles = (n + 31) // 32
    b = by_lds(lds)
    cap = cus * ((b if b > 0 else 1) if b < 2 else 2)
    return min(tiles, cap)


def wgrad_blocks(m):
    """[(arows, brows)] of the family's wgrad_block, in block order: dW[arows][brows] of each block"""
    fam = family_of(m)
    cin, cout, L = m.coords_channel, m.data_channel, m.layers
    if fam == "taper":
        return list(m._shapes)                                             # one block per Linear: (out, in)
    F = m.features
    if fam == "ffn":
        K0 = 2 * _up(m.embsize, 32)
        return [(cout, F) if l == L - 1 else ((F, K0) if l == 0 else (F, F)) for l in range(L)]
    if fam == "nerf":
        d = N.NeRF.encoding_width(cin, m.frequencies)
        sl = (L - 1) // 2 if m.skip else 0
        count = L + (1 if m.skip else 0)
        out = []
        for i in range(count):
            if i == 0:
                out.append((F, d))
            elif i == count - 1:
                out.append((cout, F))
            else:
                out.append((F, d) if sl and i == sl else (F, F))           # the skip layer's encoding columns are a block of their own
        return out
    per = 2 if m.GABOR else 1
    out = [(F, F)] * (L - 2) + [(cout, F)]
    for _ in range(L - 1):
        out += [(F, cin)] + ([(F, cin + 2)] if per == 2 else [])           # Wf / bf, then Gabor's mu / gamma
    return out


def wgrad_count(m):
    return len(wgrad_blocks(m))


def wave_jobs(m):
    """64 x 64 wave jobs of all weight-gradient blocks: mb x nb per block"""
    return sum(((a + 63) // 64) * ((b + 63) // 64) for a, b in wgrad_blocks(m))


def family_ksplit(npad, waves, cus):
    """(ns, chunk, nsplit): about eight workgroups per CU, at most 64 splits and at least 256 samples each"""
    wgs = (waves + 3) // 4
    ns = (8 * cus + wgs - 1) // wgs
    ns = min(ns, SPLIT_CAP, npad // 256)
    ns = max(ns, 1)
    chunk = _up(npad // ns, 32)
    return ns, chunk, (npad + chunk - 1) // chunk


def reach(m, n, cus):
    """what a net and a batch of n samples reach in the driver on a device of `cus` CUs"""
    nt, lds, npad = tile_count(m), lds_bytes(m), _up(n, 32)
    ns, chunk, nsplit = family_ksplit(npad, wave_jobs(m), cus)
    tiles, grid = npad // 32, family_grid(lds, n, cus)
    blocks = wgrad_count(m)
    return {"nt": nt, "mtw": mtw(nt), "lds": lds, "by_lds": by_lds(lds), "tiles": tiles, "grid": grid, "npad": npad,
            "last_lanes": n - 32 * (tiles - 1), "waves": wave_jobs(m), "ns": ns, "chunk": chunk, "nsplit": nsplit,
            "last_chunk": npad - chunk * (nsplit - 1), "blocks": blocks,
            "launches": (blocks + KWGRAD_MAX[family_of(m)] - 1) // KWGRAD_MAX[family_of(m)],
            "layers": m.layers, "cin": m.coords_channel, "cout": m.data_channel,
            "widest": max(m.widths) if family_of(m) == "taper" else m.features}


# what a row may claim, as predicates over reach()
CLAIMS = {
    "mtw": lambda f, v: f["mtw"] == v,
    "ragged_waves": lambda f, v: (f["nt"] % 4 == 1) == v,                 # wave 0 owns MTW tiles, the other waves MTW - 1
    "partial_k": lambda f, v: (f["widest"] % 8 != 0) == v,                # the last K step of a layer holds fewer than 8 features
    "tiles": lambda f, v: f["tiles"] == v,
    "last_lanes": lambda f, v: f["last_lanes"] == v,                      # samples of the last tile
    "ns": lambda f, v: f["ns"] == v,
    "ragged_chunk": lambda f, v: (f["last_chunk"] < f["chunk"]) == v,
    "nsplit_lt_ns": lambda f, v: (f["nsplit"] < f["ns"]) == v,
    "ns_cap": lambda f, v: (f["ns"] == SPLIT_CAP) == v,                   # the 64 cap decides ns
    "nsplit_cap": lambda f, v: (f["nsplit"] == SPLIT_CAP) == v,           # ... and 64 splits are launched
    "second_tile": lambda f, v: (f["tiles"] > f["grid"]) == v,            # a workgroup walks a second tile
    "uneven_walk": lambda f, v: (f["tiles"] % f["grid"] != 0) == v,       # ... and not all walk as many
    "two_wgs_per_cu": lambda f, v: (f["by_lds"] >= 2) == v,
    "by_lds": lambda f, v: f["by_lds"] == v,
    "launches": lambda f, v: f["launches"] == v,                          # k_<fam>_wgrad launches
    "layers": lambda f, v: f["layers"] == v,
    "cin_cout": lambda f, v: (f["cin"], f["cout"]) == v,
}


def unmet(claims, facts):
    """[] or the claims that do not hold"""
    return ["%s=%r" % (k, v) for k, v in claims.items() if not CLAIMS[k](facts, v)]


class Row:
    """one case: a seeded net of a public module class, a batch size, a loss setting and the claims.  `n` is the batch size on a 256-CU
    device; where the claims do not hold for it on another CU count, batch_n() searches the arithmetic for one where they do.
    `n` may be a function of the CU count."""

    def __init__(self, rid, cls, kwargs, n, li, claims, widths=None, seed=7):
        self.id, self.cls, self.kwargs, self.n, self.li, self.claims, self.widths, self.seed = rid, cls, kwargs, n, li, claims, widths, seed

    def make(self, device=None):
        torch.manual_seed(self.seed)
        m = self.cls(**self.kwargs)
        if self.widths is not None:
            assert m.widths == self.widths, (self.id, m.widths)
        return m if device is None else m.to(device)

    def batch_n(self, m, cus):
        n = self.n(cus) if callable(self.n) else self.n
        if not unmet(self.claims, reach(m, n, cus)):
            return n
        for tiles in range(1, 4097):                                       # keep the batch's shape: the same number of samples in the last tile
            cand = 32 * (tiles - 1) + (n - 1) % 32 + 1
            if not unmet(self.claims, reach(m, cand, cus)):
                return cand
        raise AssertionError("%s: no batch size reaches %s on %d CUs" % (self.id, self.claims, cus))

    def batch(self, m, n):
        """coordinates, targets, weights (ones when the loss setting is unweighted): the generator of the per-family train tests, with the
        samples at which the reference is discontinuous (close_calls) drawn again, from a generator of their own, until none is left"""
        key = (self.id, n)
        if key not in _BATCH:
            x = R.rand_coords(n, m.coords_channel, 11)
            g = torch.Generator().manual_seed(5)
            y = torch.rand(n, m.data_channel, generator=g)
            w = torch.rand(n, m.data_channel, generator=g) * 3 + 0.5
            again = torch.Generator().manual_seed(12)
            for _ in range(64):
                bad = close_calls(self, m, x)
                if not bad.any():
                    break
                x[bad] = torch.rand(int(bad.sum()), m.coords_channel, generator=again) * 2 - 1
            else:
                raise AssertionError("%s: no batch without a close call" % self.id)
            _BATCH[key] = (x, y, w if LOSSES[self.li][1] else torch.ones(n, m.data_channel))
        return _BATCH[key]


_BATCH = {}


def close_calls(row, m, x):
    """[n] bool: the samples at which the float64 reference sits so close to a discontinuity of the gradient that fp32 arithmetic inside
    the forward band may land on its other side: a ReLU whose argument z is within the band of 0 (FFN, NeRF), an output within the band
    of the loss threshold (yhat <= thr replaces the weight by 1).  There the gradient of one sample changes by its whole size, either
    value is a right answer in fp32, and no band on the gradient can hold.  `The band` is the forward band of the family applied to the
    quantity itself: BAND_FACTOR x |torch fp32 - float64| + FLOOR x max |float64| over the batch (the tapered SIRENs: 2e-5 of max |y|).
    A condition on the reference alone: nothing here comes from a kernel."""
    fam, thr = family_of(m), LOSSES[row.li][2]
    fn = _TORCH.get(row.cls, R.torch_taper)
    t64, t32 = ([], []) if fam in ("ffn", "nerf") else (None, None)
    with torch.no_grad():
        y64, y32 = (fn(m, x, dt, *([t] if t is not None else []))[0] for dt, t in ((torch.float64, t64), (torch.float32, t32)))
    band = lambda a64, a32: R.BAND_FACTOR * float((a32.double() - a64).abs().max()) + R.FLOOR * float(a64.abs().max())
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    for z64, z32 in zip(t64 or [], t32 or []):
        bad |= (z64.abs() <= band(z64, z32)).any(1)
    if thr != 0:
        margin = TAPER_FWD_TOL * float(y64.abs().max()) if fam == "taper" else band(y64, y32)
        bad |= ((y64 - thr).abs() <= margin).any(1)
    return bad


W_A = [5, 133, 261, 389, 517, 645, 773, 901, 1024]      # nt = 1, 5, .., 29 (4 MTW - 3), then the full 32; none but the last a multiple of 8
N_B = [1, 31, 32, 33, 255, 256, 257, 513, 2561]


def _rows():
    rows = []
    add = lambda *a, **k: rows.append(Row(*a, **k))
    # a. every MTW, ragged wave ownership, partial last K step; one hidden layer; n = 65: two full tiles and one sample
    for i, F in enumerate(W_A):
        cl = {"mtw": min(i + 1, 8), "ragged_waves": F != 1024, "partial_k": F != 1024, "tiles": 3, "last_lanes": 1}
        cc = dict(coords_channel=(3, 2)[i % 2], data_channel=(1, 2, 3)[i % 3])
        add("a-ffn-%d" % F, N.FFN, dict(cc, features=F, layers=3, embsize=16), 65, i % 3, cl)
        add("a-nerf-%d" % F, N.NeRF, dict(cc, features=F, layers=3, frequencies=4, skip=True), 65, (i + 1) % 3, cl)
        add("a-mfnf-%d" % F, N.MFNFourier, dict(cc, features=F, layers=3, output_act=bool(i % 2)), 65, (i + 2) % 3, cl)
        add("a-mfng-%d" % F, N.MFNGabor, dict(cc, features=F, layers=3, output_act=not i % 2), 65, i % 3, cl)
        if i % 3 == 0:
            dis = 30 if F > 60 else 1
            add("a-pyr-%d" % F, N.SIREN_Pyramid, dict(cc, features=F, features_dis=dis, layers=4), 65, (i + 1) % 3, cl, widths=[F, F - dis, F - 2 * dis])
        elif i % 3 == 1:
            add("a-ft-%d" % F, N.SIRENFT, dict(cc, features=F / 2.0, ratio=2, layers=4), 65, (i + 1) % 3, cl, widths=[F, F // 2, F // 2])
        else:
            f = (F + 0.5) / 2.25
            add("a-ps-%d" % F, N.SIRENPS, dict(cc, features=f, ratio=1.5, layers=4), 65, (i + 1) % 3, cl, widths=[F, int(f * 1.5), int(f)])
    # b. batch edges on one narrow net per family
    narrow = [("ffn", N.FFN, dict(features=40, layers=3, embsize=16)),
              ("nerf", N.NeRF, dict(features=40, layers=3, frequencies=4, skip=True)),
              ("mfng", N.MFNGabor, dict(features=40, layers=3)),
              ("pyr", N.SIREN_Pyramid, dict(features=40, features_dis=5, layers=4))]
    for k, (tag, cls, kw) in enumerate(narrow):
        for i, n in enumerate(N_B):
            cl = {"tiles": (n + 31) // 32, "last_lanes": (n - 1) % 32 + 1}
            if n <= 257:
                cl["ns"] = 1
            if n == 513:
                cl.update(ns=2, ragged_chunk=True)
            if n == 2561:
                cl = {"last_lanes": 1, "nsplit_lt_ns": True}
            add("b-%s-n%d" % (tag, n), cls, kw, n, (i + k) % 3, cl)
    # c. a persistent loop that walks a second tile, with ns at the cap; the cap in nsplit as well; the LDS-limited grid
    for k, (tag, cls, kw) in enumerate(narrow + [("mfnf", N.MFNFourier, dict(features=40, layers=3))]):
        add("c-%s-walk" % tag, cls, kw, 20001, k % 3, {"second_tile": True, "uneven_walk": True, "two_wgs_per_cu": True, "ns_cap": True, "last_lanes": 1})
    add("c-ffn-cap64", N.FFN, narrow[0][2], 20449, 1, {"second_tile": True, "two_wgs_per_cu": True, "nsplit_cap": True, "last_lanes": 1})
    add("c-ffn-lds", N.FFN, dict(features=40, layers=3, embsize=512), lambda cus: 32 * cus + 33, 2,
        {"by_lds": 1, "second_tile": True, "uneven_walk": True, "last_lanes": 1})
    # d. more than kWgradMax weight-gradient blocks: a second k_<fam>_wgrad launch
    add("d-ffn-34", N.FFN, dict(features=40, layers=34, embsize=16), 65, 0, {"launches": 2, "layers": 34})
    add("d-nerf-33", N.NeRF, dict(features=40, layers=33, frequencies=4, skip=True), 65, 1, {"launches": 2, "layers": 33})
    add("d-mfng-12", N.MFNGabor, dict(features=40, layers=12), 65, 2, {"launches": 2, "layers": 12})
    add("d-mfnf-18", N.MFNFourier, dict(features=40, layers=18), 65, 0, {"launches": 2, "layers": 18})
    # e. envelope corners
    add("e-pyr-16", N.SIREN_Pyramid, dict(features=40, features_dis=2, layers=16), 65, 0, {"layers": 16, "launches": 1}, widths=list(range(40, 11, -2)))
    add("e-ps-16", N.SIRENPS, dict(features=3.0, ratio=1.3, layers=16), 65, 1, {"layers": 16, "launches": 1},
        widths=[int(3.0 * 1.3 ** (14 - i)) for i in range(15)])
    add("e-ft-16", N.SIRENFT, dict(features=20.0, ratio=2, layers=16), 65, 2, {"layers": 16, "launches": 1}, widths=[40] + [20] * 14)
    add("e-pyr-3-c24", N.SIREN_Pyramid, dict(coords_channel=2, data_channel=4, features=40, features_dis=7, layers=3), 65, 1,
        {"layers": 3, "cin_cout": (2, 4)}, widths=[40, 33])
    add("e-nerf-f16-1024", N.NeRF, dict(data_channel=4, features=1024, layers=3, frequencies=16, skip=True), 65, 2, {"mtw": 8, "by_lds": 1})
    add("e-ffn-e512-1024", N.FFN, dict(features=1024, layers=2, embsize=512), 65, 1, {"mtw": 8, "layers": 2, "by_lds": 1})
    c24 = dict(coords_channel=2, data_channel=4)
    add("e-ffn-c24", N.FFN, dict(c24, features=40, layers=3, embsize=16), 65, 0, {"cin_cout": (2, 4)})
    add("e-nerf-c24", N.NeRF, dict(c24, features=40, layers=3, frequencies=4, skip=True), 65, 1, {"cin_cout": (2, 4)})
    add("e-mfnf-c24", N.MFNFourier, dict(c24, features=40, layers=3), 65, 2, {"cin_cout": (2, 4)})
    add("e-mfng-c24", N.MFNGabor, dict(c24, features=40, layers=3), 65, 0, {"cin_cout": (2, 4)})
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
DEEP = [r for r in ROWS if r.id.startswith("d-")]
TAPER = [r for r in ROWS if issubclass(r.cls, N._TaperBase)]


def kernel_family(row):
    """the forward kernel a row's class selects: k_ffn_fwd, k_nerf_fwd, k_mfn_fwd<Fourier>, k_mfn_fwd<Gabor> or k_taper_fwd"""
    if row.cls is N.MFNFourier:
        return "mfnf"
    if row.cls is N.MFNGabor:
        return "mfng"
    return {N.FFN: "ffn", N.NeRF: "nerf"}.get(row.cls, "taper")


# ---- the float64 / float32 reference of a row
_TORCH = {N.FFN: R.torch_ffn, N.NeRF: R.torch_nerf, N.MFNFourier: R.torch_mfn, N.MFNGabor: R.torch_mfn}
_REF = {}


def _comparisons(m):
    """[(name, key, offset, shape, column slice)]: every parameter tensor's window in the canonical gradient buffer, the skip layer of a
    NeRF as its two halves (the encoding and the hidden columns come from different weight-gradient blocks).  key indexes the leaves."""
    out = []
    if family_of(m) == "mfn":
        for k, o, shp in m._entries:
            out.append((k, k, o, tuple(shp), slice(None)))
        return out
    off = m.bv_count
    d = N.NeRF.encoding_width(m.coords_channel, m.frequencies) if family_of(m) == "nerf" else 0
    for l, (o, i) in enumerate(m._shapes):
        if family_of(m) == "nerf" and l == m.skip_layer:
            out += [("weight %d encoding half" % l, 2 * l, off, (o, i), slice(0, d)), ("weight %d hidden half" % l, 2 * l, off, (o, i), slice(d, i))]
        else:
            out.append(("weight %d" % l, 2 * l, off, (o, i), slice(None)))
        out.append(("bias %d" % l, 2 * l + 1, off + o * i, (o,), slice(None)))
        off += o * i + o
    assert off == m.param_count
    return out


def reference(row, n):
    """{dtype: (forward [n, cout], loss, {key: gradient})} of the row's net on the row's batch, float64 and float32, and the comparisons
    of _comparisons(); computed once per (row, n) for the nets small enough to keep"""
    key = (row.id, n)
    if key in _REF:
        return _REF[key]
    m = row.make()
    fn = _TORCH.get(row.cls, R.torch_taper)
    x, y, w = row.batch(m, n)
    loss, _, thr = LOSSES[row.li]
    res = {}
    for dt in (torch.float64, torch.float32):
        yh, leaves = fn(m, x, dt)
        lt = R.torch_loss(yh, y.to(dt), w.to(dt), loss, thr, BETA)
        lt.backward()
        items = leaves.items() if isinstance(leaves, dict) else enumerate(leaves)
        res[dt] = (yh.detach().numpy(), lt.item(), {k: v.grad.numpy() for k, v in items})
    out = (res, _comparisons(m))
    if m.param_count <= 1 << 18:
        _REF[key] = out
    return out


def taper_owns(row, n):
    """3 x own of every gradient comparison of a tapered row: own = relerr(torch fp32, torch float64) of the tensor (no GPU involved)"""
    res, comps = reference(row, n)
    return [3.0 * R.relerr(res[torch.float32][2][k][..., sl], res[torch.float64][2][k][..., sl]) for _, k, _, _, sl in comps]


def box_plan(cin):
    """(dims, start, stop, step) of the small box decode of a row"""
    return ((5, 6, 7), (1, 0, 2), (5, 6, 7), (2, 1, 3)) if cin == 3 else ((11, 19), (2, 1), (11, 19), (3, 2))


def np_max(a):
    return float(np.max(np.abs(np.asarray(a, np.float64))))
