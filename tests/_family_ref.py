"""The torch restatements of the four network families (FFN, NeRF, MFNFourier / MFNGabor, the tapered SIRENs), the loss of main.py:176-191
and the band the FFN, NeRF and MFN tests share: one copy for tests/test_gpu_ffn.py, test_gpu_nerf.py, test_gpu_mfn.py, test_gpu_taper.py
and the launch-space tests (tests/_family_shapes.py).

Every restatement takes the module's own parameters, evaluates the reference's forward at `dtype` (float64: the reference of a band;
float32: what plain torch gets, the yardstick the band is a multiple of) and returns the output with the leaf tensors, so a caller
can take gradients."""
import math

import numpy as np
import torch

BAND_FACTOR = 4.0     # fused fp32 vs float64  <=  4 x (torch fp32 vs float64) + floor
FLOOR = 1e-5          # relative to max |reference|: the reduction-order spread of fp32 sums over K <= 1024 (+ d) terms


def torch_ffn(m, coords, dtype, taps=None):
    """the reference's forward: emb = [sin(2 pi x B^T), cos(2 pi x B^T)], Linear + ReLU ..., Linear (skip=False); a list `taps` receives
    what every ReLU is applied to"""
    p = m.params.detach().cpu().to(dtype)
    E, cin = m.embsize, m.coords_channel
    B = p[:E * cin].view(E, cin)
    x = coords.detach().cpu().to(dtype)
    t = (2. * math.pi * x) @ B.T
    h = torch.cat([torch.sin(t), torch.cos(t)], -1)
    ws, off = [], E * cin
    for (o, i) in m._shapes:
        W = p[off:off + o * i].view(o, i).clone().requires_grad_(True)
        b = p[off + o * i:off + o * i + o].clone().requires_grad_(True)
        ws += [W, b]
        off += o * i + o
    for l in range(len(m._shapes)):
        h = h @ ws[2 * l].T + ws[2 * l + 1]
        if l < len(m._shapes) - 1:
            if taps is not None:
                taps.append(h.detach())
            h = torch.relu(h)
    return h, ws


def phases(x, frequencies):
    """[n, cin] float32 -> [n, frequencies, cin] float64: the exact fp32 phases 2^i fl32(fl32(pi) x) the reference's torch.sin sees"""
    p = (x.to(torch.float32) * torch.tensor(math.pi, dtype=torch.float32)).double()
    return torch.stack([p * (2.0 ** i) for i in range(frequencies)], 1) if frequencies else p.new_zeros(p.shape[0], 0, p.shape[1])


def encoding(x, frequencies, dtype):
    """PosEncodingNeRF column order: x, then per frequency i and channel c: sin, cos"""
    n, cin = x.shape
    ph = phases(x, frequencies).to(dtype)
    sc = torch.stack([torch.sin(ph), torch.cos(ph)], -1).reshape(n, frequencies * cin * 2)
    return torch.cat([x.to(dtype), sc], 1)


def torch_nerf(m, coords, dtype, taps=None):
    """the reference's forward at `dtype` (the skip layer on cat[encoding, h]); returns (output, [W0, b0, ...] leaf tensors); a list
    `taps` receives what every ReLU is applied to"""
    p = m.params.detach().cpu().to(dtype)
    enc = encoding(coords.detach().cpu(), m.frequencies, dtype)
    ws, off = [], 0
    for (o, i) in m._shapes:
        ws += [p[off:off + o * i].view(o, i).clone().requires_grad_(True), p[off + o * i:off + o * i + o].clone().requires_grad_(True)]
        off += o * i + o
    h = enc
    for l in range(m.layers):
        if l == m.skip_layer:
            h = torch.cat([enc, h], 1)
        h = h @ ws[2 * l].T + ws[2 * l + 1]
        if l < m.layers - 1:
            if taps is not None:
                taps.append(h.detach())
            h = torch.relu(h)
    return h, ws


def torch_mfn(m, coords, dtype):
    """the reference's forward at `dtype`; returns (output, {state_dict key: leaf tensor})"""
    p = m.params.detach().cpu().to(dtype)
    t = {}
    for k, o, shp in m._entries:
        t[k] = p[o:o + int(np.prod(shp))].view(shp).clone().requires_grad_(True)
    x = coords.detach().cpu().to(dtype)

    def filt(i):
        g = torch.sin(x @ t["filters.%d.linear.weight" % i].T + t["filters.%d.linear.bias" % i])
        if m.GABOR:
            mu, gam = t["filters.%d.mu" % i], t["filters.%d.gamma" % i]
            D = (x ** 2).sum(-1)[..., None] + (mu ** 2).sum(-1)[None, :] - 2 * x @ mu.T
            g = g * torch.exp(-0.5 * D * gam[None, :])
        return g
    z = filt(0)
    for i in range(1, m.layers - 1):
        z = filt(i) * (z @ t["linear.%d.weight" % (i - 1)].T + t["linear.%d.bias" % (i - 1)])
    out = z @ t["output_linear.weight"].T + t["output_linear.bias"]
    if m.output_act:
        out = torch.sin(out)
    return out, t


def torch_taper(m, coords, dtype):
    """the reference's forward at `dtype` on the module's parameters; returns (output, [leaf tensors in state_dict order])"""
    leaves = [v.detach().cpu().to(dtype).clone().requires_grad_(True) for v in m.state_dict().values()]
    h = coords.detach().cpu().to(dtype)
    L = m.layers
    for l in range(L):
        h = h @ leaves[2 * l].T + leaves[2 * l + 1]
        if l < L - 1 or m.output_act:
            h = torch.sin(m.w0s[l] * h)
    return h, leaves


def torch_loss(yhat, y, w, kind, thr, beta):
    we = w.clone()
    if thr != 0:
        we = torch.where(yhat.detach() <= thr, torch.ones_like(we), we)
    d = yhat - y
    if kind == "datal2":
        li = d * d
    else:
        ad = d.abs()
        li = torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)
    return (li * we).mean()


def rand_coords(n, cin, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, cin, generator=g) * 2 - 1


def band_check(got, r64, r32, what):
    got, r64, r32 = (np.asarray(v, dtype=np.float64) for v in (got, r64, r32))
    e_fused = np.max(np.abs(got - r64))
    e_torch = np.max(np.abs(r32 - r64))
    bound = BAND_FACTOR * e_torch + FLOOR * max(np.max(np.abs(r64)), 1e-30)
    assert e_fused <= bound, "%s: fused %.3e vs float64, torch fp32 %.3e, bound %.3e" % (what, e_fused, e_torch, bound)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))
