"""SIREN on the fused HIP path — the drop-in for the object init_phi() returns in the reference.

Mirrors the surface NFGR / ModelSave use (reference utils/Networks.py:246-314, 795-802;
call sites SURVEY.md section 8b): constructor kwargs, forward(coords), parameters(),
state_dict(), to()/float()/half(), net[l][0].weight/.bias (readable AND assignable),
calc_param_count / calc_features.  All arithmetic runs in libbrief_hip.so; there is no
torch.autograd MLP and no CPU fallback.
"""
import copy
import ctypes as C
import logging
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, gradient, hessian, quantize, region

__all__ = ["SIREN", "FFN", "NeRF", "MFNFourier", "MFNGabor", "SIREN_Pyramid", "SIRENFT", "SIRENPS", "init_phi", "ALLPHI", "ALL_CALC_PHI_FEATURES", "ALL_CALC_PHI_PARAM_COUNT",
           "ALL_CHECK_PARAM_COUNT", "get_nnmodule_param_count"]


class _ParamView:
    """`net[l][0].weight` / `.bias`: a window into the packed parameter buffer.
    `.data` reads a tensor view; assigning `.data = t` copies into the buffer (what
    utils/ModelSave.py:20,27 does) and marks the fragment-ordered copy stale."""

    def __init__(self, owner, off, shape):
        self._o, self._off, self._shape = owner, off, tuple(shape)

    def _view(self, buf):
        n = int(np.prod(self._shape))
        return buf[self._off:self._off + n].view(self._shape)

    @property
    def data(self):
        return self._view(self._o.params)

    @data.setter
    def data(self, value):
        v = torch.as_tensor(value, dtype=torch.float32).reshape(self._shape)
        self._view(self._o.params).copy_(v.to(self._o.params.device))
        self._o._stale = True

    @property
    def grad(self):
        return None if self._o.grads is None else self._view(self._o.grads)

    @property
    def shape(self):
        return torch.Size(self._shape)

    def size(self, dim=None):
        return self.shape if dim is None else self._shape[dim]

    def numel(self):
        return int(np.prod(self._shape))

    def detach(self):
        return self.data

    def __len__(self):
        return self._shape[0]


class _Linear:
    def __init__(self, owner, woff, wshape, boff):
        self.weight = _ParamView(owner, woff, wshape)
        self.bias = _ParamView(owner, boff, (wshape[0],))
        self.in_features, self.out_features = wshape[1], wshape[0]


class _Seq:
    """stands for nn.Sequential(Linear[, Sine]); index 0 is the Linear."""

    def __init__(self, lin):
        self._lin = lin

    def __getitem__(self, i):
        if i != 0:
            raise IndexError("only the Linear (index 0) carries parameters")
        return self._lin

    def __len__(self):
        return 1


class _SirenFn(torch.autograd.Function):
    """forward/backward of the module under torch autograd (main.py:391-396: `data_hat = phi.forward(x);
    loss = loss_func(...); loss.backward()`).  backward hands dL/dyhat to the fused train step
    (BRIEF_LOSS_EXTERNAL) and leaves the gradient in module.params.grad, where torch.optim looks for it."""

    @staticmethod
    def forward(ctx, anchor, coords, module):
        ctx.module = module
        ctx.save_for_backward(coords)
        return module._forward_plain(coords)

    @staticmethod
    def backward(ctx, gy):
        (coords,) = ctx.saved_tensors
        m = ctx.module
        cin, cout = m.coords_channel, m.data_channel
        n = coords.numel() // cin
        m.train_step(n, gy.reshape(n, cout).to(torch.float32).contiguous(), coords=coords.reshape(n, cin), loss="external")
        if m.params.grad is None:
            m.params.grad = m.grads.clone()
        else:
            m.params.grad += m.grads
        return gy.new_zeros(1), None, None


class SIREN:
    """reference: utils/Networks.py:236-314."""

    def __init__(self, coords_channel=3, data_channel=1, features=256, layers=5, w0=30, res=False,
                 output_act=False, device=None, precision="fp32", **kwargs):
        """precision: 'fp32' (exact f32 MFMA, the parity path, features <= 4096), 'bf16' (hidden GEMMs on the bf16 matrix pipe,
        f32 master weights: the MI355X counterpart of Compress.half; include/brief_hip.h: BRIEF_PREC_BF16, features <= 512) or 'bf16x3'
        (split precision inside the fp32 parity bands, BRIEF_PREC_BF16X3, features <= 256; training AND inference run the split chains)."""
        if res:
            # HalfResidual blocks cannot be saved by the reference's own ModelSave
            raise NotImplementedError("SIREN(res=True) is unsupported on the fused path")
        self.coords_channel, self.data_channel = int(coords_channel), int(data_channel)
        self.features, self.layers = int(features), int(layers)
        self.w0, self.output_act = float(w0), bool(output_act)
        self.precision = str(precision)
        self.desc = _lib.SirenDesc(self.coords_channel, self.data_channel, self.layers, self.features,
                                   self.w0, 30.0, int(self.output_act), _lib.PRECISION[self.precision])
        F = self.features
        self._shapes = [(F, self.coords_channel)] + [(F, F)] * (self.layers - 2) + [(self.data_channel, F)]
        self.param_count = sum(o * i + o for o, i in self._shapes)
        self.params = self._reference_init()          # CPU until .to(device)
        self.grads = None
        self.packed = None
        self.qparams = None
        self._stale = True
        self._seen_version = -1
        self._autograd = False
        self._anchor = None
        self._ws = None
        self._fws = None
        self._loss = None
        net, off = [], 0
        for (o, i) in self._shapes:
            net.append(_Seq(_Linear(self, off, (o, i), off + o * i)))
            off += o * i + o
        self.net = net
        if device is not None:
            self.to(device)

    # ---- initialisation: replays the reference's torch-RNG draws so that equal seeds give equal nets
    def _reference_init(self):
        """nn.Linear default init for every layer in order (weight then bias), then sine_init
        over all weights in layer order, then first_layer_sine_init (utils/Networks.py:215-226,
        246-266).  Values AND generator consumption match torch, so after
        torch.manual_seed(s) this reproduces the reference's tensors bit for bit."""
        ws, bs = [], []
        for (o, i) in self._shapes:
            w = torch.empty(o, i)
            gain = math.sqrt(2.0 / (1 + math.sqrt(5) ** 2))
            bound = math.sqrt(3.0) * gain / math.sqrt(i)
            w.uniform_(-bound, bound)
            b = torch.empty(o)
            bb = 1 / math.sqrt(i) if i > 0 else 0
            b.uniform_(-bb, bb)
            ws.append(w)
            bs.append(b)
        for w in ws:
            num_input = w.size(-1)
            w.uniform_(-np.sqrt(6 / num_input) / 30, np.sqrt(6 / num_input) / 30)
        num_input = ws[0].size(-1)
        ws[0].uniform_(-1 / num_input, 1 / num_input)
        return torch.cat([torch.cat([w.reshape(-1), b]) for w, b in zip(ws, bs)]).contiguous()

    # ---- nn.Module-like surface
    def parameters(self):
        return [self.params]

    def state_dict(self):
        sd = OrderedDict()
        for l, seq in enumerate(self.net):
            sd["net.%d.0.weight" % l] = seq[0].weight.data
            sd["net.%d.0.bias" % l] = seq[0].bias.data
        return sd

    def load_state_dict(self, sd):
        for l, seq in enumerate(self.net):
            seq[0].weight.data = sd["net.%d.0.weight" % l]
            seq[0].bias.data = sd["net.%d.0.bias" % l]

    def to(self, device):
        device = torch.device(device)
        if self.params.device != device:
            self.params = self.params.to(device)
            self.grads = None
            self.packed = None
            self.qparams = None
            self._ws = self._fws = None
            self._stale = True
        return self

    def cuda(self):
        return self.to("cuda")

    def cpu(self):
        return self.to("cpu")

    def _set_precision(self, precision):
        if precision != self.precision:
            self.precision = precision
            self.desc.precision = _lib.PRECISION[precision]
            self.packed = None          # the fragment-ordered copy has another size and content
            self._ws = self._fws = None
            self._stale = True
        return self

    def float(self):
        """nn.Module.float() as the reference's low-precision loop uses it (main.py:398: back to fp32 for the update)"""
        # (the mode half() recorded is consumed here: after a _set_precision / to() round trip a later float() cannot restore a stale one)
        return self._set_precision(self.__dict__.pop("_float_precision", self.precision))

    def half(self):
        """nn.Module.half() as the reference uses it (main.py:212, 287-288, 389): its fp16 mode.  The MI355X counterpart is the
        bf16 matrix pipe with fp32 master weights (BRIEF_PREC_BF16, what Compress.half selects in NFGR): the parameters stay
        fp32, the hidden GEMMs of forward / backward / decode run on v_mfma_f32_32x32x16_bf16.  Widths above 512 have no bf16
        kernels and stay exact."""
        if self.precision != "bf16":
            self._float_precision = self.precision
        if self.features > 512 and not getattr(SIREN, "_warned_half_wide", False):
            SIREN._warned_half_wide = True
            logging.warning("SIREN.half(): no bf16 kernels above 512 features (this net has %d): it stays in exact fp32; "
                            "callers that round coordinates / outputs to fp16 around it get the I/O rounding only", self.features)
        return self._set_precision("bf16" if self.features <= 512 else self.precision)

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def requires_grad_(self, flag=True):
        """requires_grad_(True): forward() takes part in torch autograd (the reference's own loop body then runs on
        this module: zero_grad, forward, loss, backward, torch.optim step).  Default off: forward() returns plain
        tensors and the fused Fitter path is the fast one."""
        self._autograd = bool(flag)
        return self

    @property
    def device(self):
        return self.params.device

    # ---- fused path
    def _require_gpu(self):
        if self.params.device.type != "cuda":
            raise _lib.BriefError("the fused SIREN path needs the parameters on a ROCm GPU (module.to('cuda')); "
                                  "there is no CPU fallback")

    def sync_packed(self):
        """refresh the fragment-ordered weight copy after any change of self.params"""
        self._require_gpu()
        if self.packed is None:
            n = self._abi_packed_count()
            if n < 0:      # (a shape the library refuses, e.g. precision = 'bf16' above 512 features: its message, not a torch allocation error)
                raise _lib.BriefError(_lib.lib().brief_last_error().decode())
            self.packed = torch.empty(n, dtype=torch.float32, device=self.params.device)
            self._stale = True
        if self.params._version != self._seen_version:      # torch changed the parameters in place (e.g. optimizer.step())
            self._stale = True
        if self._stale:
            _lib.check(self._abi_repack())
            self._stale = False
            self._seen_version = self.params._version

    @staticmethod
    def _grid(dims, lo, hi):
        g = _lib.GridDesc()
        g.ndim = len(dims)
        for a, v in enumerate(dims):
            g.dims[a] = int(v)
        g.lo, g.hi = float(lo), float(hi)
        return g

    def forward(self, coords):
        """SIREN.forward (utils/Networks.py:269-271): coords [..., cin] -> [..., cout].  Differentiable w.r.t. the
        parameters after requires_grad_(True) (see _SirenFn); otherwise a plain no-grad evaluation."""
        if self._autograd and torch.is_grad_enabled():
            self._require_gpu()
            if self._anchor is None or self._anchor.device != self.params.device:
                self._anchor = torch.zeros(1, device=self.params.device, requires_grad=True)
            return _SirenFn.apply(self._anchor, coords.to(self.params.device, torch.float32).contiguous(), self)
        return self._forward_plain(coords)

    def _forward_plain(self, coords):
        self._require_gpu()
        self.sync_packed()
        c = coords.to(self.params.device, torch.float32).contiguous()
        lead = c.shape[:-1]
        n = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty((n, self.data_channel), dtype=torch.float32, device=c.device)
        if n == 0:
            return out.view(*lead, self.data_channel)
        b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
        _lib.check(self._abi_forward(None, b, out, _lib.OUT_F32, (0.0, 1.0), (0.0, 1.0), n))
        return out.view(*lead, self.data_channel)

    def _forward_scratch(self, n):
        """(pointer, bytes) of the inference scratch brief_siren_forward_ws wants: nothing up to 1024 features, two ping-pong
        activation planes per workgroup above (include/brief_hip.h); allocated once, kept"""
        need = _lib.lib().brief_forward_workspace_bytes(C.byref(self.desc), int(n))
        if need < 0:
            raise _lib.BriefError(_lib.lib().brief_last_error().decode())
        if need == 0:
            return None, 0
        if self._fws is None or self._fws.numel() * 4 < need:
            self._fws = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.params.device)
        return _lib.ptr(self._fws), self._fws.numel() * 4

    def __call__(self, coords):
        return self.forward(coords)

    def decode_grid(self, dims, lo=-1.0, hi=1.0, offset=0, count=None, out=None, out_kind="f32",
                    scale=(0.0, 100.0), vrange=(0.0, 1.0)):
        """forward over `count` voxels of the flattened (d,h,w) grid starting at `offset`, coordinates
        synthesised in-kernel (replaces create_flattened_coords + the chunked loop of
        utils/misc.py:59-92).  out_kind 'u8'/'u16' fuses invnormalize_data (utils/io.py:136-147)."""
        self._require_gpu()
        self.sync_packed()
        total = int(np.prod(dims))
        count = total - offset if count is None else int(count)
        kind = {"f32": _lib.OUT_F32, "u8": _lib.OUT_U8, "u16": _lib.OUT_U16}[out_kind]
        dt = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}[out_kind]
        if out is None:
            out = torch.empty((count, self.data_channel), dtype=dt, device=self.params.device)
        g = self._grid(dims, lo, hi)
        b = _lib.BatchDesc(None, None, None, None, int(offset), count, 0, 0, 0)
        _lib.check(self._abi_forward(g, b, out, kind, scale, vrange, count))
        return out

    # voxels per brief_siren_forward_box call of decode_box: bounds one launch's length and the scratch request of a wide net
    BOX_CHUNK = 1 << 27

    def decode_box(self, dims, start=None, stop=None, step=1, lo=-1.0, hi=1.0, out_kind="f32", scale=(0.0, 100.0), vrange=(0.0, 1.0),
                   out=None, chunk=None):
        """forward over the box start:stop:step (numpy slice semantics per spatial axis) of the linspace grid `dims`, without
        evaluating the rest of it: equals decode_grid(dims).view(*dims, cout)[slices] bit for bit.  Returns [*extent, cout].
        start / stop / step: an int, None or one entry per axis; out-of-range bounds, empty boxes and steps below 1 raise
        ValueError.  `dims` may differ from the fitted shape (a resampled view).  The box runs in calls of at most `chunk` voxels
        (default BOX_CHUNK) through brief_siren_forward_box's offset / n."""
        self._require_gpu()
        self.sync_packed()
        box, ext, total = self._box_plan(dims, start, stop, step, lo, hi)
        kind = {"f32": _lib.OUT_F32, "u8": _lib.OUT_U8, "u16": _lib.OUT_U16}[out_kind]
        dt = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}[out_kind]
        if out is None:
            out = torch.empty((*ext, self.data_channel), dtype=dt, device=self.params.device)
        elif out.dtype != dt or out.numel() != total * self.data_channel or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s tensor of %d elements" % (dt, total * self.data_channel))
        flat = out.view(total, self.data_channel)
        self._box_chunks(total, chunk, lambda off, cnt: self._abi_forward_box(box, off, cnt, flat[off:off + cnt], kind, scale, vrange))
        return out

    def _box_plan(self, dims, start, stop, step, lo, hi):
        """(GridBox, extents, voxel count) of the box start:stop:step of the linspace grid `dims` over [lo, hi]: decode_box's region
        semantics, for the three box decoders"""
        nd = len(dims)
        per = (lambda v: [v] * nd if v is None or np.isscalar(v) else list(v))
        b, e = per(start), per(stop)
        if len(b) != nd or len(e) != nd:
            raise ValueError("start / stop need one entry per axis of dims")
        b0, e0, st = region.normalize_region(dims, tuple(slice(x, y) for x, y in zip(b, e)), step)
        ext = region.extents(b0, e0, st)
        box = _lib.GridBox()
        box.grid = self._grid(dims, lo, hi)
        for a in range(nd):
            box.start[a], box.step[a], box.extent[a] = b0[a], st[a], ext[a]
        return box, ext, int(np.prod(ext))

    def _box_chunks(self, total, chunk, call):
        """call(offset, count) -> status over the box's `total` voxels in runs of at most `chunk` (default BOX_CHUNK)"""
        chunk = int(chunk or self.BOX_CHUNK)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        for off in range(0, total, chunk):
            _lib.check(call(off, min(chunk, total - off)))

    # ---- spatial gradients and Hessians: value, analytic Jacobian and analytic second derivatives with respect to the coordinates
    # (csrc/brief_jac.inc, csrc/brief_hess.inc; one host driver, csrc/brief_jac_host.inc)
    def _sync_jac(self, decode=gradient):
        """the Jacobian kernel's own fragment buffer, a second derived copy of self.params: allocated on first use, and written anew
        at the head of EVERY gradient call (one launch over the net's size).  A stale copy is the bug this is built against: the
        parameters change under load_state_dict / load_model (.data), torch optimizers, to() and the in-kernel updates of a fit,
        and a flag would have to follow every one of those writers; a copy that is never reused cannot be stale.
        decode: the module (gradient, hessian) in whose words a net outside the envelope is refused."""
        self._require_gpu()
        why = decode.refusal(getattr(type(self), "kind", "SIREN"), self.precision, self.features)
        if why is not None:
            raise _lib.BriefError(why)
        L = _lib.lib()
        pk = getattr(self, "_jac_packed", None)
        if pk is None or pk.device != self.params.device:
            n = L.brief_siren_jac_packed_count(C.byref(self.desc))
            if n < 0:
                raise _lib.BriefError(L.brief_last_error().decode())
            pk = self._jac_packed = torch.empty(n, dtype=torch.float32, device=self.params.device)
        _lib.check(L.brief_siren_jac_repack(C.byref(self.desc), _lib.ptr(self.params), _lib.ptr(pk), _lib.stream_ptr()))
        return pk

    def spatial_gradient(self, coords, want_value=True):
        """(value [n, cout], jac [n, cout, cin]) at arbitrary device coordinates [n, cin]: the net's output and its analytic Jacobian
        d phi_c / d x_a in coordinate units (with output_act, of the activated output); float32, from brief_siren_jac_forward.
        value is None with want_value=False.  fp32 SIREN up to 1024 features only (BriefError otherwise)."""
        return self._derivatives_at(coords, want_value, True, False)[:2]

    def _derivative_outputs(self, lead, want_value, want_jac, want_hess):
        """the float32 results [*lead, cout], [*lead, cout, cin] and [*lead, cout, nh] of a derivative decode, None where not wanted"""
        cin, cout = self.coords_channel, self.data_channel
        new = (lambda want, *tail: torch.empty((*lead, cout, *tail), dtype=torch.float32, device=self.params.device) if want else None)
        return new(want_value), new(want_jac, cin), new(want_hess, cin * (cin + 1) // 2)

    def _derivatives_at(self, coords, want_value, want_jac, want_hess):
        """(value, jac, hess) at the coordinates [n, cin], None where not wanted: spatial_gradient's and spatial_hessian's body.  With
        want_hess the Hessian kernel runs (brief_siren_hess_forward), else the Jacobian kernel (brief_siren_jac_forward)."""
        pk = self._sync_jac(hessian if want_hess else gradient)
        c = coords.to(self.params.device, torch.float32).reshape(-1, self.coords_channel).contiguous()
        n = c.shape[0]
        outs = self._derivative_outputs((n,), want_value, want_jac, want_hess)
        if n:
            b = _lib.BatchDesc(c.data_ptr(), None, None, None, 0, n, 0, 0, 0)
            entry = _lib.lib().brief_siren_hess_forward if want_hess else _lib.lib().brief_siren_jac_forward
            _lib.check(entry(C.byref(self.desc), _lib.ptr(pk), None, C.byref(b), *[_lib.ptr(t) for t in outs[:3 if want_hess else 2]],
                             _lib.stream_ptr()))
        return outs

    def _derivatives_box(self, dims, start, stop, step, lo, hi, chunk, want_value, want_jac, want_hess):
        """(value, jac, hess) over a box of the grid `dims`, None where not wanted: decode_gradient_box's and decode_hessian_box's body
        (decode_box's plan and chunk loop around brief_siren_hess_forward_box with want_hess, else brief_siren_jac_forward_box)"""
        pk = self._sync_jac(hessian if want_hess else gradient)
        box, ext, total = self._box_plan(dims, start, stop, step, lo, hi)
        outs = self._derivative_outputs(ext, want_value, want_jac, want_hess)
        flat = [None if t is None else t.view(total, *t.shape[len(ext):]) for t in outs[:3 if want_hess else 2]]
        entry = _lib.lib().brief_siren_hess_forward_box if want_hess else _lib.lib().brief_siren_jac_forward_box
        self._box_chunks(total, chunk, lambda off, cnt: entry(C.byref(self.desc), _lib.ptr(pk), C.byref(box), off, cnt,
                                                             *[_lib.ptr(None if t is None else t[off:off + cnt]) for t in flat],
                                                             _lib.stream_ptr()))
        return outs

    def decode_gradient_box(self, dims, start=None, stop=None, step=1, lo=-1.0, hi=1.0, chunk=None, want_value=True):
        """(jac [*extent, cout, cin], value [*extent, cout] | None) over the box start:stop:step of the linspace grid `dims`, with
        decode_box's region semantics, coordinates (bit for bit) and chunk loop: a box equals the slice of the whole grid's result,
        and neither `chunk` nor a repeat of the call changes a bit.  Coordinate units: per unit of [lo, hi] (gradient.voxel_scale
        converts to grey levels per voxel step)."""
        value, jac, _ = self._derivatives_box(dims, start, stop, step, lo, hi, chunk, want_value, True, False)
        return jac, value

    def spatial_hessian(self, coords, want_value=True, want_jac=True):
        """(value [n, cout], jac [n, cout, cin], hess [n, cout, nh]) at arbitrary device coordinates [n, cin]: the net's output, its
        analytic Jacobian and its analytic Hessian d2 phi_c / d x_a d x_b in coordinate units (with output_act, of the activated
        output); float32, from brief_siren_hess_forward.  nh = 6 in the order (00, 01, 02, 11, 12, 22) for cin = 3 and nh = 3 in the
        order (00, 01, 11) for cin = 2 (hessian.full() expands to the symmetric matrix).  value / jac are None with want_value /
        want_jac False.  fp32 SIREN up to 1024 features only (BriefError otherwise).  The kernel reads the Jacobian decode's
        fragment copy (_sync_jac), written anew at the head of every call."""
        return self._derivatives_at(coords, want_value, want_jac, True)

    def decode_hessian_box(self, dims, start=None, stop=None, step=1, lo=-1.0, hi=1.0, chunk=None, want_value=False, want_jac=False):
        """hess [*extent, cout, nh] over the box start:stop:step of the linspace grid `dims`, with decode_box's region semantics,
        coordinates (bit for bit) and chunk loop: a box equals the slice of the whole grid's result, and neither `chunk` nor a repeat
        of the call changes a bit.  Coordinate units: per unit of [lo, hi] squared (hessian.voxel_scale converts to grey levels per
        voxel step squared).  With want_value or want_jac the result is (hess, value [*extent, cout] | None, jac [*extent, cout, cin]
        | None)."""
        value, jac, hess = self._derivatives_box(dims, start, stop, step, lo, hi, chunk, want_value, want_jac, True)
        return (hess, value, jac) if want_value or want_jac else hess

    def train_step(self, n, targets, idx=None, coords=None, weights=None, grid=None, offset=0,
                   loss="datal2", thr=0.0, beta=0.01, want_yhat=False, rng=None):
        """zero_grad + forward + loss + backward of main.py:385-396 for one batch of n samples.
        Fills self.grads (canonical layout) and returns (loss [1] device tensor, yhat or None).
        rng = (pop, seed, step) with neither idx nor coords: the samples are drawn inside the kernel, as fit_step draws them."""
        self._require_gpu()
        self.sync_packed()
        dev = self.params.device
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        need = self._abi_train_ws_bytes(n)
        if need < 0:
            raise _lib.BriefError(_lib.lib().brief_last_error().decode())
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        yhat = torch.empty((n, self.data_channel), dtype=torch.float32, device=dev) if want_yhat else None
        g = None
        if coords is None:
            dims, lo, hi = grid
            g = self._grid(dims, lo, hi)
        b = _lib.BatchDesc(_dev_ptr(coords, torch.float32, "coords", dev), _dev_ptr(targets, torch.float32, "targets", dev),
                           _dev_ptr(weights, torch.float32, "weights", dev), _dev_ptr(idx, torch.int64, "idx", dev),
                           int(offset), int(n), *((int(v) for v in rng) if (rng is not None and idx is None and coords is None) else (0, 0, 0)))
        _lib.check(self._abi_train_step(g, b, _lib.LOSS_KIND[loss], thr, beta, yhat))
        return self._loss, yhat

    def fit_step(self, n, targets, opt_kind, s1, s2, lr, t, idx=None, weights=None, grid=None, offset=0,
                 loss="datal2", thr=0.0, beta=0.01, betas=(0.9, 0.999), eps=1e-8, rng=None):
        """train_step + optimizer update + refresh of the packed copy in one C-ABI call (three launches);
        bit-identical to the separate calls.  Returns the device loss tensor."""
        self._require_gpu()
        self.sync_packed()
        self.ensure_train_buffers(n)
        dims, lo, hi = grid
        g = self._grid(dims, lo, hi)
        pop, seed, step = rng if (rng is not None and idx is None) else (0, 0, 0)      # rng = (pop, seed, step): in-kernel sampling
        dev = self.params.device
        b = _lib.BatchDesc(None, _dev_ptr(targets, torch.float32, "targets", dev), _dev_ptr(weights, torch.float32, "weights", dev),
                           _dev_ptr(idx, torch.int64, "idx", dev), int(offset), int(n), int(pop), int(seed), int(step))
        _lib.check(_lib.lib().brief_siren_fit_step(
            C.byref(self.desc), _lib.ptr(self.params), _lib.ptr(self.packed), C.byref(g), C.byref(b),
            _lib.LOSS_KIND[loss], float(thr), float(beta), int(opt_kind), _lib.ptr(s1), _lib.ptr(s2),
            float(lr), betas[0], betas[1], eps, int(t), _lib.ptr(self.grads), _lib.ptr(self._loss),
            _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr()))
        return self._loss

    def ensure_train_buffers(self, n):
        """gradient / loss / workspace buffers for batches of n samples (allocated once, reused)."""
        self._require_gpu()
        dev = self.params.device
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        need = self._abi_train_ws_bytes(n)
        if need < 0:
            raise _lib.BriefError(_lib.lib().brief_last_error().decode())
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)

    # ---- quantised weights (quantize.py; kernels: csrc/brief_quant.inc)
    def quant_spans(self):
        """the net's tensors (every weight matrix and every bias, in canonical order) as brief_quant_span's"""
        spans, off = [], 0
        for (o, i) in self._shapes:
            spans += [(off, o * i), (off + o * i, o)]
            off += o * i + o
        return (_lib.QuantSpan * len(spans))(*spans)

    def fake_quantise(self, bits):
        """self.qparams = deq(code(self.params)), every tensor with its own range, on the device (brief_quant_ranges +
        brief_quant_apply: three launches, nothing crosses to the host): what an artefact written now with `bits` bits decodes to.
        Returns self.qparams (canonical layout; allocated once)."""
        self._require_gpu()
        if getattr(type(self), "kind", "SIREN") not in quantize.NETS:
            raise _lib.BriefError("quantised weights exist for %s only (this net is %s)" % (", ".join(quantize.NETS), type(self).kind))
        if self.precision not in ("fp32", "f32"):
            raise _lib.BriefError("quantised weights need an fp32 net (this one runs in %s)" % self.precision)
        L = _lib.lib()
        if getattr(self, "_qspans", None) is None or self.qparams is None or self.qparams.device != self.params.device:
            self._qspans = self.quant_spans()
            n = len(self._qspans)
            if n > _lib.QUANT_MAX_TENSORS:
                raise _lib.BriefError("quantised weights: at most %d tensors (this net has %d)" % (_lib.QUANT_MAX_TENSORS, n))
            self.qparams = torch.empty_like(self.params)
            self._qlo_step = torch.empty((n, 2), dtype=torch.float32, device=self.params.device)
            self._qws = torch.empty(L.brief_quant_workspace_bytes(self.params.numel(), n) // 4, dtype=torch.float32, device=self.params.device)
        n = len(self._qspans)
        _lib.check(L.brief_quant_ranges(_lib.ptr(self.params), self._qspans, n, int(bits), _lib.ptr(self._qlo_step), _lib.ptr(self._qws),
                                        self._qws.numel() * 4, _lib.stream_ptr()))
        _lib.check(L.brief_quant_apply(_lib.ptr(self.params), self._qspans, n, int(bits), _lib.ptr(self._qlo_step), _lib.ptr(self.qparams), None,
                                       _lib.stream_ptr()))
        return self.qparams

    def pack_from(self, src):
        """the fragment-ordered copy rebuilt from `src` (canonical layout, e.g. self.qparams) instead of the master parameters; it stays
        that way until the parameters change through torch or .data, or mark_packed_stale() is called"""
        self._require_gpu()
        if self.packed is None:
            self.sync_packed()
        _lib.check(self._abi_repack(src))
        self._stale = False
        self._seen_version = self.params._version

    def mark_packed_stale(self):
        self._stale = True

    # ---- the C-ABI entries of this net kind (_FusedFamily overrides them)
    def _abi_packed_count(self):
        return _lib.lib().brief_packed_count(C.byref(self.desc))

    def _abi_repack(self, src=None):
        return _lib.lib().brief_siren_repack(C.byref(self.desc), _lib.ptr(self.params if src is None else src), _lib.ptr(self.packed), _lib.stream_ptr())

    def _abi_forward(self, grid, batch, out, kind, scale, vrange, n):
        ws, ws_bytes = self._forward_scratch(n)
        return _lib.lib().brief_siren_forward_ws(C.byref(self.desc), _lib.ptr(self.packed), C.byref(grid) if grid is not None else None,
                                                 C.byref(batch), _lib.ptr(out), kind, float(scale[0]), float(scale[1]),
                                                 float(vrange[0]), float(vrange[1]), ws, ws_bytes, _lib.stream_ptr())

    def _abi_forward_box(self, box, off, cnt, out, kind, scale, vrange):
        ws, ws_bytes = self._forward_scratch(cnt)
        return _lib.lib().brief_siren_forward_box(C.byref(self.desc), _lib.ptr(self.packed), C.byref(box), off, cnt, _lib.ptr(out),
                                                  kind, float(scale[0]), float(scale[1]), float(vrange[0]), float(vrange[1]),
                                                  ws, ws_bytes, _lib.stream_ptr())

    def _abi_train_ws_bytes(self, n):
        return _lib.lib().brief_train_workspace_bytes(C.byref(self.desc), int(n))

    def _abi_train_step(self, g, b, loss_kind, thr, beta, yhat):
        return _lib.lib().brief_siren_train_step(
            C.byref(self.desc), _lib.ptr(self.packed), C.byref(g) if g is not None else None, C.byref(b),
            loss_kind, float(thr), float(beta), _lib.ptr(self.grads), _lib.ptr(self._loss), _lib.ptr(yhat),
            _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr())

    # ---- budget -> width (utils/Networks.py:291-314)
    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, res=False, **kwargs):
        """utils/Networks.py:291-297: first layer + (layers-2) hidden F x F layers + head, weights and biases"""
        SIREN._no_res(res)
        F, hidden = features, layers - 2
        return int((coords_channel + 1) * F + hidden * (F + 1) * F + (F + 1) * data_channel)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, res=False, **kwargs):
        """utils/Networks.py:299-314: the positive root of hidden F^2 + (cin + 1 + hidden + cout) F + cout = P, rounded"""
        SIREN._no_res(res)
        hidden = layers - 2
        lin = coords_channel + 1 + hidden + data_channel
        if hidden == 0:
            return round((param_count - data_channel) / lin)
        return round((math.sqrt(lin * lin + 4 * hidden * (param_count - data_channel)) - lin) / (2 * hidden))

    @staticmethod
    def _no_res(res):
        if res:
            raise NotImplementedError("SIREN(res=True) is unsupported on the fused path")


class _FusedFamily(SIREN):
    """what FFN, NeRF, the MFNs and the tapered SIRENs share: kernels of their own, fp32 only, behind the C-ABI entries brief_<family>_*
    (one host driver: csrc/brief_family_host.inc), and a fit job type of their own.  A family names its entries and itself."""

    _abi = None                              # "brief_<family>_": the prefix of the family's C-ABI entries
    _fit_job, _fit_entry = None, None        # brief_*_fit_job type and brief_*_fit entry (Fitter, fit_step)
    _family = None                           # the family's name in half()'s warning
    _warned_half = set()                     # families that have warned

    def _set_precision(self, precision):
        return self

    def float(self):
        return self

    def half(self):
        """no low-precision kernels: the net stays in fp32 (NFGR keeps the reference's 2-bytes-per-parameter budget and records
        phi_precision: fp32)"""
        if self._family not in _FusedFamily._warned_half:
            _FusedFamily._warned_half.add(self._family)
            logging.warning("%s.half(): there are no low-precision %s kernels; the net stays in fp32" % (type(self).kind, self._family))
        return self

    def _forward_scratch(self, n):
        return None, 0

    # ---- C-ABI entries
    def _entry(self, name):
        return getattr(_lib.lib(), self._abi + name)

    def _abi_packed_count(self):
        return self._entry("packed_count")(C.byref(self.desc))

    def _abi_repack(self, src=None):
        return self._entry("repack")(C.byref(self.desc), _lib.ptr(self.params if src is None else src), _lib.ptr(self.packed), _lib.stream_ptr())

    def _abi_forward(self, grid, batch, out, kind, scale, vrange, n):
        return self._entry("forward")(C.byref(self.desc), _lib.ptr(self.packed), C.byref(grid) if grid is not None else None,
                                      C.byref(batch), _lib.ptr(out), kind, float(scale[0]), float(scale[1]),
                                      float(vrange[0]), float(vrange[1]), _lib.stream_ptr())

    def _abi_forward_box(self, box, off, cnt, out, kind, scale, vrange):
        return self._entry("forward_box")(C.byref(self.desc), _lib.ptr(self.packed), C.byref(box), off, cnt, _lib.ptr(out),
                                          kind, float(scale[0]), float(scale[1]), float(vrange[0]), float(vrange[1]),
                                          _lib.stream_ptr())

    def _abi_train_ws_bytes(self, n):
        return self._entry("train_workspace_bytes")(C.byref(self.desc), int(n))

    def _abi_train_step(self, g, b, loss_kind, thr, beta, yhat):
        return self._entry("train_step")(
            C.byref(self.desc), _lib.ptr(self.packed), C.byref(g) if g is not None else None, C.byref(b),
            loss_kind, float(thr), float(beta), _lib.ptr(self.grads), _lib.ptr(self._loss), _lib.ptr(yhat),
            _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr())

    def fit_step(self, n, targets, opt_kind, s1, s2, lr, t, idx=None, weights=None, grid=None, offset=0,
                 loss="datal2", thr=0.0, beta=0.01, betas=(0.9, 0.999), eps=1e-8, rng=None):
        """train_step + optimizer update of the MLP span + refresh of the packed copy: one step of the family's brief_*_fit"""
        self._require_gpu()
        self.sync_packed()
        self.ensure_train_buffers(n)
        dims, lo, hi = grid
        g = self._grid(dims, lo, hi)
        pop, seed, step = rng if (rng is not None and idx is None) else (0, 0, 0)
        dev = self.params.device
        b = _lib.BatchDesc(None, _dev_ptr(targets, torch.float32, "targets", dev), _dev_ptr(weights, torch.float32, "weights", dev),
                           _dev_ptr(idx, torch.int64, "idx", dev), int(offset), int(n), int(pop), int(seed), 0)
        j = self._fit_job()
        j.desc, j.grid, j.batch = self.desc, g, b
        j.params, j.packed, j.state1, j.state2 = self.params.data_ptr(), self.packed.data_ptr(), _lib.ptr(s1), _lib.ptr(s2)
        j.grads, j.loss_out, j.loss_log = self.grads.data_ptr(), self._loss.data_ptr(), None
        j.workspace, j.workspace_bytes = self._ws.data_ptr(), self._ws.numel() * 4
        j.loss_kind, j.optim_kind, j.thr, j.beta = _lib.LOSS_KIND[loss], int(opt_kind), float(thr), float(beta)
        j.lr, j.beta1, j.beta2, j.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        j.n_milestones, j.gamma, j.t0 = 0, 1.0, int(t) - 1
        j.idx_stride = int(n) if idx is not None else 0      # (in-kernel draws of step t are keyed by rng_step = t0 + 1 = t)
        _lib.check(getattr(_lib.lib(), self._fit_entry)(C.byref(j), 1, _lib.stream_ptr()))
        return self._loss


class FFN(_FusedFamily):
    """reference: utils/Networks.py:138-207 (FourierFeatureEmbedding + FFN), skip=False.  Parameters live in one canonical buffer
    [bvals | W0 b0 | hidden | head] (include/brief_hip.h, brief_ffn_desc); bvals is fixed: its gradient is zero and the optimizer
    (brief_ffn_fit) updates the MLP span only."""

    kind = "FFN"
    _abi, _fit_job, _fit_entry, _family = "brief_ffn_", _lib.FfnFitJob, "brief_ffn_fit", "FFN"

    def __init__(self, coords_channel=3, data_channel=1, embsize=256, scale=10, features=256, layers=5, skip=False,
                 device=None, precision="fp32", **kwargs):
        """w0 / output_act / res of a SIREN YAML are ignored, as FFN(**phi) ignores them.  precision: the fused path is fp32 only;
        'bf16' / 'bf16x3' run in fp32 with a warning."""
        if skip:
            raise NotImplementedError("FFN(skip=True) is unsupported on the fused path")
        if str(precision) not in ("fp32", "f32"):
            # (an artefact's phi_precision, or NFGR's Compress.half / precision, names a low-precision mode: there are no such FFN kernels)
            logging.warning("FFN: no %s kernels; the net runs in fp32" % precision)
        self.coords_channel, self.data_channel = int(coords_channel), int(data_channel)
        self.features, self.layers = int(features), int(layers)
        self.embsize, self.scale = int(embsize), float(scale)
        if self.layers < 2:
            raise NotImplementedError("FFN: layers must be >= 2")
        if not 1 <= self.features <= 1024:
            raise NotImplementedError("FFN: features must be 1..1024 on the fused path (got %d)" % self.features)
        if not 1 <= self.embsize <= 512:
            raise NotImplementedError("FFN: embsize must be 1..512 on the fused path (got %d)" % self.embsize)
        if self.coords_channel not in (2, 3) or not 1 <= self.data_channel <= 4:
            raise NotImplementedError("FFN: coords_channel must be 2 or 3 and data_channel 1..4")
        self.precision = "fp32"
        self.w0, self.output_act = 0.0, False
        self.desc = _lib.FfnDesc(self.coords_channel, self.data_channel, self.layers, self.features, self.embsize, 0)
        F, E = self.features, self.embsize
        self._shapes = [(F, 2 * E)] + [(F, F)] * (self.layers - 2) + [(self.data_channel, F)]
        self.bv_count = E * self.coords_channel
        self.param_count = self.bv_count + sum(o * i + o for o, i in self._shapes)
        self.params = self._reference_init()
        self.grads = None
        self.packed = None
        self.qparams = None
        self._stale = True
        self._seen_version = -1
        self._autograd = False
        self._anchor = None
        self._ws = None
        self._fws = None
        self._loss = None
        self.fourierfeature_embedding = _Embedding(_ParamView(self, 0, (E, self.coords_channel)))
        net, off = [], self.bv_count
        for (o, i) in self._shapes:
            net.append(_Seq(_Linear(self, off, (o, i), off + o * i)))
            off += o * i + o
        self.net = net
        if device is not None:
            self.to(device)

    def _reference_init(self):
        """FourierFeatureEmbedding.__init__ reseeds the global generator with 0 and draws bvals = normal(0, 1) * scale; the
        nn.Linear default inits (kaiming_uniform(a=sqrt 5) weight, then bias) follow in layer order.  Replayed with torch on the
        CPU: the values AND the generator state afterwards equal the reference's, whatever the caller's seed was."""
        torch.manual_seed(0)
        bv = torch.normal(0, 1, size=(self.embsize, self.coords_channel)) * self.scale
        parts = [bv.reshape(-1)]
        for (o, i) in self._shapes:
            w = torch.empty(o, i)
            gain = math.sqrt(2.0 / (1 + math.sqrt(5) ** 2))
            w.uniform_(-math.sqrt(3.0) * gain / math.sqrt(i), math.sqrt(3.0) * gain / math.sqrt(i))
            b = torch.empty(o)
            b.uniform_(-1 / math.sqrt(i), 1 / math.sqrt(i))
            parts += [w.reshape(-1), b]
        return torch.cat(parts).contiguous()

    def state_dict(self):
        sd = OrderedDict()
        sd["fourierfeature_embedding.bvals"] = self.fourierfeature_embedding.bvals.data
        sd.update(SIREN.state_dict(self))
        return sd

    def load_state_dict(self, sd):
        if "fourierfeature_embedding.bvals" in sd:
            self.fourierfeature_embedding.bvals.data = sd["fourierfeature_embedding.bvals"]
        SIREN.load_state_dict(self, sd)

    # ---- budget -> width (utils/Networks.py:188-207)
    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, embsize=256, layers=5, skip=False, **kwargs):
        """the reference's formula: first layer 2E x F + F, (layers-2) hidden F x F + F, head F x cout + cout, plus bvals E x cin"""
        FFN._no_skip(skip)
        d = 2 * embsize
        return int(d * features + features + (layers - 2) * (features ** 2 + features) + features * data_channel + data_channel
                   + coords_channel * embsize)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, embsize=256, layers=5, skip=False, **kwargs):
        """the positive root of (layers-2) F^2 + (2E + 1 + layers-2 + cout) F + cout + cin E = P, rounded (the reference's formula)"""
        FFN._no_skip(skip)
        d = 2 * embsize
        a = layers - 2
        b = d + 1 + layers - 2 + data_channel
        c = -param_count + data_channel + coords_channel * embsize
        if a == 0:
            return round(-c / b)
        return round((-b + math.sqrt(b ** 2 - 4 * a * c)) / (2 * a))

    @staticmethod
    def _no_skip(skip):
        if skip:
            raise NotImplementedError("FFN(skip=True) is unsupported on the fused path")


class NeRF(_FusedFamily):
    """reference: utils/Networks.py:64-136 (PosEncodingNeRF + NeRF).  Parameters live in one canonical buffer in state_dict() order
    [W0 b0 | hidden | head] (include/brief_hip.h, brief_nerf_desc); with skip the hidden layer sl = (layers - 1) // 2 is
    Linear(d + F, F) on cat[encoding, h].  The encoding has no parameters; the whole buffer is trained.  Like FFN it has fp32 kernels
    only (half() / low-precision modes run in fp32 with a warning)."""

    kind = "NeRF"
    _abi, _fit_job, _fit_entry, _family = "brief_nerf_", _lib.NerfFitJob, "brief_nerf_fit", "NeRF"

    def __init__(self, coords_channel=3, data_channel=1, frequencies=10, features=256, layers=5, skip=True,
                 device=None, precision="fp32", **kwargs):
        """w0 / res / output_act / embsize of another net's YAML are ignored, as NeRF(**phi) ignores them.  precision: the fused path
        is fp32 only; 'bf16' / 'bf16x3' run in fp32 with a warning."""
        if str(precision) not in ("fp32", "f32"):
            logging.warning("NeRF: no %s kernels; the net runs in fp32" % precision)
        self.coords_channel, self.data_channel = int(coords_channel), int(data_channel)
        self.features, self.layers = int(features), int(layers)
        self.frequencies, self.skip = int(frequencies), bool(skip)
        NeRF._check(self.coords_channel, self.data_channel, self.features, self.frequencies, self.layers, self.skip)
        self.precision = "fp32"
        self.w0, self.output_act = 0.0, False
        self.desc = _lib.NerfDesc(self.coords_channel, self.data_channel, self.layers, self.features, self.frequencies, int(self.skip))
        F, d = self.features, NeRF.encoding_width(self.coords_channel, self.frequencies)
        self.skip_layer = (self.layers - 1) // 2 if self.skip else -1
        self._shapes = [(F, d)] + [(F, d + F if l == self.skip_layer else F) for l in range(1, self.layers - 1)] + [(self.data_channel, F)]
        self.bv_count = 0
        self.param_count = sum(o * i + o for o, i in self._shapes)
        self.params = self._reference_init()
        self.grads = None
        self.packed = None
        self.qparams = None
        self._stale = True
        self._seen_version = -1
        self._autograd = False
        self._anchor = None
        self._ws = None
        self._fws = None
        self._loss = None
        self.positional_encoding = _PosEncoding(self.coords_channel, self.frequencies)
        net, off = [], 0
        for (o, i) in self._shapes:
            net.append(_Seq(_Linear(self, off, (o, i), off + o * i)))
            off += o * i + o
        self.net = net
        if device is not None:
            self.to(device)

    @staticmethod
    def encoding_width(coords_channel, frequencies):
        """PosEncodingNeRF.out_channel: cin (1 + 2 frequencies)"""
        return coords_channel + 2 * coords_channel * frequencies

    @staticmethod
    def _check(cin, cout, features, frequencies, layers, skip):
        """the limits of include/brief_hip.h (brief_nerf_desc); the reference itself fails on layers = 2 with skip (its forward
        concatenates the encoding with itself)"""
        if cin not in (2, 3) or not 1 <= cout <= 4:
            raise NotImplementedError("NeRF: coords_channel must be 2 or 3 and data_channel 1..4")
        if layers < 2 or (skip and layers < 3):
            raise NotImplementedError("NeRF: layers must be >= 2, and >= 3 with skip=True (got layers=%d, skip=%s)" % (layers, skip))
        if not 1 <= features <= 1024:
            raise NotImplementedError("NeRF: features must be 1..1024 on the fused path (got %d)" % features)
        if not 0 <= frequencies <= 16:
            raise NotImplementedError("NeRF: frequencies must be 0..16 on the fused path (got %d)" % frequencies)

    def _reference_init(self):
        """the nn.Linear default inits (kaiming_uniform(a=sqrt 5) weight, then bias; fan-in d + F for the skip layer) in layer order on
        the caller's global generator (NeRF does not reseed): the values AND the generator state afterwards equal the reference's"""
        parts = []
        for (o, i) in self._shapes:
            w = torch.empty(o, i)
            gain = math.sqrt(2.0 / (1 + math.sqrt(5) ** 2))
            w.uniform_(-math.sqrt(3.0) * gain / math.sqrt(i), math.sqrt(3.0) * gain / math.sqrt(i))
            b = torch.empty(o)
            b.uniform_(-1 / math.sqrt(i), 1 / math.sqrt(i))
            parts += [w.reshape(-1), b]
        return torch.cat(parts).contiguous()

    # ---- budget -> width (utils/Networks.py:118-136)
    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, frequencies, layers, skip, **kwargs):
        """the reference's signature (frequencies, layers and skip have no default) and formula: d F + F + (layers-2)(F^2 + F) [+ d F with skip] + F cout + cout, d = cin (1 + 2 frequencies)"""
        d = NeRF.encoding_width(coords_channel, frequencies)
        return int(d * features + features + (layers - 2) * (features ** 2 + features) + (d * features if skip else 0)
                   + features * data_channel + data_channel)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, frequencies, layers, skip, **kwargs):
        """the reference's signature (frequencies, layers and skip have no default); the positive root of (layers-2) F^2 + ([2] d + 1 + layers-2 + cout) F + cout = P, rounded (the reference's formula; the
        linear case layers = 2 solved directly instead of dividing by zero)"""
        d = NeRF.encoding_width(coords_channel, frequencies)
        a = layers - 2
        b = (2 * d if skip else d) + 1 + layers - 2 + data_channel
        c = -param_count + data_channel
        if a == 0:
            return round(-c / b)
        return round((-b + math.sqrt(b ** 2 - 4 * a * c)) / (2 * a))


class _MFNBase(_FusedFamily):
    """reference: utils/Networks.py:648-799 (MFNBase + FourierLayer / GaborLayer).  Parameters live in one canonical buffer in
    state_dict() order [linear.i (W b) | output_linear | per filter: (mu gamma) linear] (include/brief_hip.h, brief_mfn_desc); the whole
    buffer is trained.  `linear[i]`, `output_linear`, `filters[i].linear` and `filters[i].mu` / `.gamma` are windows into it.  There is
    no `.net`: ModelSave takes its state_dict branch (one torch.save file), as it does for the reference's MFN.  fp32 kernels only."""

    _abi, _fit_job, _fit_entry, _family = "brief_mfn_", _lib.MfnFitJob, "brief_mfn_fit", "MFN"
    GABOR = False

    def __init__(self, coords_channel=3, features=256, data_channel=1, layers=5, input_scale=256.0, weight_scale=1.0, bias=True,
                 output_act=False, device=None, precision="fp32", alpha=6.0, beta=1.0, **kwargs):
        """the reference's signature and defaults; w0 / res / embsize / frequencies / skip of another net's YAML are ignored, as its
        **kwargs ignores them.  input_scale, weight_scale, alpha and beta shape the init only."""
        name = type(self).kind
        if not bias:
            raise NotImplementedError("%s(bias=False) is unsupported on the fused path (it changes the state_dict keys and the "
                                      "reference's budget rule ignores it)" % name)
        if str(precision) not in ("fp32", "f32"):
            logging.warning("%s: no %s kernels; the net runs in fp32" % (name, precision))
        self.coords_channel, self.data_channel = int(coords_channel), int(data_channel)
        self.features, self.layers = int(features), int(layers)
        _MFNBase._check(name, self.coords_channel, self.data_channel, self.features, self.layers)
        self.input_scale, self.weight_scale = float(input_scale), float(weight_scale)
        self.alpha, self.beta = float(alpha), float(beta)
        self.precision = "fp32"
        self.w0, self.output_act = 0.0, bool(output_act)
        self.desc = _lib.MfnDesc(self.coords_channel, self.data_channel, self.layers, self.features, int(self.GABOR), int(self.output_act))
        F, cin, cout, L = self.features, self.coords_channel, self.data_channel, self.layers
        ent = []
        for i in range(L - 2):
            ent += [("linear.%d.weight" % i, (F, F)), ("linear.%d.bias" % i, (F,))]
        ent += [("output_linear.weight", (cout, F)), ("output_linear.bias", (cout,))]
        for i in range(L - 1):
            if self.GABOR:
                ent += [("filters.%d.mu" % i, (F, cin)), ("filters.%d.gamma" % i, (F,))]
            ent += [("filters.%d.linear.weight" % i, (F, cin)), ("filters.%d.linear.bias" % i, (F,))]
        self._entries, off = [], 0
        for k, shp in ent:
            self._entries.append((k, off, shp))
            off += int(np.prod(shp))
        self.bv_count = 0
        self.param_count = off
        self.params = self._reference_init()
        self.grads = None
        self.packed = None
        self.qparams = None
        self._stale = True
        self._seen_version = -1
        self._autograd = False
        self._anchor = None
        self._ws = None
        self._fws = None
        self._loss = None
        views = {k: _ParamView(self, o, shp) for k, o, shp in self._entries}
        lin = (lambda p: _Window(views[p + ".weight"], views[p + ".bias"]))
        self.linear = [lin("linear.%d" % i) for i in range(L - 2)]
        self.output_linear = lin("output_linear")
        self.filters = [_Filter(lin("filters.%d.linear" % i), views.get("filters.%d.mu" % i), views.get("filters.%d.gamma" % i))
                        for i in range(L - 1)]
        if device is not None:
            self.to(device)

    @staticmethod
    def _check(name, cin, cout, features, layers):
        """the limits of include/brief_hip.h (brief_mfn_desc)"""
        if cin not in (2, 3) or not 1 <= cout <= 4:
            raise NotImplementedError("%s: coords_channel must be 2 or 3 and data_channel 1..4" % name)
        if layers < 2:
            raise NotImplementedError("%s: layers must be >= 2 (got %d)" % (name, layers))
        if not 1 <= features <= 1024:
            raise NotImplementedError("%s: features must be 1..1024 on the fused path (got %d)" % (name, features))

    def _reference_init(self):
        """MFNBase.__init__ then the filters, replayed with torch on the caller's global CPU generator (no reseed): the hidden
        nn.Linear(F, F) and output_linear default draws, the hidden weights re-drawn as uniform(+-sqrt(weight_scale / F)), then per
        filter its nn.Linear(cin, F) draws [Gabor: mu = 2 rand(F, cin) - 1, gamma = Gamma(alpha / (L-1), beta).sample((F,))], the
        weight scaled by input_scale / sqrt(L-1) [* sqrt(gamma)] and the bias re-drawn as uniform(-pi, pi).  The values AND the
        generator state afterwards equal the reference's."""
        F, cin, cout, L = self.features, self.coords_channel, self.data_channel, self.layers
        with torch.no_grad():
            hidden = [torch.nn.Linear(F, F) for _ in range(L - 2)]
            head = torch.nn.Linear(F, cout)
            for lin in hidden:
                lin.weight.data.uniform_(-np.sqrt(self.weight_scale / F), np.sqrt(self.weight_scale / F))
            parts = []
            for lin in hidden:
                parts += [lin.weight.data.reshape(-1), lin.bias.data]
            parts += [head.weight.data.reshape(-1), head.bias.data]
            scale = self.input_scale / np.sqrt(L - 1)
            for _ in range(L - 1):
                lin = torch.nn.Linear(cin, F)
                if self.GABOR:
                    mu = 2 * torch.rand(F, cin) - 1
                    gamma = torch.distributions.gamma.Gamma(self.alpha / (L - 1), self.beta).sample((F,))
                    # torch.sqrt as the reference calls it: its CPU kernel is not correctly rounded everywhere, so these bits follow
                    # the reference on the same machine (tests/test_gpu_mfn_framework.py)
                    lin.weight.data *= scale * torch.sqrt(gamma[:, None])
                    parts += [mu.reshape(-1), gamma]
                else:
                    lin.weight.data *= scale
                lin.bias.data.uniform_(-np.pi, np.pi)
                parts += [lin.weight.data.reshape(-1), lin.bias.data]
            return torch.cat([p.to(torch.float32) for p in parts]).contiguous()

    def state_dict(self):
        """the reference's keys in its order; every value a contiguous CPU float32 tensor with its own storage of exactly its size
        (torch.save writes the whole storage of a view)"""
        sd = OrderedDict()
        for k, o, shp in self._entries:
            n = int(np.prod(shp))
            sd[k] = self.params[o:o + n].detach().to("cpu", torch.float32).clone().view(shp)
        return sd

    def load_state_dict(self, sd):
        want = [k for k, _, _ in self._entries]
        if set(sd.keys()) != set(want):
            missing, extra = [k for k in want if k not in sd], [k for k in sd if k not in want]
            raise KeyError("%s.load_state_dict: missing keys %s, unexpected keys %s" % (type(self).kind, missing, extra))
        for k, o, shp in self._entries:
            v = torch.as_tensor(sd[k], dtype=torch.float32)
            if tuple(v.shape) != tuple(shp):
                raise ValueError("%s.load_state_dict: %s has shape %s, expected %s" % (type(self).kind, k, tuple(v.shape), tuple(shp)))
            self.params[o:o + v.numel()].copy_(v.reshape(-1).to(self.params.device))
        self._stale = True

    # ---- budget -> width (utils/Networks.py:721-731, 787-797)
    FILTER_PARAMS = 1       # per feature and filter: (cin + 1) x FILTER_PARAMS

    @classmethod
    def _count(cls, coords_channel, data_channel, features, layers):
        F = features
        return int((layers - 2) * (F ** 2 + F) + F * data_channel + data_channel + (layers - 1) * cls.FILTER_PARAMS * (coords_channel * F + F))

    @classmethod
    def _features(cls, param_count, coords_channel, data_channel, layers):
        """the positive root of (L-2) F^2 + (L-2 + cout + (L-1) k (1 + cin)) F + cout = P, rounded (the reference's formula; the
        linear case L = 2, where the reference divides by zero, solved directly)"""
        a = layers - 2
        b = layers - 2 + data_channel + (layers - 1) * cls.FILTER_PARAMS * (1 + coords_channel)
        c = -param_count + data_channel
        if a == 0:
            return round(-c / b)
        return round((-b + math.sqrt(b ** 2 - 4 * a * c)) / (2 * a))


class MFNFourier(_MFNBase):
    """reference: utils/Networks.py:667-731 (MFNBase + FourierLayer): g_i = sin(Wf_i x + bf_i)"""

    kind = "MFNFourier"
    GABOR = False
    FILTER_PARAMS = 1

    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, **kwargs):
        return MFNFourier._count(coords_channel, data_channel, features, layers)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, **kwargs):
        return MFNFourier._features(param_count, coords_channel, data_channel, layers)


class MFNGabor(_MFNBase):
    """reference: utils/Networks.py:732-797 (MFNBase + GaborLayer): g_i = sin(Wf_i x + bf_i) exp(-gamma_i (|x|^2 + |mu_i|^2 - 2 x.mu_i) / 2)"""

    kind = "MFNGabor"
    GABOR = True
    FILTER_PARAMS = 2

    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, **kwargs):
        return MFNGabor._count(coords_channel, data_channel, features, layers)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, **kwargs):
        return MFNGabor._features(param_count, coords_channel, data_channel, layers)


class _TaperBase(_FusedFamily):
    """the tapered SIRENs of the reference (utils/Networks.py:316-552): a SIREN whose every Linear has its own width and every sine its
    own w0.  Parameters live in one canonical buffer in state_dict() order (W_l b_l per Linear); `.net[l][0].weight / .bias`, the
    state_dict keys, the init replay and the raw weight-l-out-in / bias-l-n artefact are SIREN's.  The subclasses give the widths and the
    budget rules.  fp32 kernels only (include/brief_hip.h, brief_taper_desc)."""

    _abi, _fit_job, _fit_entry, _family = "brief_taper_", _lib.TaperFitJob, "brief_taper_fit", "tapered-SIREN"
    MAX_LAYERS, MAX_WIDTH = _lib.TAPER_MAX_LAYERS, 1024

    def _setup(self, coords_channel, data_channel, features, layers, w0, res, output_act, device, precision, widths, w0s):
        name = type(self).kind
        _TaperBase._no_res(name, res)
        if str(precision) not in ("fp32", "f32"):
            logging.warning("%s: no %s kernels; the net runs in fp32" % (name, precision))
        self.coords_channel, self.data_channel = int(coords_channel), int(data_channel)
        self.features, self.layers = features, int(layers)       # features: as given (a float for SIRENFT / SIRENPS, truncated per layer)
        self.widths = [int(v) for v in widths]
        _TaperBase._check(name, self.coords_channel, self.data_channel, self.layers, self.widths)
        self.precision = "fp32"
        self.w0, self.output_act = float(w0), bool(output_act)
        self.w0s = [float(v) for v in w0s] + [30.0]               # the sine behind every Linear (the last: the output activation, Sine())
        wd = (C.c_int32 * self.MAX_LAYERS)(*self.widths)
        ww = (C.c_float * self.MAX_LAYERS)(*self.w0s)
        self.desc = _lib.TaperDesc(self.coords_channel, self.data_channel, self.layers, int(self.output_act), wd, ww)
        ins = [self.coords_channel] + self.widths
        outs = self.widths + [self.data_channel]
        self._shapes = list(zip(outs, ins))
        self.bv_count = 0
        self.param_count = sum(o * i + o for o, i in self._shapes)
        self.params = SIREN._reference_init(self)
        self.grads = None
        self.packed = None
        self.qparams = None
        self._stale = True
        self._seen_version = -1
        self._autograd = False
        self._anchor = None
        self._ws = None
        self._fws = None
        self._loss = None
        net, off = [], 0
        for (o, i) in self._shapes:
            net.append(_Seq(_Linear(self, off, (o, i), off + o * i)))
            off += o * i + o
        self.net = net
        if device is not None:
            self.to(device)

    @staticmethod
    def _no_res(name, res):
        if res:
            # HalfResidual blocks cannot be saved by the reference's own ModelSave (as for SIREN)
            raise NotImplementedError("%s(res=True) is unsupported on the fused path" % name)

    @staticmethod
    def _check_layers(name, layers):
        if not 3 <= layers <= _TaperBase.MAX_LAYERS:
            raise NotImplementedError("%s: layers must be 3..%d (got %d); the reference's own rules divide by zero or miscount at layers = 2"
                                      % (name, _TaperBase.MAX_LAYERS, layers))

    @staticmethod
    def _check(name, cin, cout, layers, widths):
        """the limits of include/brief_hip.h (brief_taper_desc)"""
        if cin not in (2, 3) or not 1 <= cout <= 4:
            raise NotImplementedError("%s: coords_channel must be 2 or 3 and data_channel 1..4" % name)
        _TaperBase._check_layers(name, layers)
        if min(widths) < 1:
            raise ValueError("%s: a layer of width %d (layer widths %s): every hidden width must be >= 1" % (name, min(widths), widths))
        if max(widths) > _TaperBase.MAX_WIDTH:
            raise NotImplementedError("%s: every hidden width must be 1..1024 on the fused path (layer widths %s)" % (name, widths))

    @staticmethod
    def _count(cin, cout, widths):
        ins, outs = [cin] + list(widths), list(widths) + [cout]
        return sum(o * i + o for o, i in zip(outs, ins))


class SIREN_Pyramid(_TaperBase):
    """reference: utils/Networks.py:370-457.  Hidden widths F, F - d, ..., F - (layers - 2) d (d = features_dis; negative d grows)."""

    kind = "SIREN_Pyramid"

    def __init__(self, coords_channel=3, data_channel=1, features=256, layers=5, w0=30, res=False, output_act=False, features_dis=10,
                 device=None, precision="fp32", **kwargs):
        _TaperBase._no_res(self.kind, res)
        _TaperBase._check_layers(self.kind, int(layers))
        if int(features) != features or int(features_dis) != features_dis:
            raise ValueError("SIREN_Pyramid: features and features_dis must be integers (got %r, %r)" % (features, features_dis))
        self.features_dis = int(features_dis)
        widths = SIREN_Pyramid.layer_widths(int(features), int(layers), self.features_dis)
        self._setup(coords_channel, data_channel, int(features), layers, w0, res, output_act, device, precision,
                    widths, [w0] + [30.0] * (int(layers) - 2))

    @staticmethod
    def layer_widths(features, layers, features_dis):
        return [features - i * features_dis for i in range(layers - 1)]

    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, res, features_dis, **kwargs):
        _TaperBase._no_res("SIREN_Pyramid", res)
        return int(_TaperBase._count(coords_channel, data_channel, SIREN_Pyramid.layer_widths(features, layers, features_dis)))

    @staticmethod
    def check_param_count(param_count, coords_channel, data_channel, layers, res, features_dis, **kwargs):
        """the budget floor: the pyramid whose last hidden layer has width 1"""
        _TaperBase._no_res("SIREN_Pyramid", res)
        floor = _TaperBase._count(coords_channel, data_channel, SIREN_Pyramid.layer_widths(1 + (layers - 2) * features_dis, layers, features_dis))
        return bool(param_count >= floor)

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, res, features_dis, **kwargs):
        """the positive root of the reference's quadratic in F (the widths' products summed in closed form), rounded; ValueError when
        the last hidden layer would have width <= 0 (as the reference)"""
        _TaperBase._no_res("SIREN_Pyramid", res)
        _TaperBase._check_layers("SIREN_Pyramid", layers)
        l, c, d, o = layers, coords_channel, features_dis, data_channel
        a = l - 2
        b = c + 1 + (1 - d) * (l - 2) - (l - 2) * (l - 3) * d + o
        cc = ((l - 2) * (1 - d) ** 2 / 4 - (l - 2) * (l - 3) * d + (l - 2) * (l - 3) * (2 * l - 5) * d ** 2 / 6 - (l - 2) * (1 + d) ** 2 / 4
              - (l - 2) * d * o + o - param_count)
        features = round((-b + math.sqrt(b ** 2 - 4 * a * cc)) / (2 * a))
        if features - (l - 2) * d <= 0 or features <= 0:
            raise ValueError("SIREN_Pyramid: the budget of %s parameters gives features=%d, a last hidden width of %d" % (param_count, features, features - (l - 2) * d))
        return features


class SIRENFT(_TaperBase):
    """reference: utils/Networks.py:316-369.  Hidden widths int(F ratio), int(F), ..., int(F); the sines behind Linear 0 AND Linear 1
    carry w0 (the reference's :324), the others 30."""

    kind = "SIRENFT"

    def __init__(self, coords_channel=3, data_channel=1, features=256, layers=5, w0=30, res=False, output_act=False, ratio=1,
                 device=None, precision="fp32", **kwargs):
        _TaperBase._no_res(self.kind, res)
        _TaperBase._check_layers(self.kind, int(layers))
        self.ratio = ratio
        widths = SIRENFT.layer_widths(features, int(layers), ratio)
        self._setup(coords_channel, data_channel, features, layers, w0, res, output_act, device, precision,
                    widths, [w0, w0] + [30.0] * (int(layers) - 3))

    @staticmethod
    def layer_widths(features, layers, ratio):
        return [int(features * ratio)] + [int(features)] * (layers - 2)

    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, res, ratio, **kwargs):
        _TaperBase._no_res("SIRENFT", res)
        return int(_TaperBase._count(coords_channel, data_channel, SIRENFT.layer_widths(features, layers, ratio)))

    @staticmethod
    def check_param_count(param_count, coords_channel, data_channel, layers, res, ratio, **kwargs):
        """the budget floor: features = 1"""
        _TaperBase._no_res("SIRENFT", res)
        return bool(param_count >= _TaperBase._count(coords_channel, data_channel, SIRENFT.layer_widths(1, layers, ratio)))

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, res, ratio, **kwargs):
        """the positive root of (r + L - 3) F^2 + (cin r + r + 1 + L - 3 + cout) F + cout = P as a FLOAT (the reference does not round:
        the constructor truncates F and F r)"""
        _TaperBase._no_res("SIRENFT", res)
        _TaperBase._check_layers("SIRENFT", layers)
        a = ratio + layers - 3
        b = coords_channel * ratio + ratio + 1 + layers - 3 + data_channel
        c = data_channel - param_count
        features = (-b + math.sqrt(b ** 2 - 4 * a * c)) / (2 * a)
        if min(SIRENFT.layer_widths(features, layers, ratio)) < 1:
            raise ValueError("SIRENFT: the budget of %s parameters gives features=%s, a layer of width 0" % (param_count, features))
        return features


class SIRENPS(_TaperBase):
    """reference: utils/Networks.py:458-552.  Hidden widths int(F r^(L-2)), int(F r^(L-3)), ..., int(F r), int(F) (a geometric taper)."""

    kind = "SIRENPS"

    def __init__(self, coords_channel=3, data_channel=1, features=256, layers=5, w0=30, res=False, output_act=False, ratio=1,
                 device=None, precision="fp32", **kwargs):
        _TaperBase._no_res(self.kind, res)
        _TaperBase._check_layers(self.kind, int(layers))
        SIRENPS._no_unit_ratio(ratio)
        self.ratio = ratio
        widths = SIRENPS.layer_widths(features, int(layers), ratio)
        self._setup(coords_channel, data_channel, features, layers, w0, res, output_act, device, precision,
                    widths, [w0] + [30.0] * (int(layers) - 2))

    @staticmethod
    def _no_unit_ratio(ratio):
        if ratio == 1:
            raise ValueError("SIRENPS(ratio=1) is refused: the reference's budget rule divides by zero at ratio == 1 (use SIREN)")

    @staticmethod
    def layer_widths(features, layers, ratio):
        return [int(features * ratio ** (layers - 2 - i)) for i in range(layers - 1)]

    @staticmethod
    def calc_param_count(coords_channel, data_channel, features, layers, res, ratio, **kwargs):
        """the reference's count: the head is counted with the FLOAT width (features * data_channel), so with data_channel > 1 it can
        exceed the module's own count by 1-2"""
        _TaperBase._no_res("SIRENPS", res)
        w = SIRENPS.layer_widths(features, layers, ratio)
        count = _TaperBase._count(coords_channel, data_channel, w) - w[-1] * data_channel + features * data_channel
        return int(count)

    @staticmethod
    def check_param_count(param_count, coords_channel, data_channel, layers, res, ratio, **kwargs):
        """the budget floor: features = 1"""
        _TaperBase._no_res("SIRENPS", res)
        return bool(param_count >= SIRENPS.calc_param_count(coords_channel, data_channel, 1, layers, res, ratio))

    @staticmethod
    def calc_features(param_count, coords_channel, data_channel, layers, res, ratio, **kwargs):
        """the positive root of the geometric sums in F as a FLOAT (not rounded), with the reference's own identity check (< 1 parameter)"""
        _TaperBase._no_res("SIRENPS", res)
        _TaperBase._check_layers("SIRENPS", layers)
        SIRENPS._no_unit_ratio(ratio)
        l, c, o, r = layers, coords_channel, data_channel, ratio
        a = r * (1 - (r ** 2) ** (l - 2)) / (1 - r ** 2)
        b = (1 - r ** (l - 2)) / (1 - r) + (c + 1) * r ** (l - 2) + o
        cc = o - param_count
        features = (-b + math.sqrt(b ** 2 - 4 * a * cc)) / (2 * a)
        if features <= 0:
            raise ValueError("SIRENPS: the budget of %s parameters gives features=%s" % (param_count, features))
        w = [features * r ** (l - 2 - i) for i in range(l - 1)]
        ident = _TaperBase._count(c, o, w)
        assert abs(param_count - ident) < 1, "ERROR!"
        if min(SIRENPS.layer_widths(features, layers, ratio)) < 1:
            raise ValueError("SIRENPS: the budget of %s parameters gives features=%s, a layer of width 0" % (param_count, features))
        return features


class _Window:
    """stands for an nn.Linear of an MFN: `.weight` / `.bias` are windows into the canonical buffer"""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.out_features, self.in_features = weight.shape[0], weight.shape[1]


class _Filter:
    """stands for FourierLayer / GaborLayer: `.linear`, and for Gabor `.mu` / `.gamma` (windows into the canonical buffer)"""

    def __init__(self, linear, mu=None, gamma=None):
        self.linear = linear
        if mu is not None:
            self.mu, self.gamma = mu, gamma


class _PosEncoding:
    """stands for PosEncodingNeRF (no parameters): the encoding runs inside the fused kernels"""

    def __init__(self, in_channel, frequencies):
        self.in_channel, self.frequencies = in_channel, frequencies
        self.out_channel = NeRF.encoding_width(in_channel, frequencies)


class _Embedding:
    """stands for FourierFeatureEmbedding: `.bvals` is a window into the canonical buffer (requires_grad False)"""

    def __init__(self, bvals):
        self.bvals = bvals
        self.requires_grad = False


def _dev_ptr(t, dtype, what, device):
    """data_ptr() of a tensor the C-ABI will read as `dtype`: wrong dtype / layout / device is an error here, not
    silently reinterpreted bits in the kernel"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise _lib.BriefError("%s must be a %s tensor (got %s)" % (what, dtype, getattr(t, "dtype", type(t))))
    if not t.is_contiguous():
        raise _lib.BriefError("%s must be contiguous" % what)
    if t.device != device:
        raise _lib.BriefError("%s must live on %s (got %s)" % (what, device, t.device))
    return t.data_ptr()


def get_nnmodule_param_count(module):
    """utils/Networks.py:13-17"""
    return sum(int(np.prod(p.shape)) for p in module.state_dict().values())


# registry with the reference's names (utils/Networks.py:795-802).  SIREN, FFN, NeRF, MFNFourier, MFNGabor, SIREN_Pyramid, SIRENFT and
# SIRENPS exist on the fused path; every other phi.name of the reference raises instead of silently running something else.
ALLPHI = {"SIREN": SIREN, "FFN": FFN, "NeRF": NeRF, "MFNFourier": MFNFourier, "MFNGabor": MFNGabor,
          "SIREN_Pyramid": SIREN_Pyramid, "SIRENFT": SIRENFT, "SIRENPS": SIRENPS}
ALL_CALC_PHI_FEATURES = {k: v.calc_features for k, v in ALLPHI.items()}
ALL_CALC_PHI_PARAM_COUNT = {k: v.calc_param_count for k, v in ALLPHI.items()}
# budget floors (main.py:222-234): the only nets NFGR.estimate_module_size knows by name; under its floor SIREN_Pyramid becomes SIRENFT,
# SIRENFT and SIRENPS become SIREN
ALL_CHECK_PARAM_COUNT = {"SIREN_Pyramid": SIREN_Pyramid.check_param_count, "SIRENFT": SIRENFT.check_param_count,
                         "SIRENPS": SIRENPS.check_param_count}
# keys a Module.phi spec of this net must name: the reference's NeRF budget rule (calc_features / calc_param_count,
# utils/Networks.py:118-136) takes frequencies and skip without defaults, so its NFGR cannot build a NeRF from a spec that leaves them
# out; init_phi refuses such a spec by name instead of filling in the constructor's defaults
# (the MFN budget rules, utils/Networks.py:727-731 / 793-797, take coords_channel, data_channel and layers without defaults; the
# tapered SIRENs' rules, :347-369 / :417-457 / :488-552, also res and features_dis or ratio)
_TAPER_KEYS = ("coords_channel", "data_channel", "layers", "res")
REQUIRED_PHI_KEYS = {"NeRF": ("frequencies", "skip"), "MFNFourier": ("coords_channel", "data_channel", "layers"),
                     "MFNGabor": ("coords_channel", "data_channel", "layers"), "SIREN_Pyramid": _TAPER_KEYS + ("features_dis",),
                     "SIRENFT": _TAPER_KEYS + ("ratio",), "SIRENPS": _TAPER_KEYS + ("ratio",)}


def init_phi(kwargs):
    kwargs = copy.deepcopy(dict(kwargs))
    name = kwargs.pop("name")
    if name not in ALLPHI:
        raise NotImplementedError("Module.phi.name=%r is not available on the fused MI355X path (only SIREN, FFN, NeRF, MFNFourier, "
                                  "MFNGabor, SIREN_Pyramid, SIRENFT and SIRENPS)" % name)
    missing = [k for k in REQUIRED_PHI_KEYS.get(name, ()) if k not in kwargs]
    if missing:
        raise NotImplementedError("Module.phi.name=%r without %s is not supported: the reference's budget rule for this net needs %s "
                                  "in the spec" % (name, " / ".join(missing), " and ".join(REQUIRED_PHI_KEYS[name])))
    return ALLPHI[name](**kwargs)
