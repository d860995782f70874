"""Refusals of the C-ABI entries of FFN, NeRF, MFN and the tapered SIRENs (include/brief_hip.h).  The four families run behind one host
driver (csrc/brief_family_host.inc), so every entry of every family is called here with one bad argument that it rejects on the host,
before any device work: no kernel is launched.  The return code and the exact brief_last_error() text are asserted; the texts are the
ones the entries have had since each family was added."""
import ctypes as C

import pytest
import torch

from brief_pytorch_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID, WORKSPACE = -1, -3      # BRIEF_ERR_INVALID, BRIEF_ERR_WORKSPACE
N = 64                           # samples of every well-formed batch here


def _taper_desc():
    widths = (C.c_int32 * _lib.TAPER_MAX_LAYERS)(24, 20, 16)
    w0 = (C.c_float * _lib.TAPER_MAX_LAYERS)(30.0, 30.0, 30.0, 30.0)
    return _lib.TaperDesc(3, 1, 4, 0, widths, w0)


# family: (entry prefix, a desc the library accepts, its fit job type, what its fit says about an index stream without a stride)
FAMILIES = {
    "ffn": ("brief_ffn_", lambda: _lib.FfnDesc(3, 1, 4, 24, 8, 0), _lib.FfnFitJob,
            "brief_ffn_fit needs idx_stride > 0 with batch.idx (one index set per step)"),
    "nerf": ("brief_nerf_", lambda: _lib.NerfDesc(3, 1, 4, 24, 2, 1), _lib.NerfFitJob,
             "brief_nerf_fit needs idx_stride > 0 with batch.idx (one index set per step)"),
    "mfn": ("brief_mfn_", lambda: _lib.MfnDesc(3, 1, 4, 24, 1, 0), _lib.MfnFitJob,
            "brief_mfn_fit needs idx_stride > 0 with batch.idx (one index set per step)"),
    "taper": ("brief_taper_", _taper_desc, _lib.TaperFitJob,
              "brief_taper_fit needs idx_stride > 0 with batch.idx (one index set per step)"),
}


class _Family:
    """one family's entries, a valid desc and well-formed arguments for each entry; a test replaces ONE of them"""

    def __init__(self, name):
        self.prefix, make, self.Job, self.no_stride = FAMILIES[name]
        self.d = make()
        L = _lib.lib()
        self.fn = lambda entry: getattr(L, self.prefix + entry)
        self.need = self.fn("train_workspace_bytes")(C.byref(self.d), N)
        assert self.need > 0
        self.count = self.fn("param_count")(C.byref(self.d))
        self.packed_count = self.fn("packed_count")(C.byref(self.d))
        assert self.count > 0 and self.packed_count > 0
        f32 = lambda n: torch.zeros(int(n), dtype=torch.float32, device=DEV)
        self.params, self.packed, self.grads = f32(self.count), f32(self.packed_count), f32(self.count)
        self.s1, self.s2, self.loss = f32(self.count), f32(self.count), f32(1)
        self.ws = f32((self.need + 3) // 4)
        self.coords, self.targets, self.out = f32(3 * N), f32(N), f32(N)
        self.idx = torch.zeros(2 * N, dtype=torch.int64, device=DEV)
        self.grid = _lib.GridDesc()
        self.grid.ndim = 3
        for a in range(3):
            self.grid.dims[a] = 8
        self.grid.lo, self.grid.hi = -1.0, 1.0
        self.box = _lib.GridBox()
        self.box.grid = self.grid
        for a in range(3):
            self.box.start[a], self.box.step[a], self.box.extent[a] = 0, 1, 8      # 512 voxels

    def batch(self, n=N, idx=None):
        return _lib.BatchDesc(_lib.ptr(self.coords), _lib.ptr(self.targets), None, _lib.ptr(idx), 0, n, 0, 0, 0)

    def forward(self, desc="own", packed="own", out_kind=_lib.OUT_F32, n=N):
        b = self.batch(n)
        return self.fn("forward")(C.byref(self.d) if desc == "own" else None, _lib.ptr(self.packed) if packed == "own" else None, None, C.byref(b),
                                  _lib.ptr(self.out), out_kind, 0.0, 1.0, 0.0, 1.0, None)

    def forward_box(self, desc="own", packed="own", out_kind=_lib.OUT_F32, offset=0, n=N):
        return self.fn("forward_box")(C.byref(self.d) if desc == "own" else None, _lib.ptr(self.packed) if packed == "own" else None, C.byref(self.box),
                                      offset, n, _lib.ptr(self.out), out_kind, 0.0, 1.0, 0.0, 1.0, None)

    def train_step(self, desc="own", packed="own", loss_kind=0, n=N, ws_bytes=None):
        b = self.batch(n)
        return self.fn("train_step")(C.byref(self.d) if desc == "own" else None, _lib.ptr(self.packed) if packed == "own" else None, None, C.byref(b),
                                     loss_kind, 0.0, 0.01, _lib.ptr(self.grads), _lib.ptr(self.loss), None,
                                     _lib.ptr(self.ws), self.need if ws_bytes is None else ws_bytes, None)

    def fit(self, steps=1, **change):
        """brief_<family>_fit on a well-formed Adamax job (samples drawn from the grid by offset), with the fields of `change` replaced"""
        j = self.Job()
        j.desc, j.grid = self.d, self.grid
        j.batch = _lib.BatchDesc(None, _lib.ptr(self.targets), None, None, 0, N, 0, 0, 0)
        j.params, j.packed, j.state1, j.state2 = self.params.data_ptr(), self.packed.data_ptr(), self.s1.data_ptr(), self.s2.data_ptr()
        j.grads, j.loss_out, j.loss_log = self.grads.data_ptr(), self.loss.data_ptr(), None
        j.workspace, j.workspace_bytes = self.ws.data_ptr(), self.need
        j.loss_kind, j.optim_kind, j.thr, j.beta = 0, _lib.OPT_KIND["Adamax"], 0.0, 0.01
        j.lr, j.beta1, j.beta2, j.eps = 1e-3, 0.9, 0.999, 1e-8
        j.n_milestones, j.gamma, j.t0, j.idx_stride = 0, 1.0, 0, 0
        for k, v in change.items():
            if k in ("n", "idx"):
                setattr(j.batch, k, v)
            else:
                setattr(j, k, v)
        return self.fn("fit")(C.byref(j), steps, None)


@pytest.fixture(scope="module", params=sorted(FAMILIES))
def fam(request):
    return _Family(request.param)


def _refused(rc, code, text):
    assert rc == code
    assert _lib.lib().brief_last_error().decode() == text


def test_null_desc(fam):
    _refused(fam.forward(desc=None), INVALID, "null desc")
    _refused(fam.forward_box(desc=None), INVALID, "null desc")
    _refused(fam.train_step(desc=None), INVALID, "null desc")
    assert fam.fn("train_workspace_bytes")(None, N) == -1
    assert _lib.lib().brief_last_error().decode() == "null desc"
    _refused(fam.fn("fit")(None, 1, None), INVALID, "null job")


def test_null_packed(fam):
    _refused(fam.forward(packed=None), INVALID, "null buffer")
    _refused(fam.forward_box(packed=None), INVALID, "null buffer")
    _refused(fam.train_step(packed=None), INVALID, "null buffer")
    _refused(fam.fit(packed=None), INVALID, "null buffer")


def test_bad_out_kind(fam):
    _refused(fam.forward(out_kind=3), INVALID, "bad out_kind")
    _refused(fam.forward_box(out_kind=3), INVALID, "bad out_kind")


def test_bad_loss_kind(fam):
    _refused(fam.train_step(loss_kind=3), INVALID, "bad loss_kind")
    _refused(fam.fit(loss_kind=3), INVALID, "bad loss_kind")


def test_empty_batch(fam):
    _refused(fam.forward(n=0), INVALID, "empty batch")
    _refused(fam.forward_box(n=0), INVALID, "empty batch")
    _refused(fam.train_step(n=0), INVALID, "empty batch")
    _refused(fam.fit(n=0), INVALID, "empty batch")
    assert fam.fn("train_workspace_bytes")(C.byref(fam.d), 0) == -1
    assert _lib.lib().brief_last_error().decode() == "empty batch"


def test_offset_past_the_box(fam):
    _refused(fam.forward_box(offset=512 - N + 1), INVALID, "offset + n exceeds the box's voxel count")
    _refused(fam.forward_box(offset=-1), INVALID, "offset + n exceeds the box's voxel count")


def test_workspace_one_byte_short(fam):
    _refused(fam.train_step(ws_bytes=fam.need - 1), WORKSPACE, "workspace too small")
    _refused(fam.fit(workspace_bytes=fam.need - 1), WORKSPACE, "workspace too small")


def test_fit_index_stream(fam):
    _refused(fam.fit(idx=fam.idx.data_ptr(), idx_stride=0), INVALID, fam.no_stride)
    _refused(fam.fit(idx=fam.idx.data_ptr(), idx_stride=N - 1), INVALID, "idx_stride is smaller than the batch")


def test_fit_optimizer(fam):
    _refused(fam.fit(optim_kind=3), INVALID, "bad optimizer kind")
    _refused(fam.fit(optim_kind=_lib.OPT_KIND["Adam"], state1=None), INVALID, "optimizer state required")
    _refused(fam.fit(optim_kind=_lib.OPT_KIND["Adam"], state2=None), INVALID, "optimizer state required")
