"""ctypes binding of libbrief_hip.so (include/brief_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails the
product raises.  PyTorch is used only for device memory and streams.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BRIEF_LIB", os.path.join(_HERE, "libbrief_hip.so"))   # BRIEF_LIB: A/B diagnostics only
SRC = os.path.join(_HERE, "csrc", "brief_hip.hip")
_CSRC = os.path.join(_HERE, "csrc")
# every file of the translation unit (brief_hip.hip includes the *.inc / *.h beside it) and the public header
# (an installation may ship only the prebuilt library, or point BRIEF_LIB at an external build: no csrc/ then, and nothing to rebuild)
_DEPS = sorted(os.path.join(_CSRC, f) for f in (os.listdir(_CSRC) if os.path.isdir(_CSRC) else []) if f.endswith((".hip", ".inc", ".h"))) \
    + [os.path.join(os.path.dirname(_HERE), "include", "brief_hip.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


class BriefError(RuntimeError):
    pass


class SirenDesc(C.Structure):
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("layers", C.c_int32), ("features", C.c_int32),
                ("w0_first", C.c_float), ("w0_hidden", C.c_float), ("output_act", C.c_int32), ("precision", C.c_int32)]


class GridDesc(C.Structure):
    _fields_ = [("ndim", C.c_int32), ("reserved", C.c_int32), ("dims", C.c_int64 * 3), ("lo", C.c_float), ("hi", C.c_float)]


class GridBox(C.Structure):        # brief_grid_box
    _fields_ = [("grid", GridDesc), ("start", C.c_int64 * 3), ("step", C.c_int64 * 3), ("extent", C.c_int64 * 3)]


class BatchDesc(C.Structure):
    _fields_ = [("coords", C.c_void_p), ("targets", C.c_void_p), ("weights", C.c_void_p), ("idx", C.c_void_p),
                ("offset", C.c_int64), ("n", C.c_int64), ("rng_pop", C.c_int64), ("rng_seed", C.c_uint64), ("rng_step", C.c_uint64)]


class FitJob(C.Structure):          # brief_fit_job
    _fields_ = [("desc", SirenDesc), ("grid", GridDesc), ("batch", BatchDesc),
                ("params", C.c_void_p), ("packed", C.c_void_p), ("state1", C.c_void_p), ("state2", C.c_void_p),
                ("grads", C.c_void_p), ("loss_out", C.c_void_p), ("loss_log", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("loss_kind", C.c_int32), ("optim_kind", C.c_int32), ("thr", C.c_float), ("beta", C.c_float),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("milestones", C.POINTER(C.c_int64)), ("n_milestones", C.c_int32), ("reserved", C.c_int32),
                ("gamma", C.c_double), ("t0", C.c_int64),
                ("lr_table", C.POINTER(C.c_double)), ("beta1_table", C.POINTER(C.c_double)), ("idx_stride", C.c_int64)]


class FfnDesc(C.Structure):         # brief_ffn_desc
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("layers", C.c_int32), ("features", C.c_int32),
                ("embsize", C.c_int32), ("reserved", C.c_int32)]


class FfnFitJob(C.Structure):       # brief_ffn_fit_job: brief_fit_job's fields after the desc
    _fields_ = [("desc", FfnDesc)] + FitJob._fields_[1:]


class NerfDesc(C.Structure):        # brief_nerf_desc
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("layers", C.c_int32), ("features", C.c_int32),
                ("frequencies", C.c_int32), ("skip", C.c_int32)]


class NerfFitJob(C.Structure):      # brief_nerf_fit_job: brief_fit_job's fields after the desc
    _fields_ = [("desc", NerfDesc)] + FitJob._fields_[1:]


class MfnDesc(C.Structure):         # brief_mfn_desc
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("layers", C.c_int32), ("features", C.c_int32),
                ("filter", C.c_int32), ("output_act", C.c_int32)]


class MfnFitJob(C.Structure):       # brief_mfn_fit_job: brief_fit_job's fields after the desc
    _fields_ = [("desc", MfnDesc)] + FitJob._fields_[1:]


QUANT_MAX_TENSORS = 64             # BRIEF_QUANT_MAX_TENSORS


class QuantSpan(C.Structure):       # brief_quant_span
    _fields_ = [("offset", C.c_int64), ("count", C.c_int64)]


class ViewDesc(C.Structure):        # brief_view_desc
    _fields_ = [("dims", C.c_int64 * 3), ("lo", C.c_float), ("hi", C.c_float), ("origin", C.c_float * 3),
                ("drow", C.c_float * 3), ("dcol", C.c_float * 3), ("ddepth", C.c_float * 3),
                ("rows", C.c_int32), ("cols", C.c_int32), ("depth", C.c_int32), ("reserved", C.c_int32),
                ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3)]


class RaysDesc(C.Structure):        # brief_rays_desc
    _fields_ = [("dims", C.c_int64 * 3), ("lo", C.c_float), ("hi", C.c_float),
                ("rows", C.c_int32), ("cols", C.c_int32), ("depth", C.c_int32), ("reserved", C.c_int32),
                ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3)]


class ViewPart(C.Structure):        # brief_view_part
    _fields_ = [("start", C.c_int64 * 3), ("dims", C.c_int64 * 3), ("row0", C.c_int32), ("col0", C.c_int32), ("wrows", C.c_int32), ("wcols", C.c_int32)]


class CompositeWindow(C.Structure):  # brief_composite_window
    _fields_ = [("base", C.c_int64), ("row0", C.c_int32), ("col0", C.c_int32), ("wrows", C.c_int32), ("wcols", C.c_int32)]


class CompositeShade(C.Structure):   # brief_composite_shade
    _fields_ = [("gscale", C.c_float * 3), ("light", C.c_float * 3), ("ka_q", C.c_int32), ("kd_q", C.c_int32)]


VIEW_MODE = {"max": 0, "min": 1, "mean": 2, "slice": 3}      # BRIEF_VIEW_MAX .. BRIEF_VIEW_SLICE
SURFACE_SIDE = {"above": 0, "below": 1}                      # BRIEF_SURFACE_ABOVE, BRIEF_SURFACE_BELOW

TAPER_MAX_LAYERS = 16              # BRIEF_TAPER_MAX_LAYERS


class TaperDesc(C.Structure):       # brief_taper_desc
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("layers", C.c_int32), ("output_act", C.c_int32),
                ("widths", C.c_int32 * TAPER_MAX_LAYERS), ("w0", C.c_float * TAPER_MAX_LAYERS)]


class TaperFitJob(C.Structure):     # brief_taper_fit_job: brief_fit_job's fields after the desc
    _fields_ = [("desc", TaperDesc)] + FitJob._fields_[1:]


# the network families behind the one host driver of csrc/brief_family_host.inc: (entry prefix, desc, fit job); each has the same entries
FAMILIES = (("ffn", FfnDesc, FfnFitJob), ("nerf", NerfDesc, NerfFitJob), ("mfn", MfnDesc, MfnFitJob), ("taper", TaperDesc, TaperFitJob))
FAMILY_ENTRIES = ("param_count", "packed_count", "train_workspace_bytes", "repack", "forward", "forward_box", "train_step", "fit")

LOSS_KIND = {"datal2": 0, "datasmoothl1": 1, "external": 2}
OPT_KIND = {"Adamax": 0, "Adam": 1, "SGD": 2}
OUT_F32, OUT_U8, OUT_U16 = 0, 1, 2
PRECISION = {"fp32": 0, "f32": 0, "bf16": 1, "bf16x3": 2}

EXPORTS = ["brief_version", "brief_last_error", "brief_param_count", "brief_packed_count",
           "brief_train_workspace_bytes", "brief_siren_repack", "brief_siren_forward", "brief_forward_workspace_bytes", "brief_siren_forward_ws", "brief_siren_forward_box", "brief_siren_train_step", "brief_siren_fit_step",
           "brief_siren_fit", "brief_multi_fit",
           "brief_optim_step", "brief_sample_indices", "brief_sse_u16", "brief_profile_enable", "brief_profile_fused", "brief_deblock_edge", "brief_ssim_u16", "brief_ssim_partial_count",
           "brief_sincos_probe", "brief_cu_count",
           "brief_correct_chunk_elems", "brief_correct_count", "brief_correct_emit", "brief_correct_apply",
           "brief_mip_accumulate",
           "brief_quant_workspace_bytes", "brief_quant_ranges", "brief_quant_apply", "brief_quant_decode",
           "brief_siren_jac_packed_count", "brief_siren_jac_repack", "brief_siren_jac_forward", "brief_siren_jac_forward_box",
           "brief_view_clip", "brief_view_coords", "brief_view_fold", "brief_view_finish", "brief_view_sample_host", "brief_view_clip_host",
           "brief_surface_fold", "brief_surface_bracket", "brief_surface_coords", "brief_surface_step", "brief_surface_shade",
           "brief_view_sample_t_host",
           "brief_view_part_clip", "brief_view_part_coords", "brief_view_part_fold", "brief_view_part_clip_host", "brief_view_part_sample_host",
           "brief_siren_hess_forward", "brief_siren_hess_forward_box",
           "brief_view_composite_fold", "brief_view_composite_finish", "brief_view_composite_host",
           "brief_view_composite_part_fold", "brief_view_composite_part_carry", "brief_view_composite_part_gather",
           "brief_view_composite_part_fold_host", "brief_view_composite_part_carry_host", "brief_view_composite_part_gather_host",
           "brief_surface_part_fold", "brief_surface_part_route", "brief_surface_part_coords", "brief_surface_part_step", "brief_surface_part_shade",
           "brief_surface_part_route_host", "brief_view_part_sample_t_host",
           "brief_view_composite_select", "brief_view_composite_pick", "brief_view_composite_shade_fold", "brief_view_composite_shade_host",
           "brief_composite_shade_q_host",
           "brief_rays_clip", "brief_rays_coords", "brief_rays_fold", "brief_rays_surface_fold", "brief_rays_surface_coords",
           "brief_rays_surface_shade", "brief_rays_sample_host", "brief_rays_sample_t_host", "brief_rays_clip_host"] \
    + ["brief_%s_%s" % (prefix, entry) for prefix, _, _ in FAMILIES for entry in FAMILY_ENTRIES]


def needs_build():
    if LIB_PATH != os.path.join(_HERE, "libbrief_hip.so"):
        return False          # BRIEF_LIB names somebody else's build
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in _DEPS)


DIAG_LIB_PATH = os.path.join(_HERE, "libbrief_hip_diag.so")


def build(force=False, verbose=False, diagnostics=False, defines=(), out=None):
    """hipcc --offload-arch=gfx950 -> brief_pytorch_amd/libbrief_hip.so (in-tree).

    diagnostics=True builds libbrief_hip_diag.so with -DBRIEF_DIAGNOSTICS instead: the only build that reads the
    BRIEF_* environment knobs of tools/ (select it with BRIEF_LIB=...); the product library never calls getenv."""
    target = out or (DIAG_LIB_PATH if diagnostics else os.path.join(_HERE, "libbrief_hip.so"))
    if not force and not diagnostics and not defines and out is None and not needs_build():
        return LIB_PATH
    # -ffp-contract=off: every fused multiply-add in the kernels is an explicit fmaf/MFMA, so the
    # optimizer and de-normalise epilogues keep the separate roundings of the reference arithmetic
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", target]
    if diagnostics:
        cmd.append("-DBRIEF_DIAGNOSTICS")
    cmd += ["-D" + d for d in defines]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return target


_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch first: libbrief_hip.so must bind to the HIP runtime torch already loaded, otherwise two
    # runtimes live in one process and ours sees no device
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise BriefError("libbrief_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                         "there is no CPU fallback for the fused SIREN path")
    L = C.CDLL(LIB_PATH)
    dp, gp, bp, vp = C.POINTER(SirenDesc), C.POINTER(GridDesc), C.POINTER(BatchDesc), C.c_void_p
    L.brief_version.restype = C.c_int
    if L.brief_version() != 130:
        raise BriefError("libbrief_hip.so is version %d, this binding needs 130 (brief_siren_forward_ws, widths to 4096): rebuild with __graft_entry__.build()" % L.brief_version())
    L.brief_last_error.restype = C.c_char_p
    L.brief_param_count.restype = C.c_int64
    L.brief_param_count.argtypes = [dp]
    L.brief_packed_count.restype = C.c_int64
    L.brief_packed_count.argtypes = [dp]
    L.brief_train_workspace_bytes.restype = C.c_int64
    L.brief_train_workspace_bytes.argtypes = [dp, C.c_int64]
    L.brief_siren_repack.argtypes = [dp, vp, vp, vp]
    L.brief_siren_forward.argtypes = [dp, vp, gp, bp, vp, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double, vp]
    L.brief_forward_workspace_bytes.restype = C.c_int64
    L.brief_forward_workspace_bytes.argtypes = [dp, C.c_int64]
    L.brief_siren_forward_ws.argtypes = [dp, vp, gp, bp, vp, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double, vp, C.c_int64, vp]
    L.brief_siren_forward_box.argtypes = [dp, vp, C.POINTER(GridBox), C.c_int64, C.c_int64, vp, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double,
                                          vp, C.c_int64, vp]
    L.brief_siren_train_step.argtypes = [dp, vp, gp, bp, C.c_int, C.c_float, C.c_float, vp, vp, vp, vp, C.c_int64, vp]
    L.brief_siren_fit_step.argtypes = [dp, vp, vp, gp, bp, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, vp, vp, vp, C.c_int64, vp]
    L.brief_siren_fit.argtypes = [C.POINTER(FitJob), C.c_int64, vp]
    L.brief_multi_fit.argtypes = [C.POINTER(FitJob), C.c_int32, C.c_int64, vp]
    L.brief_optim_step.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, vp]
    L.brief_sample_indices.argtypes = [vp, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, vp]
    L.brief_sse_u16.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.brief_deblock_edge.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64] + [C.c_int] * 6 + [C.c_double] * 3 + [C.c_int, vp]
    L.brief_ssim_partial_count.restype = C.c_int64
    L.brief_ssim_partial_count.argtypes = [C.c_int64] * 3
    L.brief_ssim_u16.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, C.c_double, vp, C.c_int64, vp]
    L.brief_sincos_probe.argtypes = [vp, vp, vp, C.c_int64, vp]
    L.brief_cu_count.restype = C.c_int
    L.brief_profile_enable.argtypes = [C.c_int]
    L.brief_profile_fused.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    for prefix, Desc, Job in FAMILIES:      # the same eight entries per family (csrc/brief_family_host.inc)
        fp, f = C.POINTER(Desc), (lambda name: getattr(L, "brief_%s_%s" % (prefix, name)))
        for name in ("param_count", "packed_count", "train_workspace_bytes"):
            f(name).restype = C.c_int64
        f("param_count").argtypes = [fp]
        f("packed_count").argtypes = [fp]
        f("train_workspace_bytes").argtypes = [fp, C.c_int64]
        f("repack").argtypes = [fp, vp, vp, vp]
        f("forward").argtypes = [fp, vp, gp, bp, vp, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double, vp]
        f("forward_box").argtypes = [fp, vp, C.POINTER(GridBox), C.c_int64, C.c_int64, vp, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double, vp]
        f("train_step").argtypes = [fp, vp, gp, bp, C.c_int, C.c_float, C.c_float, vp, vp, vp, vp, C.c_int64, vp]
        f("fit").argtypes = [C.POINTER(Job), C.c_int64, vp]
    L.brief_correct_chunk_elems.restype = C.c_int64
    L.brief_correct_chunk_elems.argtypes = [C.c_int]
    L.brief_correct_count.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, vp, vp]
    L.brief_correct_emit.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, vp, C.c_int64, vp, vp, vp]
    L.brief_correct_apply.argtypes = [vp, C.c_int, C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp]
    i3 = C.POINTER(C.c_int64)
    L.brief_mip_accumulate.argtypes = [vp, C.c_int, i3, C.c_int32, vp, vp, vp, i3, i3, vp]
    sp = C.POINTER(QuantSpan)
    L.brief_quant_workspace_bytes.restype = C.c_int64
    L.brief_quant_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
    L.brief_quant_ranges.argtypes = [vp, sp, C.c_int32, C.c_int32, vp, vp, C.c_int64, vp]
    L.brief_quant_apply.argtypes = [vp, sp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.brief_quant_decode.argtypes = [vp, sp, C.c_int32, vp, vp, vp]
    L.brief_siren_jac_packed_count.restype = C.c_int64
    L.brief_siren_jac_packed_count.argtypes = [dp]
    L.brief_siren_jac_repack.argtypes = [dp, vp, vp, vp]
    L.brief_siren_jac_forward.argtypes = [dp, vp, gp, bp, vp, vp, vp]
    L.brief_siren_jac_forward_box.argtypes = [dp, vp, C.POINTER(GridBox), C.c_int64, C.c_int64, vp, vp, vp]
    L.brief_siren_hess_forward.argtypes = [dp, vp, gp, bp, vp, vp, vp, vp]
    L.brief_siren_hess_forward_box.argtypes = [dp, vp, C.POINTER(GridBox), C.c_int64, C.c_int64, vp, vp, vp, vp]
    wp, i64, i32 = C.POINTER(ViewDesc), C.c_int64, C.c_int32
    L.brief_view_clip.argtypes = [wp, vp, vp, vp]
    L.brief_view_coords.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, vp]
    L.brief_view_fold.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, vp, vp]
    L.brief_view_finish.argtypes = [wp, C.c_int, i32, i32, vp, vp, vp, vp]
    L.brief_view_sample_host.argtypes = [wp, vp, vp, vp, i64, vp, vp, vp]
    L.brief_view_clip_host.argtypes = [wp, vp, vp]
    L.brief_surface_fold.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, i32, i32, vp, vp, vp]
    L.brief_surface_bracket.argtypes = [wp, vp, vp, vp, vp, vp]
    L.brief_surface_coords.argtypes = [wp, vp, vp, i32, vp, vp, vp]
    L.brief_surface_step.argtypes = [wp, vp, C.c_int, i32, i32, i32, i32, vp, vp, vp]
    L.brief_surface_shade.argtypes = [wp, vp, vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, vp, vp]
    L.brief_view_sample_t_host.argtypes = [wp, vp, vp, vp, i64, vp, vp, vp]
    pp = C.POINTER(ViewPart)
    L.brief_view_part_clip.argtypes = [wp, pp, vp, vp, vp]
    L.brief_view_part_coords.argtypes = [wp, pp, vp, vp, i64, i64, i64, i64, i32, vp, vp]
    L.brief_view_part_fold.argtypes = [wp, pp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, vp, vp]
    L.brief_view_part_clip_host.argtypes = [wp, pp, vp, vp]
    L.brief_view_part_sample_host.argtypes = [wp, pp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.brief_view_composite_fold.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, i32, vp, vp, vp, vp]
    L.brief_view_composite_finish.argtypes = [wp, C.POINTER(i32), vp, vp, vp, vp, vp]
    L.brief_view_composite_host.argtypes = [wp, vp, vp, vp, C.c_int, i32, i32, vp, i32, C.POINTER(i32), vp, vp, vp, vp]
    L.brief_view_composite_part_fold.argtypes = [wp, pp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, i32, vp, vp, vp, vp]
    L.brief_view_composite_part_carry.argtypes = [wp, vp, i32, i64, vp, vp, vp, vp, vp, vp]
    L.brief_view_composite_part_gather.argtypes = [wp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.brief_view_composite_part_fold_host.argtypes = [wp, pp, vp, vp, vp, C.c_int, i32, i32, vp, i32, vp, vp, vp]
    L.brief_view_composite_part_carry_host.argtypes = [wp, vp, i32, i64, vp, vp, vp, vp, vp]
    L.brief_view_composite_part_gather_host.argtypes = [wp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.brief_surface_part_fold.argtypes = [wp, pp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, i32, i32, vp, vp, vp]
    L.brief_surface_part_route.argtypes = [wp, vp, i32, vp, vp, i32, vp, vp]
    L.brief_surface_part_coords.argtypes = [wp, pp, vp, vp, i32, vp, i64, vp, vp, vp]
    L.brief_surface_part_step.argtypes = [vp, i64, vp, C.c_int, i32, i32, i32, i32, vp, vp, vp]
    L.brief_surface_part_shade.argtypes = [vp, i64, vp, vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, vp, vp]
    L.brief_surface_part_route_host.argtypes = [wp, vp, i32, vp, vp, i32, vp]
    L.brief_view_part_sample_t_host.argtypes = [wp, pp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    hp = C.POINTER(CompositeShade)
    L.brief_view_composite_select.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, i32, vp, vp, vp]
    L.brief_view_composite_pick.argtypes = [vp, vp, vp, i64, vp, vp]
    L.brief_view_composite_shade_fold.argtypes = [wp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, i32, vp, vp, vp, hp, vp, vp, vp, vp]
    L.brief_view_composite_shade_host.argtypes = [wp, vp, vp, vp, C.c_int, i32, i32, vp, i32, C.POINTER(i32), vp, hp, vp, vp, vp, vp, vp]
    L.brief_composite_shade_q_host.argtypes = [vp, i64, hp, vp]
    rp = C.POINTER(RaysDesc)
    L.brief_rays_clip.argtypes = [rp, vp, vp, vp, vp]
    L.brief_rays_coords.argtypes = [rp, vp, vp, vp, i64, i64, i64, i64, i32, vp, vp]
    L.brief_rays_fold.argtypes = [rp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, vp, vp, vp]
    L.brief_rays_surface_fold.argtypes = [rp, vp, vp, i64, i64, i64, i64, i32, vp, C.c_int, i32, i32, i32, i32, vp, vp, vp]
    L.brief_rays_surface_coords.argtypes = [rp, vp, vp, vp, i32, vp, vp, vp]
    L.brief_rays_surface_shade.argtypes = [rp, vp, vp, i32, i32, i32, C.POINTER(C.c_float), vp, vp, vp, vp]
    L.brief_rays_sample_host.argtypes = [rp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.brief_rays_sample_t_host.argtypes = [rp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.brief_rays_clip_host.argtypes = [rp, vp, vp, vp]
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        raise BriefError("libbrief_hip: status %d: %s" % (rc, lib().brief_last_error().decode()))


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
