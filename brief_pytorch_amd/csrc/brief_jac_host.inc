// brief_jac_host.inc — the host side of the two derivative decodes: the one driver (deriv_check, deriv_args, deriv_forward,
// deriv_forward_box) and the spatial-gradient entries brief_siren_jac_packed_count / _repack / _forward / _forward_box (kernels:
// brief_jac.inc).  The Hessian entries (brief_hess.inc) are the same two templates over HessDecode.  Part of the single translation unit
// brief_hip.hip, included behind brief_family_host.inc so that k_jac_fwd and k_jac_repack are the last kernels named
// (profiles/r12_family_driver.md: the code of a few existing kernels depends on that order).  It uses fail, HIP_TRY, check_batch,
// check_box, fill_grid, fill_box above it and family_grid / launch_fwd_mtw of the family driver.
// Every entry only enqueues on `stream`: nothing is allocated and the host never waits.
//
// A decode is a traits struct:
//     Args                          the kernel-argument struct (JacArgs, or HessArgs derived from it)
//     label, too_wide, null_buffer  its name in front of every refusal, and the two refusals that are whole sentences
//     required(jac, hess)           the output that may not be NULL
//     launch<BOX>(a, st)            the persistent grid over its sample tiles

static int deriv_check(const brief_siren_desc *d, const char *label)
{
    if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
    if (d->precision != BRIEF_PREC_F32) return fail(BRIEF_ERR_INVALID, "%s: precision must be BRIEF_PREC_F32", label);
    if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "%s: coords_channel must be 2 or 3", label);
    if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "%s: data_channel must be 1..4", label);
    if (d->layers < 2) return fail(BRIEF_ERR_INVALID, "%s: layers must be >= 2", label);
    if (d->features < 1 || d->features > 1024) return fail(BRIEF_ERR_INVALID, "%s: features must be 1..1024", label);
    return 0;
}

static int jac_lds_bytes(const JacLayout &lay) { return (int)sizeof(float) * (1024 * lay.nt + 128); }

static void deriv_set_hess(JacArgs &, float *) {}      // (the overload for HessArgs stands behind that struct, in brief_hess.inc)

template <class Args>
static void deriv_args(Args &a, const brief_siren_desc *d, const float *packed, int64_t offset, int64_t n, float *value, float *jac, float *hess)
{
    memset(&a, 0, sizeof(a));
    a.d = *d; a.lay = jac_layout(*d); a.pk = packed;
    a.offset = offset; a.n = n; a.value = value; a.jac = jac;
    deriv_set_hess(a, hess);
}

template <class D>
static int deriv_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                         float *value, float *jac, float *hess, void *stream)
{
    if (int rc = deriv_check(d, D::label)) return rc;
    if (int rc = check_batch(d->cin, grid, batch, false)) return rc;
    if (!packed || !D::required(jac, hess)) return fail(BRIEF_ERR_INVALID, D::null_buffer);
    typename D::Args a;
    deriv_args(a, d, packed, batch->offset, batch->n, value, jac, hess);
    a.coords = batch->coords; a.idx = batch->idx;
    fill_grid(a.grid, grid);
    return D::template launch<false>(a, (hipStream_t)stream);
}

template <class D>
static int deriv_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                             float *value, float *jac, float *hess, void *stream)
{
    if (int rc = deriv_check(d, D::label)) return rc;
    int64_t voxels = 0;
    if (int rc = check_box(d->cin, box, &voxels)) return rc;
    if (n < 1) return fail(BRIEF_ERR_INVALID, "empty batch");
    if (offset < 0 || offset > voxels - n) return fail(BRIEF_ERR_INVALID, "offset + n exceeds the box's voxel count");
    if (!packed || !D::required(jac, hess)) return fail(BRIEF_ERR_INVALID, D::null_buffer);
    typename D::Args a;
    deriv_args(a, d, packed, offset, n, value, jac, hess);
    fill_grid(a.grid, &box->grid);
    fill_box(a.box, box);
    return D::template launch<true>(a, (hipStream_t)stream);
}

template <bool BOX>
struct JacFwd { template <int M> static auto fn() { return k_jac_fwd<M, BOX>; } };

struct JacDecode {
    typedef JacArgs Args;
    static constexpr const char *label = "spatial gradient", *too_wide = "spatial gradient: features must be 1..1024",
                                *null_buffer = "spatial gradient: null buffer (packed and jac are required)";
    static float *required(float *jac, float *) { return jac; }
    // the persistent grid over tiles of 8 samples: family_grid counts tiles of 32
    template <bool BOX>
    static int launch(const Args &a, hipStream_t st)
    {
        const int lds = jac_lds_bytes(a.lay);
        return launch_fwd_mtw<JacFwd<BOX> >((a.lay.nt + 3) / 4, a, family_grid(lds, 4 * a.n), lds, st, too_wide);
    }
};

extern "C" {

int64_t brief_siren_jac_packed_count(const brief_siren_desc *d) { return deriv_check(d, JacDecode::label) ? -1 : jac_layout(*d).total; }

int brief_siren_jac_repack(const brief_siren_desc *d, const float *params, float *packed, void *stream)
{
    if (int rc = deriv_check(d, JacDecode::label)) return rc;
    if (!params || !packed) return fail(BRIEF_ERR_INVALID, "null buffer");
    const JacLayout lay = jac_layout(*d);
    hipLaunchKernelGGL(k_jac_repack, dim3((unsigned)((lay.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d, lay, params, packed);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_siren_jac_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                            float *value, float *jac, void *stream)
{
    return deriv_forward<JacDecode>(d, packed, grid, batch, value, jac, NULL, stream);
}

int brief_siren_jac_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                                float *value, float *jac, void *stream)
{
    return deriv_forward_box<JacDecode>(d, packed, box, offset, n, value, jac, NULL, stream);
}

}   // extern "C"
