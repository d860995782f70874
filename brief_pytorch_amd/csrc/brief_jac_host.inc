// brief_jac_host.inc — the host side of the spatial-gradient decode (brief_jac.inc): brief_siren_jac_packed_count / _repack / _forward /
// _forward_box.  Part of the single translation unit brief_hip.hip, included behind brief_family_host.inc so that k_jac_fwd and
// k_jac_repack are the last kernels named (profiles/r12_family_driver.md: the code of a few existing kernels depends on that order).  It
// uses fail, HIP_TRY, check_batch, check_box, fill_grid, fill_box above it and family_grid / launch_fwd_mtw of the family driver.
// Every entry only enqueues on `stream`: nothing is allocated and the host never waits.

static const char *kJacTooWide = "spatial gradient: features must be 1..1024";

static int jac_check(const brief_siren_desc *d)
{
    if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
    if (d->precision != BRIEF_PREC_F32) return fail(BRIEF_ERR_INVALID, "spatial gradient: precision must be BRIEF_PREC_F32");
    if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "spatial gradient: coords_channel must be 2 or 3");
    if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "spatial gradient: data_channel must be 1..4");
    if (d->layers < 2) return fail(BRIEF_ERR_INVALID, "spatial gradient: layers must be >= 2");
    if (d->features < 1 || d->features > 1024) return fail(BRIEF_ERR_INVALID, kJacTooWide);
    return 0;
}

static int jac_lds_bytes(const JacLayout &lay) { return (int)sizeof(float) * (1024 * lay.nt + 128); }

template <bool BOX>
struct JacFwd { template <int M> static auto fn() { return k_jac_fwd<M, BOX>; } };

static void jac_args(JacArgs &a, const brief_siren_desc *d, const float *packed, int64_t n, float *value, float *jac)
{
    memset(&a, 0, sizeof(a));
    a.d = *d; a.lay = jac_layout(*d); a.pk = packed;
    a.n = n; a.value = value; a.jac = jac;
}

// the persistent grid over tiles of 8 samples: family_grid counts tiles of 32
template <bool BOX>
static int jac_launch(const JacArgs &a, hipStream_t st)
{
    const int lds = jac_lds_bytes(a.lay);
    return launch_fwd_mtw<JacFwd<BOX> >((a.lay.nt + 3) / 4, a, family_grid(lds, 4 * a.n), lds, st, kJacTooWide);
}

extern "C" {

int64_t brief_siren_jac_packed_count(const brief_siren_desc *d) { return jac_check(d) ? -1 : jac_layout(*d).total; }

int brief_siren_jac_repack(const brief_siren_desc *d, const float *params, float *packed, void *stream)
{
    if (int rc = jac_check(d)) return rc;
    if (!params || !packed) return fail(BRIEF_ERR_INVALID, "null buffer");
    const JacLayout lay = jac_layout(*d);
    hipLaunchKernelGGL(k_jac_repack, dim3((unsigned)((lay.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d, lay, params, packed);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brief_siren_jac_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                            float *value, float *jac, void *stream)
{
    if (int rc = jac_check(d)) return rc;
    if (int rc = check_batch(d->cin, grid, batch, false)) return rc;
    if (!packed || !jac) return fail(BRIEF_ERR_INVALID, "spatial gradient: null buffer (packed and jac are required)");
    JacArgs a;
    jac_args(a, d, packed, batch->n, value, jac);
    a.coords = batch->coords; a.idx = batch->idx; a.offset = batch->offset;
    fill_grid(a.grid, grid);
    return jac_launch<false>(a, (hipStream_t)stream);
}

int brief_siren_jac_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                                float *value, float *jac, void *stream)
{
    if (int rc = jac_check(d)) return rc;
    int64_t voxels = 0;
    if (int rc = check_box(d->cin, box, &voxels)) return rc;
    if (n < 1) return fail(BRIEF_ERR_INVALID, "empty batch");
    if (offset < 0 || offset > voxels - n) return fail(BRIEF_ERR_INVALID, "offset + n exceeds the box's voxel count");
    if (!packed || !jac) return fail(BRIEF_ERR_INVALID, "spatial gradient: null buffer (packed and jac are required)");
    JacArgs a;
    jac_args(a, d, packed, n, value, jac);
    a.offset = offset;
    fill_grid(a.grid, &box->grid);
    fill_box(a.box, box);
    return jac_launch<true>(a, (hipStream_t)stream);
}

}   // extern "C"
