// brief_family_host.inc — the host side of the network families that train and decode on kernels of their own: FFN (brief_ffn.inc), NeRF
// (brief_nerf.inc), MFNFourier / MFNGabor (brief_mfn.inc) and the tapered SIRENs (brief_taper.inc).  Part of the single translation unit
// brief_hip.hip, which includes it last; it uses the helpers of the SIREN entries above it (fail, HIP_TRY, check_batch, check_box, fill_grid,
// fill_box, dev_attr_once, prof_live, fit_job_lr, optim_scalars).
//
// Every family runs the same step:  k_<fam>_fwd<TRAIN>  ->  k_<fam>_wgrad (split-K, one launch per kWgradMax blocks)  ->  k_ffn_reduce
// (+ k_<fam>_repack after an update), and the same decode:  k_<fam>_fwd<false, BOX>.  The driver below (family_*) is that step once, as
// templates over a traits struct; a family supplies only what differs:
//     Desc, Job, Args, Ws, WgradArgs, WgradBlock     its C-ABI desc and fit job, its kernel-argument structs, its workspace layout (FamilyWs + planes)
//     fit_name, too_wide                             the entry name and the width message of its error texts
//     check(d)                                       the desc check and its messages
//     bind_layout(a)                                 the layout fields of Args, from a.d
//     lds_bytes(a), mtw(a)                           dynamic LDS of k_<fam>_fwd and the m-tiles per wave that select its instantiation
//     param_count(a), packed_count(a)                floats of the canonical / the fragment-ordered buffer
//     plane_offsets(a, w), bind_planes(a, ws, w)     the stash planes of the workspace (returns the first float behind them) and their pointers in Args
//     kWgradMax, wgrad_count(a), wgrad_block(a, w, ws, i), wgrad_scalars(wa, a), blocks(wa), nblocks(wa), launch_wgrad(wa, grid, st)
//                                                    the weight-gradient blocks, the kernel that consumes them and its extra scalars
//     slab_len(a), reduce_bv(a)                      floats of one gradient slab, and the leading span of the canonical buffer without a gradient
//     launch_repack(a, params, pk, st)               canonical -> fragment order
//     launch_fwd<TRAIN, BOX>(a, grid, st)            the forward-kernel dispatch (launch_fwd_mtw over the family's kernel)
// A new family is a traits struct and eight one-line extern "C" entries; DESIGN.md ("One host driver for the network families") has the rest.
//
// The kernel-argument structs share field names, not a base: a common base or another field order would move kernel-argument offsets.

static const int64_t kFfnLossParts = 4096;      // >= any family_grid

// what every family's workspace layout holds besides its own planes (offsets in floats)
struct FamilyWs { int64_t npad, lpart, slabs, total, chunk; int nsplit, waves; };

// persistent grid: up to two workgroups per CU (one wave per SIMD each), fewer when the LDS image does not fit twice
static int family_grid(int lds_bytes, int64_t n)
{
    const int64_t tiles = (n + 31) / 32;
    const int by_lds = (160 * 1024) / lds_bytes;
    const int64_t cap = (int64_t)kCUs * (by_lds < 2 ? (by_lds > 0 ? by_lds : 1) : 2);
    return (int)(tiles < cap ? tiles : cap);
}

// K-splits of the weight-gradient launch (w.waves 64 x 64 blocks over w.npad samples): about eight workgroups per CU (the latency of the
// plane loads needs waves in flight), at most 64 and at least 256 samples each
static void family_ksplit(FamilyWs &w)
{
    const int64_t wgs = (w.waves + 3) / 4;
    int64_t ns = (8 * (int64_t)kCUs + wgs - 1) / wgs;
    if (ns > 64) ns = 64;
    if (ns > w.npad / 256) ns = w.npad / 256;
    if (ns < 1) ns = 1;
    w.chunk = (w.npad / ns + 31) / 32 * 32;
    w.nsplit = (int)((w.npad + w.chunk - 1) / w.chunk);
}

// one weight-gradient block, dW[arows][brows] = A B^T over the planes at workspace offsets A and B (ws == nullptr: shapes only), in 64 x 64
// wave jobs; w_off / b_off / ldw place dW and db in the slab.  wave_begin and the family's own fields are left to the caller
template <class Block>
static Block wgrad_block_of(float *ws, int64_t A, int64_t B, int arows, int brows, int64_t w_off, int64_t b_off, int ldw)
{
    Block b;
    memset(&b, 0, sizeof(b));
    b.A = ws ? ws + A : nullptr; b.B = ws ? ws + B : nullptr;
    b.arows = arows; b.brows = brows;
    b.mb = (arows + 63) / 64; b.nb = (brows + 63) / 64;
    b.w_off = w_off; b.b_off = b_off; b.ldw = ldw;
    return b;
}

// workspace of a train step of n samples: the family's planes | loss partials | nsplit gradient slabs
template <class Fam>
static typename Fam::Ws family_ws_layout(const typename Fam::Args &a, int64_t n)
{
    typename Fam::Ws w;
    w.npad = (n + 31) / 32 * 32;
    w.lpart = Fam::plane_offsets(a, w);
    w.slabs = w.lpart + kFfnLossParts;
    w.waves = 0;
    for (int i = 0; i < Fam::wgrad_count(a); ++i) {
        const typename Fam::WgradBlock b = Fam::wgrad_block(a, w, nullptr, i);      // ws == nullptr: shapes only
        w.waves += b.mb * b.nb;
    }
    family_ksplit(w);
    w.total = w.slabs + (int64_t)w.nsplit * Fam::slab_len(a);
    return w;
}

// the forward kernel for 1 .. 8 m-tiles per wave, chosen at run time: K::fn<M>() names the instantiation for M.  The table names them in
// ascending M, and the entries below name TRAIN before the decode kernels: the compiler instantiates kernels in the order they are first
// named, and how it schedules a few of them depends on that order (profiles/r12_family_driver.md)
template <class K, class Args>
static int launch_fwd_mtw(int mtw, const Args &a, int grid, int lds, hipStream_t st, const char *too_wide)
{
    typedef void (*Kernel)(Args);
    const Kernel tab[8] = {K::template fn<1>(), K::template fn<2>(), K::template fn<3>(), K::template fn<4>(),
                           K::template fn<5>(), K::template fn<6>(), K::template fn<7>(), K::template fn<8>()};
    if (mtw < 1 || mtw > 8) return fail(BRIEF_ERR_INVALID, too_wide);
    const Kernel fn = tab[mtw - 1];
    if (int rc = dev_attr_once((const void *)fn, lds)) return rc;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int check_out(const float *packed, const void *out, int out_kind)
{
    if (!packed || !out) return fail(BRIEF_ERR_INVALID, "null buffer");
    if (out_kind < BRIEF_OUT_F32 || out_kind > BRIEF_OUT_U16) return fail(BRIEF_ERR_INVALID, "bad out_kind");
    return 0;
}

// the kernel arguments of a launch over n samples, without their source (coordinates / indices / grid / box)
template <class Fam>
static void family_forward_args(typename Fam::Args &a, const typename Fam::Desc *d, const float *packed, int64_t n, void *out, int out_kind,
                                float scale_min, float scale_max, double vmin, double vmax)
{
    memset(&a, 0, sizeof(a));
    a.d = *d; a.pk = packed;
    Fam::bind_layout(a);
    a.n = n; a.npad = (n + 31) / 32 * 32;
    a.out = out; a.out_kind = out_kind;
    a.scale_min = scale_min;
    a.den = (float)((double)scale_max - (double)scale_min);
    a.span = (float)(vmax - vmin);
    a.vmin = (float)vmin;
}
// ... with nothing to write: what the size entries and the repack need of a desc
template <class Fam>
static void family_shape_args(typename Fam::Args &a, const typename Fam::Desc *d)
{
    family_forward_args<Fam>(a, d, nullptr, 0, nullptr, 0, 0.f, 1.f, 0.0, 1.0);
}

// the sample source of a batch: coordinates, or indices / an offset into the grid
template <class Args>
static void bind_batch(Args &a, const brief_grid_desc *grid, const brief_batch_desc *batch)
{
    a.coords = batch->coords; a.idx = batch->idx; a.offset = batch->offset;
    fill_grid(a.grid, grid);
}
// ... and what a train step reads besides: targets, weights, the Philox stream when the kernel draws the indices itself, the loss
template <class Args>
static void bind_training(Args &a, const brief_grid_desc *grid, const brief_batch_desc *batch, int loss_kind, float thr, float beta, float *yhat_out)
{
    bind_batch(a, grid, batch);
    a.targets = batch->targets; a.weights = batch->weights;
    if (!batch->idx && batch->rng_pop > 0) { a.rng_pop = (uint64_t)batch->rng_pop; a.rng_seed = batch->rng_seed; a.rng_step = batch->rng_step; }
    a.loss_kind = loss_kind; a.thr = thr; a.beta = beta;
    a.inv_count = (float)(1.0 / ((double)batch->n * a.d.cout));
    a.yhat_out = yhat_out;
}

template <class Fam>
static int64_t family_param_count(const typename Fam::Desc *d)
{
    if (Fam::check(d)) return -1;
    typename Fam::Args a;
    family_shape_args<Fam>(a, d);
    return Fam::param_count(a);
}
template <class Fam>
static int64_t family_packed_count(const typename Fam::Desc *d)
{
    if (Fam::check(d)) return -1;
    typename Fam::Args a;
    family_shape_args<Fam>(a, d);
    return Fam::packed_count(a);
}
template <class Fam>
static int64_t family_train_workspace_bytes(const typename Fam::Desc *d, int64_t n)
{
    if (Fam::check(d)) return -1;
    if (n < 1) { fail(BRIEF_ERR_INVALID, "empty batch"); return -1; }
    typename Fam::Args a;
    family_shape_args<Fam>(a, d);
    return family_ws_layout<Fam>(a, n).total * (int64_t)sizeof(float);
}

template <class Fam>
static int family_repack(const typename Fam::Desc *d, const float *params, float *packed, void *stream)
{
    if (int rc = Fam::check(d)) return rc;
    if (!params || !packed) return fail(BRIEF_ERR_INVALID, "null buffer");
    typename Fam::Args a;
    family_shape_args<Fam>(a, d);
    Fam::launch_repack(a, params, packed, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// one train step: gradients and loss of the batch; with upd, the optimizer update and the refreshed fragment copy as well (the step of family_fit)
template <class Fam>
static int family_train(const typename Fam::Desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                        int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                        void *workspace, int64_t workspace_bytes, void *stream, const UpdatePayload *upd)
{
    if (int rc = Fam::check(d)) return rc;
    if (int rc = check_batch(d->cin, grid, batch, true)) return rc;
    if (!packed || !grads || !loss_out || !workspace) return fail(BRIEF_ERR_INVALID, "null buffer");
    if (loss_kind < BRIEF_LOSS_L2 || loss_kind > BRIEF_LOSS_EXTERNAL) return fail(BRIEF_ERR_INVALID, "bad loss_kind");
    typename Fam::Args a;
    family_forward_args<Fam>(a, d, packed, batch->n, nullptr, 0, 0.f, 1.f, 0.0, 1.0);
    const typename Fam::Ws w = family_ws_layout<Fam>(a, batch->n);
    if (workspace_bytes < w.total * (int64_t)sizeof(float)) return fail(BRIEF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    bind_training(a, grid, batch, loss_kind, thr, beta, yhat_out);
    Fam::bind_planes(a, ws, w);
    a.lpart = ws + w.lpart;
    a.npad = w.npad;
    const int grid1 = family_grid(Fam::lds_bytes(a), batch->n);
    const bool prof = prof_live();
    hipEvent_t *pev = prof ? dev_state()->prof_ev : nullptr;
    if (prof) HIP_TRY(hipEventRecord(pev[2 * g_prof_n], st));
    if (int rc = Fam::template launch_fwd<true, false>(a, grid1, st)) return rc;
    if (prof) { HIP_TRY(hipEventRecord(pev[2 * g_prof_n + 1], st)); ++g_prof_n; }
    // weight gradients, at most kWgradMax blocks per launch
    const int64_t mlp = Fam::slab_len(a), bv = Fam::reduce_bv(a);
    const int nblocks = Fam::wgrad_count(a);
    for (int b0 = 0; b0 < nblocks; b0 += Fam::kWgradMax) {
        typename Fam::WgradArgs wa;
        memset(&wa, 0, sizeof(wa));
        wa.npad = w.npad; wa.chunk = w.chunk; wa.mlp = mlp; wa.slabs = ws + w.slabs;
        Fam::wgrad_scalars(wa, a);
        const int nb = (nblocks - b0) < Fam::kWgradMax ? (nblocks - b0) : Fam::kWgradMax;
        Fam::nblocks(wa) = nb;
        int waves = 0;
        for (int i = 0; i < nb; ++i) {
            typename Fam::WgradBlock &blk = Fam::blocks(wa)[i];
            blk = Fam::wgrad_block(a, w, ws, b0 + i);
            blk.wave_begin = waves;
            waves += blk.mb * blk.nb;
        }
        wa.waves = waves;
        Fam::launch_wgrad(wa, dim3((unsigned)((waves + 3) / 4), (unsigned)w.nsplit), st);
        HIP_TRY(hipGetLastError());
    }
    const int64_t nred = mlp > bv ? mlp : bv;
    OptimScalars o;
    memset(&o, 0, sizeof(o));
    if (upd) o = upd->opt;
    hipLaunchKernelGGL(k_ffn_reduce, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, (const float *)(ws + w.slabs), w.nsplit, mlp, bv, grads,
                       (const float *)(ws + w.lpart), grid1, loss_kind == BRIEF_LOSS_EXTERNAL ? 0.f : a.inv_count, loss_out,
                       upd ? 1 : 0, o, upd ? upd->params : nullptr, upd ? upd->s1 : nullptr, upd ? upd->s2 : nullptr);
    HIP_TRY(hipGetLastError());
    if (upd) {
        Fam::launch_repack(a, (const float *)upd->params, upd->pk, st);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// `steps` optimizer steps of one net from one call: brief_siren_fit's contract (schedule, index stream, loss log) on the family's step
template <class Fam>
static int family_fit(const typename Fam::Job *j, int64_t steps, void *stream)
{
    if (!j) return fail(BRIEF_ERR_INVALID, "null job");
    if (int rc = Fam::check(&j->desc)) return rc;
    if (steps < 0) return fail(BRIEF_ERR_INVALID, "bad step count");
    if (j->batch.idx && j->idx_stride <= 0) return fail(BRIEF_ERR_INVALID, "%s needs idx_stride > 0 with batch.idx (one index set per step)", Fam::fit_name);
    if (j->batch.idx && j->idx_stride < j->batch.n) return fail(BRIEF_ERR_INVALID, "idx_stride is smaller than the batch");
    if (!j->params || !j->packed || !j->grads || !j->loss_out || !j->workspace) return fail(BRIEF_ERR_INVALID, "null buffer");
    if (j->t0 < 0) return fail(BRIEF_ERR_INVALID, "bad step count");
    if (j->n_milestones < 0 || (j->n_milestones > 0 && !j->milestones)) return fail(BRIEF_ERR_INVALID, "bad lr milestones");
    if (j->optim_kind < BRIEF_OPT_ADAMAX || j->optim_kind > BRIEF_OPT_SGD) return fail(BRIEF_ERR_INVALID, "bad optimizer kind");
    if (j->optim_kind != BRIEF_OPT_SGD && (!j->state1 || !j->state2)) return fail(BRIEF_ERR_INVALID, "optimizer state required");
    hipStream_t st = (hipStream_t)stream;
    // the schedule fields mean what they mean in brief_fit_job: brief_siren_fit's rule (fit_job_lr) evaluates them
    brief_fit_job sched;
    memset(&sched, 0, sizeof(sched));
    sched.milestones = j->milestones; sched.n_milestones = j->n_milestones; sched.gamma = j->gamma; sched.t0 = j->t0;
    sched.lr_table = j->lr_table;
    double lr = j->lr;
    for (int64_t k = 0; k < steps; ++k) {
        const int64_t t = j->t0 + 1 + k;
        fit_job_lr(&sched, t, k, &lr);
        brief_batch_desc b = j->batch;
        if (b.idx) b.idx = b.idx + k * j->idx_stride;
        else if (b.rng_pop > 0) b.rng_step = (uint64_t)t;
        UpdatePayload up;
        up.opt = optim_scalars(j->optim_kind, lr, j->beta1_table ? j->beta1_table[k] : j->beta1, j->beta2, j->eps, t);
        up.params = j->params; up.s1 = j->state1; up.s2 = j->state2; up.pk = j->packed;
        if (int rc = family_train<Fam>(&j->desc, j->packed, &j->grid, &b, j->loss_kind, j->thr, j->beta, j->grads,
                                       j->loss_log ? j->loss_log + k : j->loss_out, nullptr, j->workspace, j->workspace_bytes, (void *)st, &up))
            return rc;
    }
    if (j->loss_log && steps > 0)
        HIP_TRY(hipMemcpyAsync(j->loss_out, j->loss_log + steps - 1, sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

template <class Fam>
static int family_forward(const typename Fam::Desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                          void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    if (int rc = Fam::check(d)) return rc;
    if (int rc = check_batch(d->cin, grid, batch, false)) return rc;
    if (int rc = check_out(packed, out, out_kind)) return rc;
    typename Fam::Args a;
    family_forward_args<Fam>(a, d, packed, batch->n, out, out_kind, scale_min, scale_max, vmin, vmax);
    bind_batch(a, grid, batch);
    return Fam::template launch_fwd<false, false>(a, family_grid(Fam::lds_bytes(a), batch->n), (hipStream_t)stream);
}

template <class Fam>
static int family_forward_box(const typename Fam::Desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                              void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    if (int rc = Fam::check(d)) return rc;
    int64_t voxels = 0;
    if (int rc = check_box(d->cin, box, &voxels)) return rc;
    if (n < 1) return fail(BRIEF_ERR_INVALID, "empty batch");
    if (offset < 0 || offset > voxels - n) return fail(BRIEF_ERR_INVALID, "offset + n exceeds the box's voxel count");
    if (int rc = check_out(packed, out, out_kind)) return rc;
    typename Fam::Args a;
    family_forward_args<Fam>(a, d, packed, n, out, out_kind, scale_min, scale_max, vmin, vmax);
    a.offset = offset;
    fill_grid(a.grid, &box->grid);
    fill_box(a.box, box);
    return Fam::template launch_fwd<false, true>(a, family_grid(Fam::lds_bytes(a), n), (hipStream_t)stream);
}

// =============================================================================================
// FFN (Fourier-feature network, brief_ffn.inc): k_ffn_fwd, k_ffn_wgrad, k_ffn_reduce over the MLP span (the B matrix, the first bv floats of
// the canonical buffer, takes no gradient), k_ffn_repack
struct FfnWs : FamilyWs { int64_t H, D, EMB, G; };
template <bool TRAIN, bool BOX>
struct FfnFwd { template <int M> static auto fn() { return k_ffn_fwd<M, TRAIN, BOX>; } };
struct FfnFamily {
    typedef brief_ffn_desc Desc;
    typedef brief_ffn_fit_job Job;
    typedef FfnArgs Args;
    typedef FfnWs Ws;
    typedef FfnWgradArgs WgradArgs;
    typedef FfnWgradLayer WgradBlock;
    static constexpr const char *fit_name = "brief_ffn_fit";
    static constexpr const char *too_wide = "FFN: features must be 1..1024 on the fused path";
    static const int kWgradMax = FFN_WGRAD_LAYERS;

    static int check(const Desc *d)
    {
        if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
        if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "FFN: coords_channel must be 2 or 3");
        if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "FFN: data_channel must be 1..4");
        if (d->layers < 2) return fail(BRIEF_ERR_INVALID, "FFN: layers must be >= 2");
        if (d->features < 1 || d->features > 1024) return fail(BRIEF_ERR_INVALID, too_wide);
        if (d->embsize < 1 || d->embsize > 512) return fail(BRIEF_ERR_INVALID, "FFN: embsize must be 1..512 on the fused path");
        if (d->reserved != 0) return fail(BRIEF_ERR_INVALID, "FFN: reserved must be 0 (skip connections are not supported)");
        return 0;
    }
    static void bind_layout(Args &a)
    {
        const FfnLayout lay = ffn_layout(a.d);
        a.nt = lay.nt; a.EP = lay.EP;
    }
    static int lds_bytes(const Args &a)
    {
        const FfnLayout l = ffn_layout(a.d);
        return (int)sizeof(float) * (32 * (l.K0 > l.FP ? l.K0 : l.FP) + 128);
    }
    static int mtw(const Args &a) { return (a.nt + 3) / 4; }
    static int64_t param_count(const Args &a) { return ffn_canon_count(a.d); }
    static int64_t packed_count(const Args &a) { return ffn_layout(a.d).total; }
    static int64_t reduce_bv(const Args &a) { return ffn_canon_w0(a.d); }
    static int64_t slab_len(const Args &a) { return ffn_canon_count(a.d) - ffn_canon_w0(a.d); }
    static int64_t plane_offsets(const Args &a, Ws &w)
    {
        const FfnLayout lay = ffn_layout(a.d);
        const int64_t plane = (int64_t)lay.FP * w.npad;
        w.H = 0;
        w.D = w.H + (int64_t)(a.d.layers - 1) * plane;
        w.EMB = w.D + (int64_t)(a.d.layers - 1) * plane;
        w.G = w.EMB + (int64_t)lay.K0 * w.npad;
        return w.G + 4 * w.npad;
    }
    static void bind_planes(Args &a, float *ws, const Ws &w) { a.H = ws + w.H; a.D = ws + w.D; a.EMB = ws + w.EMB; a.G = ws + w.G; }
    // weight-gradient block of layer l (0 .. layers - 1): offsets relative to the MLP span; planes at the workspace offsets of w
    // (ws == nullptr: shapes only), wave_begin left to the caller
    static int wgrad_count(const Args &a) { return a.d.layers; }
    static WgradBlock wgrad_block(const Args &a, const Ws &w, float *ws, int l)
    {
        const Desc &d = a.d;
        const FfnLayout lay = ffn_layout(d);
        const int F = d.features, L = d.layers;
        const int64_t plane = (int64_t)lay.FP * w.npad, bv = ffn_canon_w0(d);
        int64_t A, B, w_off, b_off;
        int arows = F, brows = F, ldw = F, emb = 0;
        if (l == L - 1) {
            A = w.G; B = w.H + (int64_t)(L - 2) * plane; arows = d.cout;
            w_off = ffn_canon_head(d) - bv; b_off = w_off + (int64_t)d.cout * F;
        } else if (l == 0) {
            A = w.D; B = w.EMB; brows = lay.K0; emb = 1;
            w_off = 0; ldw = 2 * d.embsize; b_off = 2 * (int64_t)d.embsize * F;
        } else {
            A = w.D + (int64_t)l * plane; B = w.H + (int64_t)(l - 1) * plane;
            w_off = ffn_canon_hidden(d, l) - bv; b_off = w_off + (int64_t)F * F;
        }
        WgradBlock b = wgrad_block_of<WgradBlock>(ws, A, B, arows, brows, w_off, b_off, ldw);
        b.emb = emb;
        return b;
    }
    static void wgrad_scalars(WgradArgs &wa, const Args &a) { wa.EP = a.EP; wa.E = a.d.embsize; }
    static WgradBlock *blocks(WgradArgs &wa) { return wa.lay; }
    static int &nblocks(WgradArgs &wa) { return wa.nlayers; }
    static void launch_wgrad(const WgradArgs &wa, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(k_ffn_wgrad, grid, dim3(256), 0, st, wa); }
    static void launch_repack(const Args &a, const float *params, float *pk, hipStream_t st)
    {
        hipLaunchKernelGGL(k_ffn_repack, dim3((unsigned)((packed_count(a) + 255) / 256)), dim3(256), 0, st, a.d, params, pk);
    }
    template <bool TRAIN, bool BOX>
    static int launch_fwd(const Args &a, int grid, hipStream_t st)
    {
        return launch_fwd_mtw<FfnFwd<TRAIN, BOX> >(mtw(a), a, grid, lds_bytes(a), st, too_wide);
    }
};

extern "C" {

int64_t brief_ffn_param_count(const brief_ffn_desc *d) { return family_param_count<FfnFamily>(d); }
int64_t brief_ffn_packed_count(const brief_ffn_desc *d) { return family_packed_count<FfnFamily>(d); }
int64_t brief_ffn_train_workspace_bytes(const brief_ffn_desc *d, int64_t n) { return family_train_workspace_bytes<FfnFamily>(d, n); }
int brief_ffn_repack(const brief_ffn_desc *d, const float *params, float *packed, void *stream) { return family_repack<FfnFamily>(d, params, packed, stream); }
int brief_ffn_train_step(const brief_ffn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                         int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                         void *workspace, int64_t workspace_bytes, void *stream)
{
    return family_train<FfnFamily>(d, packed, grid, batch, loss_kind, thr, beta, grads, loss_out, yhat_out, workspace, workspace_bytes, stream, nullptr);
}
int brief_ffn_fit(const brief_ffn_fit_job *j, int64_t steps, void *stream) { return family_fit<FfnFamily>(j, steps, stream); }
int brief_ffn_forward(const brief_ffn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                      void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward<FfnFamily>(d, packed, grid, batch, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}
int brief_ffn_forward_box(const brief_ffn_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                          void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward_box<FfnFamily>(d, packed, box, offset, n, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}

}   // extern "C"

// =============================================================================================
// NeRF (positional-encoding network, brief_nerf.inc): k_nerf_fwd, k_nerf_wgrad, k_ffn_reduce (bv = 0), k_nerf_repack
struct NerfWs : FamilyWs { int64_t H, D, ENC, G; };
template <bool TRAIN, bool BOX>
struct NerfFwd { template <int M> static auto fn() { return k_nerf_fwd<M, TRAIN, BOX>; } };
struct NerfFamily {
    typedef brief_nerf_desc Desc;
    typedef brief_nerf_fit_job Job;
    typedef NerfArgs Args;
    typedef NerfWs Ws;
    typedef NerfWgradArgs WgradArgs;
    typedef NerfWgradBlock WgradBlock;
    static constexpr const char *fit_name = "brief_nerf_fit";
    static constexpr const char *too_wide = "NeRF: features must be 1..1024 on the fused path";
    static const int kWgradMax = NERF_WGRAD_BLOCKS;

    static int check(const Desc *d)
    {
        if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
        if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "NeRF: coords_channel must be 2 or 3");
        if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "NeRF: data_channel must be 1..4");
        if (d->skip != 0 && d->skip != 1) return fail(BRIEF_ERR_INVALID, "NeRF: skip must be 0 or 1");
        if (d->layers < 2) return fail(BRIEF_ERR_INVALID, "NeRF: layers must be >= 2");
        if (d->skip && d->layers < 3) return fail(BRIEF_ERR_INVALID, "NeRF: layers must be >= 3 with skip");
        if (d->features < 1 || d->features > 1024) return fail(BRIEF_ERR_INVALID, too_wide);
        if (d->frequencies < 0 || d->frequencies > 16) return fail(BRIEF_ERR_INVALID, "NeRF: frequencies must be 0..16 on the fused path");
        return 0;
    }
    static void bind_layout(Args &a)
    {
        const NerfLayout lay = nerf_layout(a.d);
        a.nt = lay.nt; a.DP = lay.DP;
    }
    static int lds_bytes(const Args &a)
    {
        const NerfLayout l = nerf_layout(a.d);
        return (int)sizeof(float) * (32 * (l.DP + l.FP) + 128);
    }
    static int mtw(const Args &a) { return (a.nt + 3) / 4; }
    static int64_t param_count(const Args &a) { return nerf_canon_count(a.d); }
    static int64_t packed_count(const Args &a) { return nerf_layout(a.d).total; }
    static int64_t reduce_bv(const Args &) { return 0; }
    static int64_t slab_len(const Args &a) { return nerf_canon_count(a.d); }
    static int64_t plane_offsets(const Args &a, Ws &w)
    {
        const NerfLayout lay = nerf_layout(a.d);
        const int64_t plane = (int64_t)lay.FP * w.npad;
        w.H = 0;
        w.D = w.H + (int64_t)(a.d.layers - 1) * plane;
        w.ENC = w.D + (int64_t)(a.d.layers - 1) * plane;
        w.G = w.ENC + (int64_t)lay.DP * w.npad;
        return w.G + 4 * w.npad;
    }
    static void bind_planes(Args &a, float *ws, const Ws &w) { a.H = ws + w.H; a.D = ws + w.D; a.ENC = ws + w.ENC; a.G = ws + w.G; }
    // weight-gradient block i (0 .. wgrad_count - 1) of the net, in canonical order: W0 | per hidden layer (the skip layer's encoding
    // columns first) | head; planes at the workspace offsets of w (ws == nullptr: shapes only), wave_begin left to the caller
    static int wgrad_count(const Args &a) { return a.d.layers + (a.d.skip ? 1 : 0); }
    static WgradBlock wgrad_block(const Args &a, const Ws &w, float *ws, int i)
    {
        const Desc &d = a.d;
        const NerfLayout lay = nerf_layout(d);
        const int F = d.features, L = d.layers;
        const int64_t plane = (int64_t)lay.FP * w.npad;
        int64_t A, B, w_off, b_off;
        int arows = F, brows = F, ldw = F;
        if (i == 0) {
            A = w.D; B = w.ENC; brows = lay.d; ldw = lay.d; w_off = 0; b_off = (int64_t)F * lay.d;
        } else if (i == wgrad_count(a) - 1) {
            A = w.G; B = w.H + (int64_t)(L - 2) * plane; arows = d.cout;
            w_off = nerf_canon_head(d); b_off = w_off + (int64_t)d.cout * F;
        } else {
            const bool past = lay.sl && i > lay.sl;                        // block index i: layer i, or i - 1 past the skip layer's extra block
            const int l = past ? i - 1 : i;
            const bool enc = lay.sl && i == lay.sl;                        // the skip layer's encoding columns
            const int coff = l == lay.sl ? lay.d : 0;
            const int64_t c = nerf_canon_hidden(d, l);
            A = w.D + (int64_t)l * plane; ldw = F + coff;
            if (enc) { B = w.ENC; brows = lay.d; w_off = c; b_off = -1; }
            else { B = w.H + (int64_t)(l - 1) * plane; w_off = c + coff; b_off = c + (int64_t)F * ldw; }
        }
        return wgrad_block_of<WgradBlock>(ws, A, B, arows, brows, w_off, b_off, ldw);
    }
    static void wgrad_scalars(WgradArgs &, const Args &) {}
    static WgradBlock *blocks(WgradArgs &wa) { return wa.blk; }
    static int &nblocks(WgradArgs &wa) { return wa.nblocks; }
    static void launch_wgrad(const WgradArgs &wa, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(k_nerf_wgrad, grid, dim3(256), 0, st, wa); }
    static void launch_repack(const Args &a, const float *params, float *pk, hipStream_t st)
    {
        hipLaunchKernelGGL(k_nerf_repack, dim3((unsigned)((packed_count(a) + 255) / 256)), dim3(256), 0, st, a.d, params, pk);
    }
    template <bool TRAIN, bool BOX>
    static int launch_fwd(const Args &a, int grid, hipStream_t st)
    {
        return launch_fwd_mtw<NerfFwd<TRAIN, BOX> >(mtw(a), a, grid, lds_bytes(a), st, too_wide);
    }
};

extern "C" {

int64_t brief_nerf_param_count(const brief_nerf_desc *d) { return family_param_count<NerfFamily>(d); }
int64_t brief_nerf_packed_count(const brief_nerf_desc *d) { return family_packed_count<NerfFamily>(d); }
int64_t brief_nerf_train_workspace_bytes(const brief_nerf_desc *d, int64_t n) { return family_train_workspace_bytes<NerfFamily>(d, n); }
int brief_nerf_repack(const brief_nerf_desc *d, const float *params, float *packed, void *stream) { return family_repack<NerfFamily>(d, params, packed, stream); }
int brief_nerf_train_step(const brief_nerf_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                          int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    return family_train<NerfFamily>(d, packed, grid, batch, loss_kind, thr, beta, grads, loss_out, yhat_out, workspace, workspace_bytes, stream, nullptr);
}
int brief_nerf_fit(const brief_nerf_fit_job *j, int64_t steps, void *stream) { return family_fit<NerfFamily>(j, steps, stream); }
int brief_nerf_forward(const brief_nerf_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                       void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward<NerfFamily>(d, packed, grid, batch, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}
int brief_nerf_forward_box(const brief_nerf_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                           void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward_box<NerfFamily>(d, packed, box, offset, n, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}

}   // extern "C"

// =============================================================================================
// MFN (multiplicative filter networks, brief_mfn.inc): k_mfn_fwd<.., GABOR>, k_mfn_wgrad, k_ffn_reduce (bv = 0), k_mfn_repack
struct MfnWs : FamilyWs { int64_t Z, U, DU, DA, Q, XP, G; };
template <bool TRAIN, bool BOX, bool GABOR>
struct MfnFwd { template <int M> static auto fn() { return k_mfn_fwd<M, TRAIN, BOX, GABOR>; } };
struct MfnFamily {
    typedef brief_mfn_desc Desc;
    typedef brief_mfn_fit_job Job;
    typedef MfnArgs Args;
    typedef MfnWs Ws;
    typedef MfnWgradArgs WgradArgs;
    typedef MfnWgradBlock WgradBlock;
    static constexpr const char *fit_name = "brief_mfn_fit";
    static constexpr const char *too_wide = "MFN: features must be 1..1024 on the fused path";
    static const int kWgradMax = MFN_WGRAD_BLOCKS;

    static int check(const Desc *d)
    {
        if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
        if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "MFN: coords_channel must be 2 or 3");
        if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "MFN: data_channel must be 1..4");
        if (d->layers < 2) return fail(BRIEF_ERR_INVALID, "MFN: layers must be >= 2");
        if (d->features < 1 || d->features > 1024) return fail(BRIEF_ERR_INVALID, too_wide);
        if (d->filter != 0 && d->filter != 1) return fail(BRIEF_ERR_INVALID, "MFN: filter must be 0 (Fourier) or 1 (Gabor)");
        if (d->output_act != 0 && d->output_act != 1) return fail(BRIEF_ERR_INVALID, "MFN: output_act must be 0 or 1");
        return 0;
    }
    static void bind_layout(Args &a) { a.nt = mfn_layout(a.d).nt; }
    static int lds_bytes(const Args &a) { return (int)sizeof(float) * (32 * mfn_layout(a.d).FP + 128); }
    static int mtw(const Args &a) { return (a.nt + 3) / 4; }
    static int64_t param_count(const Args &a) { return mfn_canon_count(a.d); }
    static int64_t packed_count(const Args &a) { return mfn_layout(a.d).total; }
    static int64_t reduce_bv(const Args &) { return 0; }
    static int64_t slab_len(const Args &a) { return mfn_canon_count(a.d); }
    static int64_t plane_offsets(const Args &a, Ws &w)
    {
        const int64_t plane = (int64_t)mfn_layout(a.d).FP * w.npad;
        const int nf = a.d.layers - 1, nh = a.d.layers - 2;
        w.Z = 0;
        w.U = w.Z + nf * plane;
        w.DU = w.U + nh * plane;
        w.DA = w.DU + nh * plane;
        w.Q = w.DA + nf * plane;
        w.XP = w.Q + (a.d.filter ? nf : 0) * plane;
        w.G = w.XP + 5 * w.npad;
        return w.G + 4 * w.npad;
    }
    static void bind_planes(Args &a, float *ws, const Ws &w)
    {
        a.Z = ws + w.Z; a.U = ws + w.U; a.DU = ws + w.DU; a.DA = ws + w.DA; a.Q = ws + w.Q; a.XP = ws + w.XP; a.G = ws + w.G;
    }
    // weight-gradient block i (0 .. wgrad_count - 1) of the net: hidden layers | head | per filter (W / b, then Gabor's mu / gamma);
    // planes at the workspace offsets of w (ws == nullptr: shapes only), wave_begin left to the caller
    static int wgrad_count(const Args &a) { return a.d.layers - 1 + (a.d.layers - 1) * (a.d.filter ? 2 : 1); }
    static WgradBlock wgrad_block(const Args &a, const Ws &w, float *ws, int i)
    {
        const Desc &d = a.d;
        const MfnLayout lay = mfn_layout(d);
        const int F = d.features, L = d.layers, cin = d.cin;
        const int64_t plane = (int64_t)lay.FP * w.npad;
        int64_t A, B, w_off, b_off;
        int arows = F, brows = F, ldw = F, gabor = 0;
        const float *fg = nullptr;
        if (i < L - 2) {                                                   // hidden layer l = i + 1
            const int l = i + 1;
            A = w.DU + (int64_t)(l - 1) * plane; B = w.Z + (int64_t)(l - 1) * plane;
            w_off = mfn_canon_hidden(d, l); b_off = w_off + (int64_t)F * F;
        } else if (i == L - 2) {                                           // head
            A = w.G; B = w.Z + (int64_t)(L - 2) * plane; arows = d.cout;
            w_off = mfn_canon_head(d); b_off = w_off + (int64_t)d.cout * F;
        } else {
            const int per = d.filter ? 2 : 1, j = i - (L - 1), fi = j / per;
            B = w.XP; ldw = cin;
            if (j % per == 0) {                                            // filter fi: Wf / bf
                A = w.DA + (int64_t)fi * plane; brows = cin;
                w_off = mfn_canon_filter_w(d, fi); b_off = w_off + (int64_t)F * cin;
            } else {                                                       // Gabor filter fi: mu / gamma
                A = w.Q + (int64_t)fi * plane; brows = cin + 2;
                w_off = mfn_canon_filter(d, fi); b_off = -1; gabor = 1;
                fg = a.pk ? a.pk + lay.filt + (int64_t)fi * lay.filt_stride + 4 * (int64_t)lay.FP : nullptr;
            }
        }
        WgradBlock b = wgrad_block_of<WgradBlock>(ws, A, B, arows, brows, w_off, b_off, ldw);
        b.gabor = gabor; b.fg = fg;
        return b;
    }
    static void wgrad_scalars(WgradArgs &wa, const Args &a) { wa.cin = a.d.cin; wa.FP = mfn_layout(a.d).FP; }
    static WgradBlock *blocks(WgradArgs &wa) { return wa.blk; }
    static int &nblocks(WgradArgs &wa) { return wa.nblocks; }
    static void launch_wgrad(const WgradArgs &wa, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(k_mfn_wgrad, grid, dim3(256), 0, st, wa); }
    static void launch_repack(const Args &a, const float *params, float *pk, hipStream_t st)
    {
        hipLaunchKernelGGL(k_mfn_repack, dim3((unsigned)((packed_count(a) + 255) / 256)), dim3(256), 0, st, a.d, params, pk);
    }
    template <bool TRAIN, bool BOX>
    static int launch_fwd(const Args &a, int grid, hipStream_t st)
    {
        return a.d.filter ? launch_fwd_mtw<MfnFwd<TRAIN, BOX, true> >(mtw(a), a, grid, lds_bytes(a), st, too_wide)
                          : launch_fwd_mtw<MfnFwd<TRAIN, BOX, false> >(mtw(a), a, grid, lds_bytes(a), st, too_wide);
    }
};

extern "C" {

int64_t brief_mfn_param_count(const brief_mfn_desc *d) { return family_param_count<MfnFamily>(d); }
int64_t brief_mfn_packed_count(const brief_mfn_desc *d) { return family_packed_count<MfnFamily>(d); }
int64_t brief_mfn_train_workspace_bytes(const brief_mfn_desc *d, int64_t n) { return family_train_workspace_bytes<MfnFamily>(d, n); }
int brief_mfn_repack(const brief_mfn_desc *d, const float *params, float *packed, void *stream) { return family_repack<MfnFamily>(d, params, packed, stream); }
int brief_mfn_train_step(const brief_mfn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                         int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                         void *workspace, int64_t workspace_bytes, void *stream)
{
    return family_train<MfnFamily>(d, packed, grid, batch, loss_kind, thr, beta, grads, loss_out, yhat_out, workspace, workspace_bytes, stream, nullptr);
}
int brief_mfn_fit(const brief_mfn_fit_job *j, int64_t steps, void *stream) { return family_fit<MfnFamily>(j, steps, stream); }
int brief_mfn_forward(const brief_mfn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                      void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward<MfnFamily>(d, packed, grid, batch, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}
int brief_mfn_forward_box(const brief_mfn_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                          void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward_box<MfnFamily>(d, packed, box, offset, n, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}

}   // extern "C"

// =============================================================================================
// Tapered SIRENs (SIREN_Pyramid, SIRENFT, SIRENPS; brief_taper.inc): k_taper_fwd, k_taper_wgrad, k_ffn_reduce (bv = 0), k_taper_repack
struct TaperWs : FamilyWs { int64_t Z, D, X, G; };
template <bool TRAIN, bool BOX>
struct TaperFwd { template <int M> static auto fn() { return k_taper_fwd<M, TRAIN, BOX>; } };
struct TaperFamily {
    typedef brief_taper_desc Desc;
    typedef brief_taper_fit_job Job;
    typedef TaperArgs Args;
    typedef TaperWs Ws;
    typedef TaperWgradArgs WgradArgs;
    typedef TaperWgradBlock WgradBlock;
    static constexpr const char *fit_name = "brief_taper_fit";
    static constexpr const char *too_wide = "tapered SIREN: every hidden width must be 1..1024 on the fused path";
    static const int kWgradMax = BRIEF_TAPER_MAX_LAYERS;      // one rectangular block per Linear, all in one launch

    static int check(const Desc *d)
    {
        if (!d) return fail(BRIEF_ERR_INVALID, "null desc");
        if (d->cin != 2 && d->cin != 3) return fail(BRIEF_ERR_INVALID, "tapered SIREN: coords_channel must be 2 or 3");
        if (d->cout < 1 || d->cout > 4) return fail(BRIEF_ERR_INVALID, "tapered SIREN: data_channel must be 1..4");
        if (d->layers < 3 || d->layers > BRIEF_TAPER_MAX_LAYERS) return fail(BRIEF_ERR_INVALID, "tapered SIREN: layers must be 3..16");
        if (d->output_act != 0 && d->output_act != 1) return fail(BRIEF_ERR_INVALID, "tapered SIREN: output_act must be 0 or 1");
        for (int l = 0; l < d->layers - 1; ++l)
            if (d->widths[l] < 1 || d->widths[l] > 1024) return fail(BRIEF_ERR_INVALID, too_wide);
        return 0;
    }
    static void bind_layout(Args &a) { a.lay = taper_layout(a.d); }
    static int lds_bytes(const Args &a) { return (int)sizeof(float) * (1024 * a.lay.ntmax + 128); }
    static int mtw(const Args &a) { return (a.lay.ntmax + 3) / 4; }
    static int64_t param_count(const Args &a) { return a.lay.count; }
    static int64_t packed_count(const Args &a) { return a.lay.total; }
    static int64_t reduce_bv(const Args &) { return 0; }
    static int64_t slab_len(const Args &a) { return a.lay.count; }
    static int64_t plane_offsets(const Args &a, Ws &w)
    {
        w.Z = 0;
        w.D = w.Z + (int64_t)a.lay.rows * w.npad;
        w.X = w.D + (int64_t)a.lay.rows * w.npad;
        w.G = w.X + 4 * w.npad;
        return w.G + 4 * w.npad;
    }
    static void bind_planes(Args &a, float *ws, const Ws &w) { a.Z = ws + w.Z; a.D = ws + w.D; a.X = ws + w.X; a.G = ws + w.G; }
    // weight-gradient block of Linear i (0 .. layers - 1) in canonical order; planes at the workspace offsets of w (ws == nullptr: shapes
    // only), wave_begin left to the caller
    static int wgrad_count(const Args &a) { return a.lay.L; }
    static WgradBlock wgrad_block(const Args &a, const Ws &w, float *ws, int i)
    {
        const TaperLayout &lay = a.lay;
        const int L = lay.L;
        const int64_t A = i == L - 1 ? w.G : w.D + (int64_t)lay.row0[i] * w.npad;
        const int64_t B = i == 0 ? w.X : w.Z + (int64_t)lay.row0[i - 1] * w.npad;
        WgradBlock b = wgrad_block_of<WgradBlock>(ws, A, B, lay.out[i], lay.in[i], lay.canon[i], lay.canon[i] + (int64_t)lay.out[i] * lay.in[i], lay.in[i]);
        b.bsin = i > 0;
        return b;
    }
    static void wgrad_scalars(WgradArgs &, const Args &) {}
    static WgradBlock *blocks(WgradArgs &wa) { return wa.blk; }
    static int &nblocks(WgradArgs &wa) { return wa.nblocks; }
    static void launch_wgrad(const WgradArgs &wa, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(k_taper_wgrad, grid, dim3(256), 0, st, wa); }
    static void launch_repack(const Args &a, const float *params, float *pk, hipStream_t st)
    {
        hipLaunchKernelGGL(k_taper_repack, dim3((unsigned)((packed_count(a) + 255) / 256)), dim3(256), 0, st, a.d, a.lay, params, pk);
    }
    template <bool TRAIN, bool BOX>
    static int launch_fwd(const Args &a, int grid, hipStream_t st)
    {
        return launch_fwd_mtw<TaperFwd<TRAIN, BOX> >(mtw(a), a, grid, lds_bytes(a), st, too_wide);
    }
};

extern "C" {

int64_t brief_taper_param_count(const brief_taper_desc *d) { return family_param_count<TaperFamily>(d); }
int64_t brief_taper_packed_count(const brief_taper_desc *d) { return family_packed_count<TaperFamily>(d); }
int64_t brief_taper_train_workspace_bytes(const brief_taper_desc *d, int64_t n) { return family_train_workspace_bytes<TaperFamily>(d, n); }
int brief_taper_repack(const brief_taper_desc *d, const float *params, float *packed, void *stream) { return family_repack<TaperFamily>(d, params, packed, stream); }
int brief_taper_train_step(const brief_taper_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                           int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                           void *workspace, int64_t workspace_bytes, void *stream)
{
    return family_train<TaperFamily>(d, packed, grid, batch, loss_kind, thr, beta, grads, loss_out, yhat_out, workspace, workspace_bytes, stream, nullptr);
}
int brief_taper_fit(const brief_taper_fit_job *j, int64_t steps, void *stream) { return family_fit<TaperFamily>(j, steps, stream); }
int brief_taper_forward(const brief_taper_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                        void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward<TaperFamily>(d, packed, grid, batch, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}
int brief_taper_forward_box(const brief_taper_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                            void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream)
{
    return family_forward_box<TaperFamily>(d, packed, box, offset, n, out, out_kind, scale_min, scale_max, vmin, vmax, stream);
}

}   // extern "C"
