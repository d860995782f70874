/* brief_hip.h — C-ABI of libbrief_hip.so: the MI355X-native SIREN fit/decode hot path of BRIEF.
 *
 * The reference (RichealYoung/BRIEF_PyTorch) has no FFI for this path: it sits behind the
 * Python object returned by init_phi() (utils/Networks.py:795-802) and the loop body in
 * main.py:385-400.  Each entry point below names the reference code it replaces.  All pointers
 * are DEVICE pointers (e.g. torch.Tensor.data_ptr()), `stream` is a hipStream_t passed as
 * void*.  The compute entry points only enqueue kernels on `stream`: no device memory is allocated or freed and the
 * host never waits (exceptions, all outside the per-step path: brief_multi_fit creates its internal stream pool on
 * first use and forks / joins it with events; brief_profile_* record and wait for events; brief_sse_u16 issues a
 * hipMemsetAsync).  Every function returns 0 on success or a negative brief_status; the message of the
 * last failure on the calling thread is available through brief_last_error().
 */
#ifndef BRIEF_HIP_H
#define BRIEF_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BRIEF_VERSION 130 /* 0.1.3: features up to 4096 (k_wide; brief_siren_forward_ws + brief_forward_workspace_bytes: inference above 1024 features needs a
                           * scratch), library state per device; struct layouts as in 0.1.1 (brief_fit_job with lr_table, beta1_table, idx_stride) */

typedef enum {
    BRIEF_OK = 0,
    BRIEF_ERR_INVALID = -1,      /* bad argument / unsupported configuration (e.g. res=True, F > 4096) */
    BRIEF_ERR_LAUNCH = -2,       /* HIP launch / runtime error */
    BRIEF_ERR_WORKSPACE = -3     /* workspace too small */
} brief_status;

/* SIREN(coords_channel, data_channel, features, layers, w0, output_act)  utils/Networks.py:246-266.
 * layers = number of Linear layers; hidden Sine() is hard-coded w0=30 in the reference (:228,259). */
typedef struct {
    int32_t cin;         /* 2 | 3 */
    int32_t cout;        /* 1 .. 4 */
    int32_t layers;      /* >= 2 */
    int32_t features;    /* 1 .. 4096 for BRIEF_PREC_F32 (padded internally to whole 32-feature tiles; SIREN.calc_features, utils/Networks.py:299-314,
                          * has no width limit: the shipped default.yaml solves to 527 on a 512^3 uint16 volume and to 1494 on a 1024^3 one), 1 .. 512 for BRIEF_PREC_BF16,
                          * 1 .. 256 for BRIEF_PREC_BF16X3 */
    float w0_first;
    float w0_hidden;
    int32_t output_act;
    int32_t precision;   /* BRIEF_PREC_F32 (0): exact f32 MFMA everywhere.  BRIEF_PREC_BF16 (1): the hidden F x F GEMMs run on the
                          * bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, f32 accumulate, f32 master weights, f32 first layer, head,
                          * loss, reductions and optimizer); activations/deltas are stashed as bf16.  The MI355X counterpart of the
                          * reference's low-precision mode (Compress.half, main.py:388-399), pinned by a PSNR band, not bitwise.
                          * BRIEF_PREC_BF16X3 (2), features <= 256: split precision — weights, activations and deltas of the hidden GEMMs
                          * are split into hi + lo 16-bit halves and every product is three 16-bit MFMAs (hi.hi + hi.lo + lo.hi, f32
                          * accumulate): fp16 halves in the forward chains (22 significant bits), bf16 halves in the backward chains and
                          * the weight-gradient GEMM (16 bits, bf16's exponent range).  Held to the SAME oracle bands as BRIEF_PREC_F32
                          * (forward 2e-5, gradients 1e-4, traces 1e-4) but not bit-identical to it; never the default.  Inference
                          * (brief_siren_forward / _decode) runs the same fp16-halves forward chains (~1e-6 from the f32 kernel).  Needs |w0 W / 2 pi| < 1000 for every hidden weight (fp16 range of the scaled forward copy). */
} brief_siren_desc;
enum { BRIEF_PREC_F32 = 0, BRIEF_PREC_BF16 = 1, BRIEF_PREC_BF16X3 = 2 };

/* create_flattened_coords(shape, mode)  utils/dataset.py:36-60: linspace(lo,hi,n) per axis, (d,h,w) order */
typedef struct {
    int32_t ndim;        /* == cin */
    int32_t reserved;
    int64_t dims[3];
    float lo, hi;
} brief_grid_desc;

/* where the samples of one step come from.
 *   j = idx ? idx[n] : (rng_pop > 0 ? philox(rng_seed, rng_step, n) mod-free-scaled to [0, rng_pop) : n + offset)
 *                                            (RandompointSampler main.py:154-163 / full-volume cube :112-125;
 *                                             the in-kernel stream equals brief_sample_indices(.., rng_pop, rng_seed, rng_step))
 *   x = coords ? coords[j, :] : grid coordinate of voxel j
 *   y = targets[j, :]      w = weights ? weights[j, :] : 1 */
typedef struct {
    const float *coords;     /* [*, cin] or NULL */
    const float *targets;    /* [*, cout]  (ignored by forward) */
    const float *weights;    /* [*, cout] or NULL */
    const int64_t *idx;      /* [n] or NULL */
    int64_t offset;
    int64_t n;               /* samples in this call */
    int64_t rng_pop;         /* > 0 with idx == NULL: draw the voxel indices in-kernel (train step only) */
    uint64_t rng_seed, rng_step;
} brief_batch_desc;

typedef enum {
    BRIEF_LOSS_L2 = 0, BRIEF_LOSS_SMOOTHL1 = 1,      /* main.py:176-191 */
    BRIEF_LOSS_EXTERNAL = 2   /* `targets` holds dL/dyhat per sample and channel (what autograd hands to the module's backward,
                               * main.py:396 `loss.backward()`): it is used as is (no weights, no 1/N), loss_out receives 0 */
} brief_loss_kind;
typedef enum { BRIEF_OPT_ADAMAX = 0, BRIEF_OPT_ADAM = 1, BRIEF_OPT_SGD = 2 } brief_optim_kind; /* utils/misc.py:174-183 */
typedef enum { BRIEF_OUT_F32 = 0, BRIEF_OUT_U8 = 1, BRIEF_OUT_U16 = 2 } brief_out_kind;

int brief_version(void);
const char *brief_last_error(void);

/* number of floats in the canonical packed parameter buffer (W0,b0,W1,b1,... == torch parameters()
 * order; W_l row-major [out,in] as in utils/ModelSave.py:32-50).  == SIREN.calc_param_count */
int64_t brief_param_count(const brief_siren_desc *d);
/* floats in the derived MFMA-fragment-ordered weight buffer produced by brief_siren_repack */
int64_t brief_packed_count(const brief_siren_desc *d);
/* bytes of scratch a train step of n samples needs (activation stash + gradient slabs) */
int64_t brief_train_workspace_bytes(const brief_siren_desc *d, int64_t n);
/* Scratch.  This holds for every workspace of the train, fit and decode entries (this one, brief_forward_workspace_bytes,
 * brief_quant_workspace_bytes, the families' brief_*_train_workspace_bytes) and for the fragment-ordered copies (brief_packed_count,
 * brief_siren_jac_packed_count, the families' *_packed_count): what the buffer holds on entry is irrelevant: it need not be
 * initialised and may hold anything, NaN bit patterns and the data of an earlier, larger batch included; what it holds on exit is
 * unspecified.  No entry reads or writes outside [workspace, workspace + bytes) of the size its *_bytes function returns for the call's
 * n (a larger buffer is accepted; the part behind that size is left alone), and no entry keeps state in a workspace from one call to
 * the next: brief_multi_fit writes the device table of a group into the first job's workspace again in every call.
 * brief_siren_repack (and the families' *_repack, brief_siren_jac_repack) writes all brief_packed_count floats of `packed`, padding
 * included.  A train step writes all brief_param_count floats of `grads` (the bvals span of an FFN as zeros), loss_out, and n * cout
 * floats of yhat_out where given.  The only caller memory that carries state between calls is what the signatures name as such:
 * params, packed, state1 / state2.  tests/test_gpu_scratch_contract.py holds every train, fit and decode kernel to this. */

/* canonical params -> fragment-ordered copies read by the kernels.  Call after every change of
 * `params` made outside brief_optim_step's caller loop (init, load_model utils/ModelSave.py:8-27). */
int brief_siren_repack(const brief_siren_desc *d, const float *params, float *packed, void *stream);

/* SIREN.forward under no_grad (main.py:266-268 sample_nf; utils/misc.py:59-92 reconstruct_flattened).
 * out_kind F32: out = yhat [n,cout] float.  U8/U16: fused invnormalize_data('minmaxany_a_b')
 * (utils/io.py:136-147): clip((yhat-a)/(b-a),0,1)*(vmax-vmin)+vmin truncated to the integer type. */
int brief_siren_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid,
                        const brief_batch_desc *batch, void *out, int out_kind,
                        float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* The same with a caller-provided scratch.  Nets of more than 1024 features keep no layer in LDS whole: their activations travel
 * through two ping-pong planes per workgroup in `workspace` (brief_forward_workspace_bytes(d, n) bytes, 0 up to 1024 features, where
 * workspace may be NULL); brief_siren_forward refuses such a net with BRIEF_ERR_WORKSPACE. */
int64_t brief_forward_workspace_bytes(const brief_siren_desc *d, int64_t n);
int brief_siren_forward_ws(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid,
                           const brief_batch_desc *batch, void *out, int out_kind,
                           float scale_min, float scale_max, double vmin, double vmax, void *workspace, int64_t workspace_bytes, void *stream);

/* A strided box of a grid: box voxel (i0, i1, i2), in (d,h,w) order ((h,w) for ndim 2), is grid voxel start[a] + step[a] * i[a] on every
 * axis; its coordinates are the grid's (create_flattened_coords on grid.dims), bit for bit.  grid.dims may differ from the shape the net
 * was fitted on (a resampled view).  Entries past grid.ndim are ignored. */
typedef struct {
    brief_grid_desc grid;
    int64_t start[3], step[3], extent[3];
} brief_grid_box;
/* Inference over a box without evaluating the rest of the grid (region of interest, strided preview, resampling): sample n of the call
 * is box voxel b = offset + n in box-linear order ((i0 * extent[1] + i1) * extent[2] + i2), and out row n holds it, with the out_kind
 * epilogue of brief_siren_forward.  Refused with BRIEF_ERR_INVALID: grid.ndim != cin, a dim outside 1 .. 2^31 - 1, extent < 1,
 * step < 1, start < 0 or start + step (extent - 1) >= dims on an axis, n < 1, offset < 0 or offset + n beyond the box's voxel count.
 * Scratch as brief_siren_forward_ws: brief_forward_workspace_bytes(d, n) bytes (BRIEF_ERR_WORKSPACE above 1024 features without). */
int brief_siren_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box,
                            int64_t offset, int64_t n, void *out, int out_kind,
                            float scale_min, float scale_max, double vmin, double vmax,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* zero_grad + forward + loss + backward of main.py:385-396 for one batch.
 * grads: canonical packed layout, fully overwritten.  loss_out: one float (mean loss).
 * yhat_out: optional [n,cout].  thr: normalised weight_thres (0 disables, main.py:178-179). */
int brief_siren_train_step(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid,
                           const brief_batch_desc *batch, int loss_kind, float thr, float beta,
                           float *grads, float *loss_out, float *yhat_out,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* One whole iteration of the loop body main.py:385-400 in three launches: brief_siren_train_step followed by the
 * optimizer update of brief_optim_step, with the update applied inside the gradient reduction and written through
 * to BOTH the canonical `params` and the fragment-ordered `packed` copy (no separate repack).  `packed` must hold
 * a repack of `params` on entry.  Results are bit-identical to train_step + optim_step + repack. */
int brief_siren_fit_step(const brief_siren_desc *d, float *params, float *packed, const brief_grid_desc *grid,
                         const brief_batch_desc *batch, int loss_kind, float thr, float beta,
                         int optim_kind, float *state1, float *state2, double lr, double beta1, double beta2, double eps, int64_t t,
                         float *grads, float *loss_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- many steps per call -------------------------------------------------------------------------
 * One independent fit (one block of a DivideTask partition, or the whole volume of a SingleTask): everything
 * the loop `for steps in range(1, max_steps + 1)` of main.py:385-402 touches, as plain device pointers.
 * `batch` is the per-step template: with idx == NULL and rng_pop > 0 the voxel indices of step t are drawn
 * in-kernel with rng_step = t (RandompointSampler, main.py:154-163); with rng_pop == 0 every step sees the
 * same batch (RandomCubeSampler at its default: the whole volume, main.py:112-125).  A per-step idx stream
 * cannot be expressed here: use brief_siren_fit_step for replayed indices.
 * lr schedule = torch MultiStepLR stepped after every optimizer step (utils/misc.py:184-197, main.py:400):
 * `lr` is the value in force for step t0 + 1; whenever the number of finished steps equals a milestone the
 * running value is multiplied by gamma (once per occurrence).  n_milestones == 0: constant lr. */
typedef struct brief_fit_job {
    brief_siren_desc desc;
    brief_grid_desc grid;
    brief_batch_desc batch;
    float *params, *packed;        /* canonical parameters and their fragment-ordered copy (repacked on entry) */
    float *state1, *state2;        /* optimizer state (exp_avg | exp_inf or exp_avg_sq); unused for SGD */
    float *grads;                  /* [param_count]: gradient of the last step */
    float *loss_out;               /* device scalar: loss of the last step */
    float *loss_log;               /* device [steps] or NULL: loss of every step of this call */
    void *workspace;               /* brief_train_workspace_bytes(desc, batch.n); private to this job */
    int64_t workspace_bytes;
    int32_t loss_kind, optim_kind;
    float thr, beta;
    double lr, beta1, beta2, eps;
    const int64_t *milestones;     /* host array, ascending */
    int32_t n_milestones, reserved;
    double gamma;
    int64_t t0;                    /* optimizer steps already taken; this call runs steps t0+1 .. t0+steps */
    /* closed-form schedules (StepLR, CyclicLR of utils/misc.py:184-197, which torch evaluates from the epoch count, not as a
     * running product): host arrays with one entry per step of THIS call, entry k for step t0+1+k.  lr_table overrides
     * lr / milestones / gamma; beta1_table (CyclicLR cycles the momentum of Adam-family optimizers) overrides beta1. */
    const double *lr_table, *beta1_table;
    /* batch.idx with idx_stride > 0: a device-resident index STREAM, step t0+1+k reads batch.idx + k * idx_stride (int64
     * elements).  How the windowed RandomCubeSampler (main.py:38-125) runs without a host round trip per step: the caller
     * expands the window draws of a run of steps into voxel indices once.  idx_stride == 0 with batch.idx set is refused. */
    int64_t idx_stride;
} brief_fit_job;

/* `steps` iterations of brief_siren_fit_step enqueued back to back on `stream` (3 launches each, no host
 * synchronisation, nothing allocated).  Bit-identical to calling brief_siren_fit_step `steps` times. */
int brief_siren_fit(const brief_fit_job *job, int64_t steps, void *stream);

/* Grouped independent fits (the per-block loop of main.py:547-575 for the blocks one GPU owns).  Narrow nets (features <= 64:
 * what BRIEF's own YAMLs produce) of one kernel variant are trained by ONE launch pair per step for up to 64 jobs (k_small_group +
 * k_reduce_group: workgroup ranges per job, the jobs' static arguments in a device table inside the first job's workspace) — the
 * many small blocks of a DivideTask no longer cost a launch pair per block and step; every other job runs its own launches.  Units
 * (groups and single jobs) run on internal HIP streams, unit u on stream u mod 8, forked from and joined back into `stream` with
 * events, so that kernels of different units overlap.  Each job's results are bit-identical to brief_siren_fit on its own; jobs
 * must not share any buffer except read-only targets/weights.  Call from one host thread per process (one process per GPU). */
int brief_multi_fit(const brief_fit_job *jobs, int32_t njobs, int64_t steps, void *stream);

/* optimizer.step() of main.py:399 (torch.optim.Adamax/Adam/SGD single-tensor rules); t is the
 * 1-based step count, lr the scheduler's current value.  state1/state2: exp_avg / exp_inf|exp_avg_sq. */
int brief_optim_step(int kind, float *params, const float *grads, float *state1, float *state2, int64_t count,
                     double lr, double beta1, double beta2, double eps, int64_t t, void *stream);

/* uniform voxel indices in [0, pop) for one step: the device-side stand-in for
 * torch.randint(0, pop_size, (n,)) of main.py:156 (counter-based Philox4x32-10, keyed by seed/step). */
int brief_sample_indices(int64_t *idx, int64_t n, int64_t pop, uint64_t seed, uint64_t step, void *stream);

/* sum of squared differences of two integer volumes (for PSNR, utils/misc.py:451-456); sse_out: one double */
int brief_sse_u16(const uint16_t *a, const uint16_t *b, int64_t n, double *sse_out, void *stream);

/* ---- error-bounded mode: stored corrections (csrc/brief_correct.inc) ----------------------------------------------------
 * dec (the decoded artefact) and src (the volume) are device arrays of n uint8 / uint16 elements (elem_bytes 1 | 2), both 16-byte
 * aligned.  With m = 2 bound + 1, d = src - dec and q = floor((d + bound) / m) (floor division), q != 0 <=> |d| > bound and
 * |d - q m| <= bound: the corrections are the (index, q) pairs with q != 0, and clamp(dec + q m, 0, type max) is within `bound`
 * of src.  Finding them is two passes without atomics (the result is the same on every run, ascending in the index):
 *   brief_correct_count  counts[c] = number of q != 0 among elements [c E, (c + 1) E) of the arrays, E = brief_correct_chunk_elems
 *                        (elem_bytes), for the ceil(n / E) chunks;
 *   (caller)             offsets = exclusive scan of counts (int64), total = their sum;
 *   brief_correct_emit   writes idx_out[k] = base + element index (int64) and q_out[k] = q (int32), k = 0 .. total - 1.
 *   brief_correct_apply  out[idx[k] - base] = clamp(out[idx[k] - base] + q[k] m, 0, type max) for `count` corrections with distinct
 *                        indices in [base, base + n) (others are skipped); out: n elements.
 * `base` is the index of element 0 of the arrays within the volume they are a part of: indices are 64-bit, base + n <= 2^40.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit): elem_bytes 1 | 2, bound 0 .. 65535, n >= 1, alignment as above. */
int64_t brief_correct_chunk_elems(int elem_bytes);
int brief_correct_count(const void *dec, const void *src, int elem_bytes, int64_t n, int64_t bound, int64_t base, int32_t *counts, void *stream);
int brief_correct_emit(const void *dec, const void *src, int elem_bytes, int64_t n, int64_t bound, int64_t base, const int64_t *offsets, int64_t total,
                       int64_t *idx_out, int32_t *q_out, void *stream);
int brief_correct_apply(void *out, int elem_bytes, int64_t n, const int64_t *idx, const int32_t *q, int64_t count, int64_t bound, int64_t base,
                        void *stream);

/* ---- max-intensity projections (csrc/brief_mip.inc) -------------------------------------------------------------------------
 * fold a dense decoded box src[e0][e1][e2][channels] (uint8 | uint16) into three projection images by elementwise MAX:
 *   mip_d[I1][I2][c] = max(mip_d, max over axis 0),  mip_h[I0][I2][c] = max(.., axis 1),  mip_w[I0][I1][c] = max(.., axis 2)
 * the box sits at `origin` inside the image frame `frame` = (I0, I1, I2); images are dense, caller-initialised (0 = identity) */
/* All three images are read-modify-write, so the chunks of a region and the blocks of a partition can be folded one after another on
 * one stream (calls that share an image must not run concurrently).  Exact and the same bits on every run; no atomics and no scratch.
 * Two launches, each reading the box once.  16-byte loads when src is 16-byte aligned and extent[2] * channels * element size is a
 * multiple of 16.  Limits (BRIEF_ERR_INVALID with a message naming the limit): no null buffer, elem_kind BRIEF_OUT_U8 | BRIEF_OUT_U16,
 * channels 1 .. 4, every extent and frame entry >= 1 (frame entries <= 2^31 - 1), origin >= 0 and origin + extent <= frame on every
 * axis, the box and each image at most 2^40 elements. */
int brief_mip_accumulate(const void *src, int elem_kind /* BRIEF_OUT_U8 | BRIEF_OUT_U16 */, const int64_t extent[3], int32_t channels,
                         void *mip_d, void *mip_h, void *mip_w, const int64_t origin[3], const int64_t frame[3], void *stream);

/* ---- weight quantisation (csrc/brief_quant.inc, csrc/brief_quant.h) ----------------------------------------------------------
 * The quantiser of the quantised artefact (module/quantized.bin) and of the quantised fine-tune: uniform, affine, per tensor, every
 * fp32 operation rounded on its own (nothing fused), so that plain numpy float32 arithmetic gives the same bits:
 *     lo = min(w); hi = max(w); top = 2^bits - 1;  step = (hi - lo) / top
 *     code = clamp(rint((w - lo) / step), 0, top)   (rint: ties to even; step == 0: code = 0);   deq = code * step + lo
 * A tensor is a span {offset, count} (elements) of the canonical parameter buffer; `tensors` is a HOST array of ntensors spans, in
 * any order, which travels by value in the kernel arguments.  lo_step: device float [ntensors][2] = (lo, step) per tensor, in the
 * order of `tensors`.  Every call only enqueues on `stream`; there are no atomics and nothing crosses to the host.
 *   brief_quant_workspace_bytes  scratch of brief_quant_ranges for spans of total_count elements altogether in ntensors tensors;
 *   brief_quant_ranges           two launches: a partial (min, max) per 16 Ki-element chunk of a tensor, then lo and step per tensor;
 *   brief_quant_apply            one launch: qparams[i] = deq(code(params[i])) (float, canonical layout; may be NULL) and codes[i] =
 *                                code(params[i]) (uint16 per element, canonical layout; may be NULL) for every element of a span.
 *                                Elements of a GAP between two spans are copied through to qparams unchanged (their codes are left
 *                                alone); nothing in front of the first span or behind the last one is read or written;
 *   brief_quant_decode           one launch: params_out[i] = deq(codes[i]) for every element of a span (gaps are left alone).
 * Limits (BRIEF_ERR_INVALID with a message naming the limit): no null buffer (apply: at least one of qparams / codes), bits 2 .. 16,
 * ntensors 1 .. BRIEF_QUANT_MAX_TENSORS, every span count >= 1 and offset >= 0 with offset + count <= 2^40, no two spans overlapping;
 * a workspace smaller than brief_quant_workspace_bytes: BRIEF_ERR_WORKSPACE. */
#define BRIEF_QUANT_MAX_TENSORS 64
typedef struct {
    int64_t offset, count;
} brief_quant_span;
int64_t brief_quant_workspace_bytes(int64_t total_count, int32_t ntensors);
int brief_quant_ranges(const float *params, const brief_quant_span *tensors, int32_t ntensors, int32_t bits, float *lo_step,
                       void *workspace, int64_t workspace_bytes, void *stream);
int brief_quant_apply(const float *params, const brief_quant_span *tensors, int32_t ntensors, int32_t bits, const float *lo_step,
                      float *qparams, uint16_t *codes, void *stream);
int brief_quant_decode(const uint16_t *codes, const brief_quant_span *tensors, int32_t ntensors, const float *lo_step,
                       float *params_out, void *stream);

/* cal_ssim of utils/misc.py:458-475 for single-channel uint16 volumes [D,H,W]: per z-slice 2-D SSIM (utils/ssim.py:
 * 11-tap Gaussian `window11`, valid padding, K=(0.01,0.03)).  Writes one double per 16x64 output tile, slice-major
 * (brief_ssim_partial_count of them; tiles of slice z are contiguous); slice mean = sum of its tiles / ((H-10)(W-10)),
 * SSIM = mean over slices.  Across ranks: all-reduce [sum of slice means, slices]. */
int64_t brief_ssim_partial_count(int64_t D, int64_t H, int64_t W);
int brief_ssim_u16(const uint16_t *a, const uint16_t *b, int64_t D, int64_t H, int64_t W, const float *window11, double data_range,
                   double *partial, int64_t partial_count, void *stream);

/* Block-boundary filter of DivideTask outputs (reference deblock.py:52-78 / deblock.cpp:277-319): filters the
 * boundary line  x == fixed, y in [a1,a2]  (vertical != 0)  or  y == fixed, x in [a1,a2]  (vertical == 0)  of
 * every slice z1..z2 of a uint16 volume [D,H,W] in place.  mode 1 = deblock.py arithmetic, 0 = deblock.cpp
 * arithmetic.  Lines must be issued in the reference's order (they overlap); see brief_pytorch_amd/deblock.py. */
int brief_deblock_edge(uint16_t *img, int64_t D, int64_t H, int64_t W, int z1, int z2, int fixed, int a1, int a2, int vertical,
                       double index_a, double index_b, double thres, int mode, void *stream);

/* measurement hooks (bench.py): while enabled, every train step records a HIP event pair on the
 * caller's stream around its dominant kernel (the fused forward/loss/dgrad launch);
 * brief_profile_fused waits for them and returns the summed duration and the launch count. */
int brief_profile_enable(int on);
int brief_profile_fused(double *total_ms, int64_t *launches);

/* diagnostics: the kernels' sine / cosine (two-term reduction to revolutions + v_sin_f32 / v_cos_f32, csrc/brief_math.h)
 * evaluated elementwise on device: s[i] = sin(x[i]), c[i] = cos(x[i]).  tests/test_sincos_host.py measures it against
 * float64 (Sine.forward of the reference goes through torch's ~1-ulp sin, utils/Networks.py:227-234). */
int brief_sincos_probe(const float *x, float *s, float *c, int64_t n, void *stream);

/* compute units of the current device as the library sized its grids and workspaces from (256 on a whole MI355X) */
int brief_cu_count(void);

/* ---- FFN: Fourier-feature network (Tancik et al.)  utils/Networks.py:138-207 --------------------------------------------
 *   emb = [sin(2 pi x B^T), cos(2 pi x B^T)]  (B = bvals [embsize, cin], fixed: no gradient, no optimizer state)
 *   Linear(2 embsize, F) + ReLU, (layers - 2) x (Linear(F, F) + ReLU), Linear(F, cout)  (no output activation; skip=False only)
 * Limits (anything else: BRIEF_ERR_INVALID with a message naming the limit): fp32 only, cin 2 | 3, cout 1 .. 4, layers >= 2,
 * features 1 .. 1024 and embsize 1 .. 512 (both padded internally to whole 32-wide tiles), reserved == 0.
 * Canonical parameter buffer (== torch parameters() / state_dict() order):
 *   bvals [embsize][cin] | W0 [F][2 embsize] b0 [F] | (W_l [F][F] b_l [F]) x (layers - 2) | Wh [cout][F] bh [cout]
 * The gradient of the bvals span is written as zero; the optimizer (brief_ffn_fit) updates the MLP span only, and the optimizer
 * state buffers have the canonical buffer's size (their bvals span is not touched). */
typedef struct {
    int32_t cin;         /* 2 | 3 */
    int32_t cout;        /* 1 .. 4 */
    int32_t layers;      /* >= 2 */
    int32_t features;    /* 1 .. 1024 */
    int32_t embsize;     /* 1 .. 512 */
    int32_t reserved;    /* 0 */
} brief_ffn_desc;

/* floats of the canonical buffer (== FFN.calc_param_count, bvals included) / of the fragment-ordered copy / train-step scratch bytes */
int64_t brief_ffn_param_count(const brief_ffn_desc *d);
int64_t brief_ffn_packed_count(const brief_ffn_desc *d);
int64_t brief_ffn_train_workspace_bytes(const brief_ffn_desc *d, int64_t n);
/* canonical params -> fragment-ordered copy (call after every change of params made outside brief_ffn_fit) */
int brief_ffn_repack(const brief_ffn_desc *d, const float *params, float *packed, void *stream);
/* FFN.forward under no_grad, with the out_kind epilogue of brief_siren_forward (no scratch) */
int brief_ffn_forward(const brief_ffn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                      void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* the box decode of brief_siren_forward_box (same box rules and refusals) */
int brief_ffn_forward_box(const brief_ffn_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                          void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* forward + loss + backward of one batch, as brief_siren_train_step (grads: canonical layout, bvals span zero) */
int brief_ffn_train_step(const brief_ffn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                         int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* brief_fit_job with an FFN desc: every field after `desc` means exactly what it means in brief_fit_job
 * (workspace: brief_ffn_train_workspace_bytes(desc, batch.n)) */
typedef struct brief_ffn_fit_job {
    brief_ffn_desc desc;
    brief_grid_desc grid;
    brief_batch_desc batch;
    float *params, *packed;
    float *state1, *state2;
    float *grads;
    float *loss_out;
    float *loss_log;
    void *workspace;
    int64_t workspace_bytes;
    int32_t loss_kind, optim_kind;
    float thr, beta;
    double lr, beta1, beta2, eps;
    const int64_t *milestones;
    int32_t n_milestones, reserved;
    double gamma;
    int64_t t0;
    const double *lr_table, *beta1_table;
    int64_t idx_stride;
} brief_ffn_fit_job;
/* `steps` optimizer steps (train step + reduction + update + repack: four launches each, no host synchronisation) */
int brief_ffn_fit(const brief_ffn_fit_job *job, int64_t steps, void *stream);

/* ---- NeRF: positional-encoding network (Mildenhall et al.)  utils/Networks.py:64-136 ----------------------------------------
 *   enc = [x_0 .. x_{cin-1}, sin(2^0 pi x_0), cos(2^0 pi x_0), sin(2^0 pi x_1), cos(2^0 pi x_1), ..., cos(2^{Lf-1} pi x_{cin-1})]
 *   (d = cin (1 + 2 frequencies) columns; the phase is the fp32 number 2^i fl32(fl32(pi) x), as the reference's fp32 torch.sin sees it)
 *   Linear(d, F) + ReLU, (layers - 2) x (Linear(F, F) + ReLU), Linear(F, cout)  (no output activation)
 *   skip != 0: the hidden layer sl = (layers - 1) / 2 is Linear(d + F, F) + ReLU on cat[enc, h] (encoding columns first)
 * Limits (anything else: BRIEF_ERR_INVALID with a message naming the limit): fp32 only, cin 2 | 3, cout 1 .. 4, layers >= 2 (>= 3 with
 * skip), features 1 .. 1024 (padded internally to whole 32-wide tiles), frequencies 0 .. 16, skip 0 | 1.
 * Canonical parameter buffer (== torch parameters() / state_dict() order):
 *   W0 [F][d] b0 [F] | (W_l [F][F] b_l [F]) x (layers - 2), W_sl [F][d + F] with skip | Wh [cout][F] bh [cout]
 * The whole buffer is trained (the encoding has no parameters). */
typedef struct {
    int32_t cin;          /* 2 | 3 */
    int32_t cout;         /* 1 .. 4 */
    int32_t layers;       /* >= 2; >= 3 with skip */
    int32_t features;     /* 1 .. 1024 */
    int32_t frequencies;  /* 0 .. 16 */
    int32_t skip;         /* 0 | 1 */
} brief_nerf_desc;

/* floats of the canonical buffer (== NeRF.calc_param_count) / of the fragment-ordered copy / train-step scratch bytes */
int64_t brief_nerf_param_count(const brief_nerf_desc *d);
int64_t brief_nerf_packed_count(const brief_nerf_desc *d);
int64_t brief_nerf_train_workspace_bytes(const brief_nerf_desc *d, int64_t n);
/* canonical params -> fragment-ordered copy (call after every change of params made outside brief_nerf_fit) */
int brief_nerf_repack(const brief_nerf_desc *d, const float *params, float *packed, void *stream);
/* NeRF.forward under no_grad, with the out_kind epilogue of brief_siren_forward (no scratch) */
int brief_nerf_forward(const brief_nerf_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                       void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* the box decode of brief_siren_forward_box (same box rules and refusals) */
int brief_nerf_forward_box(const brief_nerf_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                           void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* forward + loss + backward of one batch, as brief_siren_train_step (grads: canonical layout) */
int brief_nerf_train_step(const brief_nerf_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                          int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                          void *workspace, int64_t workspace_bytes, void *stream);
/* brief_fit_job with a NeRF desc: every field after `desc` means exactly what it means in brief_fit_job
 * (workspace: brief_nerf_train_workspace_bytes(desc, batch.n)) */
typedef struct brief_nerf_fit_job {
    brief_nerf_desc desc;
    brief_grid_desc grid;
    brief_batch_desc batch;
    float *params, *packed;
    float *state1, *state2;
    float *grads;
    float *loss_out;
    float *loss_log;
    void *workspace;
    int64_t workspace_bytes;
    int32_t loss_kind, optim_kind;
    float thr, beta;
    double lr, beta1, beta2, eps;
    const int64_t *milestones;
    int32_t n_milestones, reserved;
    double gamma;
    int64_t t0;
    const double *lr_table, *beta1_table;
    int64_t idx_stride;
} brief_nerf_fit_job;
/* `steps` optimizer steps (train step + reduction + update + repack: four launches each, no host synchronisation) */
int brief_nerf_fit(const brief_nerf_fit_job *job, int64_t steps, void *stream);

/* ---- MFN: multiplicative filter networks MFNFourier / MFNGabor (Fathony et al.)  utils/Networks.py:648-799 -------------------
 *   filter i = 0 .. layers-2:  a_i = Wf_i x + bf_i;  g_i = sin(a_i)  (filter 0, Fourier)  or
 *                              g_i = sin(a_i) exp(-0.5 gamma_i (|x|^2 + |mu_i|^2 - 2 x.mu_i))  (filter 1, Gabor)
 *   z_0 = g_0,  z_i = g_i . (W_i z_{i-1} + b_i)  (i = 1 .. layers-2),  out = Wo z_{layers-2} + bo,  sin(out) with output_act (no w0)
 * Limits (anything else: BRIEF_ERR_INVALID with a message naming the limit): fp32 only, cin 2 | 3, cout 1 .. 4, layers >= 2,
 * features 1 .. 1024 (padded internally to whole 32-wide tiles), filter 0 | 1, output_act 0 | 1; every Linear carries a bias.
 * Canonical parameter buffer (== torch state_dict() order):
 *   (W_i [F][F] b_i [F]) x (layers - 2) | Wo [cout][F] bo [cout] | per filter: [mu [F][cin] gamma [F]] (Gabor) Wf [F][cin] bf [F]
 * The whole buffer is trained (input_scale / weight_scale / alpha / beta of the reference shape the init only). */
typedef struct {
    int32_t cin;          /* 2 | 3 */
    int32_t cout;         /* 1 .. 4 */
    int32_t layers;       /* >= 2 */
    int32_t features;     /* 1 .. 1024 */
    int32_t filter;       /* 0 Fourier | 1 Gabor */
    int32_t output_act;   /* 0 | 1 */
} brief_mfn_desc;

/* floats of the canonical buffer (== MFNFourier / MFNGabor.calc_param_count) / of the fragment-ordered copy / train-step scratch bytes */
int64_t brief_mfn_param_count(const brief_mfn_desc *d);
int64_t brief_mfn_packed_count(const brief_mfn_desc *d);
int64_t brief_mfn_train_workspace_bytes(const brief_mfn_desc *d, int64_t n);
/* canonical params -> fragment-ordered copy (call after every change of params made outside brief_mfn_fit) */
int brief_mfn_repack(const brief_mfn_desc *d, const float *params, float *packed, void *stream);
/* MFN forward under no_grad, with the out_kind epilogue of brief_siren_forward (no scratch) */
int brief_mfn_forward(const brief_mfn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                      void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* the box decode of brief_siren_forward_box (same box rules and refusals) */
int brief_mfn_forward_box(const brief_mfn_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                          void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* forward + loss + backward of one batch, as brief_siren_train_step (grads: canonical layout) */
int brief_mfn_train_step(const brief_mfn_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                         int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* brief_fit_job with an MFN desc: every field after `desc` means exactly what it means in brief_fit_job
 * (workspace: brief_mfn_train_workspace_bytes(desc, batch.n)) */
typedef struct brief_mfn_fit_job {
    brief_mfn_desc desc;
    brief_grid_desc grid;
    brief_batch_desc batch;
    float *params, *packed;
    float *state1, *state2;
    float *grads;
    float *loss_out;
    float *loss_log;
    void *workspace;
    int64_t workspace_bytes;
    int32_t loss_kind, optim_kind;
    float thr, beta;
    double lr, beta1, beta2, eps;
    const int64_t *milestones;
    int32_t n_milestones, reserved;
    double gamma;
    int64_t t0;
    const double *lr_table, *beta1_table;
    int64_t idx_stride;
} brief_mfn_fit_job;
/* `steps` optimizer steps (train step + reduction + update + repack: four launches each, no host synchronisation) */
int brief_mfn_fit(const brief_mfn_fit_job *job, int64_t steps, void *stream);

/* ---- tapered SIRENs: SIREN_Pyramid, SIRENFT, SIRENPS  utils/Networks.py:316-552 ---------------------------------------------
 *   a SIREN whose every Linear has its own width and every sine its own w0:
 *   h_0 = sin(w0[0] (W_0 x + b_0)),  h_l = sin(w0[l] (W_l h_{l-1} + b_l))  (l = 1 .. layers-2),  y = Wh h_{layers-2} + bh,
 *   sin(w0[layers-1] y) with output_act.  W_l is [widths[l]][widths[l-1]] (W_0: [widths[0]][cin], Wh: [cout][widths[layers-2]]).
 * Limits (anything else: BRIEF_ERR_INVALID with a message naming the limit): fp32 only, cin 2 | 3, cout 1 .. 4, layers 3 ..
 * BRIEF_TAPER_MAX_LAYERS, every hidden width 1 .. 1024 (each layer padded on its own to whole 32-wide tiles), output_act 0 | 1.
 * Canonical parameter buffer (== torch state_dict() order): (W_l b_l) per Linear in layer order.  The whole buffer is trained. */
#define BRIEF_TAPER_MAX_LAYERS 16
typedef struct {
    int32_t cin;          /* 2 | 3 */
    int32_t cout;         /* 1 .. 4 */
    int32_t layers;       /* 3 .. BRIEF_TAPER_MAX_LAYERS Linear layers, the head included */
    int32_t output_act;   /* 0 | 1 */
    int32_t widths[BRIEF_TAPER_MAX_LAYERS];   /* outputs of Linear 0 .. layers-2 (1 .. 1024 each); the rest is ignored */
    float w0[BRIEF_TAPER_MAX_LAYERS];         /* w0 of the sine behind Linear l (l = layers-1: the output activation) */
} brief_taper_desc;

/* floats of the canonical buffer / of the fragment-ordered copy / train-step scratch bytes */
int64_t brief_taper_param_count(const brief_taper_desc *d);
int64_t brief_taper_packed_count(const brief_taper_desc *d);
int64_t brief_taper_train_workspace_bytes(const brief_taper_desc *d, int64_t n);
/* canonical params -> fragment-ordered copy (call after every change of params made outside brief_taper_fit) */
int brief_taper_repack(const brief_taper_desc *d, const float *params, float *packed, void *stream);
/* forward under no_grad, with the out_kind epilogue of brief_siren_forward (no scratch) */
int brief_taper_forward(const brief_taper_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                        void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* the box decode of brief_siren_forward_box (same box rules and refusals) */
int brief_taper_forward_box(const brief_taper_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                            void *out, int out_kind, float scale_min, float scale_max, double vmin, double vmax, void *stream);
/* forward + loss + backward of one batch, as brief_siren_train_step (grads: canonical layout) */
int brief_taper_train_step(const brief_taper_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                           int loss_kind, float thr, float beta, float *grads, float *loss_out, float *yhat_out,
                           void *workspace, int64_t workspace_bytes, void *stream);
/* brief_fit_job with a tapered desc: every field after `desc` means exactly what it means in brief_fit_job
 * (workspace: brief_taper_train_workspace_bytes(desc, batch.n)) */
typedef struct brief_taper_fit_job {
    brief_taper_desc desc;
    brief_grid_desc grid;
    brief_batch_desc batch;
    float *params, *packed;
    float *state1, *state2;
    float *grads;
    float *loss_out;
    float *loss_log;
    void *workspace;
    int64_t workspace_bytes;
    int32_t loss_kind, optim_kind;
    float thr, beta;
    double lr, beta1, beta2, eps;
    const int64_t *milestones;
    int32_t n_milestones, reserved;
    double gamma;
    int64_t t0;
    const double *lr_table, *beta1_table;
    int64_t idx_stride;
} brief_taper_fit_job;
/* `steps` optimizer steps (train step + reduction + update + repack: four launches each, no host synchronisation) */
int brief_taper_fit(const brief_taper_fit_job *job, int64_t steps, void *stream);

/* ---- spatial-gradient decode of an fp32 SIREN (csrc/brief_jac.inc) ---------------------------------------------------------------
 * value[n][cout] = phi(x_n) and jac[n][cout][cin] = d phi_c / d x_a (x_n), the analytic Jacobian with respect to the coordinates, in
 * coordinate units (per unit of the grid's [lo, hi] range); with output_act, of the activated output.  Forward mode on the matrix pipe:
 * the value and its cin tangents travel through the layers together, 8 samples x 4 quantities per 32-column MFMA tile.  Both outputs
 * are float32; value may be NULL.  The kernels read a forward-only fragment buffer of their own (brief_siren_jac_packed_count floats,
 * written by brief_siren_jac_repack from the canonical parameters: call it after every change of them).  Sample sources are those of
 * brief_siren_forward (batch.coords, batch.idx, batch.offset, grid coordinates) and of brief_siren_forward_box (the same box rules and
 * refusals; coordinates bit-identical to it), so a box equals the slice of the whole and results do not depend on how a box is cut
 * into calls.  Enqueue-only on `stream`: no allocation, no synchronisation.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): precision BRIEF_PREC_F32, features 1 .. 1024,
 * layers >= 2, cin 2 | 3, cout 1 .. 4, packed and jac not NULL, n >= 1, and everything the forward entries refuse of a batch / box. */
int64_t brief_siren_jac_packed_count(const brief_siren_desc *d);
int brief_siren_jac_repack(const brief_siren_desc *d, const float *params, float *packed, void *stream);
int brief_siren_jac_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                            float *value /* [n][cout] or NULL */, float *jac /* [n][cout][cin] */, void *stream);
int brief_siren_jac_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                                float *value, float *jac, void *stream);

/* ---- orthographic view decode: oblique slices and projections along any direction (csrc/brief_view.inc, csrc/brief_view.h) --------
 * A view is a lattice of rows x cols rays with `depth` samples each, in voxel-index units of the fitted grid `dims` ((d,h,w) order):
 *     position    p_a = fl(fl(fl(origin_a + fl(row * drow_a)) + fl(col * dcol_a)) + fl(k * ddepth_a))       (fp32, nothing contracted)
 *     inside      box_lo_a <= p_a <= box_hi_a on every axis (an inclusive clip box within [0, dims_a - 1])
 *     coordinate  p_a < (float)(dims_a / 2) ? fma(step_a, p_a, lo) : fma(-step_a, (float)(dims_a - 1) - p_a, hi),
 *                 step_a = (hi - lo) / (float)(dims_a - 1): at an integer position the grid's own coordinate, bit for bit.
 * Only samples inside the clip box are evaluated, by the net's own forward entry on explicit coordinates (integer output kind):
 *   brief_view_clip    k0[r], cnt[r] (int32, r = row * cols + col): the inside samples of ray r are exactly k0 <= k < k0 + cnt (along a
 *                      ray every p_a is monotone in k, so they are one interval, found by bisection on the position itself);
 *   (caller)           off = exclusive scan of cnt (int64, rows * cols + 1 entries): the compacted, ray-major sample list, sample
 *                      off[r] + j being (row, col, k0[r] + j);
 *   brief_view_coords  coords[s - s0][3] for the samples s0 <= s < s1 of the list;
 *   (caller)           vals[s - s0][channels] = the forward entry on coords, out_kind BRIEF_OUT_U8 | BRIEF_OUT_U16;
 *   brief_view_fold    folds vals into the accumulators: hits[r] (int32, inside samples so far) and acc, int32 [rays][channels] for
 *                      BRIEF_VIEW_MAX / _MIN / _SLICE (running max / min; a slice is the max over its single plane) or int64
 *                      [rays][channels] for BRIEF_VIEW_MEAN (running sum).  The caller initialises hits = 0 and acc = 0 (min: INT32_MAX);
 *   brief_view_finish  out[r][c] = acc as uint8 / uint16 (elem_kind), or for _MEAN the float (float)((double)sum / hits); 0 where hits == 0.
 * [r0, r1) names the rays that may hold a sample of [s0, s1) (off[r + 1] > s0 and off[r] < s1); `lanes` (a power of two, 1 .. 64) is
 * the number of adjacent lanes that share a ray, best near the mean cnt.  No atomics: within a launch a pixel has one owner; all
 * accumulators are read-modify-write, so the chunks of a view follow each other on one stream.  Integers throughout: the result is
 * exact and independent of chunking, `lanes` and the run.  Every device entry only enqueues on `stream`.
 * brief_view_sample_host / brief_view_clip_host evaluate the same header on the host CPU, without any GPU call (pos, coord: [n][3];
 * any of pos / coord / inside may be NULL).
 * Limits (BRIEF_ERR_INVALID with a message naming the limit): rows, cols, depth 1 .. 2^24 - 1; dims 2 .. 2^31 - 1; everything finite;
 * 0 <= box_lo <= box_hi <= dims - 1; at most 2^40 rays; no null buffer; channels 1 .. 4; sample indices inside the lattice. */
typedef struct {
    int64_t dims[3];
    float lo, hi;                            /* coordinate range of the fitted grid */
    float origin[3];                         /* position of sample (0, 0, 0) */
    float drow[3], dcol[3], ddepth[3];       /* position steps per row, column and depth sample */
    int32_t rows, cols, depth, reserved;
    float box_lo[3], box_hi[3];              /* inclusive clip box */
} brief_view_desc;
enum { BRIEF_VIEW_MAX = 0, BRIEF_VIEW_MIN = 1, BRIEF_VIEW_MEAN = 2, BRIEF_VIEW_SLICE = 3 };
int brief_view_clip(const brief_view_desc *view, int32_t *k0, int32_t *cnt, void *stream);
int brief_view_coords(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                      int32_t lanes, float *coords, void *stream);
int brief_view_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                    int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits, void *acc, void *stream);
int brief_view_finish(const brief_view_desc *view, int elem_kind, int32_t channels, int32_t mode, const int32_t *hits, const void *acc, void *out,
                      void *stream);
int brief_view_sample_host(const brief_view_desc *view, const int32_t *row, const int32_t *col, const int32_t *k, int64_t n, float *pos, float *coord,
                           uint8_t *inside);
int brief_view_clip_host(const brief_view_desc *view, int32_t *k0, int32_t *cnt);

/* ---- view decode of a partition (a DivideTask artefact, one net per block): the nearest block owns a sample (csrc/brief_view.h) ----
 * The view stays the view of the WHOLE volume (view->dims, positions p_a as above).  A block with the inclusive index range
 * [start_a, start_a + dims_a - 1] owns the half-open cell start_a - 0.5 <= p_a < start_a + dims_a - 0.5 on every axis; a sample is
 * evaluated for the block iff it is inside the clip box and owned.  The cells of a tiling partition are disjoint and cover
 * [-0.5, N - 0.5), and both tests read the global float p_a: every sample inside the clip box has exactly one owner.
 *     local       q_a = fl(p_a - (float)start_a)
 *     coordinate  q_a < (float)(dims_a / 2) ? fma(step_a, q_a, lo) : fma(-step_a, (float)(dims_a - 1) - q_a, hi),
 *                 step_a = (hi - lo) / (float)(dims_a - 1): the BLOCK grid's own coordinate at an integer position, bit for bit; up to
 *                 half a voxel outside the block's grid for q_a in [-0.5, 0) or (dims_a - 1, dims_a - 0.5).  lo / hi: view->lo / hi.
 * Only the rays of the block's window [row0, row0 + wrows) x [col0, col0 + wcols) are clipped and walked; WINDOW RAY w is the image
 * ray (row0 + w / wcols, col0 + w % wcols).  k0, cnt and off are indexed by window ray, hits and acc by image ray:
 *   brief_view_part_clip    k0[w], cnt[w] (wrows * wcols entries): the samples the block evaluates on window ray w;
 *   (caller)                off = exclusive scan of cnt (int64, wrows * wcols + 1 entries; it may be a slice of one scan over the
 *                           windows of all blocks: s0 / s1 below are in off's own numbering);
 *   brief_view_part_coords  coords[s - s0][3], block-local, for the samples s0 <= s < s1 of the list; [r0, r1) are WINDOW rays;
 *   brief_view_part_fold    brief_view_fold with the exact test (clip box and cell) on every sample; lane 0 of a ray's group does one
 *                           plain read-modify-write of the image pixel's hits and acc.  No atomics: within a launch a pixel has one
 *                           owner, and the launches of a view (all blocks) follow each other on one stream.
 * brief_view_finish is the finish of a partition as well.  Integers throughout: blocks fold in any order to the same bits.
 * brief_view_part_clip_host / brief_view_part_sample_host evaluate the same header on the host CPU (pos, local, coord: [n][3]; any
 * output may be NULL; inside: the clip box's closed test; owned: the cell's half-open test).
 * Limits, besides those of the view entries: every view->dims below 2^23 (the cell bounds are exact floats); start >= 0, dims >= 2,
 * start + dims <= view->dims; row0, col0 >= 0, wrows, wcols >= 1, the window inside the image. */
typedef struct {
    int64_t start[3];                        /* the block's first voxel in the whole volume */
    int64_t dims[3];                         /* the block's own grid */
    int32_t row0, col0, wrows, wcols;        /* the window of image rays that can meet the block */
} brief_view_part;
int brief_view_part_clip(const brief_view_desc *view, const brief_view_part *part, int32_t *k0, int32_t *cnt, void *stream);
int brief_view_part_coords(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                           int64_t r0, int64_t r1, int32_t lanes, float *coords, void *stream);
int brief_view_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                         int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits,
                         void *acc, void *stream);
int brief_view_part_clip_host(const brief_view_desc *view, const brief_view_part *part, int32_t *k0, int32_t *cnt);
int brief_view_part_sample_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *row, const int32_t *col, const int32_t *k,
                                int64_t n, float *pos, float *local, float *coord, uint8_t *inside, uint8_t *owned);

/* ---- surface view: first-hit depth, sub-sample refinement and shaded normals of an isosurface (csrc/brief_view.inc) ----------------
 * For every ray of a view: the first inside sample at which channel `channel` of the integer decode passes the side test,
 * value >= level (BRIEF_SURFACE_ABOVE) or value <= level (BRIEF_SURFACE_BELOW); a bisection of that crossing; a Lambert shading from
 * the analytic Jacobian at the hit.  Clip, scan and the march's coordinates are brief_view_clip / (caller) / brief_view_coords:
 *   brief_surface_fold     brief_view_fold's arguments and walk; folds first[r] (int32, caller-initialised to INT32_MAX: the smallest
 *                          inside k whose value passes) and hits[r] (int32, caller-initialised to 0), read-modify-write, one owner per
 *                          pixel, no atomics;
 *   brief_surface_bracket  t_lo[r], t_hi[r] (float): (first - 1, first) where first > k0 (sample first - 1 is inside and fails the test),
 *                          (first, first) for a CUT ray (first == k0: the clip box slices the object open; never refined), (NaN, NaN)
 *                          without a hit (first < 0 or INT32_MAX);
 *   brief_surface_coords   DENSE coords[r][3], and pos[r][3] unless NULL, of every ray at depth t = fl(t_lo + fl(0.5f * fl(t_hi - t_lo)))
 *                          where t_lo < t_hi and midpoint == 1, else at t = t_hi: position p_a = fl(base_a + fl(t * ddepth_a)), base_a
 *                          the position of sample (row, col, 0); at an integer t the sample's own position, bit for bit.  A ray
 *                          without a hit gets the clip box's corner box_lo as a valid coordinate (its value is never read), pos NaN;
 *   (caller)               vals[r][channels] = the forward entry on coords, out_kind BRIEF_OUT_U8 | BRIEF_OUT_U16;
 *   brief_surface_step     where t_lo < t_hi: t_hi = t_mid if vals[r][channel] passes the test, else t_lo = t_mid.  The test fails at
 *                          t_lo and passes at t_hi before and after; t_hi is the hit;
 *   brief_surface_shade    from jac[r][channels][3] (brief_siren_jac_forward on the hits' coordinates): g_a = jac[r][channel][a] *
 *                          gscale[a] (the host's grey levels per physical unit), normal[r][3] = -g / |g| (ABOVE: out of a bright object)
 *                          or +g / |g| (BELOW), shade[r] = max(0, -(normal . light)), light[3] the unit direction the light travels.
 *                          normal and shade are 0 where t[r] is NaN (no hit) or |g| is 0 or not finite.
 * Every decision compares decoded integers: first, t_lo and t_hi are exact and independent of chunking, `lanes` and the run.  gscale
 * and light are HOST pointers to three floats; every other buffer is device memory.  Every device entry only enqueues on `stream`.
 * brief_view_sample_t_host is brief_view_sample_host at a real depth 0 <= t <= depth - 1, on the host CPU.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of the view entries; no null buffer (pos of
 * brief_surface_coords excepted); channels 1 .. 4; channel 0 .. channels - 1; level 0 .. 255 (uint8) or 0 .. 65535 (uint16); side
 * BRIEF_SURFACE_ABOVE | _BELOW; midpoint 0 | 1; gscale and light finite. */
enum { BRIEF_SURFACE_ABOVE = 0, BRIEF_SURFACE_BELOW = 1 };
int brief_surface_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                       int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side, int32_t *hits,
                       int32_t *first, void *stream);
int brief_surface_bracket(const brief_view_desc *view, const int32_t *k0, const int32_t *first, float *t_lo, float *t_hi, void *stream);
int brief_surface_coords(const brief_view_desc *view, const float *t_lo, const float *t_hi, int32_t midpoint, float *coords, float *pos, void *stream);
int brief_surface_step(const brief_view_desc *view, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                       float *t_lo, float *t_hi, void *stream);
int brief_surface_shade(const brief_view_desc *view, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                        const float *gscale, const float *light, float *normal, float *shade, void *stream);
int brief_view_sample_t_host(const brief_view_desc *view, const int32_t *row, const int32_t *col, const float *t, int64_t n, float *pos, float *coord,
                             uint8_t *inside);

/* ---- surface view of a partition: hits are routed across blocks (csrc/brief_surface_part.inc, csrc/brief_view.h) ------------------------
 * The view is brief_view_part_*'s, the test and the bracket are the surface view's.  first[r] is the smallest owned inside k whose value
 * passes, a min over all blocks; the bracket comes from brief_view_clip on the whole view and brief_surface_bracket: (first - 1, first)
 * where first > k0[r], whether sample first - 1 is owned or lies in a gap.  A bracket can straddle a face, so every point a round
 * evaluates, and the hit itself, is routed to the block whose half-open cell holds its global position p_a = fl(base_a + fl(t *
 * ddepth_a)): a point exactly on a face belongs to the upper block.  The gap rule `empty`: a point no block owns holds nothing and
 * fails the test on either side.
 *   brief_surface_part_fold    brief_view_part_fold's arguments and walk (window rays, the exact clip-box-and-cell test on every sample)
 *                              with brief_surface_fold's fold; lane 0 of a ray's group does one plain read-modify-write of the IMAGE
 *                              pixel's hits and first (caller-initialised to 0 and INT32_MAX).  No atomics;
 *   brief_surface_part_route   owner[r] (int32, one per image ray) = the index in parts[0 .. nparts) of the block whose cell holds the ray's
 *                              point at t = the bracket's midpoint (midpoint == 1) or t_hi (midpoint == 0); -1 where the ray has nothing
 *                              to evaluate: t is NaN; with midpoint == 1, not t_lo < t_hi; with midpoint == 1, no block owns the point,
 *                              and then the kernel itself sets t_lo[r] = t_mid.  parts is a DEVICE array of brief_view_part (an empty
 *                              window, wrows == wcols == 0, is allowed here: the window plays no part); O(nparts) per ray;
 *   (caller)                   buckets the rays by owner: per block a LIST of image-ray indices, int64, each ray in at most one list;
 *   brief_surface_part_coords  coords[i][3], block-local (brief_view_part_coords' rule at the real depth t), of the point of ray rays[i],
 *                              i < n; where pos is not NULL also the global pos[rays[i]][3] (NaN where the ray has no point);
 *   (caller)                   vals[i][channels] = the owner's forward entry on coords, with the block's own integer epilogue;
 *   brief_surface_part_step    brief_surface_step on a list: vals[i] moves the bracket of ray rays[i];
 *   brief_surface_part_shade   brief_surface_shade on a list, jac[i][channels][3] for ray rays[i] and the owner's own gscale; it writes
 *                              normal[rays[i]] and shade[rays[i]] only: the caller zero-initialises both.
 * Every decision compares decoded integers, or floats that depend on the ray alone: first, t_lo, t_hi and owner do not depend on the
 * order of the blocks, on chunking, on the bucketing, on `lanes` or on the run.  gscale and light are HOST pointers to three floats.
 * brief_surface_part_route_host is the route on the host CPU (every buffer host memory, t_lo updated in place);
 * brief_view_part_sample_t_host is brief_view_part_sample_host at a real depth 0 <= t <= depth - 1.  Neither makes a GPU call.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of brief_view_part_fold and of the surface
 * entries; nparts 1 .. 2^31 - 1; n >= 1; midpoint 0 | 1; no null buffer (pos excepted).  A DEVICE table or list cannot be read before a
 * launch: the route trusts parts (it only compares floats against it), brief_surface_part_coords skips a list entry outside the image,
 * _step and _shade a negative one; the host entry checks every block as brief_view_part_clip does. */
int brief_surface_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1,
                            int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level,
                            int32_t side, int32_t *hits, int32_t *first, void *stream);
int brief_surface_part_route(const brief_view_desc *view, const brief_view_part *parts, int32_t nparts, float *t_lo, const float *t_hi, int32_t midpoint,
                             int32_t *owner, void *stream);
int brief_surface_part_coords(const brief_view_desc *view, const brief_view_part *part, const float *t_lo, const float *t_hi, int32_t midpoint,
                              const int64_t *rays, int64_t n, float *coords, float *pos, void *stream);
int brief_surface_part_step(const int64_t *rays, int64_t n, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                            float *t_lo, float *t_hi, void *stream);
int brief_surface_part_shade(const int64_t *rays, int64_t n, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                             const float *gscale, const float *light, float *normal, float *shade, void *stream);
int brief_surface_part_route_host(const brief_view_desc *view, const brief_view_part *parts, int32_t nparts, float *t_lo, const float *t_hi,
                                  int32_t midpoint, int32_t *owner);
int brief_view_part_sample_t_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *row, const int32_t *col, const float *t,
                                  int64_t n, float *pos, float *local, float *coord, uint8_t *inside, uint8_t *owned);

/* ---- composite view: front-to-back emission-absorption rendering through a transfer table (csrc/brief_composite.inc, .h) ------------
 * Clip, scan and the march's coordinates are brief_view_clip / (caller) / brief_view_coords.  Channel `channel` of the integer decode is
 * classified by the table tf, int32 [2^tf_bits][4] = (tau, eR, eG, eB), at the index value >> (bits of the dtype - tf_bits):
 *     tau   the sample's optical depth in units of 2^-16 octaves (the sample multiplies the transmittance by 2^(-tau / 65536)),
 *           0 .. TAU_SAT = 32 * 65536, TAU_SAT being opaque;
 *     e_c   the premultiplied emission round(256 * colour_c * (1 - 2^(-tau / 65536))), 0 .. 65280.
 * Over the inside samples of a ray in ascending k, all in integers: P_i = min(sum of the tau before sample i, TAU_SAT);
 * acc_c = sum of W(P_i) * e_c(i) (uint64), W the transmittance in Q0.32 from two 256-entry constant tables, W(0) = 2^32, W(TAU_SAT) = 0;
 *   brief_view_composite_fold    brief_view_fold's arguments and walk; per pass a scan of tau over the lanes of a ray's group plus the
 *                                ray's running carry gives P_i; lane 0 does one plain read-modify-write of the pixel's state: hits[r]
 *                                (int32), tau_run[r] (int32: the saturated running optical depth, the carry-in of the ray's next chunk)
 *                                and acc[r][3] (uint64), all caller-initialised to 0.  No atomics; the chunks of a view follow the
 *                                list's order on one stream, so the earlier part of a ray is folded first;
 *   brief_view_composite_finish  out[r][4] (uint8) = R, G, B, A: out_c = min(255, (acc_c + bg_c * 256 * W(P_total) + 2^39) >> 40), RGB already
 *                                composited over background[3] (a HOST pointer, 0 .. 255 each), A = min(255, ((2^32 - W(P_total)) * 255
 *                                + 2^31) >> 32).
 * Sums of integers, and a prefix that depends on a sample's place along its ray alone: the image is exact and independent of chunking,
 * `lanes` and the run.  Every device entry only enqueues on `stream`; tf is device memory there.
 * brief_view_composite_host is the same fold and finish on the host CPU, without any GPU call: every buffer is host memory, off[0] is 0 and
 * vals [off[rays]][channels] holds the whole list; hits, tau_run and acc may be NULL.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of the view entries; no null buffer; elem_kind
 * BRIEF_OUT_U8 | BRIEF_OUT_U16; channels 1 .. 4; channel 0 .. channels - 1; tf_bits 1 .. 8 (uint8) or 1 .. 16 (uint16); tf 16-byte and out
 * 4-byte aligned; background 0 .. 255.  The table's entries are checked where it is host-visible (brief_view_composite_host: tau 0 ..
 * TAU_SAT, e_c 0 .. 65280; composite.make_transfer); the kernel reads them as they are. */
int brief_view_composite_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                              int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                              int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream);
int brief_view_composite_finish(const brief_view_desc *view, const int32_t *background, const int32_t *hits, const int32_t *tau_run, const uint64_t *acc,
                                uint8_t *out, void *stream);
int brief_view_composite_host(const brief_view_desc *view, const int32_t *k0, const int64_t *off, const void *vals, int elem_kind, int32_t channels,
                              int32_t channel, const int32_t *tf, int32_t tf_bits, const int32_t *background, int32_t *hits, int32_t *tau_run,
                              uint64_t *acc, uint8_t *out);

/* ---- composite view of a partition: the prefix is carried across blocks (csrc/brief_composite.inc, .h) -----------------------------
 * The view of a partition is brief_view_part_*'s: per pixel and block the owned samples are one interval of k, a SEGMENT; a pixel's
 * segments are disjoint and their k0 order them front to back.  The image is the composite above over a pixel's owned samples in
 * ascending k, whichever block owns them: the weight of a sample is W(min(C + L, TAU_SAT)), L the optical depth in front of it inside
 * its own segment, C = min(sum of the totals T of the segments in front, TAU_SAT).  The blocks are evaluated in separate passes, in no
 * depth order, so the state lives per WINDOW RAY (k0, cnt and off's numbering), in block-major arrays over the windows of all blocks:
 *   brief_view_composite_part_fold    brief_view_composite_fold on a block's list with brief_view_part_fold's exact test (clip box and
 *                                     cell); lane 0 of a ray's group does one plain read-modify-write of hits_w[w] (int32; may be NULL),
 *                                     tau_w[w] (int32: the carry-in, then the carry-out) and acc_w[w][3] (uint64), w the window ray within
 *                                     the block's slice.  PASS A: all state 0; it leaves T = tau_w and the colour sums under carry-in 0;
 *   brief_view_composite_part_carry   one thread per window ray of all blocks: carry[w] = C over the segments of the same pixel with a
 *                                     smaller k0, and cnt2[w] = cnt[w] where 0 < C < TAU_SAT, else 0.  wins: the DEVICE table of the
 *                                     blocks' windows and slice bases (base[0] = 0, base[b + 1] = base[b] + wrows * wcols of b, the
 *                                     last one ending at window_rays; an empty window has wrows = wcols = 0);
 *   PASS B                            the same march and fold over the scan of cnt2, tau_w2 preloaded with carry, acc_w2 zeroed: only
 *                                     segments behind something partly opaque are evaluated a second time (C == 0: pass A is final;
 *                                     C == TAU_SAT: nothing is visible);
 *   brief_view_composite_part_gather  one thread per pixel, over the blocks whose window holds it: hits = sum of hits_w, tau_run = the
 *                                     saturated sum of tau_w (pass A's), acc = sum of acc_w where carry == 0 and of acc_w2 where
 *                                     0 < carry < TAU_SAT; hits, tau_run, acc are per image ray, for brief_view_composite_finish.
 * Integers throughout, and the carry follows k0, not the order of the blocks: the image does not depend on that order, on chunking,
 * `lanes` or the run.  No atomics: a window ray has one owner in a launch, and a block's chunks follow each other on one stream.
 * The *_host entries are the same arithmetic on the host CPU, without any GPU call: every buffer is host memory; the fold's vals holds
 * the block's whole list (sample s at s - off[0]); the table of windows is checked entry by entry there.  A DEVICE table cannot be read
 * before a launch: the device entries trust it, and a malformed one is undefined behaviour.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of brief_view_part_fold and
 * brief_view_composite_fold; no null buffer (hits_w of the fold excepted); blocks >= 1; window_rays >= 1. */
typedef struct {
    int64_t base;                            /* the first entry of the block's slice of the window-ray arrays */
    int32_t row0, col0, wrows, wcols;        /* the block's window (brief_view_part's) */
} brief_composite_window;
int brief_view_composite_part_fold(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off, int64_t s0,
                                   int64_t s1, int64_t r0, int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels,
                                   int32_t channel, const int32_t *tf, int32_t tf_bits, int32_t *hits_w, int32_t *tau_w, uint64_t *acc_w,
                                   void *stream);
int brief_view_composite_part_carry(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                    const int32_t *k0, const int32_t *cnt, const int32_t *tau_w, int32_t *carry, int32_t *cnt2, void *stream);
int brief_view_composite_part_gather(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                     const int32_t *hits_w, const int32_t *tau_w, const uint64_t *acc_w, const int32_t *carry,
                                     const uint64_t *acc_w2, int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream);
int brief_view_composite_part_fold_host(const brief_view_desc *view, const brief_view_part *part, const int32_t *k0, const int64_t *off,
                                        const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                                        int32_t *hits_w, int32_t *tau_w, uint64_t *acc_w);
int brief_view_composite_part_carry_host(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                         const int32_t *k0, const int32_t *cnt, const int32_t *tau_w, int32_t *carry, int32_t *cnt2);
int brief_view_composite_part_gather_host(const brief_view_desc *view, const brief_composite_window *wins, int32_t blocks, int64_t window_rays,
                                          const int32_t *hits_w, const int32_t *tau_w, const uint64_t *acc_w, const int32_t *carry,
                                          const uint64_t *acc_w2, int32_t *hits, int32_t *tau_run, uint64_t *acc);

/* ---- shaded composite: every sample's emission lit by the net's analytic gradient (csrc/brief_composite.inc, .h) ---------------------
 * Opacity is not touched: tau, the prefix P_i, hits, tau_run and the image's A are the plain composite's, bit for bit.  The emission of
 * a sample is scaled by a two-sided Lambert term in Q8 (csrc/brief_composite.h has the arithmetic, every fp32 operation rounded on its
 * own): g_a = jac[.][channel][a] * gscale[a], c_q = round(256 * |g . light| / |g|) (256 where |g| is 0 or not finite),
 * s_q = min(256, ka_q + ((kd_q * c_q + 128) >> 8)), e'_c = (e_c * s_q + 128) >> 8, acc_c += W(P_i) * e'_c.
 * A sample NEEDS a gradient iff it is inside the clip box, its table row has eR | eG | eB != 0 and P_i < TAU_SAT; every other sample
 * contributes 0 whatever its shade, so the Jacobian is evaluated on the needed samples alone.  Per chunk of the list, after
 * brief_view_coords and the integer forward:
 *   brief_view_composite_select      brief_view_composite_fold's walk, lookup and scan, with the ray's carry read from tau_run[r]; it
 *                                    writes nothing to the pixel state, only need[s - s0] (int32 0 | 1) for every sample of the chunk;
 *   (caller)                         slot (int64) = the exclusive scan of need, m = its total (one host read); m == 0: the chunk lights
 *                                    nothing, fold it with brief_view_composite_fold;
 *   brief_view_composite_pick        coords_sel[slot[i]] = coords[i] where need[i], i < n: the needed samples in the list's order (an
 *                                    entry whose slot lies outside 0 .. n - 1 is skipped);
 *   (caller)                         jac[m][channels][3] = brief_siren_jac_forward on coords_sel[0 .. m), value NULL;
 *   brief_view_composite_shade_fold  brief_view_composite_fold with the lit emission: the same walk, scan, butterfly and single plain
 *                                    read-modify-write of hits, tau_run and acc by the pixel's owner, no atomics.  A lane reads jac only
 *                                    where need is 1, at row slot[s - s0]; slot == NULL is the identity (a dense jac, one row per
 *                                    sample of the chunk).
 * The finish is brief_view_composite_finish.  need reads integers only: the selection, like the image, does not depend on chunking,
 * `lanes` or the run.  ka_q = 256, kd_q = 0 is the plain composite.  Every device entry only enqueues on `stream`.
 * brief_view_composite_shade_host is select, shade_fold and finish on the host CPU, without any GPU call: every buffer is host memory,
 * off[0] is 0, vals and the dense jac [off[rays]][channels][3] hold the whole list; need (int32 [off[rays]]), hits, tau_run and acc may
 * be NULL.  brief_composite_shade_q_host gives s_q[i] of the rows jac[i][3], i < n.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of brief_view_composite_fold; no null buffer
 * (slot of the fold excepted); n >= 1; ka_q and kd_q 0 .. 256; gscale and light finite. */
typedef struct {
    float gscale[3];                         /* grey levels per physical unit and coordinate unit, per axis (z, y, x) */
    float light[3];                          /* the unit direction the light travels, physical (z, y, x) */
    int32_t ka_q, kd_q;                      /* round(256 * KA), round(256 * KD): 0 .. 256 */
} brief_composite_shade;
int brief_view_composite_select(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                                int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits,
                                const int32_t *tau_run, int32_t *need, void *stream);
int brief_view_composite_pick(const int32_t *need, const int64_t *slot, const float *coords, int64_t n, float *coords_sel, void *stream);
int brief_view_composite_shade_fold(const brief_view_desc *view, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0,
                                    int64_t r1, int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel,
                                    const int32_t *tf, int32_t tf_bits, const int32_t *need, const int64_t *slot, const float *jac,
                                    const brief_composite_shade *shade, int32_t *hits, int32_t *tau_run, uint64_t *acc, void *stream);
int brief_view_composite_shade_host(const brief_view_desc *view, const int32_t *k0, const int64_t *off, const void *vals, int elem_kind,
                                    int32_t channels, int32_t channel, const int32_t *tf, int32_t tf_bits, const int32_t *background,
                                    const float *jac, const brief_composite_shade *shade, int32_t *need, int32_t *hits, int32_t *tau_run,
                                    uint64_t *acc, uint8_t *out);
int brief_composite_shade_q_host(const float *jac, int64_t n, const brief_composite_shade *shade, int32_t *s_q);

/* ---- Hessian decode of an fp32 SIREN (csrc/brief_hess.inc) ------------------------------------------------------------------------
 * value[n][cout] and jac[n][cout][cin] as brief_siren_jac_forward gives them, and hess[n][cout][nh] = d2 phi_c / d x_a d x_b (x_n), the
 * analytic second derivatives with respect to the coordinates in coordinate units; with output_act, of the activated output.  nh = 6 in
 * the order (00, 01, 02, 11, 12, 22) over the axes in coordinate order for cin = 3, nh = 3 in the order (00, 01, 11) for cin = 2 (the
 * Hessian is symmetric: only the upper triangle is stored).  Forward mode of second order on the matrix pipe: the value, its tangents and
 * its second derivatives travel through the layers together, a 10-column slot (cin = 3: 3 samples per 32-column MFMA tile) or a
 * 6-column slot (cin = 2: 5 samples) per sample.  All outputs are float32; value and jac may be NULL, hess may not.  `packed` is the
 * Jacobian decode's fragment buffer (brief_siren_jac_packed_count floats, written by brief_siren_jac_repack: call it after every change
 * of the parameters).  Sample sources, box rules, refusals and the envelope are those of brief_siren_jac_forward / _forward_box
 * (precision BRIEF_PREC_F32, features 1 .. 1024, layers >= 2, cin 2 | 3, cout 1 .. 4, packed and hess not NULL, n >= 1); the messages
 * name the limit.  Enqueue-only on `stream`: no allocation, no synchronisation.  The result is deterministic, and a sample's result does
 * not depend on its slot in a tile, on its neighbours or on how a box is cut into calls. */
int brief_siren_hess_forward(const brief_siren_desc *d, const float *packed, const brief_grid_desc *grid, const brief_batch_desc *batch,
                             float *value /* [n][cout] or NULL */, float *jac /* [n][cout][cin] or NULL */, float *hess /* [n][cout][nh] */,
                             void *stream);
int brief_siren_hess_forward_box(const brief_siren_desc *d, const float *packed, const brief_grid_box *box, int64_t offset, int64_t n,
                                 float *value, float *jac, float *hess, void *stream);

/* ---- ray view: a view whose rays come from a table, e.g. a perspective camera (csrc/brief_rays.inc, csrc/brief_rays.h) -------------
 * A ray view is rows x cols rays with `depth` samples each.  Ray r = row * cols + col is six floats of a DEVICE table,
 * rays[r] = (base_z, base_y, base_x, dd_z, dd_y, dd_x), in voxel-index units of the fitted grid `dims`: the orthographic view's
 * arithmetic with a foot and a step per ray, so the bundle may fan out from a point.
 *     position    p_a(r, k) = fl(base_a[r] + fl((float)k * dd_a[r]))                                (fp32, nothing contracted)
 *     real depth  p_a(r, t) = fl(base_a[r] + fl(t * dd_a[r]))
 *     inside, coordinate: the view entries' rules on the descriptor's clip box, dims and lo / hi.
 * A table filled from an orthographic view (base = its sample (row, col, 0), dd = its ddepth) reproduces that view bit for bit.
 *   brief_rays_clip            k0[r], cnt[r]: the inside samples of ray r are exactly k0 <= k < k0 + cnt (every p_a is monotone in k
 *                              along a ray, whatever its direction: one interval, found by bisection on the ray's own position; a
 *                              zero step component is legal).  0 <= k0 <= k0 + cnt <= depth whatever the table holds, NaN included;
 *   (caller)                   off = exclusive scan of cnt, the compacted ray-major sample list, as for brief_view_coords;
 *   brief_rays_coords          coords[s - s0][3] for the samples s0 <= s < s1 of the list;
 *   (caller)                   vals[s - s0][channels] = the forward entry on coords, out_kind BRIEF_OUT_U8 | BRIEF_OUT_U16;
 *   brief_rays_fold            brief_view_fold's fold for BRIEF_VIEW_MAX / _MIN / _MEAN (_SLICE is refused), GEOMETRY-FREE: the list of
 *                              brief_rays_clip is exact, so no sample is tested again, the table is not read, and hits[r] grows by the
 *                              samples of [s0, s1) that belong to ray r.  hits and acc as brief_view_fold's; the finish is
 *                              brief_view_finish;
 *   brief_rays_surface_fold    brief_surface_fold's first-hit fold over the same walk, likewise geometry-free; the bracket and the step
 *                              are brief_surface_bracket / brief_surface_step;
 *   brief_rays_surface_coords  brief_surface_coords' rule (dense, midpoint or t_hi, box_lo and NaN without a hit) at the ray's real depth;
 *   brief_rays_surface_shade   brief_surface_shade's arithmetic with a light per ray: light is a DEVICE table [rays][3] of unit
 *                              directions the light travels (a point light at a camera's eye: the rays' own directions); gscale
 *                              stays a HOST pointer to three floats.
 * brief_view_finish, brief_surface_bracket and brief_surface_step read rows x cols of their descriptor only: call them with a
 * brief_view_desc that carries the ray view's dims, lo / hi, box, rows, cols and depth, with origin and steps zero.
 * The walk (`lanes`, [r0, r1), one owner per pixel, no atomics, integer folds: exact, independent of chunking, `lanes` and the run)
 * is the view entries'.  Every device entry only enqueues on `stream`.  The device table is trusted: a bad one may give a wrong
 * image, never an access outside a buffer or an unbounded loop.
 * brief_rays_sample_host / _sample_t_host / _clip_host evaluate the same header on the host CPU without any GPU call: every buffer,
 * the table included, is host memory, and a table entry that is not finite is refused.
 * Limits (BRIEF_ERR_INVALID with a message naming the limit, before any launch): those of the view and surface entries (rows, cols,
 * depth 1 .. 2^24 - 1; dims 2 .. 2^31 - 1; lo / hi and the box finite, 0 <= box_lo <= box_hi <= dims - 1; at most 2^40 rays; lanes a
 * power of two 1 .. 64; channels 1 .. 4; no null buffer, pos of brief_rays_surface_coords excepted). */
typedef struct {
    int64_t dims[3];
    float lo, hi;                            /* coordinate range of the fitted grid */
    int32_t rows, cols, depth, reserved;
    float box_lo[3], box_hi[3];              /* inclusive clip box */
} brief_rays_desc;
int brief_rays_clip(const brief_rays_desc *desc, const float *rays, int32_t *k0, int32_t *cnt, void *stream);
int brief_rays_coords(const brief_rays_desc *desc, const float *rays, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0,
                      int64_t r1, int32_t lanes, float *coords, void *stream);
int brief_rays_fold(const brief_rays_desc *desc, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                    int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t mode, int32_t *hits, void *acc, void *stream);
int brief_rays_surface_fold(const brief_rays_desc *desc, const int32_t *k0, const int64_t *off, int64_t s0, int64_t s1, int64_t r0, int64_t r1,
                            int32_t lanes, const void *vals, int elem_kind, int32_t channels, int32_t channel, int32_t level, int32_t side,
                            int32_t *hits, int32_t *first, void *stream);
int brief_rays_surface_coords(const brief_rays_desc *desc, const float *rays, const float *t_lo, const float *t_hi, int32_t midpoint, float *coords,
                              float *pos, void *stream);
int brief_rays_surface_shade(const brief_rays_desc *desc, const float *t, const float *jac, int32_t channels, int32_t channel, int32_t side,
                             const float *gscale, const float *light, float *normal, float *shade, void *stream);
int brief_rays_sample_host(const brief_rays_desc *desc, const float *rays, const int32_t *row, const int32_t *col, const int32_t *k, int64_t n,
                           float *pos, float *coord, uint8_t *inside);
int brief_rays_sample_t_host(const brief_rays_desc *desc, const float *rays, const int32_t *row, const int32_t *col, const float *t, int64_t n,
                             float *pos, float *coord, uint8_t *inside);
int brief_rays_clip_host(const brief_rays_desc *desc, const float *rays, int32_t *k0, int32_t *cnt);

#ifdef __cplusplus
}
#endif
#endif
