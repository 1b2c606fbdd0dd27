/* mvsdf_hip.h -- C ABI of libmvsdf_hip.so, the MI355X (gfx950) native hot path of MVSDF.
 *
 * The reference (jzhangbs/MVSDF) has no FFI for this path: it is eager PyTorch behind nn.Module classes
 * (SURVEY.md section 8b).  Each entry point below replaces the PyTorch op sequence of the cited reference
 * lines; the Python mirror (mvsdf_amd/model/...) binds them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: all pointers are DEVICE pointers unless marked host; tensors are dense row-major fp32;
 * masks are uint8 (0/1); `stream` is a hipStream_t passed as void*; every call is asynchronous on that
 * stream and returns 0 on success or a nonzero code (hipError_t value, or negative for bad arguments);
 * mvsdf_last_error() gives a message.  No call allocates or synchronises.
 *
 * What this boundary REFUSES (the call returns a negative code and mvsdf_last_error() names the reason; the Python mirror raises
 * NotImplementedError / ValueError before it gets here) -- every other constructor option of the reference's three modules is accepted:
 *      (a skip connection into the LAST Linear of the SDF network, `skip_in` containing num_layers - 2 (idr.py:46-49,86), is accepted since round 5:
 *      u_L = W_L[0, :] splits like any skip layer's adjoint, its PE columns start the PE adjoint of the normal chain)
 *   1. `d_in != 3` for ImplicitNetwork (idr.py:22,34): points are 3-vectors everywhere on this path (camera rays, PE of 3 + 6 * multires columns).
 *   2. hidden widths above 512 (column tiles per wave of the fused engines: 2 up to 256, 4 up to 512), and more than MVSDF_MAX_LAYERS = 12 Linears.
 *   3. quaternion poses in get_camera_params (rend_util.py:49-54: the `pose.shape[1] == 7` branch): the reference switches it off
 *      (exp_runner.py:40 train_cameras = False; scene_dataset.py hands 4 x 4 matrices); mvsdf_camera_rays takes pose[B][4][4] only.
 */
#ifndef MVSDF_HIP_H
#define MVSDF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVSDF_MAX_LAYERS 12

/* A weight-norm-folded MLP in MFMA-packed form (see mvsdf_fold_pack).  host struct, device pointers. */
typedef struct {
    int n_layers;
    int K[MVSDF_MAX_LAYERS];            /* in features per Linear */
    int N[MVSDF_MAX_LAYERS];            /* out features per Linear */
    const float* wp[MVSDF_MAX_LAYERS];  /* packed weights, mvsdf_packed_floats(N, K) floats */
    const float* bias[MVSDF_MAX_LAYERS]; /* [N] floats.  trace_dtype 3 / 4 / 5 read each vector with 16-byte loads up to the next multiple of 16 entries (the
                                         * entries past N are loaded and never used): the buffer must be READABLE that far.  Every hipMalloc'd or torch-allocated
                                         * buffer is (allocation granularity >= 64 bytes); a caller that carves biases out of its own arena pads each vector to a
                                         * multiple of 16 floats (a vector that ends exactly at the end of a mapped range would fault otherwise) */
    const float* w[MVSDF_MAX_LAYERS];   /* folded weights, row-major [N][K] (only the last layer's row 0 is read: u_L = W_L[0,:]); may be NULL when no normals are needed */
    int skip_layer;                     /* layer whose input is cat([x, PE(x)])/sqrt(2) (idr.py:86-87), -1 if none (see skip_mask for several) */
    int multires;                       /* positional-encoding frequencies (embedder.py:38-50) */
    const void* wp16[MVSDF_MAX_LAYERS]; /* trace_dtype 2: fp32 packs of the rounded weights
                                         * (mvsdf_pack_bf16w_net); 3 / 4: bf16 packs made by mvsdf_pack_bf16s_net; 5: three-term packs made by mvsdf_pack_bf16x3_net;
                                         * NULL for trace_dtype 0 */
    int trace_dtype;                    /* arithmetic of the no-grad tracing MLP (mvsdf_trace, mvsdf_sdf_col0): 0 = fp32 weights and fp32-input
                                         * MFMA (bit-exact against the fmaf-chain oracle), 1 = REMOVED in round 5 (bf16 weights AND 8-bit activations: every entry point refuses it),
                                         * 2 = bf16-ROUNDED WEIGHTS ONLY: wp16[l] holds an fp32 pack (mvsdf_packed_floats(N, K) floats, made by
                                         * mvsdf_pack_bf16w_net) of the weights rounded to bf16, activations stay fp32 on the fp32-input MFMA -- bit-exact
                                         * against the oracle run on the rounded weights,
                                         * 3 / 4 = bf16 weights on the bf16 MFMA with every activation carried as 2 / 3 bf16 TERMS (a = t0 + t1 [+ t2], 16 / all 24
                                         * mantissa bits; csrc/tile_engine_bf16s.h): the arithmetic of mode 2 (idr.py:77-94 on bf16-rounded weights) up to the order
                                         * of the fp32 additions inside the matrix core -- the fast mode that is parity-checked against that oracle (hit masks
                                         * equal except at recorded ties, depths 1e-4).  bias[] is read with 16-byte loads up to the next multiple of 16 entries,
                                         * 5 = the fp32 weights UNROUNDED as three bf16 terms too (w = w0 + w1 + w2 exactly): the reference's fp32 Linear
                                         * (idr.py:89) from the six exact products a_s w_j, s + j <= 2, on the bf16 MFMA -- fp32-accurate (measured closer to an
                                         * fp64 evaluation than mode 0's fmaf chain) and reproduced BIT FOR BIT by the oracle's model of the matrix instruction
                                         * (oracle_mvsdf.c::sdf_row_f32x3); det_math's softplus like mode 0; values below 2^-40 count as zero.  Not bit-identical
                                         * to mode 0 (another summation order).  bias[] is read like in modes 3 / 4 */
    unsigned skip_mask;                 /* several skip connections (skip_in with more than one entry, idr.py:46,86): bit l set = the input of layer l
                                         * is cat([x, PE(x)])/sqrt(2).  0 = use skip_layer alone.  Any layer but layer 0 (the last Linear included). */
    const void* wx3[MVSDF_MAX_LAYERS];  /* optional: three-term bf16 packs of THIS descriptor's matrices (mvsdf_pack_bf16x3_net for W_l; mvsdf_pack_bf16x3t_net for the
                                         * transposed descriptor's W_l^T).  When every layer of both descriptors has one, the differentiable passes of the SDF network
                                         * (mvsdf_sdf_forward / _backward / _backward_pair, the training step) run their fused chains in the three-term fp32 arithmetic
                                         * on the bf16 matrix cores (csrc/chain_x3.h) instead of the fp32-input MFMA chains; NULL: the fp32 chains.  bias[] is then read
                                         * like in trace_dtype 3 / 4 / 5 */
} MvsdfNetDesc;

/* RayTracing constructor arguments (ray_tracing.py:7-25) + the hard-coded dist_clip (ray_tracing.py:127-131). */
typedef struct {
    float r;                 /* object_bounding_sphere */
    float thr;               /* sdf_threshold */
    float line_search_step;
    int line_step_iters;
    int st_iters;            /* sphere_tracing_iters */
    int n_steps;
    int n_secant;            /* n_secant_steps */
    float dist_clip;         /* 0.5 (0.05 in IDR_RENDER mode) */
} MvsdfTraceParams;

/* indices into the uint64 counters[16] array filled by mvsdf_trace (device memory) */
enum {
    MVSDF_CNT_ROWS_SPHERE = 0,  /* sdf() rows evaluated by sphere_tracing   (ray_tracing.py:134,137,168,171,185,186) */
    MVSDF_CNT_ROWS_SAMPLER = 1, /* ... by ray_sampler                       (ray_tracing.py:218) */
    MVSDF_CNT_ROWS_SECANT = 2,  /* ... by secant                            (ray_tracing.py:266) */
    MVSDF_CNT_ROWS_MINSDF = 3,  /* ... by minimal_sdf_points                (ray_tracing.py:301) */
    MVSDF_CNT_N_SECANT = 4,     /* rays that ran the secant */
    MVSDF_CNT_N_SAMPLER = 5,    /* rays on the sampler work list */
    MVSDF_CNT_N_MINSDF = 6,     /* rays on the min-sdf work list */
    MVSDF_CNT_N_SAMPLER_REST = 7,    /* sampler rays whose first sample window did not settle them (no sign change yet) */
    MVSDF_CNT_ROWS_SAMPLER_EVAL = 8, /* ray_sampler rows actually evaluated here: the samples AFTER a ray's first sign change cannot
                                      * influence any output (ray_tracing.py:221-256 reads only sdf_val[ind-1], sdf_val[ind]) and are
                                      * skipped.  counters[1] keeps the reference's count (n_rays * n_steps). */
    /* tail filling of the sphere-tracing kernel (training): the min-sdf rows are a queue that finished sphere-tracing workgroups serve until
     * the slowest one is done, the min-sdf launch takes the rest */
    MVSDF_CNT_TAIL_NEXT = 9,    /* next unit of min-sdf rows to hand out */
    MVSDF_CNT_TAIL_READY = 10,  /* min-sdf list items completely written */
    MVSDF_CNT_TAIL_WGS = 11,    /* sphere-tracing workgroups whose rays are done */
    MVSDF_CNT_TAIL_ROWS = 12,   /* min-sdf rows evaluated inside the sphere-tracing kernel (a subset of counters[3]) */
    /* the sphere cut (mvsdf_trace_cut_stage): the sphere launch stops after a round limit, a resume launch finishes the rays that were not done */
    MVSDF_CNT_N_SPILL = 13,         /* rays the limited launch handed to the resume launch */
    MVSDF_CNT_N_SAMPLER_LATE = 14,  /* sampler rays the resume launch listed (their own list; counters[5] counts the first list only) */
    MVSDF_CNT_LATE_ROUNDS = 15      /* evaluations the slowest workgroup of the resume launch still ran */
};

int mvsdf_version(void);
/* sizeof() of the structs of this header as the library was compiled, in the order MvsdfNetDesc, MvsdfTraceParams, MvsdfStepDesc, MvsdfStepParams,
 * MvsdfStepInputs, MvsdfStepLayout, MvsdfLossArgs, MvsdfLossLayout -> out[8]; a binding checks its own struct definitions against it
 * (tests/test_abi.py does for the ctypes binding).  Returns 8. */
int mvsdf_abi_struct_sizes(size_t* out);
const char* mvsdf_last_error(void);

/* number of floats of the packed form of an [N][K] Linear (both dims rounded up to 16) */
size_t mvsdf_packed_floats(int N, int K);

/* weight_norm fold  w = v * (g / ||v||_row)  (idr.py:70-71, torch._weight_norm dim=0) + MFMA packing.
 * v[N][K], g[N] -> w[N][K] (row-major, required), wp (packed W, mvsdf_packed_floats(N, K) floats, may be NULL),
 * wpT (packed W^T for contractions over the OUT dimension, mvsdf_packed_floats(K, N) floats, may be NULL). */
int mvsdf_fold_pack(const float* v, const float* g, int N, int K, float* w, float* wp, float* wpT, void* stream);
/* all layers of a network -- or of several networks, up to 24 layers in total -- at once (one fold launch + one pack launch).  g[l] may be
 * NULL for a layer without weight norm (weight_norm=False, idr.py:70-71 skipped): w = v, and the backward gives dv = dW, no dg.  The
 * pointer arrays are HOST arrays of n_layers device pointers; wp[l] / wpT[l] may be NULL. */
int mvsdf_fold_pack_net(int n_layers, const float* const* v, const float* const* g, const int* N, const int* K, float* const* w,
                        float* const* wp, float* const* wpT, void* stream);
/* backward of every fold in one launch.  db / dbias (both NULL or both given; entries may be NULL pairwise) route the bias
 * gradients db[l][N_l] to dbias[l] in the same launch; accumulate != 0 adds into dv / dg / dbias (the targets may be the
 * parameters' .grad buffers: what autograd's AccumulateGrad would do with ~3 launches per layer). */
int mvsdf_fold_backward_net(int n_layers, const float* const* v, const float* const* g, const float* const* dW, const float* const* db,
                            const int* N, const int* K, float* const* dv, float* const* dg, float* const* dbias, int accumulate,
                            void* stream);
/* backward of the fold: dW[N][K] -> dv[N][K], dg[N]    */
int mvsdf_fold_backward(const float* v, const float* g, const float* dW, int N, int K, float* dv, float* dg, void* stream);

/* bytes of one layer's bf16 pack in the layout of v_mfma_f32_16x16x32_bf16 (wp16[l] of trace_dtype 3 / 4; three times that for trace_dtype 5) */
size_t mvsdf_packed_bf16_bytes(int N, int K);
/* trace_dtype = 2: fp32 MFMA packs (layout of mvsdf_fold_pack's wp) of the folded weights w[l] rounded to bf16 (nearest even) */
int mvsdf_pack_bf16w_net(int n_layers, const float* const* w, const int* N, const int* K, float* const* wp_rounded, void* stream);
/* trace_dtype = 3 / 4: bf16 packs (v_mfma_f32_16x16x32_bf16 B-operand layout) WITHOUT duplicated columns (the positional-encoding inputs are split into bf16 terms like
 * every other activation); wp16[l]: mvsdf_packed_bf16_bytes(N, K) bytes.  idr.py:77-94 on bf16-rounded weights. */
int mvsdf_pack_bf16s_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wp16, void* stream);
/* trace_dtype = 5: the folded fp32 weights as three bf16 terms (t0 = bf16(w), t1 = bf16(w - t0), t2 = bf16(w - t0 - t1)), layout of mvsdf_pack_bf16s_net
 * with a k-block's three term fragments behind each other; wp16[l]: 3 * mvsdf_packed_bf16_bytes(N, K) bytes.  idr.py:77-94 on the fp32 weights.
 * The weights must be finite with |w| <= 0x7f7f7fff as a bit pattern (the largest float whose bf16 rounding stays finite); |w| < 2^-40 packs as +0. */
int mvsdf_pack_bf16x3_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wp16, void* stream);
/* the same three-term pack of W_l^T (N, K are W_l's dims): 3 * mvsdf_packed_bf16_bytes(K, N) bytes per layer -- MvsdfNetDesc.wx3 of the transposed descriptor */
int mvsdf_pack_bf16x3t_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wx3t, void* stream);

/* ImplicitNetwork.forward(x)[:, 0] (idr.py:77-94) for n points: the tracing MLP alone. */
int mvsdf_sdf_col0(const MvsdfNetDesc* net, const float* x, int n, float* y, int mt, void* stream);

/* rend_util.get_camera_params + lift, pose-matrix branch (rend_util.py:48-75, 87-100):
 * uv[B][P][2], pose[B][4][4], intrinsics[B][4][4] -> ray_dirs[B][P][3], cam_loc[B][3]. */
int mvsdf_camera_rays(const float* uv, const float* pose, const float* intrinsics, int B, int P, float* ray_dirs, float* cam_loc,
                      void* stream);

/* rend_util.get_sphere_intersection (rend_util.py:141-162): -> t[B*P][2] (near, far; clamped at 0), mask[B*P] (disc > 0). */
int mvsdf_sphere_intersection(const float* cam_loc, const float* ray_dirs, int B, int P, float r, float* t, uint8_t* mask, void* stream);

/* RayTracing.forward (ray_tracing.py:27-98) with the SDF given by `net`:
 * cam_loc[B][3], ray_dirs[B][P][3], object_mask[B*P] -> points[B*P][3], mask[B*P], dists[B*P].
 * intervals[n_steps] = torch.linspace(0, 1, n_steps) (ray_tracing.py:206); minsdf_steps[n_steps] = the uniform draws
 * of minimal_sdf_points (ray_tracing.py:287), used only when training != 0.
 * counters: uint64[16], zeroed by the call.  workspace: mvsdf_trace_workspace_bytes(B*P) bytes (n_steps <= 128) or
 * mvsdf_trace_workspace_bytes_n(B*P, n_steps).
 * mt: row tiles (16 rows) per workgroup of the sphere-tracing kernel (8*mt rays), 1..4;
 * mt_samples: row tiles per chunk of the flattened sample-row kernels (sampler / min-sdf), 1..4. */
size_t mvsdf_trace_workspace_bytes(int R);   /* = mvsdf_trace_workspace_bytes_n(R, 128) */
size_t mvsdf_trace_workspace_bytes_n(int R, int n_steps);
int mvsdf_trace(const MvsdfNetDesc* net, const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs,
                const uint8_t* object_mask, int B, int P, int training, const float* intervals, const float* minsdf_steps,
                float* points, uint8_t* mask, float* dists, unsigned long long* counters, void* workspace,
                size_t workspace_bytes, int mt, int mt_samples, void* stream);
/* the launches of mvsdf_trace separately, same arguments and workspace.  stage 1: sphere tracing (zeroes the counters);
 * stage 2: ray sampler + secant + min-sdf; or stage 3: ray sampler rows only -- `mask` is FINAL after it (ray_tracing.py:61) --
 * followed by stage 4: secant + min-sdf (only points / dists still change, ray_tracing.py:63-96); stage 4 may be split further into
 * stage 5: min-sdf rows + their reduction alone (independent of stage 3: they only need stage 1's work list, and use their own sample-value
 * buffer, so a caller may run them on another stream concurrently with stage 3) and stage 6: secant alone.  Lets a caller bracket each
 * kernel with events, and fetch the hit count to the host while stage 4 still runs.
 * stage 7: secant alone like stage 6, in the sphere tracer's engine form where the engine has one for these latency chains (the three-weight-term engine up to
 * hidden width 256: sixteen waves x one column tile, k_secant_chains); the stage-6 instance everywhere else.  Same results as stage 6, bit for bit. */
int mvsdf_trace_stage(int stage, const MvsdfNetDesc* net, const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs,
                      const uint8_t* object_mask, int B, int P, int training, const float* intervals, const float* minsdf_steps,
                      float* points, uint8_t* mask, float* dists, unsigned long long* counters, void* workspace,
                      size_t workspace_bytes, int mt, int mt_samples, void* stream);

/* The sphere cut: stage 1 of mvsdf_trace_stage as two launches, for a caller with a second stream.  Most rays are final after st_iters + 1 dependent evaluations;
 * stage 1 here stops every workgroup after max_rounds of them (<= 0: st_iters + 1), finalises its finished rays as usual and appends the complete state of the
 * others to a spill list.  Stage 2 is the resume launch: the same kernel over the spilled rays, eight * mt per workgroup, to the end; its sampler rays go on a
 * late list of their own.  Stage 3 evaluates the late list's sample rows (all n_steps in one pass) and reduces them.  Stages 2 and 3 touch nothing that
 * mvsdf_trace_stage 3 (the sampler rows of the first list) reads or writes except atomic appends to the secant list, so the two may run concurrently; behind both,
 * mvsdf_trace_stage 4 / 6 / 7 finds one secant list and mvsdf_trace_stage 4 / 5 one min-sdf list.  No launch uses tail filling.  Results are those of mvsdf_trace bit for
 * bit; list orders and counters[8] (the late rays take one pass) may differ, counters[13..15] report the cut.  Same arguments as mvsdf_trace_stage; the workspace is
 * mvsdf_trace_cut_workspace_bytes(B*P, n_steps) bytes for ALL launches of such a sequence: the regions of mvsdf_trace, then the spill list, the late list and its sample
 * values (late list: int32[R] at byte offset al256(44 R + 8 R n_steps + 256) + 64 R). */
size_t mvsdf_trace_cut_workspace_bytes(int R, int n_steps);
int mvsdf_trace_cut_stage(int stage, int max_rounds, const MvsdfNetDesc* net, const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs,
                          const uint8_t* object_mask, int B, int P, int training, const float* intervals, const float* minsdf_steps, float* points, uint8_t* mask,
                          float* dists, unsigned long long* counters, void* workspace, size_t workspace_bytes, int mt, int mt_samples, void* stream);
/* The sample rows of such a sequence in the sixteen-wave form (k_row_chunks: sixteen waves x one column tile over the two row tiles of a chunk, the sphere tracer's
 * carried weight ring and ping-pong tiles; one workgroup per compute unit at most, each taking every grid-th chunk) -- for launches of about one chunk per compute unit,
 * which are one dependent evaluation.  part 1: mvsdf_trace_stage 3 with the FIRST sampler window in that form (the rest of the samples keeps its launch); part 2:
 * mvsdf_trace_cut_stage 3 with the late list's rows in that form.  rows16 == 0: exactly the launches of those stages.  grid_cap > 0: at most that many workgroups
 * (tests: the stride loop at small sizes).  The form exists for the three-weight-term engine (trace_dtype 5) up to hidden width 256 with mt_samples >= 2; -3 elsewhere.
 * Same values as the stages it stands for, bit for bit. */
int mvsdf_trace_rows_stage(int part, int rows16, int grid_cap, const MvsdfNetDesc* net, const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs,
                           const uint8_t* object_mask, int B, int P, int training, const float* intervals, const float* minsdf_steps, float* points, uint8_t* mask,
                           float* dists, unsigned long long* counters, void* workspace, size_t workspace_bytes, int mt, int mt_samples, void* stream);

/* ---- RayTracing.forward for an OPAQUE `sdf` callable (ray_tracing.py:27-32, called with a lambda at idr.py:194) ----
 * The per-ray state machine of mvsdf_trace split at its evaluation points, so that a host-side callable can be run between the launches:
 *   init   : sphere intersection + first requests.  state: mvsdf_tracegen_state_bytes(R) bytes; req[R][2] (uint8: start / end side wants a
 *            value), pts[R][2][3] (the requested points, dense); zeroes counters[16].
 *   step   : consumes vals[R][2] (the callable's values at the requested entries, anything elsewhere), advances every ray by one round
 *            (ray_tracing.py:139-194) and emits the next requests.  The caller loops until no entry of req is set.
 *   finish : masks / dists / points of the sphere-tracing stage, sampler and min-sdf work lists IN RAY ORDER (counters[MVSDF_CNT_N_SAMPLER],
 *            [MVSDF_CNT_N_MINSDF]); workspace as for mvsdf_trace.
 *   rows   : the n_steps sample points of each listed ray (kind 0: ray_sampler with `zs` = intervals, ray_tracing.py:206-213; kind 1:
 *            minimal_sdf_points with `zs` = the uniform draws, 287-297) -> out_pts[n_list * n_steps][3].
 *   reduce : the per-ray decisions on the callable's values sv[n_list][n_steps] (kind 0: ray_tracing.py:221-256, fills the secant list sorted
 *            by ray, marks[R] is scratch; kind 1: 303-307).
 *   secant : op 0 emits the n_sec points of one secant round -> pts_out[n_sec][3]; op 1 consumes vals[n_sec]; op 2 writes the final result. */
size_t mvsdf_tracegen_state_bytes(int R);
int mvsdf_tracegen_init(const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs, const uint8_t* object_mask, int B, int P,
                        void* state, uint8_t* req, float* pts, unsigned long long* counters, void* stream);
int mvsdf_tracegen_step(const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs, int B, int P, void* state, const float* vals,
                        uint8_t* req, float* pts, unsigned long long* counters, void* stream);
int mvsdf_tracegen_finish(const MvsdfTraceParams* tp, const float* cam_loc, const float* ray_dirs, int B, int P, int training, const void* state,
                          float* points, uint8_t* mask, float* dists, unsigned long long* counters, void* workspace, size_t workspace_bytes,
                          void* stream);
int mvsdf_tracegen_rows(const MvsdfTraceParams* tp, int kind, const float* cam_loc, const float* ray_dirs, int B, int P, const float* zs, int n_list,
                        void* workspace, float* out_pts, void* stream);
int mvsdf_tracegen_reduce(const MvsdfTraceParams* tp, int kind, const float* cam_loc, const float* ray_dirs, int B, int P, int training,
                          const float* intervals, const float* minsdf_steps, const float* sv, float* points, uint8_t* mask, float* dists,
                          unsigned long long* counters, void* workspace, uint8_t* marks, void* stream);
int mvsdf_tracegen_secant(const MvsdfTraceParams* tp, int op, const float* cam_loc, const float* ray_dirs, int B, int P, int n_sec, const float* vals,
                          float* pts_out, float* points, float* dists, unsigned long long* counters, void* workspace, void* stream);

/* ---- differentiable SDF network: value + normal and their first/second-order backward ----
 * Replaces ImplicitNetwork.forward / .gradient (idr.py:77-107) and autograd's (double) backward through them.
 * net: packs of W_l; netT: packs of W_l^T (K and N swapped per layer).  x[M][3].  The first Mg rows also get the normal
 * n = d out[:,0] / dx (NOT normalised, idr.py:327).  y[M][Nout], nrm[Mg][3].  ctx: mvsdf_sdf_ctx_floats(net, M, Mg) floats,
 * kept by the caller until the backward.  */
size_t mvsdf_sdf_ctx_floats(const MvsdfNetDesc* net, int M, int Mg);
int mvsdf_sdf_forward(const MvsdfNetDesc* net, const MvsdfNetDesc* netT, const float* x, int M, int Mg, float* y, float* nrm, float* ctx,
                      void* stream);
/* Backward over rows [row0, row0 + Mb) (inside [0, M); inside [0, Mg) when dn is given): dy[Mb][Nout], dn[Mb][3] or NULL ->
 * dW_cat (all layers, row-major [N][K], concatenated), db_cat (both NULL: input adjoint only), dx[Mb][3] or NULL.  ws: mvsdf_sdf_bwd_ws_floats(net, Mb) floats. */
size_t mvsdf_sdf_bwd_ws_floats(const MvsdfNetDesc* net, int Mb);
int mvsdf_sdf_backward(const MvsdfNetDesc* net, const MvsdfNetDesc* netT, const float* x, int M, int Mg, int row0, int Mb, const float* dy,
                       const float* dn, const float* ctx, float* dW_cat, float* db_cat, float* dx, float* ws, void* stream);

/* The training step's SDF backward in two chain launches instead of three sequential ones (functional._IdrStep.backward):
 *   pair   : pass A = full backward over rows [0, MbA) with (dyA[MbA][Nout], dnA[MbA][3]), per-layer adjoints kept in wsA
 *            (mvsdf_sdf_bwd_ws_floats(net, MbA)); pass X = input adjoint only over rows [row0X, row0X + MbX) with (dyX, dnX) -> dx[MbX][3]
 *            (scratch wsX).  Independent, ONE grid.  Returns -3 when the fused chain kernels do not cover the network (use mvsdf_sdf_backward).
 *   finish : delta pass over rows [row0D, row0D + MbD): extra upstream fbar[MbD] on output column 0 only (SampleNetwork's scalar, known
 *            after pass X), its first-order adjoints are ADDED to wsA's (linearity); dy must already include fbar in column 0 of those rows.
 *            Then the weight / bias gradients of every layer -> dW_cat, db_cat. */
int mvsdf_sdf_backward_pair(const MvsdfNetDesc* net, const MvsdfNetDesc* netT, int M, int Mg, int MbA, const float* dyA, const float* dnA, float* wsA,
                            int row0X, int MbX, const float* dyX, const float* dnX, float* wsX, float* dx, const float* ctx, void* stream);
int mvsdf_sdf_backward_finish(const MvsdfNetDesc* net, const MvsdfNetDesc* netT, int M, int Mg, int Mb, const float* dy, const float* ctx, float* ws,
                              int row0D, int MbD, const float* fbar, float* dW_cat, float* db_cat, void* stream);

/* ---- rendering network (idr.py:145-167): rgb = tanh(MLP(cat[points, PE(view), normals, feat])) ----
 * multires_view: low 8 bits = positional-encoding frequencies of the view direction (0: the raw direction); bit 8 (0x100) = mode 'no_view_dir'
 * (input cat[points, normals, feat]); bit 9 (0x200) = mode 'no_normal' (cat[points, PE(view), feat]); neither = mode 'idr'.  The unused input
 * pointer must still be valid device memory. */
size_t mvsdf_render_ctx_floats(const MvsdfNetDesc* net, int N);
size_t mvsdf_render_bwd_ws_floats(const MvsdfNetDesc* net, int N);
int mvsdf_render_forward(const MvsdfNetDesc* net, const float* points, const float* view, const float* normals, const float* feat,
                         int ldfeat, int N, int multires_view, float* rgb, float* ctx, void* stream);
/* din[N][K0]: adjoint of the concatenated input (points = [:,0:3], normals = [:,3+dv:6+dv], feat = [:,6+dv:], dv = 3+6*multires_view).
 * ctx was made by mvsdf_render_forward over Nctx >= N rows; the backward covers its first N rows (a training step renders every sorted
 * ray before the host knows how many of them hit). */
int mvsdf_render_backward(const MvsdfNetDesc* net, const MvsdfNetDesc* netT, int N, int Nctx, const float* drgb, const float* ctx,
                          float* dW_cat, float* db_cat, float* din, float* ws, void* stream);

/* The form of the weight gradients dW = P^T Q of every backward above and of the training step (process-wide, for the calls that follow):
 *   mode < 0 : by rule -- the three-term bf16 arithmetic (csrc/wgrad_x3.h) where the call's SDF descriptor carries the three-term packs (wx3), i.e. wherever
 *              the chains run in that arithmetic; the fp32-input matrix instruction (k_wgrad_net) elsewhere.  The default.
 *   mode 0 / 1 : the fp32 form / the three-term form for every call, whatever the descriptors carry.
 * Returns the mode that was set before.  mvsdf_wgrad_x3_stage_rows: rows of the contraction the three-term form stages at a time.
 * mvsdf_wgrad_uses_x3: 1 when a backward with this SDF descriptor forms its weight gradients in the three-term arithmetic now, else 0 -- a training step's one
 * launch covers the rendering layers too, so a caller that runs the step's passes one by one sets that form around its mvsdf_render_backward to get the step's bits. */
int mvsdf_set_wgrad_x3(int mode);
int mvsdf_wgrad_x3_stage_rows(void);
int mvsdf_wgrad_uses_x3(const MvsdfNetDesc* sdf);

/* ---- IDRLoss.get_feat_loss_corr (model/loss.py:115-165 + utils/my_utils.py:98-110,152-165 + F.grid_sample) ----
 * forward AND analytic d(loss)/d(points) in one launch (feature maps are constants).  pts[N][3] = diff_surf_pts (hit points,
 * view-major); view_start[B+1] (device int32) = prefix sums of per-view hit counts; feat[B][C][H][W], feat_src[B][V][C][H][W]
 * addressed through element strides (NCHW or channels_last, C <= 32); cam[B][2][4][4], src_cams[B][V][2][4][4], size[1],
 * center[3] on the device.  loss_pp[N]: per-point terms (their sum is the loss); dpts[N][3]. */
int mvsdf_feat_corr(const float* pts, int N, const int* view_start, int B, int V, int C, int H, int W, const float* feat,
                    const long long* feat_strides, const float* feat_src, const long long* src_strides, const float* cam,
                    const float* src_cams, const float* size, const float* center, float* loss_pp, float* dpts, void* stream);

/* ---- depth-carving target of IDRLoss.get_depth_loss (loss.py:37-63 -> my_utils.py:269-331 carving_t2) ----
 * pts[M][pts_ld] (first 3 columns: normalised sample points, e.g. eikonal_points_hom with pts_ld = 4), depths[B][h][w],
 * cams[B][2][4][4] -> dist_r[M], weight[M]; pts_world (may be NULL, may alias pts, same row stride) receives the points rescaled to
 * world coordinates -- the reference does that in place on eikonal_points_hom (loss.py:38,42);
 * loss = mean(|eikonal_output + dist_r| * weight)  (weight = far/near attenuation * in_range).
 * use_invalid != 0: carving_t (conf.use_invalid, loss.py:43-44 -> my_utils.py:204-266): a view that sees the point but has no depth there counts as half an
 * 'outside' vote, and `in_range` is "some view sees the point" instead of "some view has a depth there". */
int mvsdf_depth_carve(const float* pts, int pts_ld, int M, const float* depths, int B, int h, int w, const float* cams, const float* size,
                      const float* center, float out_thresh_perc, float far_thresh, float far_att, float near_thresh, float near_att, int use_invalid,
                      float* dist_r, float* weight, float* pts_world, void* stream);

/* ---- the elementwise terms of IDRLoss.forward + weighted total (loss.py:21-35, 58-61, 167-174, 206-210), one launch ----
 * rgb[R][3], rgb_gt[R][3], rgb_mask[R] (network_object_mask & object_mask); grad_theta[n_eik][3]; eik_out / dist_r / dweight[n_depth]
 * (dist_r, dweight from mvsdf_depth_carve); surf[n_surf] logits with targets (i < *n_pos); feat_pp[n_feat] from mvsdf_feat_corr or NULL.
 * smooth: 0 = the L1 depth term (loss.py:60), s > 0 = SmoothL1(eikonal_output / s, -dist_r / s) * s (loss.py:57-58).
 * out[6] = {loss, rgb_loss, eikonal_loss, depth_loss, feat_loss, surf_loss}; d_*: unit gradients of each term w.r.t. its input.
 * inv_counts (device, [3], may be NULL): replaces 1/n_eik, 1/n_depth, 1/n_surf of the three count-normalised means -- with
 * world_size / (count summed over the data-parallel ranks) the rank-averaged gradient equals the single-process one. */
int mvsdf_loss_terms(const float* rgb, const float* rgb_gt, const uint8_t* rgb_mask, int R, const float* grad_theta, int n_eik,
                     const float* eik_out, const float* dist_r, const float* dweight, int n_depth, const float* surf, int n_surf,
                     const long long* n_pos, const float* feat_pp, int n_feat, float w_rgb, float w_eik, float w_surf, float w_feat,
                     float w_depth, float smooth, int surf_on, int feat_on, const float* inv_counts, float* out, float* d_rgb, float* d_grad,
                     float* d_eik_out, float* d_surf, void* stream);

/* ---- bookkeeping of one training step of IDRNetwork.forward (idr.py:202-304) between the big kernels ----
 * mvsdf_partition_rays: stable partition of the R rays by surface = net_mask & object_mask (object_mask / true_mask may be NULL = all
 * ones): perm[R] = [surface rays in ray order | the others in ray order], inv[R] its inverse, true_rows[R] = ranks among the surface
 * rays of those inside true_mask (first counts[1] entries valid), counts[2] = {#surface, #surface & true}; view_sorted[R][3]
 * (may be NULL) = -ray_dirs[perm[r]].  Replaces the boolean-mask indexing of idr.py:202-213, 272 (which syncs the host per mask). */
int mvsdf_partition_rays(const uint8_t* net_mask, const uint8_t* object_mask, const uint8_t* true_mask, const float* ray_dirs, int R,
                         long long* perm, long long* inv, long long* true_rows, long long* counts, float* view_sorted, void* stream);
/* Output tensors of the training forward gathered from ONE fused evaluation over the rows [E sample points | R rays sorted, hit first]
 * (x_eval[E+R][3], y_eval[E+R][Nout], n_eval[E+R][3]).  The sample rows are [n_eik eikonal | n_ds on-surface | n_ds jittered]
 * (E = n_eik + 2 n_ds).  Point groups in the reference's order: 0 = hit rays, 1 = eikonal, 2 = on-surface, 3 = jittered;
 * d_mask / e_mask (bit g = group g) select the groups of the depth term (eikonal_output, eikonal_points_hom) and of the eikonal term
 * (grad_theta), idr.py:258-286.  counts (DEVICE, {N, n_true} from mvsdf_partition_rays): the kernel reads the hit counts there, so it
 * can be enqueued before the host knows them; every output is sized for the worst case (N = R) and the first
 * [N + selected samples] rows are valid.  rgb_values[R][3] (rgb_sorted[r] for sorted rows r < N, 1 elsewhere; idr.py:302-304),
 * sdf_output[R], diff_pts[R][3], eik_out[.], points_hom[.][4] (x, 1), grad_theta[.][3], surf[R + n_eik] = column 1 at the true-mask hit
 * rows, then at the n_eik eikonal rows (idr.py:270-276). */
int mvsdf_step_outputs(int R, int n_eik, int n_ds, int Nout, const long long* counts, const float* x_eval, const float* y_eval,
                       const float* n_eval, const long long* inv, const long long* true_rows, const float* rgb_sorted, int d_mask,
                       int e_mask, float* rgb_values, float* sdf_output, float* diff_pts, float* eik_out, float* points_hom, float* grad_theta,
                       float* surf, void* stream);
/* Upstream gradients dy[E+N][Nout], dn[E+N][3] of the fused SDF backward (N, n_true known on the host by now).  stage 0: zero + the
 * rendering net's input adjoint din[N][din_ld] (features from column din_feat0 -> dy[:, 2:], normals from din_nrm0 -> dn when use_geo).
 * stage 1 (after the input-adjoint pass produced dx[N][3]): SampleNetwork's scalar -(xbar . v)/(n . v), xbar = d_diff + din[:, 0:3]
 * (use_geo) + dx (sample_network.py:10-20), added to dy[E+i][0]; d_eo / d_gth / d_si (upstream of eikonal_output / grad_theta /
 * surf_indicator_output, any may be NULL) scattered over the same groups as mvsdf_step_outputs. */
int mvsdf_step_backward_inputs(int stage, int n_eik, int n_ds, int N, int Nout, int n_true, const float* din, int din_ld, int din_feat0,
                               int din_nrm0, int use_geo, const float* d_diff, const float* dx, const float* view_sorted, const float* n_eval,
                               const long long* true_rows, const float* d_eo, const float* d_gth, const float* d_si, int d_mask, int e_mask,
                               float* dy, float* dn, void* stream);
/* stage 2 of mvsdf_step_backward_inputs = stage 1 without SampleNetwork's scalar; this adds it afterwards: fbar[i] = -(xbar_i . v_i) / (n_i . v_i)
 * (sample_network.py:10-20), xbar = d_diff + din[:, 0:3] (if use_geo) + dx, written to fbar[N] and added to dy[(E + i) * Nout]. */
int mvsdf_step_backward_fbar(int n_eik, int n_ds, int N, int Nout, const float* din, int din_ld, int use_geo, const float* d_diff, const float* dx,
                             const float* view_sorted, const float* n_eval, float* dy, float* fbar, void* stream);

/* ---- phase-0 depth-surface sampling of IDRNetwork.forward (idr.py:226-247, my_utils.py:71-95) ----
 * Two uniformly random n-subsets (without replacement) of the depth pixels (depths[N][H][W] > 0) whose unprojected, normalised point
 * -- set 0 -- or jittered point (+U(-jitter_rad, jitter_rad)^3) -- set 1 -- lies inside the box |x| < bb: the kernel visits the
 * pixels in a keyed random order and unprojects only the candidates it visits.  kinv[N][3][3] / einv[N][4][4]: inverse intrinsics /
 * extrinsics of the depth cameras; size[1], center[3] on the device.  idx[2][n] (pre-filled by the caller with a value >= N*H*W)
 * receives the pixel indices in visiting order, counts[2] how many were found (n unless the image holds fewer valid pixels).
 * mvsdf_dsurf_points turns the SORTED indices (the reference sorts, np.sort) into the points pts_on[n][3], pts_jit[n][3]; same
 * seed = same jitter as during the selection. */
int mvsdf_dsurf_select(const float* depths, const float* kinv, const float* einv, int N, int H, int W, const float* size, const float* center,
                       float bb, float jitter_rad, unsigned long long seed, int n, long long* idx, long long* counts, void* stream);
int mvsdf_dsurf_points(const float* depths, const float* kinv, const float* einv, int N, int H, int W, const float* size, const float* center,
                       float bb, float jitter_rad, unsigned long long seed, int n, const long long* idx_sorted, const long long* counts,
                       float* pts_on, float* pts_jit, void* stream);

/* ---- optimiser tail on flat buffers (idr_train.py:289-302: all_norm, clip_grad_norm_(grad_cap), Adam.step), two launches ----
 * p, g, m, v: flat fp32 buffers of n elements (parameters, gradients, exp_avg, exp_avg_sq).  step >= 1 is the Adam step count AFTER
 * this update.  max_norm <= 0 disables clipping; otherwise g is scaled in place by min(1, max_norm / (||g|| + 1e-6)).
 * beta1 / beta2 are DOUBLES: 1 - beta and the bias corrections 1 - beta1^step, sqrt(1 - beta2^step) are formed from them in double and rounded once
 * (a float 0.999 would put 1.3e-5 of relative error on 1 - beta2).
 * norm_out (device, 2 floats, may be NULL) receives {||g||, clip coefficient}; ws: mvsdf_adam_ws_floats() floats, written before they are read.
 * Alignment: the four buffers need only 4-byte alignment and no padding; when all four are 16-byte aligned the update uses 16-byte accesses, with the
 * same per-element arithmetic (identical bits either way).  Nothing outside [0, n) of a buffer is written; the sums have a fixed order (the same call on
 * the same state gives the same bits).
 * Non-finite gradients are plain data: the coefficient applies only when it is below 1 (torch 1.7.1's clip_grad_norm_, `if clip_coef < 1:`), so a NaN norm
 * clips nothing and the NaN stays in its own elements; an infinite norm gives coefficient 0 (finite gradients vanish, infinite ones become NaN). */
size_t mvsdf_adam_ws_floats(void);
int mvsdf_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, double beta1, double beta2, float eps, int step, float max_norm,
                    float* norm_out, float* ws, void* stream);
/* Same with every gradient multiplied by grad_scale first (norm and clip see the scaled gradient): grad_scale = 1 / world size turns the
 * SUM of a data-parallel all-reduce into the rank average inside the optimiser launch -- no separate division pass over the bucket. */
int mvsdf_adam_step_scaled(float* p, float* g, float* m, float* v, size_t n, float lr, double beta1, double beta2, float eps, int step,
                           float max_norm, float grad_scale, float* norm_out, float* ws, void* stream);
/* ... and, with zero_grad != 0, ZEROS left in g instead of the scaled / clipped gradient: the `optimizer.zero_grad()` that opens the next iteration
 * (idr_train.py:283) then needs no launch of its own (the update pass touches every gradient element anyway). */
int mvsdf_adam_step_fused(float* p, float* g, float* m, float* v, size_t n, float lr, double beta1, double beta2, float eps, int step,
                          float max_norm, float grad_scale, int zero_grad, float* norm_out, float* ws, void* stream);

/* masks -> what IDRLoss.forward needs from them, one launch: hit[R] = network_object_mask & object_mask (loss.py:21,206), view_start[B+1]
 * = prefix sums of the per-view hit counts (rows of diff_surf_pts per view, loss.py:119-127; R = B * P rays, view-major),
 * n_pos = #(network_object_mask & object_mask_true) (positives of the surface-indicator BCE, loss.py:167-173). */
int mvsdf_loss_prep(const uint8_t* net_mask, const uint8_t* obj_mask, const uint8_t* true_mask, int R, int B, uint8_t* hit, int* view_start,
                    long long* n_pos, void* stream);
/* backward of the weighted total of mvsdf_loss_terms: g = HOST array of 6 device pointers to the scalar upstream gradients of {loss, rgb,
 * eikonal, depth, feat, surf} (NULL = no gradient, the usual case for all but `loss`); every unit
 * gradient tensor is scaled by (g[0] * weight + g[term]) into its output; coef_feat[1] (may be NULL) = g[0] * w_feat + g[4]. */
int mvsdf_loss_scale(const float* const* g, float w_rgb, float w_eik, float w_surf, float w_feat, float w_depth, const float* d_rgb, float* g_rgb,
                     int n_rgb, const float* d_grad, float* g_grad, int n_grad, const float* d_eo, float* g_eo, int n_eo, const float* d_sf,
                     float* g_sf, int n_sf, float* coef_feat, void* stream);

/* device self-test of the deterministic math: op 0 softplus100, 1 expneg, 2 log1p01, 3 sincos (y0=sin, y1=cos),
 * 4 div100 / div_sqrt2 (y0, y1), 5 sqrt / reciprocal (y0, y1), 6 two-wide softplus100 (y0 = f(x), y1 = f(-x)). */
int mvsdf_det_math(int op, const float* x, int n, float* y0, float* y1, void* stream);

/* ==== native step driver: one training step as a handful of calls, no host code between the launches ====
 * Replaces the host side of IDRNetwork.forward in training mode (idr.py:179-322), of IDRLoss.forward (loss.py:176-219) and of
 * `loss.backward()` through both (idr_train.py:283-287) -- the reference issues ~2 000 framework ops there; the Python mirror of this
 * library used to issue ~45 ctypes calls plus autograd glue (1.6 ms of host time per step).  Each call below enqueues ALL launches of its
 * phase on `stream` from C++; launch shapes that depend on the hit count N read it from device memory or are sized for the worst case.
 *
 * Memory: the caller owns two blocks.  `fwd` (MvsdfStepLayout.fwd_bytes, one per forward, kept until its backward has run) receives every
 * output tensor of the forward at the byte offsets of the layout and everything the backward reads (folded weights, packs, saved
 * activations); `bwd` (bwd_bytes) is scratch of the backward.  Offsets are multiples of 256 bytes.  */
#define MVSDF_STEP_MAX_LAYERS 24

typedef struct {
    int B, P;                              /* this batch: B views x P pixels, R = B * P rays (uv[B][P][2], idr.py:183-190) */
    int n_eik;                             /* eikonal sample points (idr.py:216-217: R / 2) */
    int n_ds;                              /* depth-surface samples per set (idr.py:226-247), 0 outside phase 0 */
    int n_sdf, n_render;                   /* Linear layers of ImplicitNetwork / RenderingNetwork */
    int N[MVSDF_STEP_MAX_LAYERS];          /* out features per Linear: the n_sdf SDF layers, then the n_render rendering layers */
    int K[MVSDF_STEP_MAX_LAYERS];          /* in features */
    unsigned skip_mask;                    /* bit l: the input of SDF layer l is cat([x, PE(x)]) / sqrt(2) (idr.py:86-87) */
    int multires;                          /* PE frequencies of the SDF net */
    int view_spec;                         /* multires_view | mode bits, as mvsdf_render_forward takes them */
    int trace_dtype;                       /* 0: fp32 tracing MLP; 1: bf16 packs are made each forward and the tracer uses them; 2: fp32 packs of the bf16-rounded weights; 3 / 4: bf16 packs without duplicated columns, activations as 2 / 3 bf16 terms (MvsdfNetDesc.trace_dtype) */
    int use_object_mask;                   /* conf.use_mask (idr.py:187): 0 = the ray partition ignores object_mask */
    MvsdfTraceParams tp;
    int mt, mt_samples;                    /* tiling of the tracer kernels (see mvsdf_trace) */
} MvsdfStepDesc;

typedef struct {                           /* raw parameters (device pointers), SDF layers first; g[l] NULL = no weight norm */
    const float* v[MVSDF_STEP_MAX_LAYERS];
    const float* g[MVSDF_STEP_MAX_LAYERS];
    const float* b[MVSDF_STEP_MAX_LAYERS];
} MvsdfStepParams;

typedef struct {
    const float* uv; const float* pose; const float* intrinsics;         /* [B][P][2], [B][4][4], [B][4][4] */
    const uint8_t* object_mask;            /* [R] the mask the tracer sees (all ones when conf.use_mask is off, idr.py:187) */
    const uint8_t* object_mask_true;       /* [R] input['object_mask'] */
    const float* intervals;                /* [n_steps] linspace(0, 1) (ray_tracing.py:206) */
    const float* minsdf_steps;             /* [n_steps] uniform draws of minimal_sdf_points (ray_tracing.py:287) */
    const float* eik_points;               /* [n_eik][3] uniform draws in the eikonal box (idr.py:216-221) */
    const float* ds_on; const float* ds_jit;  /* [n_ds][3] each (mvsdf_dsurf_points), NULL when n_ds == 0 */
    const long long* ds_counts;            /* [2] device: samples found per set (mvsdf_dsurf_select), NULL when n_ds == 0 */
    const float* host_stage;               /* optional: PINNED host memory (hipHostMalloc / a torch pinned tensor) holding [minsdf_steps | eik_points]
                                            * = tp.n_steps + 3 n_eik floats.  When given, minsdf_steps / eik_points are uninitialised device buffers and
                                            * the forward's first kernel fills them from here (no copy node, and no copy-to-kernel bubble, in front of
                                            * the step); the host may rewrite the memory once mvsdf_step_wait_counts has returned.  NULL: the two
                                            * device buffers already hold the draws. */
} MvsdfStepInputs;

typedef struct {
    size_t fwd_bytes, bwd_bytes;
    /* byte offsets into `fwd` of the tensors of the reference's output dict (idr.py:306-322); every N-dependent tensor is sized for N = R
     * and its first rows are valid (see mvsdf_step_outputs) */
    size_t ray_dirs, cam_loc;              /* [R][3], [B][3] */
    size_t points, mask, dists, counters;  /* tracer outputs: [R][3] f32, [R] u8, [R] f32, uint64[16] */
    size_t object_mask_out;                /* [R] u8: all ones (out['object_mask'] when conf.use_mask is off) */
    size_t rgb_values, sdf_output, diff_pts, eik_out, points_hom, grad_theta, surf;
    size_t perm;                           /* int64 [R]: sorted row -> ray (hit rays first) */
    size_t dflat;                          /* offset into `bwd`: the gradient of the folded parameters [dW | db of the SDF net | dW | db of the rendering net] */
    size_t dflat_floats;
} MvsdfStepLayout;

/* create / destroy the host-side state of a step (a pinned 4 x int64 staging buffer and HIP events; no device memory) */
int mvsdf_step_create(const MvsdfStepDesc* desc, MvsdfStepLayout* layout, void** step);
void mvsdf_step_destroy(void* step);
/* IDRNetwork.forward, training mode: fold (+ bf16 packs) -> camera rays -> RayTracing.forward -> ray partition (hit counts start travelling
 * to the pinned buffer) -> ONE fused value + normal evaluation over [sample points | rays, hit first] -> rendering net -> output gather.
 * d_mask / e_mask: point groups of the depth / eikonal terms (see mvsdf_step_outputs).
 * mode: MVSDF_STEP_UNHIT_DEFER leaves out what only the rays WITHOUT a hit need and no training step reads -- minimal_sdf_points (ray_tracing.py:280-308: the
 *   min-sdf rows, ~44 % of the tracer's rows at the bench shape), their evaluation rows [E + N, E + R) and their sdf_output: the last tracer launch runs the secant
 *   chains only (stage 7 of mvsdf_trace_stage), the fused evaluation and the output gather bound the rays' rows by the device-side hit count.  Until
 *   mvsdf_step_resolve_unhit has run on the block, `points` / `dists` / `sdf_output` of those rays and counters[MVSDF_CNT_ROWS_MINSDF] are not final.
 *   MVSDF_STEP_UNHIT_EAGER: everything in the forward (the launch sequence up to round 6).  Same values either way. */
#define MVSDF_STEP_UNHIT_DEFER 0
#define MVSDF_STEP_UNHIT_EAGER 1
int mvsdf_step_forward(void* step, const MvsdfStepParams* prm, const MvsdfStepInputs* in, int d_mask, int e_mask, int mode, void* fwd, void* stream);
/* What a MVSDF_STEP_UNHIT_DEFER forward left out, enqueued on `stream` from the forward block ALONE (folded weights and packs, the forward's own copy of the SDF
 * biases and of the min-sdf steps, the tracer's workspace and counters, rays, perm and counts live there: no parameter, input or staging buffer is read), so it may
 * run after any number of later forwards and optimiser steps and still evaluates at that forward's network: (1) the min-sdf rows alone + their reduction (stage 5),
 * (2) the evaluation rows [E + N, E + R) through the eager step's chain kernel, (3) the scatter of their sdf_output.  Same kernels, rows independent of their
 * chunk: the eager step's bits.  Nothing to do (every launch leaves at once) when no ray is without a hit.  Call it ONCE per block (a second call would count the
 * min-sdf rows again); a MVSDF_STEP_UNHIT_EAGER block must not be passed.
 * mvsdf_step_can_defer_unhit: 1 when this step's SDF network runs through the fused forward chain, which both calls need (else only MVSDF_STEP_UNHIT_EAGER).
 * mvsdf_step_last_tracer_grid: out[2] = {secant workgroups, sample-row workgroups} of the last tracer launch of the last forward (0 row workgroups: deferred). */
int mvsdf_step_resolve_unhit(void* step, void* fwd, void* stream);
int mvsdf_step_can_defer_unhit(void* step);
/* The sphere cut in MVSDF_STEP_UNHIT_DEFER forwards (mvsdf_trace_cut_stage: the late rays finish on a second stream beside the sampler windows, joined before the ray
 * partition; no host wait).  enable < 0 (the default): where it pays (three-weight-term engine, one row tile per sphere workgroup, between half a workgroup and one per compute unit); 0: never -- the launch
 * sequence without it; > 0: always.  max_rounds <= 0: st_iters + 1.  Same values with and without. */
int mvsdf_step_set_sphere_cut(void* step, int enable, int max_rounds);
/* The fork of a forward that takes the sphere cut, part by part (each: < 0 by its rule, 0 the launch sequence without that part exactly, > 0 on wherever the cut is on;
 * none of them touches a forward without the cut).  late_on_main: the late branch (resume launch, late rows, their reduction) stays on the forward's stream with no
 * event in front of it and the sampler windows go to the second stream.  partition_beside_secant: the ray partition (and the count record it sends to the host) runs on
 * the second stream beside the secant chains; the forward's stream waits for it in front of the fused evaluation.  rows16: the late list's rows and the first
 * sampler window in the sixteen-wave form (mvsdf_trace_rows_stage; 1: both, 2: the late rows alone, 3: the first window alone); -3 from the forward where it is
 * forced on for a network without that form.  rows16_grid_cap > 0:
 * at most that many workgroups in those launches.  Same values in every combination. */
int mvsdf_step_set_fork(void* step, int late_on_main, int partition_beside_secant, int rows16, int rows16_grid_cap);
int mvsdf_step_last_tracer_grid(void* step, int out[2]);
/* blocks until the counts of the last mvsdf_step_forward are on the host: {N hit, N hit & true mask, depth-surface samples found per set x 2}.
 * The one host wait of a CLASSIC training step (the fused evaluation enqueued behind the count record keeps the GPU busy meanwhile); a DEFERRED
 * step (below) never calls it. */
int mvsdf_step_wait_counts(void* step, long long counts[4]);
/* ---- the deferred step: no host wait between the forward and the optimiser ----
 * The counts stay on the device: mvsdf_loss_forward with MvsdfLossArgs.counts_dev set and mvsdf_step_backward with N < 0 take {N, n_true} from
 * the forward block (written by the ray partition), size their launches for N = R and bound every row loop by the device values, so a training
 * loop `forward -> loss -> backward -> optimiser` enqueues whole steps ahead of the GPU and its rate no longer depends on the host's latency
 * (idr_train.py:253-315 is the loop; its per-step print is the only reader of host-side numbers).  Results are bit-identical to the classic step.
 * mvsdf_step_seq: sequence number (1, 2, ...) of the last mvsdf_step_forward of this step object.
 * mvsdf_step_counts_offset: byte offset inside `fwd` of its int64 counts[4] = {N, n_true, ds found x 2} (the `counts_dev` of that forward); 32 bytes behind
 *   it float term_rows[3] = rows of grad_theta / eikonal_output / surf_indicator_output for these counts (what a data-parallel step all-reduces to
 *   normalise the three count-based means by the global counts, MvsdfLossArgs.inv_counts).
 * mvsdf_step_wait_counts_seq: blocks until forward `seq` has delivered its counts (a short spin, then sleeps); -4 when that record was overwritten
 *   (more than MVSDF_STEP_COUNT_RING forwards ago: read the counts from the forward block instead).
 * mvsdf_step_done_seq: newest forward whose partition kernel is known to have run (non-blocking; its counts -> counts[4] when not NULL).
 * mvsdf_step_can_defer: 1 when mvsdf_step_backward accepts N < 0 for this step's networks (every launch has a fused device-count form). */
#define MVSDF_STEP_COUNT_RING 64
long long mvsdf_step_seq(void* step);
size_t mvsdf_step_counts_offset(void* step);
int mvsdf_step_wait_counts_seq(void* step, long long seq, long long counts[4]);
long long mvsdf_step_done_seq(void* step, long long counts[4]);
int mvsdf_step_can_defer(void* step);
/* byte offsets inside `fwd` of what the forward saved for the backward, for inspection (tests read the rendering net's own ReLU masks there):
 * out[6] = {x_eval [E+R][3] evaluation rows [samples | rays, hit first], y_eval [E+R][Nout], n_eval [E+R][3], view_sorted [R][3],
 * render_ctx (mvsdf_render_forward's context for R rows: the input [R][K_0], then the post-ReLU activations [R][K_l] of layers 1.., then rgb),
 * rgb_sorted [R][3]} */
int mvsdf_step_saved_offsets(void* step, size_t out[6]);
/* byte offsets inside `fwd` of what the prologue of the forward prepared for layer `layer` (SDF layers first, then the rendering net's), for inspection
 * (tests compare the block's packs with the stand-alone pack entry points): out[7] = {w [N][K] folded weights, wp (the pack of W), wpT (of W^T),
 * wp16 (the tracing MLP's pack under trace_dtype 2..5: fp32 pack of the bf16-rounded weights / bf16 pack / three-term bf16 pack), wx3, wx3T (three-term
 * bf16 packs of W and W^T for the differentiable chains; wx3 == wp16 under trace_dtype 5), bias copy [N] (SDF layers; written by a forward in mode
 * MVSDF_STEP_UNHIT_DEFER only)}; (size_t)-1 where the block holds none for this layer and trace_dtype. */
int mvsdf_step_pack_offsets(void* step, int layer, size_t out[7]);
/* backward of mvsdf_step_forward: upstream gradients of diff_surf_pts [N][3], rgb_values [R][3], grad_theta, eikonal_output,
 * surf_indicator_output (any may be NULL = zero) -> gradient of every raw parameter.  N, n_true: the counts mvsdf_step_wait_counts returned;
 * N < 0: the deferred step -- both counts are read on the device from `fwd`, the upstream tensors hold their valid rows first (sized for N = R),
 * and n_true carries a HINT of N (a recent step's, or < 0 for none) that only selects kernel forms.
 * use_geo: 0 = points / normals / view directions detached in front of the rendering net (idr.py:331-334).
 * dv / dg / db: per-layer targets (device pointers; dg[l] NULL where g[l] is); accumulate != 0 ADDS into them (the parameters' .grad). */
int mvsdf_step_backward(void* step, const MvsdfStepParams* prm, int N, int n_true, int d_mask, int e_mask, int use_geo, const float* d_diff,
                        const float* d_rgb, const float* d_gth, const float* d_eo, const float* d_si, const void* fwd, void* bwd,
                        float* const* dv, float* const* dg, float* const* db, int accumulate, void* stream);
/* per-kernel timing of the tracer for bench.py's roofline: enable != 0 makes every forward record HIP events on the launch stream around
 * k_sphere_trace, the sampler launches and the secant / min-sdf launch; mvsdf_step_trace_times (after the stream was synchronised) ->
 * ms[3] = {sphere tracing, sampler rows, secant + min-sdf rows} of the last forward. */
int mvsdf_step_set_timing(void* step, int enable);
int mvsdf_step_trace_times(void* step, float ms[3]);
/* ... and of the differentiable half (idr.py:240-322 forward, its backward): ms[6] = {the three above, the forward behind the tracer (fused value +
 * normal evaluation, rendering net, output gather: no bubbles on the stream, so the event distance IS the kernel time; sample rows evaluated on the side
 * stream beside the tracer are not in it), mvsdf_step_backward, the whole mvsdf_step_forward from its first launch (fold + packs + rays) to its last} of the
 * last step. */
int mvsdf_step_times(void* step, float ms[6]);

/* ---- IDRLoss.forward / backward (loss.py:176-219) as one call each ---- */
typedef struct {
    int R, B;                              /* rays, views of this batch */
    int N, n_grad, n_depth, n_surf;        /* rows of diff_surf_pts / grad_theta / eikonal_output / surf_indicator_output */
    const uint8_t* net_mask; const uint8_t* obj_mask; const uint8_t* true_mask;      /* [R] */
    const float* rgb; const float* rgb_gt;                                           /* [R][3] */
    const float* grad_theta; const float* eik_out; const float* surf; const float* diff_pts;
    float* points_hom;                     /* [n_depth][4]: rescaled to world coordinates IN PLACE (loss.py:38,42) */
    int feat_on, surf_on;                  /* phase switches (loss.py:195-204) */
    int V, C, H, W;                        /* source views, feature channels, feature map size */
    const float* feat; long long feat_strides[4]; const float* feat_src; long long src_strides[5];
    const float* cam; const float* src_cams; const float* size; const float* center;
    const float* depths; int dB, dh, dw; const float* depth_cams;                    /* [dB][dh][dw], [dB][2][4][4] */
    float out_thresh_perc, far_thresh, far_att, near_thresh, near_att;
    float w_rgb, w_eik, w_surf, w_feat, w_depth;
    int use_invalid;                       /* conf.use_invalid: carving_t instead of carving_t2 (see mvsdf_depth_carve) */
    float smooth;                          /* depth term: 0 = L1, s > 0 = SmoothL1(eikonal_output / s, -dist_r / s) * s (loss.py:57-58: conf.smooth(train_progress)) */
    const float* inv_counts;               /* see mvsdf_loss_terms */
    /* deferred step: device pointer to {N, n_true} (int64, the forward block's counts).  N / n_grad / n_depth / n_surf above are then UPPER BOUNDS
     * (N = R) that size the block's layout and the grids; the kernels derive the true row counts from the device values and the step's point groups:
     * n_grad / n_depth = rows of the groups e_mask / d_mask select among [N hit | n_eik | n_ds | n_ds] (mvsdf_step_outputs), n_surf = n_true + n_eik. */
    const long long* counts_dev;
    int n_eik, n_ds, d_mask, e_mask;
} MvsdfLossArgs;
typedef struct {
    size_t bytes, out, hit, view_start, n_pos, loss_pp, dpts, dist_r, weight, d_rgb, d_grad, d_eo, d_sf;
    /* gradients of the TOTAL loss w.r.t. rgb_values / grad_theta / eikonal_output / surf_indicator_output / diff_surf_pts (unit gradient x term weight:
     * exactly what mvsdf_loss_backward returns for an upstream of 1 on `loss` alone), written by mvsdf_loss_forward */
    size_t s_rgb, s_grad, s_eo, s_sf, s_diff;
} MvsdfLossLayout;
/* layout of the block both calls work in (out: float[6] = loss, rgb, eikonal, depth, feat, surf) */
int mvsdf_loss_layout(const MvsdfLossArgs* a, MvsdfLossLayout* lo);
/* mask bookkeeping || depth carving, feature consistency, all terms and their unit gradients: 3 launches */
int mvsdf_loss_forward(const MvsdfLossArgs* a, void* blk, void* stream);
/* g: HOST array of 6 device pointers (upstream of the six scalars, NULL = none) -> gradients of rgb_values [R][3], grad_theta [n_grad][3],
 * eikonal_output [n_depth], surf_indicator_output [n_surf], diff_surf_pts [N][3] (any target may be NULL): one launch */
int mvsdf_loss_backward(const MvsdfLossArgs* a, const void* blk, const float* const* g, float* g_rgb, float* g_grad, float* g_eo, float* g_sf,
                        float* g_diff, void* stream);

/* ==== the scene-side calls: result words, error bits and limits ====
 * Most calls below leave int64 result words at the start of their workspace (or of a 256-byte `hdr`), one of them an error word.  The enum blocks
 * beside the calls name the word indices (MVSDF_<CALL>_H_<WORD>; _H_WORDS = the words a host may read; a run of words is named by its first index
 * and ends at the next enumerator), the bits of the error word (MVSDF_<MOD>_ERR_<WHAT>) and the argument limits both sides check
 * (MVSDF_<MOD>_MAX_<WHAT>; a limit beyond int is given as its exponent, _LOG2).  mvsdf_amd/_lib.py reads them from this file. */
/* the calls that say they leave {0, error bits}, and mvsdf_fusion_fuse */
enum {
    MVSDF_RES_H_COUNT = 0,  /* mvsdf_fusion_fuse: the points kept; 0 from every other call */
    MVSDF_RES_H_ERR = 1,    /* the error bits of the call's module */
    MVSDF_RES_H_WORDS = 2
};
/* the calls that say they leave {error bits} alone */
enum {
    MVSDF_ERRW_H_ERR = 0,   /* the error bits of the call's module */
    MVSDF_ERRW_H_WORDS = 1
};
/* the calls that say they leave {rows kept} (mvsdf_cloud_compact, mvsdf_reg_crop) */
enum {
    MVSDF_ROWS_H_ROWS = 0,  /* the rows kept */
    MVSDF_ROWS_H_WORDS = 1
};

/* ---- mesh extraction (mesh_kernels.hip; Python: mvsdf_amd/mesh.py, which states the vertex / face conventions) ----
 * Marching cubes of an fp32 volume vol[i][j][k] = vol[i * strides[0] + j * strides[1] + k * strides[2]] (element strides, host arrays shape[3] /
 * strides[3]) at `level`; a corner is inside when its value is < level.  Two calls: mvsdf_mc_count classifies the grid and leaves the
 * MVSDF_MC_H_* words at the start of the workspace; the caller reads them (the one host synchronisation), allocates and calls
 * mvsdf_mc_emit with the same volume and workspace.  Every extent must be >= 2.
 * workspace bytes: 4 per grid point + O(points / 1024); 0 = refused (an extent below 2 or a grid the kernels cannot index).
 * nv_cap / nf_cap: the rows verts / normals and faces can hold (nothing is written beyond them).  Vertex ids are int32: a caller refuses a
 * volume whose counts exceed INT32_MAX. */
enum {                          /* mvsdf_mc_count, mvsdf_mcm_count */
    MVSDF_MC_H_VERTS = 0,       /* vertices of the mesh */
    MVSDF_MC_H_FACES = 1,       /* faces of the mesh */
    MVSDF_MC_H_BAD = 2,         /* non-zero: a non-finite value was seen (mvsdf_mcm_count: a non-finite VALID value) */
    MVSDF_MC_H_WORDS = 3
};
size_t mvsdf_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int mvsdf_mc_count(const float* vol, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes, void* stream);
int mvsdf_mc_emit(const float* vol, const int64_t* shape, const int64_t* strides, float level, const float* spacing, const float* origin, void* ws,
                  size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream);
/* Connected components of a mesh (vertex connectivity through faces, union-find) -> vert_label[nv], face_label[nf]: components numbered by their lowest
 * vertex id; the workspace starts with the MVSDF_CC_H_* words.  1 <= nv, nf <= INT32_MAX, else the workspace query gives 0. */
enum {
    MVSDF_CC_H_COMPONENTS = 0,  /* components */
    MVSDF_CC_H_LABEL = 1,       /* label of the largest by area (ties: the lowest face index) */
    MVSDF_CC_H_VERTS = 2,       /* its vertices */
    MVSDF_CC_H_FACES = 3,       /* its faces */
    MVSDF_CC_H_BOUND = 4,       /* 1 if a union-find loop hit its bound */
    MVSDF_CC_H_WORDS = 5
};
size_t mvsdf_mesh_cc_workspace_bytes(int64_t nv, int64_t nf);
int mvsdf_mesh_components(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, int32_t* vert_label,
                          int32_t* face_label, void* stream);
/* The vertices and faces with the given label, in their original order, faces re-indexed (trimesh's submesh).  normals / colors ([nv][3] fp32) may be NULL.
 * Same workspace size as mvsdf_mesh_components. */
int mvsdf_mesh_select(const int32_t* vert_label, const int32_t* face_label, int64_t nv, int64_t nf, int32_t label, const float* verts, const float* normals,
                      const float* colors, const int32_t* faces, void* ws, size_t ws_bytes, float* out_verts, float* out_normals, float* out_colors,
                      int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream);

/* ---- sparse mesh extraction (mesh_sparse.hip; Python: mesh.sparse_marching_cubes, whose doc states the contract) ----
 * The marching-cubes mesh of the n^3 lattice (value at point (i, j, k) = sdf(axis[i], axis[j], axis[k]), axis: fp32 [n]) over the cells of the
 * active blocks of B^3 cells only, in the dense path's vertex / face order.  The caller evaluates the SDF at the points these calls generate:
 *   mvsdf_smc_coarse_points: points [start, start + count) of the (nb + 1)^3 block corners, nb = ceil((n - 1) / B), as fp32 [count][3];
 *   mvsdf_smc_seed: the corner values -> seed blocks (corners on both sides of `level`, or one within `tol` of it), given slots 0 .. seeds - 1;
 *   mvsdf_smc_brick_points: points [start, start + count) of the bricks, item slot * (B + 3)^3 + local (lattice indices b B - 1 + local, clamped);
 *   mvsdf_smc_closure: values of the slots [slot0, slot0 + count) (values[slot * (B + 3)^3 + local]) -> inactive neighbours across a face with a
 *     crossing grid edge get the next slots, from slot0 + count on;
 *   mvsdf_smc_count / mvsdf_smc_emit: the values of all `nactive` slots -> the mesh (like mvsdf_mc_count / mvsdf_mc_emit).
 * The workspace starts with the MVSDF_SMC_H_* words (the words between them are 0): the caller reads the count after each seed / closure call and
 * the totals after mvsdf_smc_count.  Workspace queries give 0 for n < 3, B < 2 (or > 1024) or sizes the kernels cannot index; the emit workspace
 * holds (B + 1)^3 int32 per active block. */
enum {
    MVSDF_SMC_H_COUNT = 0,      /* the last seed / closure count; after mvsdf_smc_count the active blocks it listed */
    MVSDF_SMC_H_BAD = 3,        /* 1 once a non-finite evaluated value was seen */
    MVSDF_SMC_H_STORES = 4,     /* closure flag stores (per-wave sums; a block can be flagged by several faces) */
    MVSDF_SMC_H_OWNER = 5,      /* 1 if a face's edge has no active vertex owner (the closure did not close: never expected) */
    MVSDF_SMC_H_VERTS = 8,      /* mvsdf_smc_count: vertices */
    MVSDF_SMC_H_FACES = 9,      /* mvsdf_smc_count: faces */
    MVSDF_SMC_H_NEGATIVE = 10,  /* mvsdf_smc_count: 1 if a per-workgroup count was negative (never expected) */
    MVSDF_SMC_H_WORDS = 11
};
size_t mvsdf_smc_workspace_bytes(int64_t n, int64_t block);
size_t mvsdf_smc_emit_workspace_bytes(int64_t n, int64_t block, int64_t nactive);
int mvsdf_smc_coarse_points(const float* axis, int64_t n, int64_t block, int64_t start, int64_t count, float* pts, void* stream);
int mvsdf_smc_seed(const float* coarse, int64_t n, int64_t block, float level, float tol, void* ws, size_t ws_bytes, void* stream);
int mvsdf_smc_brick_points(const float* axis, int64_t n, int64_t block, const void* ws, size_t ws_bytes, int64_t start, int64_t count, float* pts,
                           void* stream);
int mvsdf_smc_closure(const float* values, int64_t n, int64_t block, float level, int64_t slot0, int64_t count, void* ws, size_t ws_bytes, void* stream);
int mvsdf_smc_count(const float* values, int64_t n, int64_t block, float level, int64_t nactive, void* ws, size_t ws_bytes, void* ews, size_t ews_bytes,
                    void* stream);
int mvsdf_smc_emit(const float* values, int64_t n, int64_t block, float level, const float* spacing, const float* origin, int64_t nactive, void* ws,
                   size_t ws_bytes, void* ews, size_t ews_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream);

/* ---- mesh trimming (mesh_cut.hip; Python: Mesh.cut_mask / Mesh.trim in mvsdf_amd/mesh.py, which states the semantics) ----
 * The minimum cut of reference code/mesh_cut/mesh_cut.py over the faces: S* = the faces reachable from the source in the residual graph of a maximum
 * flow (bright faces, red > thresh / 255 on average, tie to the source; faces sharing an edge are joined by 2 * smooth).  1 <= nv <= INT32_MAX,
 * 1 <= nf <= INT32_MAX / 8, else the workspace query gives 0.  colors: fp32 [nv][3] (only the red channel is read).
 * mvsdf_mesh_cut waits for the stream (its round loop reads flags from the device) -> removed[nf] (1 = in S*) and the MVSDF_CUT_H_* words
 * at the start of the workspace.  With error bits (MVSDF_CUT_ERR_*) set nothing else is valid.  smooth in [0, INT32_MAX / 6]. */
enum {
    MVSDF_CUT_H_FLOW = 0,           /* the flow value */
    MVSDF_CUT_H_REMOVED = 1,        /* removed faces */
    MVSDF_CUT_H_KEPT_VERTS = 2,     /* vertices the kept faces use */
    MVSDF_CUT_H_ERR = 3,            /* error bits */
    MVSDF_CUT_H_ROUNDS = 4,         /* push rounds */
    MVSDF_CUT_H_RELABELS = 5,       /* relabel launches */
    MVSDF_CUT_H_WORDS = 6
};
enum {
    MVSDF_CUT_ERR_DUP_EDGE = 1,     /* a directed edge in two faces (non-manifold edge or inconsistent winding) */
    MVSDF_CUT_ERR_REPEATED = 2,     /* a face repeats a vertex id */
    MVSDF_CUT_ERR_RANGE = 4,        /* a vertex id outside [0, nv) */
    MVSDF_CUT_ERR_HASH = 8,         /* the half-edge table's probe bound (cannot happen at load factor 1/2) */
    MVSDF_CUT_ERR_ROUNDS = 16,      /* the round limit was reached */
    MVSDF_CUT_ERR_RELABEL = 32      /* a global relabel did not settle within its launch limit */
};
size_t mvsdf_mesh_cut_workspace_bytes(int64_t nv, int64_t nf);
int mvsdf_mesh_cut(const float* colors, const int32_t* faces, int64_t nv, int64_t nf, int32_t thresh, int32_t smooth, void* ws, size_t ws_bytes,
                   uint8_t* removed, void* stream);
/* After a successful mvsdf_mesh_cut with the same workspace: the kept faces and the vertices they use, in their original order, faces re-indexed.
 * normals / colors may be NULL; nv_cap / nf_cap bound what is written. */
int mvsdf_mesh_trim(const float* verts, const float* normals, const float* colors, const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes,
                    float* out_verts, float* out_normals, float* out_colors, int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream);

/* ---- mesh simplification (mesh_simplify.hip; Python: Mesh.simplify in mvsdf_amd/mesh.py, which states the definition) ----
 * Vertex clustering on the uniform grid of edge `cell` from `origin` (a HOST array of 3 doubles, or NULL = the low corner of the vertices' box) with
 * quadric-error placement (quadric != 0) or the clusters' means (0).  1 <= nv <= INT32_MAX, 1 <= nf <= INT32_MAX / 3, else the workspace query gives 0.
 * normals / colors ([nv][3] fp32) may be NULL.  mvsdf_mesh_simplify is the count pass: it waits for the stream (the host reads the box and the cluster
 * count) and leaves the MVSDF_SP_H_* words at the start of the workspace.  With error bits (MVSDF_SP_ERR_*) set nothing else
 * is valid.  counts_only != 0 skips the per-cluster sums and the placement: the counts are the same (quadric-placed stays 0), and no emit may follow.
 * mvsdf_mesh_simplify_emit, after a successful full count with the same workspace: the used clusters ascending, and the kept faces in their original
 * order and corner order, re-indexed.  out_normals / out_colors may be NULL (colours are 0 when the count pass got none); nv_cap / nf_cap bound
 * what is written. */
enum {
    MVSDF_SP_H_CLUSTERS = 0,    /* occupied clusters */
    MVSDF_SP_H_VERTS = 1,       /* output vertices */
    MVSDF_SP_H_FACES = 2,       /* output faces */
    MVSDF_SP_H_DEGENERATE = 3,  /* degenerate faces */
    MVSDF_SP_H_DUPLICATES = 4,  /* duplicate faces */
    MVSDF_SP_H_PLACED = 5,      /* vertices placed by the quadric */
    MVSDF_SP_H_ERR = 6,         /* error bits */
    MVSDF_SP_H_WORDS = 7
};
enum {
    MVSDF_SP_ERR_FINITE = 1,    /* a non-finite vertex */
    MVSDF_SP_ERR_RANGE = 2,     /* a vertex id outside [0, nv) */
    MVSDF_SP_ERR_CELLS = 4      /* a cell index outside [0, 2^21) */
};
size_t mvsdf_mesh_simplify_workspace_bytes(int64_t nv, int64_t nf);
int mvsdf_mesh_simplify(const float* verts, const float* normals, const float* colors, const int32_t* faces, int64_t nv, int64_t nf, double cell,
                        const double* origin, int32_t quadric, int32_t counts_only, void* ws, size_t ws_bytes, void* stream);
int mvsdf_mesh_simplify_emit(const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, float* out_verts, float* out_normals,
                             float* out_colors, int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream);

/* ---- DTU Chamfer evaluation (chamfer.hip; Python: mvsdf_amd/chamfer.py, which states the metric) ----
 * All four operations leave int64 results at the start of their workspace; fp64 throughout.  Error bits: MVSDF_PC_ERR_*, the one numbering of
 * the point-cloud modules (Chamfer, cloud cleaning, registration, normals, global registration).  With error bits set nothing else is valid.
 * mvsdf_chamfer_key: the visiting key splitmix64(seed ^ i) of point i.
 * Sampling, two calls: mvsdf_chamfer_sample_count waits for the stream -> MVSDF_CH_SAMPLE_H_*; the caller allocates
 * out[points][3] and calls mvsdf_chamfer_sample_emit with the same workspace (out = the vertices, then the samples in face order; cap bounds the rows
 * written).  1 <= nv, nf <= INT32_MAX, else the workspace query gives 0. */
enum {
    MVSDF_PC_ERR_POINTS = 1,    /* sampling: more points than max_points */
    MVSDF_PC_ERR_RANGE = 2,     /* sampling: a vertex id outside [0, nv) */
    MVSDF_PC_ERR_FINITE = 4,    /* a non-finite coordinate (normals: or view centre) */
    MVSDF_PC_ERR_COORD = 8,     /* a coordinate too far from the origin for the cell grid: downsampling; the voxel filter (an index of 2^21 or more) */
    MVSDF_PC_ERR_HASH = 16,     /* the cell table's probe bound (cannot happen at load factor 1/2) */
    MVSDF_PC_ERR_ROUNDS = 32,   /* the round limit of a host round loop (downsampling, components, orientation) was reached */
    MVSDF_PC_ERR_WALK = 64,     /* a tree walk hit its bound (cannot happen) */
    MVSDF_PC_ERR_NORMAL = 128,  /* a non-finite normal */
    MVSDF_PC_ERR_INDEX = 256,   /* a neighbour or correspondence index out of range */
    MVSDF_PC_ERR_CODE = 512     /* global registration: a code outside 0 .. 127 */
};
enum { MVSDF_PC_MAX_K = 32 };   /* the most neighbours per point (cloud cleaning, normals, global registration) */
enum {
    MVSDF_CH_SAMPLE_H_POINTS = 0,   /* points (nv + samples) */
    MVSDF_CH_SAMPLE_H_SAMPLES = 1,  /* samples */
    MVSDF_CH_SAMPLE_H_ERR = 2,      /* error bits */
    MVSDF_CH_SAMPLE_H_WORDS = 3
};
enum {
    MVSDF_CH_DOWN_H_KEPT = 0,       /* points kept */
    MVSDF_CH_DOWN_H_ROUNDS = 1,     /* rounds run */
    MVSDF_CH_DOWN_H_ERR = 2,        /* error bits */
    MVSDF_CH_DOWN_H_WORDS = 3
};
enum {
    MVSDF_CH_MASK_H_IN = 0,         /* rows of d_in */
    MVSDF_CH_MASK_H_OBS = 1,        /* rows of d_obs */
    MVSDF_CH_MASK_H_ABOVE = 2,      /* rows of s_above */
    MVSDF_CH_MASK_H_ERR = 3,        /* error bits (MVSDF_PC_ERR_FINITE: a non-finite stl point) */
    MVSDF_CH_MASK_H_WORDS = 4
};
enum {
    MVSDF_CH_NEAR_H_COUNT = 0,      /* distances below the cut-off */
    MVSDF_CH_NEAR_H_SUM = 1,        /* their fp64 sum (bits, fixed order) */
    MVSDF_CH_NEAR_H_ERR = 2,        /* error bits */
    MVSDF_CH_NEAR_H_WORDS = 3
};
uint64_t mvsdf_chamfer_key(uint64_t seed, int64_t i);
size_t mvsdf_chamfer_sample_workspace_bytes(int64_t nv, int64_t nf);
int mvsdf_chamfer_sample_count(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, double density, int64_t max_points, void* ws, size_t ws_bytes,
                               void* stream);
int mvsdf_chamfer_sample_emit(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, double density, void* ws, size_t ws_bytes, double* out,
                              int64_t cap, void* stream);
/* The greedy radius filter: kept[n] (1 = kept) is the lexicographically-first maximal set with no two points within density (d^2 <= density^2) under
 * ascending keys.  Waits for the stream (its round loop reads counts) -> MVSDF_CH_DOWN_H_*; stops with MVSDF_PC_ERR_ROUNDS after max_rounds rounds
 * (n rounds always suffice).  1 <= n <= INT32_MAX / 4. */
size_t mvsdf_chamfer_downsample_workspace_bytes(int64_t n);
int mvsdf_chamfer_downsample(const double* pts, int64_t n, double density, uint64_t seed, int64_t max_rounds, void* ws, size_t ws_bytes, uint8_t* kept,
                             void* stream);
/* The masks, no host wait: d_in / d_obs (capacity n rows) = the kept points inside the box / also observed, s_above (capacity m rows) = the stl points
 * above the plane, each in input order -> MVSDF_CH_MASK_H_*.  box: HOST fp32 [9] = lo[3], hi[3], bb[0][3]; obs: uint8
 * [X][Y][Z] on the device, obs_shape: HOST int64 [3]; plane: HOST fp64 [4]. */
size_t mvsdf_chamfer_mask_workspace_bytes(int64_t n, int64_t m);
int mvsdf_chamfer_mask(const double* pts, const uint8_t* kept, int64_t n, const double* stl, int64_t m, const float* box, double res, const uint8_t* obs,
                       const int64_t* obs_shape, const double* plane, void* ws, size_t ws_bytes, double* d_in, double* d_obs, double* s_above, void* stream);
/* dist[q] = min over refs of sqrt((dx dx + dy dy) + dz dz), exact, +inf where it is not < max_dist.  Waits for the stream -> MVSDF_CH_NEAR_H_*.
 * 0 <= nq, 1 <= nr <= INT32_MAX. */
size_t mvsdf_chamfer_nearest_workspace_bytes(int64_t nq, int64_t nr);
int mvsdf_chamfer_nearest(const double* queries, int64_t nq, const double* refs, int64_t nr, double max_dist, void* ws, size_t ws_bytes, double* dist,
                          void* stream);

/* ---- Depth-map fusion (fusion.hip; Python: mvsdf_amd/fusion.py, which states the definition) ----
 * Two calls.  mvsdf_fusion_fuse validates every argument on the host, then (no host wait) writes masked[V][H][W], fused[V][H][W], counts[V][H][W]
 * and leaves MVSDF_RES_H_* at the start of the workspace.  Error bits: MVSDF_FU_ERR_*; with any set nothing is launched.
 * depths fp32 [V][H][W] and probs fp32 [V][3][H][W] (or NULL) on the device; pthresh: HOST fp32 [3]; pair_off: HOST int32 [V + 1] (pair_off[0] = 0),
 * pair_src: HOST int32 [pair_off[V]], the source views of every view already cut to its first `view` entries; mats: HOST fp64, per pair slot T_rs
 * then T_sr (row-major 4x4 each), followed by Pinv of every view.  The host arrays must stay alive until the caller has read the header.
 * mvsdf_fusion_emit (same workspace, same V, H, W, npairs = pair_off[V]) writes the kept pixels in (view, y, x) order: points fp64 [cap][3],
 * colors uint8 [cap][3] from images uint8 [V][H][W][3] (both NULL: no colours), view / pixel int32 [cap]; rows at or beyond cap are not written. */
enum {
    MVSDF_FU_ERR_FINITE = 1,    /* a non-finite matrix entry or threshold; mvsdf_fusion_normals: or a NaN or negative jump */
    MVSDF_FU_ERR_PAIR = 2,      /* a pair index outside [0, V) */
    MVSDF_FU_ERR_VIEW = 4,      /* view < 1 */
    MVSDF_FU_ERR_SHAPE = 8,     /* V < 1, H or W < 2, V*H*W > 2^40, H*W > INT32_MAX, a pair list longer than view; mvsdf_fusion_normals: or n < 1 */
    MVSDF_FU_ERR_INDEX = 16     /* mvsdf_fusion_normals: a view / pixel index outside the maps (found on the device; that point's normal is 0) */
};
size_t mvsdf_fusion_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t npairs);
int mvsdf_fusion_fuse(const float* depths, const float* probs, const float* pthresh, int64_t V, int64_t H, int64_t W, const int32_t* pair_off,
                      const int32_t* pair_src, const double* mats, int32_t view, int32_t vthresh, double pix_thresh, double dep_thresh, void* ws,
                      size_t ws_bytes, float* masked, float* fused, int32_t* counts, void* stream);
int mvsdf_fusion_emit(const uint8_t* images, int64_t V, int64_t H, int64_t W, int64_t npairs, void* ws, size_t ws_bytes, double* points,
                      uint8_t* colors, int32_t* view, int32_t* pixel, int64_t cap, void* stream);
/* Normals of fused points (fusion.py: depth_normals): one lane per point reads fused fp32 [V][H][W] and view / pixel int32 [n] (device) and writes
 * normals fp64 [n][3].  mats: HOST fp64 [V][19], Pinv of the view (row-major 4x4) then its camera centre; it must stay alive until the caller has
 * read the header.  Leaves MVSDF_RES_H_* at the start of the workspace, no host wait.  Error bits: MVSDF_FU_ERR_FINITE, _SHAPE
 * and _INDEX. */
size_t mvsdf_fusion_normals_workspace_bytes(int64_t V);
int mvsdf_fusion_normals(const float* fused, int64_t V, int64_t H, int64_t W, const int32_t* view, const int32_t* pixel, int64_t n, const double* mats,
                         double jump, void* ws, size_t ws_bytes, double* normals, void* stream);

/* ---- Poisson surface reconstruction (poisson.hip; Python: mvsdf_amd/poisson.py, which states the definition) ----
 * mvsdf_poisson_reconstruct validates its scalar arguments on the host, then (no host wait) runs the stages whose bits are set in `stages` (1 the
 * splat and the right-hand side, 2 the multigrid solve, 4 the isovalue; a later stage needs the earlier ones to have run on the same workspace; 7 =
 * everything) and leaves MVSDF_PO_H_* at the start of the workspace.  Error bits: MVSDF_PO_ERR_*.  points / normals fp64 [n][3] on the device; origin: HOST fp64 [3]; N = 2^depth + 1; chi and density fp64 [N][N][N],
 * values fp64 [n] (the first `points used` rows are the c_i, the rest 0).  workspace bytes: about 43 per lattice point + 9 per point; 0 = refused.
 * mvsdf_poisson_valid: valid uint8 [N][N][N] = density > min_density dilated `dilate` times over the 6-neighbourhood (tmp: uint8 [N][N][N], needed
 * when dilate > 0).  mvsdf_poisson_volume: out[i] = (float)(chi[i] - iso) for count values.  Neither waits. */
enum {
    MVSDF_PO_H_USED = 0,        /* points used */
    MVSDF_PO_H_ERR = 1,         /* error bits */
    MVSDF_PO_H_T = 2,           /* T (fp64 bits) */
    MVSDF_PO_H_RESIDUAL0 = 3,   /* the solve's first residual (fp64 bits) */
    MVSDF_PO_H_RESIDUAL = 4,    /* its last residual (fp64 bits) */
    MVSDF_PO_H_WORDS = 5
};
enum {
    MVSDF_PO_ERR_FINITE = 1,    /* a non-finite coordinate, normal (found on the device), origin or voxel */
    MVSDF_PO_ERR_RANGE = 2,     /* depth outside [MVSDF_PO_MIN_DEPTH, MVSDF_PO_MAX_DEPTH], cycles < 0, sweeps < 1 or voxel <= 0 */
    MVSDF_PO_ERR_SHAPE = 4      /* n < 1 or n > INT32_MAX */
};
enum { MVSDF_PO_MIN_DEPTH = 2, MVSDF_PO_MAX_DEPTH = 10 };
size_t mvsdf_poisson_workspace_bytes(int64_t n, int32_t depth);
int mvsdf_poisson_reconstruct(const double* points, const double* normals, int64_t n, const double* origin, double voxel, int32_t depth, int32_t cycles,
                              int32_t sweeps, int32_t stages, void* ws, size_t ws_bytes, double* chi, double* density, double* values, void* stream);
int mvsdf_poisson_valid(const double* density, int32_t depth, double min_density, int32_t dilate, uint8_t* tmp, uint8_t* valid, void* stream);
int mvsdf_poisson_volume(const double* chi, int64_t count, double iso, float* out, void* stream);

/* ---- TSDF fusion (tsdf.hip; Python: mvsdf_amd/tsdf.py, which states the definition) ----
 * mvsdf_tsdf_integrate validates every argument on the host, then (no host wait) writes tsdf fp32, weight int32 and valid uint8, each
 * [dims[0]][dims[1]][dims[2]] on the device, and leaves MVSDF_RES_H_* at the start of the workspace.  Error bits: MVSDF_TS_ERR_*; with any set nothing is launched.
 * depths fp32 [V][H][W] on the device (a texel that is <= 0 or not finite is a hole); mats: HOST fp64 [nviews][16], P of the q-th visited view
 * (row-major 4x4); views: HOST int32 [nviews], the depth map of the q-th visited view; origin: HOST fp64 [3]; dims: HOST int64 [3].  The host
 * arrays must stay alive until the caller has read the header.
 * Marching cubes under a validity mask (conventions: mvsdf_amd/mesh.py): like mvsdf_mc_count / mvsdf_mc_emit with valid uint8
 * [shape[0]][shape[1]][shape[2]] (contiguous) beside the volume; the workspace starts with MVSDF_MC_H_*.
 * workspace bytes: 6 per grid point + O(points / 1024); 0 = refused. */
enum {
    MVSDF_TS_ERR_FINITE = 1,    /* a non-finite matrix, origin, voxel or trunc, or a NaN jump */
    MVSDF_TS_ERR_VIEW = 2,      /* a view index outside [0, V) */
    MVSDF_TS_ERR_RANGE = 4,     /* voxel <= 0, trunc <= 0, jump < 0 or min_views < 1 */
    MVSDF_TS_ERR_SHAPE = 8      /* V < 1, H or W < 2, H*W > INT32_MAX, nviews < 1, a dim below 2 or above INT32_MAX, more than 2^40 lattice points */
};
size_t mvsdf_tsdf_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t nviews);
int mvsdf_tsdf_integrate(const float* depths, int64_t V, int64_t H, int64_t W, const double* mats, const int32_t* views, int64_t nviews,
                         const double* origin, double voxel, const int64_t* dims, double trunc, double jump, int32_t min_views, void* ws,
                         size_t ws_bytes, float* tsdf, int32_t* weight, uint8_t* valid, void* stream);
size_t mvsdf_mcm_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int mvsdf_mcm_count(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes,
                    void* stream);
int mvsdf_mcm_emit(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, const float* spacing,
                   const float* origin, void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap,
                   void* stream);

/* ---- Plane-sweep stereo (stereo.hip; Python: mvsdf_amd/stereo.py, which states the definition) ----
 * mvsdf_stereo_normalize: feats fp32 [n][C] on the device -> out fp32 [n][C], every texel divided by its fp64 norm (0 where the norm is 0); hdr: 16
 * device bytes that receive MVSDF_RES_H_* (MVSDF_PS_ERR_FINITE: a non-finite feature).  mvsdf_stereo_patches: images uint8 [V][H][W][3] -> out fp32
 * [V][H][W][(2 radius + 1)^2], the mean-free grey patch with a clamped border (0 <= radius <= 15).  Neither waits for the host.
 * mvsdf_stereo_sweep validates every argument on the host, then (no host wait) sweeps the views views[0 .. nviews) in turn over desc fp32
 * [V][R][S][C] (device) and writes, for each of them, depths[view][R][S], probs[view][3][R][S], best_k[view][R][S] (-1: no valid hypothesis) and
 * counts[view][R][S]; other views' outputs are not touched.  It leaves MVSDF_RES_H_* at the start of the workspace.  Error bits: MVSDF_PS_ERR_*; with any but a non-finite descriptor set
 * nothing is launched.  HOST arrays, alive until the caller has read the header: views int32 [nviews]; pair_off int32 [nviews + 1] (pair_off[0] = 0)
 * and pair_src int32 [pair_off[nviews]], the sources of views[i]; mats fp64 [pair_off[nviews]][16], T_rs per pair slot (row-major 4x4); ranges fp64
 * [nviews][2] = {depth_min, interval}; nhyp int32 [nviews].  The workspace (mvsdf_stereo_workspace_bytes with D = the largest nhyp and npairs =
 * pair_off[nviews]; 0 beyond the limits) afterwards holds the last view's score volume, fp64 [D][R][S] with a quiet NaN where a hypothesis is
 * invalid, at byte offset mvsdf_stereo_volume_offset (same arguments). */
enum {
    MVSDF_PS_ERR_FINITE = 1,    /* a non-finite descriptor / feature, matrix entry, depth_min or interval; mvsdf_stereo_regularize: an infinite score */
    MVSDF_PS_ERR_PAIR = 2,      /* a view or pair index outside [0, V) */
    MVSDF_PS_ERR_DEPTHS = 4,    /* a hypothesis count outside [1, MVSDF_PS_MAX_D] */
    MVSDF_PS_ERR_SHAPE = 8,     /* V < 1, R or S < 2, C < 1, R*S > INT32_MAX, R*S*D or V*R*S*C > 2^40, more than MVSDF_PS_MAX_SRC sources for a view */
    MVSDF_PS_ERR_SGM = 16,      /* the regularisation's p1, p2 or paths refused, or a hypothesis count above MVSDF_PS_MAX_D_SGM */
    MVSDF_PS_ERR_BAND = 32,     /* the band's depth_num outside [1, MVSDF_PS_MAX_D_BAND], a step that is not finite and positive, a view listed twice */
    MVSDF_PS_ERR_CENTRE = 64,   /* an infinite centre (found on the device) */
    MVSDF_PS_ERR_CODE = 128,    /* keypoints: a descriptor code outside 0 .. 127 */
    MVSDF_PS_ERR_INDEX = 256,   /* keypoints: a keypoint index outside its view, or offsets that do not ascend */
    MVSDF_PS_ERR_ROUNDS = 512,  /* keypoints: the round limit of the track labelling was reached */
    MVSDF_PS_ERR_BEHIND = 1024  /* bundle adjustment: an active observation's point lies behind its camera (q2 <= 0) at the initial parameters */
};
enum {
    MVSDF_PS_MAX_D = 65535,     /* hypotheses of a sweep */
    MVSDF_PS_MAX_SRC = 255,     /* sources of a view: n_k travels as a byte */
    MVSDF_PS_MAX_D_SGM = 4096,  /* the most hypotheses the regularisation takes */
    MVSDF_PS_MAX_D_BAND = 64,   /* the most hypotheses of a band: the tile's scores and counts are then 36 KB of LDS */
    MVSDF_PS_MAX_ELEMS_LOG2 = 40    /* elements of a score volume or a descriptor array: 2^40 */
};
size_t mvsdf_stereo_workspace_bytes(int64_t R, int64_t S, int64_t D, int64_t npairs);
size_t mvsdf_stereo_volume_offset(int64_t R, int64_t S, int64_t D, int64_t npairs);
int mvsdf_stereo_normalize(const float* feats, int64_t n, int64_t C, float* out, void* hdr, void* stream);
int mvsdf_stereo_patches(const uint8_t* images, int64_t V, int64_t H, int64_t W, int32_t radius, float* out, void* stream);
int mvsdf_stereo_sweep(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views, const int32_t* pair_off,
                       const int32_t* pair_src, const double* mats, const double* ranges, const int32_t* nhyp, void* ws, size_t ws_bytes, float* depths,
                       float* probs, int32_t* best_k, int32_t* counts, void* stream);
/* Semi-global regularisation of a score volume (the definition: mvsdf_amd/stereo.py).  mvsdf_stereo_regularize: score fp64 [D][R][S] on the device
 * (a NaN = an invalid hypothesis) -> out fp64 [D][R][S], the regularised scores A (NaN where the input is); out must not overlap score.  paths is 4 or
 * 8, 0 <= p1 <= p2 finite, R and S >= 1, 1 <= D <= MVSDF_PS_MAX_D_SGM, R*S <= INT32_MAX, R*S*D <= 2^40.  ws: mvsdf_stereo_sgm_workspace_bytes (0
 * beyond the limits) device bytes; they receive MVSDF_RES_H_*: MVSDF_PS_ERR_FINITE an infinite score (out is then not valid), MVSDF_PS_ERR_SGM a
 * refused argument (nothing is launched).  No host wait unless an argument is refused.
 * mvsdf_stereo_sweep_sgm is mvsdf_stereo_sweep with the regularisation between the scores and the pick of every view: the winner, the refinement and
 * prob2 come from A, prob1 is the raw score at the winner, prob3 and counts its n_k.  MVSDF_PS_ERR_SGM: p1, p2 or paths refused, or a hypothesis count
 * above MVSDF_PS_MAX_D_SGM.  Its workspace is mvsdf_stereo_sweep_sgm_workspace_bytes (same arguments as mvsdf_stereo_workspace_bytes); afterwards the last view's raw
 * volume is at mvsdf_stereo_volume_offset and its regularised volume, fp64 [D][R][S], at byte offset mvsdf_stereo_workspace_bytes. */
size_t mvsdf_stereo_sgm_workspace_bytes(int64_t R, int64_t S, int64_t D);
int mvsdf_stereo_regularize(const double* score, int64_t R, int64_t S, int64_t D, double p1, double p2, int32_t paths, void* ws, size_t ws_bytes,
                            double* out, void* stream);
size_t mvsdf_stereo_sweep_sgm_workspace_bytes(int64_t R, int64_t S, int64_t D, int64_t npairs);
int mvsdf_stereo_sweep_sgm(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views,
                           const int32_t* pair_off, const int32_t* pair_src, const double* mats, const double* ranges, const int32_t* nhyp, double p1,
                           double p2, int32_t paths, void* ws, size_t ws_bytes, float* depths, float* probs, int32_t* best_k, int32_t* counts,
                           void* stream);
/* The cascade (mvsdf_amd/stereo.py, "Cascade").  mvsdf_stereo_upsample: depth fp32 [V][r][s] and best_k int32 [V][r][s] of a coarser sweep (device)
 * -> out fp64 [V][R][S], the centres at the finer size (a quiet NaN where no parent of a pixel has a winner); r and s >= 2, R and S >= 1; no host wait.
 * mvsdf_stereo_band is mvsdf_stereo_sweep over a band of depth_num hypotheses (1 .. MVSDF_PS_MAX_D_BAND) per pixel, centres[view][R][S] fp64 on the device
 * (NaN: no centre) + (k - depth_num / 2) * steps[i]: all of views[0 .. nviews) in one launch (1 <= nviews <= 65535, no view twice), no score volume
 * in global memory, best_k = the index within the band.  steps: HOST fp64 [nviews], finite and positive; the other host arrays as
 * mvsdf_stereo_sweep's.  Further error bits: MVSDF_PS_ERR_BAND (nothing is launched) and MVSDF_PS_ERR_CENTRE
 * (the outputs are then not valid).  The workspace (mvsdf_stereo_band_workspace_bytes, 0 beyond the limits) holds the header, the per-view
 * arrays, the matrices and the source indices: it depends on nviews and npairs = pair_off[nviews] only, not on depth_num, R or S. */
int mvsdf_stereo_upsample(const float* depth, const int32_t* best_k, int64_t V, int64_t r, int64_t s, int64_t R, int64_t S, double* out, void* stream);
size_t mvsdf_stereo_band_workspace_bytes(int64_t R, int64_t S, int64_t depth_num, int64_t nviews, int64_t npairs);
int mvsdf_stereo_band(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views, const int32_t* pair_off,
                      const int32_t* pair_src, const double* mats, const double* steps, const double* centres, int32_t depth_num, void* ws,
                      size_t ws_bytes, float* depths, float* probs, int32_t* best_k, int32_t* counts, void* stream);

/* ---- Point-cloud cleaning (cloud.hip; Python: mvsdf_amd/cloud.py, which states the definition) ----
 * pts fp64 [n][3] on the device, fp64 throughout.  mvsdf_cloud_knn, _components and _clean share one workspace (mvsdf_cloud_clean_workspace_bytes,
 * 0 unless 2 <= n <= INT32_MAX) and leave MVSDF_CLOUD_H_* at its start; entries a call does not compute are 0.  Error bits: MVSDF_PC_ERR_FINITE, _ROUNDS (the
 * components loop) and _WALK; with any set nothing else is valid.  Every argument is validated before the first launch;
 * each call waits for the stream once for the coordinate check, _components and _clean once more per round of the components loop (normally one).
 * mvsdf_cloud_knn: d[i] = the mean of sqrt over the k smallest (dx dx + dy dy) + dz dz from point i to every other point (by index), summed in
 * ascending order.  1 <= k <= MVSDF_PC_MAX_K, n >= k + 1.
 * mvsdf_cloud_components: labels[i] = the smallest index in i's connected component under d2 <= eps * eps (every point takes part).
 * mvsdf_cloud_clean: d as above; m = the element of rank (n - 1) / 2 of d; a point passes iff d <= knn_ratio * m; eps = eps_ratio * m; labels over
 * the passed points (-1 elsewhere); keep[i] = 1 iff i passed and its component holds >= cluster_frac * (the largest component's count) points.
 * Ratios finite and > 0, cluster_frac <= 1.
 * mvsdf_cloud_compact (no host wait): the rows with keep != 0 of pts, colors uint8 [n][3], a and b int32 [n] (each of the three may be NULL with
 * its output) in input order; rows at or beyond cap are not written -> MVSDF_ROWS_H_*. */
enum {
    MVSDF_CLOUD_H_PASSED = 0,       /* points that passed the k-NN test */
    MVSDF_CLOUD_H_CLUSTERS = 1,     /* components */
    MVSDF_CLOUD_H_LARGEST = 2,      /* the largest component's count */
    MVSDF_CLOUD_H_KEPT = 3,         /* points kept */
    MVSDF_CLOUD_H_M = 4,            /* m (fp64 bits) */
    MVSDF_CLOUD_H_THRESHOLD = 5,    /* knn_ratio * m (fp64 bits) */
    MVSDF_CLOUD_H_EPS = 6,          /* eps (fp64 bits) */
    MVSDF_CLOUD_H_ROUNDS = 7,       /* rounds of the components loop */
    MVSDF_CLOUD_H_ERR = 8,          /* error bits */
    MVSDF_CLOUD_H_WORDS = 9
};
size_t mvsdf_cloud_clean_workspace_bytes(int64_t n);
size_t mvsdf_cloud_compact_workspace_bytes(int64_t n);
int mvsdf_cloud_knn(const double* pts, int64_t n, int32_t k, void* ws, size_t ws_bytes, double* d, void* stream);
int mvsdf_cloud_components(const double* pts, int64_t n, double eps, void* ws, size_t ws_bytes, int32_t* labels, void* stream);
int mvsdf_cloud_clean(const double* pts, int64_t n, int32_t k, double knn_ratio, double eps_ratio, double cluster_frac, void* ws, size_t ws_bytes,
                      double* d, int32_t* labels, uint8_t* keep, void* stream);
int mvsdf_cloud_compact(const double* pts, const uint8_t* colors, const int32_t* a, const int32_t* b, const uint8_t* keep, int64_t n, void* ws,
                        size_t ws_bytes, double* out_pts, uint8_t* out_colors, int32_t* out_a, int32_t* out_b, int64_t cap, void* stream);

/* ---- Mesh rendering (raster.hip; Python: mvsdf_amd/raster.py, which states the definition) ----
 * A triangle mesh (verts fp32 [nv][3], faces int32 [nf][3], on the device) drawn into `views` cameras of H x W pixels.  P: fp64 [views][4][4] on the
 * DEVICE, world -> pixels, rows 0..2 used, row 2 the camera depth; pixel (x, y) has its centre at (x + pixel_center, y + pixel_center), pixel_center
 * 0.5 or 0.0.  fp64 throughout, no clipping (a face with a vertex not in front of its camera is skipped), no back-face culling.
 * mvsdf_raster_draw fills the workspace's key buffer (mvsdf_raster_workspace_bytes; 0 unless 0 <= nv, nf <= INT32_MAX, 1 <= views <= MVSDF_RA_MAX_VIEWS, H and W
 * >= 2, H * W and nf * views <= INT32_MAX, views * H * W <= 2^40): per pixel the minimum of (bits(fp32 depth) << 32) | face id over the faces that
 * cover the pixel centre, so the result does not depend on the schedule.  Faces whose clamped pixel box holds more than large_face_pixels pixels
 * are compacted to a list and drawn by one wave each; the others by one lane each.  flags: 1 = issue every atomic (no plain-load test before it),
 * 2 = count the atomics issued and the covered pixels (measurement builds of the call; slower).  The workspace starts with MVSDF_RA_H_*.
 * Error bits: MVSDF_RA_ERR_*; with any set nothing else is valid.  A chunk of the views is drawn by passing P + 16 * first.
 * mvsdf_raster_resolve (same workspace, views, H, W) writes depth fp32 [views][H][W] (0 where nothing was drawn) and face int32 (-1).
 * mvsdf_raster_visibility: vis uint8 [views][nv] = the vertex is in front, the pixel whose centre is nearest lies in the image, holds a depth
 * D > 0 with z <= D * (1 + depth_tol), and (masks uint8 [views][H][W] or NULL) its mask is set.  The workspace is its 256-byte header (MVSDF_RA_H_ERR: MVSDF_RA_ERR_FINITE).
 * mvsdf_raster_colors: per vertex, over the views in order, where visible as above: weight (n . g) / |g| with g = centers[v] - X (fp64 [views][3] on
 * the device) if above cos_min, a zero normal weighing 1 with ignore_normals and skipping the vertex without; images uint8 [views][H][W][3]
 * sampled bilinearly at (sx - pixel_center, sy - pixel_center); colors fp32 [nv][3] = sum / weights / 255 or the fallback, n_views int32 [nv] the
 * views that contributed.  No call waits for the host. */
enum {
    MVSDF_RA_H_ERR = 0,         /* error bits */
    MVSDF_RA_H_ITEMS = 1,       /* listed (face, view) items */
    MVSDF_RA_H_ATOMICS = 2,     /* atomics issued (flags 2) */
    MVSDF_RA_H_COVERED = 3,     /* covered pixels (flags 2) */
    MVSDF_RA_H_WORDS = 4
};
enum {
    MVSDF_RA_ERR_FINITE = 1,    /* a camera entry is NaN or infinite */
    MVSDF_RA_ERR_INDEX = 2      /* a face refers to a vertex outside [0, nv) (such a face is not drawn) */
};
enum {
    MVSDF_RA_MAX_VIEWS = 65535,     /* cameras of a raster or texture call */
    MVSDF_RA_MAX_PIXELS_LOG2 = 40   /* views * H * W: 2^40 */
};
size_t mvsdf_raster_workspace_bytes(int64_t nv, int64_t nf, int64_t views, int64_t H, int64_t W);
int mvsdf_raster_draw(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, const double* P, int64_t views, int64_t H, int64_t W,
                      double pixel_center, int64_t large_face_pixels, int32_t flags, void* ws, size_t ws_bytes, void* stream);
int mvsdf_raster_resolve(int64_t views, int64_t H, int64_t W, void* ws, size_t ws_bytes, float* depth, int32_t* face, void* stream);
int mvsdf_raster_visibility(const float* verts, int64_t nv, const double* P, int64_t views, int64_t H, int64_t W, double pixel_center,
                            const float* depth, const uint8_t* masks, double depth_tol, void* ws, size_t ws_bytes, uint8_t* vis, void* stream);
int mvsdf_raster_colors(const float* verts, const float* normals, int64_t nv, const double* P, const double* centers, int64_t views, int64_t H,
                        int64_t W, double pixel_center, const float* depth, const uint8_t* masks, const uint8_t* images, double depth_tol,
                        double cos_min, int32_t ignore_normals, float fallback_r, float fallback_g, float fallback_b, void* ws, size_t ws_bytes,
                        float* colors, int32_t* n_views, void* stream);

/* ---- Texture atlases (texture.hip; Python: mvsdf_amd/texture.py, which states the definition) ----
 * A texture image for a mesh from the photographs: every face labelled with the view that sees it largest, one patch per face (a half of a square
 * cell of edge n = 4 << class, class 0 .. 6) packed along a Morton curve over blocks of 4 x 4 texels, the classes in descending order, and the
 * texels filled by an affine copy of the face's image triangle.  Mesh, P, centers, depth, masks, images and pixel_center as in the raster calls,
 * all on the device; fp64 throughout; 0 <= nf <= 2^MVSDF_TX_MAX_FACES_LOG2.  Every call starts by zeroing the 256-byte header of its workspace; no call waits.
 * mvsdf_texture_face_views: label int32 [nf] (-1: no view), score fp64 [nf] (|A| in that view, 0 without one) and screen fp64 [nf][6] (sx, sy of
 * the three corners in that view, 0 without one).  Header: MVSDF_TX_H_ERR: MVSDF_TX_ERR_FINITE, MVSDF_TX_ERR_INDEX (the face stays
 * unlabelled).
 * mvsdf_texture_classify: cls uint8 [nf] at a texel density (finite, > 0).  Header: the seven words from MVSDF_TX_H_COUNTS.
 * The atlas follows from the counts alone: T = sum over the classes of ceil(count / 2) * 4^class blocks, B the smallest integer with T <= 2^B,
 * Wt = 4 << ceil(B / 2) by Ht = 4 << floor(B / 2) texels; Wt beyond MVSDF_TX_MAX_SIDE is refused.
 * mvsdf_texture_pack (workspace: mvsdf_texture_workspace_bytes(nf), 0 beyond the limit; counts int64 [7] on the HOST, as classify left them): order int32
 * [nf] (the faces by class descending, index ascending), patch int32 [nf][4] = {x0, y0, n, half}, uv fp32 [nf][3][2].  Header: MVSDF_TX_H_ERR, the flagged total behind it:
 * MVSDF_TX_ERR_COUNTS (nothing else is valid).
 * mvsdf_texture_fill: texture uint8 [Ht][Wt][3] and valid uint8 [Ht][Wt] of the atlas those counts give (another Ht x Wt is refused), both
 * 4-byte aligned; texels nobody owns, and those of
 * unlabelled faces, get the fallback (each 0 .. 255) and valid 0.  flags 1: the screen coordinates are projected again from verts / faces / P
 * (the same bits) instead of read from `screen`; without it verts, faces and P may be NULL. */
enum {
    MVSDF_TX_H_ERR = 0,         /* error bits */
    MVSDF_TX_H_COUNTS = 1,      /* mvsdf_texture_classify: the faces per class, seven words; mvsdf_texture_pack: the flagged total in the first */
    MVSDF_TX_H_WORDS = 8
};
enum {                          /* bits 1 and 2 are MVSDF_RA_ERR_*'s */
    MVSDF_TX_ERR_FINITE = 1,    /* a camera or centre entry is NaN or infinite */
    MVSDF_TX_ERR_INDEX = 2,     /* a face refers to a vertex outside [0, nv) */
    MVSDF_TX_ERR_COUNTS = 4,    /* the class counts passed to the pack are not those of cls; seams: the counts passed to mvsdf_seams_graph are not the header's */
    MVSDF_TX_ERR_LABEL = 8,     /* seams, charts: a face label outside [-1, V), or a node's view outside [0, V) */
    MVSDF_TX_ERR_ROUNDS = 16    /* charts: the components did not settle within MVSDF_CA_MAX_ROUNDS rounds */
};
enum {
    MVSDF_TX_MAX_SIDE = 32768,      /* texels: block coordinates fit 13 bits, block indices 26 */
    MVSDF_TX_MAX_FACES_LOG2 = 28    /* faces: 2^28 */
};
size_t mvsdf_texture_workspace_bytes(int64_t nf);
int mvsdf_texture_face_views(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                             const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                             double depth_tol, double cos_min, int32_t ignore_normals, void* ws, size_t ws_bytes, int32_t* label, double* score,
                             double* screen, void* stream);
int mvsdf_texture_classify(const int32_t* label, const double* screen, int64_t nf, double density, void* ws, size_t ws_bytes, uint8_t* cls,
                           void* stream);
int mvsdf_texture_pack(const uint8_t* cls, int64_t nf, const int64_t* counts, void* ws, size_t ws_bytes, int32_t* order, int32_t* patch, float* uv,
                       void* stream);
int mvsdf_texture_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, double pixel_center, const int32_t* label, const double* screen,
                       const int32_t* order, int64_t nf, const int64_t* counts, const float* verts, const int32_t* faces, int64_t nv, const double* P,
                       int32_t flags, int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, int64_t Ht, int64_t Wt, uint8_t* texture,
                       uint8_t* valid, void* stream);

/* ---- Seam levelling of a texture atlas (seams.hip, the fill in texture.hip; Python: mvsdf_amd/seams.py, which states the definition) ----
 * An additive colour correction g per node = (vertex, view) pair that a labelled face's corner makes, so that the corrected colours agree where
 * labels meet.  All on the device, fp64, no call waits.  Every workspace starts with the MVSDF_SL_H_* words (256 bytes); error bits are
 * MVSDF_TX_ERR_*.  Every call but mvsdf_seams_graph starts by zeroing that header.  mvsdf_seams_workspace_bytes(nf, nv, views, nodes): what
 * the node / graph calls need for nf faces and the solve for `nodes` nodes, whichever is more (0 beyond the limits).
 * mvsdf_seams_nodes: corner_node int32 [nf][3] (-1 on unlabelled faces); header: MVSDF_SL_H_NODES = K, MVSDF_SL_H_NNZ = the adjacency entries;
 * MVSDF_TX_ERR_INDEX (a vertex id outside [0, nv)), MVSDF_TX_ERR_LABEL (a label outside [-1, views)); such a face counts as unlabelled.
 * mvsdf_seams_graph: with the SAME workspace, untouched since mvsdf_seams_nodes, and the K and nnz read from it: node_vertex, node_view int32 [K],
 * adj_off int64 [K + 1], adj_seam int32 [K] (the leading entries of a node's list that are seam partners), adj_node int32 [nnz].
 * MVSDF_TX_ERR_COUNTS: K or nnz are not the header's, or corner_node is not the one written (nothing else is valid).
 * mvsdf_seams_colors: f fp64 [K][3]; MVSDF_TX_ERR_FINITE (P or a node's vertex), _INDEX (a node's vertex id), _LABEL (a node's view).
 * mvsdf_seams_apply: out [K][3] = A x.  mvsdf_seams_solve: g [K][3]; header: per channel MVSDF_SL_H_ITERS + c, the final rho (fp64 bits) at
 * MVSDF_SL_H_RHO + c and the first at MVSDF_SL_H_RHO0 + c; cg_iters in [0, MVSDF_SL_MAX_CG], cg_tol >= 0, smoothness >= 0, anchor > 0, all finite.
 * Both raise MVSDF_TX_ERR_INDEX for an offset, a seam count or an entry out of range (such an entry is skipped).
 * mvsdf_seams_fill: mvsdf_texture_fill (from the screen table) with the correction of the face's three nodes blended by the texel's barycentric
 * weights; MVSDF_TX_ERR_INDEX: a labelled face's corner_node outside [0, K) (its texels stay uncorrected). */
enum {
    MVSDF_SL_H_ERR = 0,         /* error bits */
    MVSDF_SL_H_NODES = 1,       /* mvsdf_seams_nodes: K */
    MVSDF_SL_H_NNZ = 2,         /* mvsdf_seams_nodes: adjacency entries */
    MVSDF_SL_H_ITERS = 3,       /* the solve, three words each, one per colour channel: iterations run */
    MVSDF_SL_H_RHO = 6,         /* r . z, fp64 bits */
    MVSDF_SL_H_RHO0 = 9,        /* the first r . z, fp64 bits */
    MVSDF_SL_H_DONE = 12,       /* the channel has ended */
    MVSDF_SL_H_SIGMA = 15,      /* p . A p of the running iteration, fp64 bits */
    MVSDF_SL_H_RHON = 18,       /* r . z of the running iteration, fp64 bits */
    MVSDF_SL_H_WORDS = 21
};
enum {
    MVSDF_SL_MAX_CG = 100000    /* iterations of one solve */
};
size_t mvsdf_seams_workspace_bytes(int64_t nf, int64_t nv, int64_t views, int64_t nodes);
int mvsdf_seams_nodes(const int32_t* faces, const int32_t* label, int64_t nv, int64_t nf, int64_t views, void* ws, size_t ws_bytes,
                      int32_t* corner_node, void* stream);
int mvsdf_seams_graph(int64_t nv, int64_t nf, int64_t views, int64_t nodes, int64_t nnz, const int32_t* corner_node, void* ws, size_t ws_bytes,
                      int32_t* node_vertex, int32_t* node_view, int64_t* adj_off, int32_t* adj_seam, int32_t* adj_node, void* stream);
int mvsdf_seams_colors(const int32_t* node_vertex, const int32_t* node_view, int64_t nodes, const float* verts, int64_t nv, const double* P,
                       int64_t views, int64_t H, int64_t W, double pixel_center, const uint8_t* images, void* ws, size_t ws_bytes, double* f,
                       void* stream);
int mvsdf_seams_apply(const int64_t* adj_off, const int32_t* adj_seam, const int32_t* adj_node, int64_t nodes, int64_t nnz, const double* x,
                      double smoothness, double anchor, void* ws, size_t ws_bytes, double* out, void* stream);
int mvsdf_seams_solve(const int64_t* adj_off, const int32_t* adj_seam, const int32_t* adj_node, int64_t nodes, int64_t nnz, const double* f,
                      double smoothness, double anchor, int32_t cg_iters, double cg_tol, void* ws, size_t ws_bytes, double* g, void* stream);
int mvsdf_seams_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, double pixel_center, const int32_t* label, const double* screen,
                     const int32_t* order, int64_t nf, const int64_t* counts, const int32_t* corner_node, const double* g, int64_t nodes,
                     int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, void* ws, size_t ws_bytes, int64_t Ht, int64_t Wt, uint8_t* texture,
                     uint8_t* valid, void* stream);

/* ---- Chart atlases (charts.hip; Python: mvsdf_amd/charts.py, which states the definition) ----
 * A chart is a connected region of faces with one label; its patch is a rectangle cut from that view's photograph with a margin of `pad` texels
 * (1, 2, 4 or 8).  All on the device, fp64.  Every workspace starts with the MVSDF_CA_H_* words (256 bytes), which every call zeroes first; error
 * bits are MVSDF_TX_ERR_*.  mvsdf_charts_workspace_bytes(nf, texels): what every call needs for nf faces, and mvsdf_charts_face_map for an atlas of
 * `texels` texels (0 beyond the limits).  Only mvsdf_charts_components waits (it reads one word per MVSDF_CA_ROUND_BATCH rounds).
 * mvsdf_charts_face_scores: texture.hip's test of face f in the one view view[f] -> score fp64 [nf] (|A|, 0 where the view is no candidate or -1),
 * screen fp64 [nf][6].  MVSDF_TX_ERR_INDEX (a vertex id), _LABEL (a view outside [-1, views)), _FINITE; such a face scores 0.
 * mvsdf_charts_neighbors: nbr int32 [nf][3], across edge e (corners e, (e + 1) % 3) the other face, -1 unless exactly two of the 3 nf edges join these
 * two different vertex ids and belong to two faces.  MVSDF_TX_ERR_INDEX: a vertex id outside [0, nv) (its edges have no neighbour).
 * mvsdf_charts_components: face_chart int32 [nf] (-1: unlabelled), and in the first C entries of chart_view and chart_faces int32 [nf] each chart's
 * label and faces; charts ascending by their lowest face.  Header: MVSDF_CA_H_CHARTS = C.  MVSDF_TX_ERR_LABEL (a label below -1: unlabelled),
 * _INDEX (a neighbour outside [-1, nf): none), _ROUNDS.
 * mvsdf_charts_absorb: one round of the absorption of charts with fewer than min_faces faces: label_out int32 [nf]; score and screen are updated
 * where a label changed.  Header: MVSDF_CA_H_CHANGES.
 * mvsdf_charts_pack: chart_rect int32 [C][6] = {X, Y, w, h, u0, t0}, order int32 [C] (the charts by h descending, id ascending), xs int32 [C] (X by
 * place in that order) and shelves int32 [C + 1][2] = {first place, Y}, entry MVSDF_CA_H_SHELVES = {C, Ht}.  Header: MVSDF_CA_H_WT, _HT, _SHELVES,
 * _AREA, _MAXW, _MAXH.  MVSDF_TX_ERR_INDEX: a face's chart outside [-1, C); MVSDF_TX_ERR_COUNTS: a chart without a face.
 * mvsdf_charts_uv: uv fp32 [nf][3][2].  mvsdf_charts_face_map: face_map int32 [Ht][Wt], the lowest covering face, dilated `pad` rounds.
 * mvsdf_charts_fill: texture uint8 [Ht][Wt][3] and valid uint8 [Ht][Wt] (both 4-byte aligned, Wt a multiple of 4); with face_map (else NULL, and
 * the arguments from face_chart to nodes unused) the correction g fp64 [nodes][3] of the face's three nodes is added before the rounding.
 * MVSDF_TX_ERR_INDEX: an entry of the tables, of face_map or of corner_node out of range (the texel gets the fallback, or stays uncorrected). */
enum {
    MVSDF_CA_H_ERR = 0,         /* error bits */
    MVSDF_CA_H_CHARTS = 1,      /* mvsdf_charts_components: C */
    MVSDF_CA_H_CHANGES = 2,     /* mvsdf_charts_absorb: the labels that changed */
    MVSDF_CA_H_WT = 3,          /* mvsdf_charts_pack: the atlas */
    MVSDF_CA_H_HT = 4,
    MVSDF_CA_H_SHELVES = 5,     /* shelves */
    MVSDF_CA_H_AREA = 6,        /* the sum of w * h */
    MVSDF_CA_H_MAXW = 7,        /* the largest w and h */
    MVSDF_CA_H_MAXH = 8,
    MVSDF_CA_H_ROUNDS = 9,      /* mvsdf_charts_components: the rounds enqueued */
    MVSDF_CA_H_WORDS = 10
};
enum {
    MVSDF_CA_MAX_ROUNDS = 64,       /* hook-and-jump rounds of the components */
    MVSDF_CA_ROUND_BATCH = 8,       /* rounds between two reads of the settled word */
    MVSDF_CA_RECT_CAP = 65536,      /* the cap of a rectangle's side: 2 * MVSDF_TX_MAX_SIDE, a multiple of every pad */
    MVSDF_CA_LARGE_FACE = 256       /* texels in a face's box above which a wave draws it into the face map */
};
size_t mvsdf_charts_workspace_bytes(int64_t nf, int64_t texels);
int mvsdf_charts_face_scores(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                             const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                             double depth_tol, double cos_min, int32_t ignore_normals, const int32_t* view, void* ws, size_t ws_bytes, double* score,
                             double* screen, void* stream);
int mvsdf_charts_neighbors(const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, int32_t* nbr, void* stream);
int mvsdf_charts_components(const int32_t* label, const int32_t* nbr, int64_t nf, void* ws, size_t ws_bytes, int32_t* face_chart,
                            int32_t* chart_view, int32_t* chart_faces, void* stream);
int mvsdf_charts_absorb(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                        const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                        double depth_tol, double cos_min, int32_t ignore_normals, const int32_t* label, const int32_t* nbr, const int32_t* face_chart,
                        const int32_t* chart_faces, int64_t charts, int64_t min_faces, void* ws, size_t ws_bytes, int32_t* label_out, double* score,
                        double* screen, void* stream);
int mvsdf_charts_pack(const int32_t* face_chart, const double* screen, int64_t nf, int64_t charts, double pixel_center, int64_t H, int64_t W,
                      double density, int32_t pad, void* ws, size_t ws_bytes, int32_t* chart_rect, int32_t* order, int32_t* xs, int32_t* shelves,
                      void* stream);
int mvsdf_charts_uv(const int32_t* face_chart, const double* screen, int64_t nf, const int32_t* chart_rect, int64_t charts, double pixel_center,
                    double density, int32_t pad, int64_t Ht, int64_t Wt, void* ws, size_t ws_bytes, float* uv, void* stream);
int mvsdf_charts_face_map(const int32_t* face_chart, const double* screen, int64_t nf, double pixel_center, const int32_t* chart_rect,
                          const int32_t* order, const int32_t* xs, const int32_t* shelves, int64_t charts, int64_t nshelves, double density,
                          int32_t pad, int64_t Ht, int64_t Wt, void* ws, size_t ws_bytes, int32_t* face_map, void* stream);
int mvsdf_charts_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, const int32_t* chart_view, const int32_t* chart_rect,
                      const int32_t* order, const int32_t* xs, const int32_t* shelves, int64_t charts, int64_t nshelves, double density, int32_t pad,
                      int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, int64_t Ht, int64_t Wt, const int32_t* face_map,
                      const int32_t* face_chart, const double* screen, double pixel_center, int64_t nf, const int32_t* corner_node, const double* g,
                      int64_t nodes, void* ws, size_t ws_bytes, uint8_t* texture, uint8_t* valid, void* stream);

/* ---- MVS feature extraction (featext.hip; Python: mvsdf_amd/features.py, which states the network) ----
 * Inference of the Vis-MVSNet feature CNN FeatExt on NHWC fp32 activations, eval-mode BatchNorm folded into the weights at pack time.
 * raw: fp32 [mvsdf_featext_raw_floats()] on the device, the layers in the order of mvsdf_amd/features.py::LAYERS, each its weight in PyTorch layout
 * (Conv2d [cout][cin][k][k], ConvTranspose2d [cin][cout][k][k]) followed, where the layer has one, by its BatchNorm's weight, bias, running_mean and
 * running_var.  mvsdf_featext_pack writes the folded weights to packed (mvsdf_featext_pack_bytes(), 256-byte aligned), stream-ordered.
 * mvsdf_featext_forward: x NHWC [n][h][w][3]; ceil(h / 2) and ceil(w / 2) must be multiples of 4, else the workspace query gives 0.  out1 / out2 /
 * out3 (NHWC, 32 channels, at ceil(h / 2) / 4, / 2 and / 1; each may be NULL) = final_conv_1/2/3 of the network.  Runs the stages
 * [first_stage, last_stage) of 0 init_conv, 1..3 the encoder stages, 4..5 the decoder stages, 6 the heads (0, 7 = all); the workspace carries the
 * activations between calls.  No host wait.  Results do not depend on n or on the call (no atomics). */
size_t mvsdf_featext_raw_floats(void);
size_t mvsdf_featext_pack_bytes(void);
int mvsdf_featext_pack(const float* raw, void* packed, size_t packed_bytes, void* stream);
size_t mvsdf_featext_workspace_bytes(int64_t n, int64_t h, int64_t w);
int mvsdf_featext_forward(const float* packed, const float* x, int64_t n, int64_t h, int64_t w, void* ws, size_t ws_bytes, float* out1, float* out2,
                          float* out3, int first_stage, int last_stage, void* stream);
/* One layer alone: kind 0 = Conv2d(k in {1, 3, 5}, stride in {1, 2}, padding k / 2), kind 1 = ConvTranspose2d(3, 2, 1, output_padding 1); no
 * BatchNorm.  weight: PyTorch layout over c1 + c2 input channels; bias [cout] or NULL; x1 NHWC [n][h][w][c1], x2 NHWC [n][h][w][c2] (read as the
 * channels after x1's; c2 = 0: none); res NHWC [n][ho][wo][cout] or NULL; out = relu?(conv + bias + res) NHWC.  cout in {16, 32, 64, 128}; c1 and c2
 * multiples of 16, or c2 = 0, kind 0 and cout <= 32.  The workspace holds the packed weights (0 from the query: unsupported). */
size_t mvsdf_featext_layer_workspace_bytes(int kind, int cin, int cout, int k, int stride);
int mvsdf_featext_layer(int kind, const float* weight, const float* bias, int cout, int k, int stride, const float* x1, int c1, const float* x2, int c2,
                        int64_t n, int64_t h, int64_t w, const float* res, int relu, void* ws, size_t ws_bytes, float* out, void* stream);


/* ---- View selection (viewsel.hip; Python: mvsdf_amd/viewsel.py, which states the definition) ----
 * The pairwise score behind pair.txt from points fp64 [P][3], camera centres fp64 [V][3] and visibility, all on the device; fp64 throughout with the
 * written-out atan2 / exp of csrc/det_math64.h.  1 <= V <= MVSDF_VS_MAX_VIEWS, 0 <= P <= INT32_MAX.  hdr: 256 device bytes, MVSDF_RES_H_*; the two pack
 * calls reset it, the other calls OR into it, and the caller reads it once at the end.  Error bits: MVSDF_VS_ERR_*.
 * mvsdf_viewsel_pack_dense: vis uint8 [V][P] (non-zero = seen) -> bits uint64 [P][ceil(V / 64)] (mvsdf_viewsel_bits_bytes; 0 beyond the limits), bit
 * v mod 64 of word v / 64 of row p.  mvsdf_viewsel_pack_tracks: the same from CSR tracks, track_off int64 [P + 1] and track_view int32 [nnz]; a
 * duplicate entry counts once.
 * mvsdf_viewsel_scores: scores fp64 [V][V] (symmetric, zero diagonal) and counts int64 [V][V] (common points; the diagonal: the points a view sees);
 * the workspace (mvsdf_viewsel_workspace_bytes) holds the int64 sums of the quantised weights.  theta0 finite, sigma1 and sigma2 finite and > 0.
 * mvsdf_viewsel_depths: z fp64 [nviews][P] for the views first .. first + nviews: ((e0*x + e1*y) + e2*z) + e3 with e = ext_row2[v] (fp64 [V][4] on the
 * device, row 2 of the extrinsic) where view v sees the point, +inf elsewhere.  P >= 1.  No call waits for the host (but for MVSDF_VS_ERR_SHAPE).
 * mvsdf_viewsel_weights_host is a HOST function (no GPU needed): theta [n] in degrees and the quantised weight wq [n] of the definition for n pairs
 * of vectors a = c_i - p, b = c_j - p (fp64 [n][3], host memory), evaluated by the functions the kernel runs. */
enum {
    MVSDF_VS_ERR_FINITE = 1,    /* a non-finite point, centre or extrinsic entry */
    MVSDF_VS_ERR_TRACK = 2,     /* a track entry outside [0, V) (or track offsets that do not ascend within [0, nnz]) */
    MVSDF_VS_ERR_SHAPE = 4      /* V or P outside the limits above (nothing is launched) */
};
enum { MVSDF_VS_MAX_VIEWS = 65535 };    /* views of a visibility bit matrix (view selection, normals) */
size_t mvsdf_viewsel_bits_bytes(int64_t V, int64_t P);
size_t mvsdf_viewsel_workspace_bytes(int64_t V);
int mvsdf_viewsel_pack_dense(const uint8_t* vis, int64_t V, int64_t P, void* bits, void* hdr, void* stream);
int mvsdf_viewsel_pack_tracks(const int64_t* track_off, const int32_t* track_view, int64_t nnz, int64_t V, int64_t P, void* bits, void* hdr,
                              void* stream);
int mvsdf_viewsel_scores(const double* points, const double* centers, const void* bits, int64_t V, int64_t P, double theta0, double sigma1,
                         double sigma2, void* ws, size_t ws_bytes, double* scores, int64_t* counts, void* hdr, void* stream);
int mvsdf_viewsel_depths(const double* points, const void* bits, const double* ext_row2, int64_t V, int64_t P, int64_t first, int64_t nviews,
                         double* z, void* hdr, void* stream);
int mvsdf_viewsel_weights_host(const double* a, const double* b, int64_t n, double theta0, double sigma1, double sigma2, double* theta, int64_t* wq);

/* ---- Image undistortion (undistort.hip; Python: mvsdf_amd/undistort.py, which states the definition) ----
 * COLMAP's distorted camera models to pinhole views; fp64 throughout, the fisheye atan2 the written-out one of csrc/det_math64.h.  model: 0 no
 * distortion, 1 radial (k1, k2), 2 OpenCV (k1, k2, p1, p2, k3, k4, k5, k6), 3 fisheye (k1 .. k4).  params: HOST fp64 [12] = fx, fy, cx, cy of the
 * distorted camera and the model's coefficients, the unused ones 0.  pinhole / out_pinhole: HOST fp64 [4] = fx, fy, cx, cy of the undistorted view.
 * Every value must be finite and the focal lengths > 0.
 * mvsdf_undistort_points: points fp64 [n][2] on the device.  inverse != 0: source pixels -> pixels of the pinhole through the Newton iteration of the
 * inverse map; inverse == 0: pixels of the pinhole -> source pixels through the forward map.  hdr: 256 device bytes, MVSDF_RES_H_*, reset by
 * the call and read by the caller; error bits: MVSDF_UD_ERR_*.
 * mvsdf_undistort_images: src [views][H][W][C] -> dst [views][oH][oW][C] on the device, C in 1 .. 4, dtype 0 uint8 or 1 float32, bilinear; pixels that
 * look outside the source are 0.  mask: uint8 [oH][oW] (1 = looks inside) or NULL.  Sides up to 2^24; all offsets are 64-bit.  No call waits.
 * The _host functions run the same arithmetic on the CPU over host memory (no GPU needed); *err receives the error bits. */
enum {
    MVSDF_UD_ERR_FINITE = 1,    /* a non-finite value or a zero determinant */
    MVSDF_UD_ERR_CONVERGE = 2   /* an iteration that ended above 1e-10 px */
};
int mvsdf_undistort_points(const double* points, int64_t n, int model, const double* params, const double* pinhole, int inverse, double* out, void* hdr,
                           void* stream);
int mvsdf_undistort_images(const void* src, int64_t views, int64_t H, int64_t W, int64_t C, int dtype, int model, const double* params,
                           const double* out_pinhole, int64_t oH, int64_t oW, void* dst, uint8_t* mask, void* stream);
int mvsdf_undistort_points_host(const double* points, int64_t n, int model, const double* params, const double* pinhole, int inverse, double* out,
                                int64_t* err);
int mvsdf_undistort_images_host(const void* src, int64_t views, int64_t H, int64_t W, int64_t C, int dtype, int model, const double* params,
                                const double* out_pinhole, int64_t oH, int64_t oW, void* dst, uint8_t* mask);

/* ---- Training batches assembled on the device (batch_kernels.hip; Python: mvsdf_amd/datasets/device_batches.py) ----
 * One launch builds the whole step batch of SceneDataset.__getitem__ + collate_fn (mvsdf_amd/datasets/scene_dataset.py) for B views from pools that
 * stay on the device for the whole run: per view b (v = views[b]) and per sampled pixel p (id = pix[p], or p itself when pix is NULL: full images)
 *   rgb[b][p][3] = rgb_pool[v][id][3]; uv[b][p] = (id mod img_w, id div img_w) as floats; object_mask[b][p] = omask_pool[v][id] (perfect_mask likewise,
 *   skipped when either pointer is NULL); pose / intrinsics [b][4][4]; cam [b][2][4][4] = cams_hd[v]; src_cams [b][s] = cams_hd[src[v][s]];
 *   depths [b][1][dh][dw] and depth_cams [b][2][4][4] of the view itself (sel_depth_num = 1); size [b] and center [b][3] = the scene's.
 * The feature maps: feats is the [n][32][fh][fw] pool in channels-last storage ([n][fh][fw][32] in memory), feat [b] = feats[v] and
 * feat_src [b][s] = feats[src[v][s]] in the same storage, i.e. one contiguous block of fmap_floats = 32 fh fw per map: copied with 16-byte loads and
 * stores (every map pointer 16-byte aligned, fmap_floats a multiple of 4).  Masks are bytes (torch.bool); ids int64.  View and pixel ids outside
 * the pools leave their outputs unwritten.  No host wait, no allocation. */
typedef struct {
    int B, n, num_src;
    int64_t P, img_w, total_pixels, depth_floats, fmap_floats;
    const int64_t* views;                /* [B] */
    const int64_t* pix;                  /* [P], or NULL: P == total_pixels, the whole image */
    const int64_t* src;                  /* [n][num_src] source views (pair.txt) */
    const float* rgb;                    /* [n][total_pixels][3] */
    const uint8_t* omask;                /* [n][total_pixels] */
    const uint8_t* pmask;                /* [n][total_pixels] or NULL */
    const float* pose;                   /* [n][4][4] */
    const float* intrinsics;             /* [n][4][4] */
    const float* cams_hd;                /* [n][2][4][4] */
    const float* depth_cams;             /* [n][2][4][4] */
    const float* depths;                 /* [n][depth_floats] */
    const float* size;                   /* [1] */
    const float* center;                 /* [3] */
    const float* feats;                  /* [n][fmap_floats] */
    float* o_rgb; float* o_uv; uint8_t* o_omask; uint8_t* o_pmask;
    float* o_pose; float* o_intrinsics; float* o_cam; float* o_src_cams; float* o_depths; float* o_depth_cams; float* o_size; float* o_center;
    float* o_feat;                       /* [B][fmap_floats] */
    float* o_feat_src;                   /* [B][num_src][fmap_floats] */
} MvsdfBatchArgs;
size_t mvsdf_batch_args_bytes(void);     /* sizeof(MvsdfBatchArgs) as compiled: the binding checks its mirror against it */
int mvsdf_batch_gather(const MvsdfBatchArgs* a, void* stream);

/* ---- Registration and F-score evaluation (registration.hip; Python: mvsdf_amd/registration.py, which states the definitions) ----
 * Points are fp64 [n][3] on the device; fp64 throughout, no contraction, every sum in a written order.  Error bits: MVSDF_PC_ERR_FINITE,
 * _COORD (a voxel index of 2^21 or more) and _WALK.
 * The kept tree: mvsdf_reg_tree_build sorts refs [nr][3] by Morton code and builds the box tree once, inside the workspace
 * (mvsdf_reg_tree_workspace_bytes; 0 unless 1 <= nr <= INT32_MAX).  It waits for the stream once (the coordinate check) and leaves
 * MVSDF_REG_TREE_H_* at the start of the workspace, which IS the tree from then on: keep it, pass it as `tree`.
 * mvsdf_reg_tree_query (no host wait): per query q (first moved by transform, HOST fp64 [16] row-major or NULL, row a =
 * ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]) the minimum of (dx dx + dy dy) + dz dz over the references and the smallest input index that
 * attains it: index int32 [nq], d2 (the minimum) and dist (its sqrt), each fp64 [nq] or NULL.  Where sqrt(d2) is not < max_dist (> 0, may be
 * +inf): dist = d2 = +inf, index = -1.  Error bits are ORed into the device word *err (the caller zeroes it), with them nothing else is valid.
 * mvsdf_reg_icp_step: that query of src under transform, then the 17 sums of one ICP iteration over the matched pairs in source order (a lane sums
 * 8 consecutive items from 0, a 256-lane halving tree, block partials, a 1024-lane final): with c the tree's centre, p = T src - c and
 * q = refs[index] - c (refs: the array the tree was built from).  Waits for the stream -> MVSDF_REG_ICP_H_* at the start of the workspace
 * (mvsdf_reg_pairs_workspace_bytes(ns), ns >= 1). */
enum {
    MVSDF_REG_TREE_H_ERR = 0,       /* error bits */
    MVSDF_REG_TREE_H_CENTRE = 1,    /* the centre of the references' box: 3 fp64 as bits */
    MVSDF_REG_TREE_H_WORDS = 4
};
enum {
    MVSDF_REG_ICP_H_N = 0,          /* matched pairs */
    MVSDF_REG_ICP_H_SUMS = 1,       /* 16 fp64 as bits: sum d2, sum p [3], sum q [3], sum p_a q_b [9] (a major) */
    MVSDF_REG_ICP_H_ERR = 17,       /* error bits */
    MVSDF_REG_ICP_H_WORDS = 18
};
enum {
    MVSDF_REG_VOXEL_H_VOXELS = 0,   /* occupied voxels */
    MVSDF_REG_VOXEL_H_ERR = 1,      /* error bits */
    MVSDF_REG_VOXEL_H_WORDS = 2
};
enum { MVSDF_REG_MAX_POLYGON = 4096 };  /* vertices of mvsdf_reg_crop's polygon */
size_t mvsdf_reg_tree_workspace_bytes(int64_t nr);
int mvsdf_reg_tree_build(const double* refs, int64_t nr, void* ws, size_t ws_bytes, void* stream);
int mvsdf_reg_tree_query(const void* tree, size_t tree_bytes, int64_t nr, const double* queries, int64_t nq, const double* transform, double max_dist,
                         double* dist, double* d2, int32_t* index, int32_t* err, void* stream);
size_t mvsdf_reg_pairs_workspace_bytes(int64_t ns);
int mvsdf_reg_icp_step(const void* tree, size_t tree_bytes, int64_t nr, const double* refs, const double* src, int64_t ns, const double* transform,
                       double max_dist, void* ws, size_t ws_bytes, double* d2, int32_t* index, void* stream);
/* No host wait in any of these.  mvsdf_reg_transform: out = the points under transform (HOST fp64 [16], as above); out may be pts.
 * mvsdf_reg_crop: keep uint8 [n] and out (capacity n rows, input order) = the points inside the prism whose axis is `axis` (0 X, 1 Y, 2 Z) between
 * axis_min and axis_max (inclusive) and whose section is the polygon fp64 [nverts][3] on the DEVICE, 3 <= nverts <= MVSDF_REG_MAX_POLYGON, by the crossing rule
 * registration.py writes out -> MVSDF_ROWS_H_*.  Workspace: mvsdf_reg_crop_workspace_bytes(n), n >= 1.
 * mvsdf_reg_voxel: the voxel filter at edge `voxel` (finite, > 0): origin o = min - voxel / 2 per axis, cell g = floor((p - o) / voxel), key
 * gx | gy << 21 | gz << 42; means (capacity n rows) = per occupied voxel in ascending key the sum of its points in ascending input index from 0,
 * divided by their count; counts int32 -> MVSDF_REG_VOXEL_H_*.  Workspace: mvsdf_reg_voxel_workspace_bytes(n), 1 <= n <= INT32_MAX.
 * mvsdf_reg_hist: out int64 [1 + nedges - 1] on the device = {the distances < tau, then the histogram: the bin of d is the number of edges[1..]
 * that are <= d, a d at or beyond the last edge is dropped}; edges fp64 [nedges] ascending on the DEVICE, 2 <= nedges <= 4097; n >= 0. */
int mvsdf_reg_transform(const double* pts, int64_t n, const double* transform, double* out, void* stream);
size_t mvsdf_reg_crop_workspace_bytes(int64_t n);
int mvsdf_reg_crop(const double* pts, int64_t n, int32_t axis, double axis_min, double axis_max, const double* polygon, int32_t nverts, void* ws,
                   size_t ws_bytes, uint8_t* keep, double* out, void* stream);
size_t mvsdf_reg_voxel_workspace_bytes(int64_t n);
int mvsdf_reg_voxel(const double* pts, int64_t n, double voxel, void* ws, size_t ws_bytes, double* means, int32_t* counts, void* stream);
int mvsdf_reg_hist(const double* dist, int64_t n, const double* edges, int32_t nedges, double tau, int64_t* out, void* stream);

/* ---- Normals of unoriented clouds (normals.hip; Python: mvsdf_amd/normals.py, which states the definition) ----
 * pts fp64 [n][3] on the device, fp64 throughout.  Error bits: MVSDF_PC_ERR_FINITE, _ROUNDS, _WALK, _NORMAL and _INDEX (a neighbour index
 * outside [0, n)); with any set nothing else is valid.  Every argument is validated before the first
 * launch.
 * mvsdf_normals_knn: idx int32 [n][k] = per point the k other points (by index) smallest under (d2, index), d2 = (dx dx + dy dy) + dz dz, ascending;
 * d2 fp64 [n][k] (may be NULL) their squared distances.  normals fp64 [n][3] and variation fp64 [n] (both or neither NULL): the eigenvector of the
 * smallest eigenvalue of each neighbourhood's covariance by cyclic Jacobi, in its canonical sign, and l_min / (l_0 + l_1 + l_2).  1 <= k <= MVSDF_PC_MAX_K,
 * k + 1 <= n <= INT32_MAX.  Workspace: mvsdf_normals_knn_workspace_bytes(n) (0 unless 2 <= n <= INT32_MAX) -> MVSDF_ERRW_H_*; waits for the
 * stream once for the coordinate check.
 * mvsdf_normals_orient: out fp64 [n][3] (not normals itself) = the normals with their signs made consistent along the spanning forest of largest
 * |n_i . n_j| over the edges of neighbors int32 [n][k], each component signed by (ux, uy, uz) at its highest point or, with centers fp64 [V][3] and
 * bits uint64 [n][ceil(V / 64)] (mvsdf_viewsel_pack_*; both or neither NULL, 1 <= V <= MVSDF_VS_MAX_VIEWS), by the votes of the views that see its points;
 * labels int32 [n] = the smallest index of each point's component.  Workspace: mvsdf_normals_orient_workspace_bytes(n) (0 unless
 * 1 <= n <= INT32_MAX) -> MVSDF_NR_ORIENT_H_*; waits for the stream once per round.
 * mvsdf_normals_to_views (no host wait): out = each normal, negated iff more of the views that see its point have n . (c - p) < 0 than > 0 ->
 * hdr (256 bytes on the device): MVSDF_ERRW_H_*. */
enum {
    MVSDF_NR_ORIENT_H_COMPONENTS = 0,   /* components of the neighbour graph */
    MVSDF_NR_ORIENT_H_ROUNDS = 1,       /* rounds run */
    MVSDF_NR_ORIENT_H_ERR = 2,          /* error bits */
    MVSDF_NR_ORIENT_H_WORDS = 3
};
size_t mvsdf_normals_knn_workspace_bytes(int64_t n);
size_t mvsdf_normals_orient_workspace_bytes(int64_t n);
int mvsdf_normals_knn(const double* pts, int64_t n, int32_t k, void* ws, size_t ws_bytes, int32_t* idx, double* d2, double* normals, double* variation,
                      void* stream);
int mvsdf_normals_orient(const double* pts, const double* normals, const int32_t* neighbors, int64_t n, int32_t k, double ux, double uy, double uz,
                         const double* centers, const void* bits, int64_t V, void* ws, size_t ws_bytes, double* out, int32_t* labels, void* stream);
int mvsdf_normals_to_views(const double* pts, const double* normals, int64_t n, const double* centers, const void* bits, int64_t V, double* out, void* hdr,
                           void* stream);

/* ---- Global registration (global_reg.hip; Python: mvsdf_amd/global_reg.py, which states the definition) ----
 * No host wait in any of these.  Error bits: MVSDF_PC_ERR_FINITE, _NORMAL, _INDEX and _CODE.  err: int32 [1] on the device, zeroed by the caller, the bits are OR-ed into it.  radius2: the squared feature
 * radius, +inf for none.  1 <= n <= INT32_MAX, 1 <= k <= MVSDF_PC_MAX_K.
 * mvsdf_greg_spfh: hist int32 [n][33] and count int32 [n] = the binned pair features of every point's neighbour row (neighbors int32 [n][k]).
 * mvsdf_greg_fpfh: features fp64 [n][33] = the rows' sums of hist / count weighted by 1 / d2, each group of 11 scaled to a sum of 100; codes int8
 * [n][33] = min(127, floor(1.27 features)).
 * mvsdf_greg_match: index int32 [ns] = the target code row nearest to each source row under (D, j), D = the squared difference summed over the 33
 * codes, dist int32 [ns] = that D; with mutual, index = -1 where the nearest source of that target is another row.  On the int8 matrix cores.
 * Workspace: mvsdf_greg_match_workspace_bytes(ns, nt) (0 unless 1 <= ns, nt <= INT32_MAX) -> MVSDF_ERRW_H_*.  mvsdf_greg_match_splits: over how
 * many workgroups the walk over the targets is split at these sizes (they combine by a 64-bit atomicMin).
 * mvsdf_greg_ransac: corr int32 [m][2] (source index, target index), m >= 3; 1 <= hypotheses <= MVSDF_GREG_MAX_HYPOTHESES; mask uint8 [m] = the winner's inliers.
 * Workspace: mvsdf_greg_ransac_workspace_bytes(m, hypotheses) -> MVSDF_GREG_RANSAC_H_*. */
enum {
    MVSDF_GREG_RANSAC_H_HYP = 0,        /* the winning hypothesis, or -1 */
    MVSDF_GREG_RANSAC_H_INLIERS = 1,    /* its inliers */
    MVSDF_GREG_RANSAC_H_CHECKED = 2,    /* hypotheses that passed the pre-checks */
    MVSDF_GREG_RANSAC_H_ERR = 3,        /* error bits */
    MVSDF_GREG_RANSAC_H_T = 4,          /* the 12 entries of the winner's 3 x 4 transformation as fp64 bits */
    MVSDF_GREG_RANSAC_H_WORDS = 16
};
enum { MVSDF_GREG_MAX_HYPOTHESES = 1 << 22 };
int mvsdf_greg_spfh(const double* pts, const double* normals, const int32_t* neighbors, int64_t n, int32_t k, double radius2, int32_t* hist,
                    int32_t* count, int32_t* err, void* stream);
int mvsdf_greg_fpfh(const double* pts, const int32_t* neighbors, const int32_t* hist, const int32_t* count, int64_t n, int32_t k, double radius2,
                    double* features, int8_t* codes, int32_t* err, void* stream);
size_t mvsdf_greg_match_workspace_bytes(int64_t ns, int64_t nt);
int32_t mvsdf_greg_match_splits(int64_t ns, int64_t nt);
int mvsdf_greg_match(const int8_t* src, int64_t ns, const int8_t* dst, int64_t nt, int32_t mutual, void* ws, size_t ws_bytes, int32_t* index,
                     int32_t* dist, void* stream);
size_t mvsdf_greg_ransac_workspace_bytes(int64_t m, int64_t hypotheses);
int mvsdf_greg_ransac(const double* src, int64_t ns, const double* dst, int64_t nd, const int32_t* corr, int64_t m, int64_t hypotheses, uint64_t seed,
                      double edge_ratio, double max_dist, void* ws, size_t ws_bytes, uint8_t* mask, void* stream);

/* ---- Sparse points from posed images (keypoints.hip; Python: mvsdf_amd/keypoints.py, which states the definition) ----
 * Keypoints of V views (1 <= V <= MVSDF_VS_MAX_VIEWS) lie one view after the other: view v owns the rows view_off[v] .. view_off[v + 1] of xy fp64 [N][2]
 * and codes int8 [N][MVSDF_KP_DIM] (codes in 0 .. 127), N = view_off[V] <= MVSDF_KP_MAX_KEYPOINTS per view and INT32_MAX in all.  Error bits: MVSDF_PS_ERR_FINITE (a
 * coordinate or matrix entry), _PAIR (a view index), _SHAPE (a count outside the limits: nothing is launched), _CODE, _INDEX and _ROUNDS.  Every workspace
 * starts with MVSDF_RES_H_* (COUNT: the rows written) unless another block is named; outputs are sized by the caller for the largest possible result.
 * mvsdf_kp_match: view_off int64 [V + 1] and pairs int32 [M][2] (views a < b, 1 <= M <= MVSDF_KP_MAX_PAIRS) are HOST arrays.  For every pair and every
 * keypoint i of view a: the nearest (j1, D1) and the second distance D2 over the keypoints of view b under (D, j), D = the squared code difference,
 * on the int8 matrix cores (both directions of every pair in one launch); kept iff (no D2 or fp64(D1) < ratio2 * fp64(D2)) and D1 <= max_dist and
 * (no mutual or the search from b sends j1 back to i).  off int64 [M + 1], idx int32 [cap][2], dist int32 [cap] with cap = the sum over the pairs of
 * view a's keypoints; kept matches by i ascending.  Waits for the stream once (its tables travel from the host).  mvsdf_kp_match_splits: over how many
 * workgroups the walk over a view's targets is split at these sizes.
 * mvsdf_kp_verify: everything on the device: pairs int32 [M][2], off int64 [M + 1], idx int32 [E][2], dist int32 [E] (E = off[M] >= 1), F fp64 [M][9] (row-major,
 * x_b^T F x_a = 0).  A match is kept iff both point-line distances are <= max_epipolar.  Outputs as mvsdf_kp_match's, cap = E.  No host wait.
 * mvsdf_kp_tracks: nodes = the N keypoints, edges = the E matches (same arrays as mvsdf_kp_verify's inputs); components by minimum-label rounds, at
 * most max_rounds of them (the host reads a flag every MVSDF_KP_ROUND_BATCH rounds: MVSDF_PS_ERR_ROUNDS); a component with two keypoints of one view
 * is dropped.  track_off int64 [N / 2 + 1], track_view and track_kp int32 [N] -> MVSDF_KP_TRACKS_H_*.
 * mvsdf_kp_triangulate: per-view fp64 arrays on the device: centers [V][3], rays [V][9] (R^T K^-1, row-major), proj [V][12] (K [R | t]).  One lane per
 * track -> xyz fp64 [T][3], error fp64 [T], keep uint8 [T], obs_keep uint8 [nnz].  hdr: 256 device bytes, MVSDF_ERRW_H_*, zeroed by the call.  No host wait. */
enum {
    MVSDF_KP_DIM = 128,                 /* codes of a descriptor */
    MVSDF_KP_MAX_KEYPOINTS = 1 << 20,   /* keypoints of one view */
    MVSDF_KP_MAX_PAIRS = 32767,         /* view pairs of one matcher call: both directions ride on one grid axis */
    MVSDF_KP_MAX_DIST = 2064512,        /* 128 * 127 * 127: the largest squared code difference */
    MVSDF_KP_ROUND_BATCH = 4            /* labelling rounds per host check */
};
enum {
    MVSDF_KP_TRACKS_H_TRACKS = 0,       /* tracks written */
    MVSDF_KP_TRACKS_H_ENTRIES = 1,      /* their entries */
    MVSDF_KP_TRACKS_H_ERR = 2,          /* error bits */
    MVSDF_KP_TRACKS_H_ROUNDS = 3,       /* labelling rounds run */
    MVSDF_KP_TRACKS_H_WORDS = 4
};
size_t mvsdf_kp_match_workspace_bytes(const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M);
int32_t mvsdf_kp_match_splits(const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M);
int mvsdf_kp_match(const int8_t* codes, const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M, double ratio2, int32_t max_dist,
                   int32_t mutual, void* ws, size_t ws_bytes, int64_t* off, int32_t* idx, int32_t* dist, void* stream);
size_t mvsdf_kp_verify_workspace_bytes(int64_t E);
int mvsdf_kp_verify(const double* xy, const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M, const int64_t* off, const int32_t* idx,
                    const int32_t* dist, int64_t E, const double* F, double max_epipolar, void* ws, size_t ws_bytes, int64_t* off_out,
                    int32_t* idx_out, int32_t* dist_out, void* stream);
size_t mvsdf_kp_tracks_workspace_bytes(int64_t N, int64_t E);
int mvsdf_kp_tracks(const int64_t* view_off, int64_t V, int64_t N, const int32_t* pairs, int64_t M, const int64_t* off, const int32_t* idx, int64_t E,
                    int32_t max_rounds, void* ws, size_t ws_bytes, int64_t* track_off, int32_t* track_view, int32_t* track_kp, void* stream);
/* The detector: scale space, extrema, orientation and descriptor (Python composes them: keypoints.detect).  All arrays on the device.  mvsdf_kp_grey: n pixels of `channels` (1 or 3) uint8
 * (is_float == 0) or fp32 values -> fp64 grey, (299 R + 587 G + 114 B) / 1000 (integers for uint8, ((299 R + 587 G) + 114 B) / 1000 in fp64 for fp32), one
 * channel as it is.  mvsdf_kp_blur: planes x [h][w] fp64 -> dst, separable, rows first then columns, every sum from 0.0 over taps[0 .. 2 radius] left
 * to right with clamped borders (0 <= radius <= MVSDF_KP_MAX_RADIUS; tmp: as large as src; dst may be src).  mvsdf_kp_half: every second pixel,
 * [h][w] -> [(h + 1) / 2][(w + 1) / 2].  mvsdf_kp_dog: L [planes][levels][hw] -> D [planes][levels - 1][hw], D_s = L_(s+1) - L_s.  No host wait. */
/* mvsdf_kp_extrema: D fp64 [V][5][h][w] (mvsdf_kp_dog of six levels) -> the refined extrema of levels s = 1 .. 3 at least `border` (>= 1) pixels from the
 * edges, in the order (view, level, y, x): cand int32 [cap][4] = (view, level, y, x), out fp64 [cap][4] = (X, Y, scale, response) with X = ((x + off_x)
 * + 0.5) * step, scale = sigma[level - 1] * step (sigma: three HOST doubles).  Workspace: mvsdf_kp_extrema_workspace_bytes(V, h, w) (0 beyond 2^31 - 1
 * sites) -> MVSDF_RES_H_* (COUNT: the extrema found; more than cap: MVSDF_PS_ERR_SHAPE and only cap are written).  No host wait. */
enum { MVSDF_KP_MAX_RADIUS = 64 };
size_t mvsdf_kp_extrema_workspace_bytes(int64_t V, int64_t h, int64_t w);
int mvsdf_kp_extrema(const double* D, int64_t V, int64_t h, int64_t w, double contrast, double edge_ratio, int32_t border, double step,
                     const double* sigma, int64_t cap, void* ws, size_t ws_bytes, int32_t* cand, double* out, void* stream);
int mvsdf_kp_grey(const void* images, int32_t is_float, int32_t channels, int64_t n, double* out, void* stream);
int mvsdf_kp_blur(const double* src, int64_t planes, int64_t h, int64_t w, const double* taps, int32_t radius, double* tmp, double* dst, void* stream);
int mvsdf_kp_half(const double* src, int64_t planes, int64_t h, int64_t w, double* dst, void* stream);
int mvsdf_kp_dog(const double* L, int64_t planes, int64_t levels, int64_t hw, double* D, void* stream);
/* mvsdf_kp_describe: L fp64 [V][6][h][w] of one octave, cand int32 [n][4] = (view, level 1 .. 3, y, x) as mvsdf_kp_extrema writes them -> angle fp64 [n]
 * (radians in [0, 2 pi); 0 with upright != 0), codes int8 [n][128] and valid uint8 [n] (0: an all-zero descriptor or a site outside the level).
 * HOST arrays of 3 (levels 1 .. 3): cell = the descriptor's cell width, radius = its window radius, ogauss = 1 / (2 sigma_w^2) of the orientation
 * window, oradius = its radius (radii <= 4 MVSDF_KP_MAX_RADIUS).  trig: DEVICE fp64 [MVSDF_KP_TRIG_WORDS], the coefficients of the sine (14) and
 * cosine (15) polynomials in ascending order.  acc: int64 [n][128] device scratch.  Histogram entries and votes are quantised to 2^-32 and summed as
 * integers.  No host wait. */
enum { MVSDF_KP_TRIG_WORDS = 29 };
int mvsdf_kp_describe(const double* L, int64_t V, int64_t h, int64_t w, const int32_t* cand, int64_t n, int32_t upright, const double* cell,
                      const int32_t* radius, const double* ogauss, const int32_t* oradius, const double* trig, int64_t* acc, double* angle,
                      int8_t* codes, uint8_t* valid, void* stream);
int mvsdf_kp_triangulate(const double* xy, const int64_t* view_off, int64_t V, const int64_t* track_off, const int32_t* track_view,
                         const int32_t* track_kp, int64_t T, int64_t nnz, const double* centers, const double* rays, const double* proj,
                         double max_reproj, double cos_min_angle, double* xyz, double* error, uint8_t* keep, uint8_t* obs_keep, void* hdr,
                         void* stream);

/* ---- Bundle adjustment (bundle.hip; Python: mvsdf_amd/bundle.py, which states the definition) ----
 * Levenberg-Marquardt over the poses of V views (1 <= V <= MVSDF_BA_MAX_VIEWS: the 6 V unknowns of the reduced system fill one chunk of the sum tree) and P
 * points (1 <= P <= INT32_MAX) with nnz observations (1 <= nnz <= MVSDF_BA_MAX_OBS), the points eliminated and the reduced system solved by
 * preconditioned conjugate gradients.  All arrays on the device, fp64 unless named: pose [V][12] (R row-major, then t), intr [V][5] (fx, s, cx, fy, cy),
 * xyz [P][3], track_off int64 [P + 1], track_view int32 [nnz], obs fp64 [nnz][2], fixed uint8 [V] (non-zero: the pose stays), rod [MVSDF_BA_ROD_WORDS]
 * (the coefficients of sin t / t and (1 - cos t) / t^2 in t^2, ascending, MVSDF_BA_ROD_TERMS each, valid for t <= MVSDF_BA_MAX_THETA radians).
 * The workspace (mvsdf_ba_workspace_bytes; 0 outside the limits) starts with MVSDF_BA_H_*.  Error bits: MVSDF_PS_ERR_SHAPE (a count outside the limits:
 * nothing is launched), _FINITE, _INDEX (offsets that do not ascend from 0 to nnz, a view index outside [0, V)) and _BEHIND; with any set the
 * remaining launches return at once.  No call waits for the stream.
 * mvsdf_ba_residuals: r [nnz][2] (unweighted; 0 for an inactive observation), terms [nnz] (robust cost terms; +inf behind a camera when trial != 0, else
 * MVSDF_PS_ERR_BEHIND), the cost into MVSDF_BA_H_COST0 and _COST.  mvsdf_ba_blocks: linearises at the given parameters and leaves the workspace ready
 * for the three calls below (which take the same V, P, nnz): U [V][36], gc [V][6], Vb [P][9], gp [P][3] undamped, bvec [V][6] the right-hand side at lambda.
 * mvsdf_ba_schur: out [V][6] = S x.  mvsdf_ba_solve: b == NULL: the workspace's right-hand side; x [V][6]; the iterations into MVSDF_BA_H_CG.
 * mvsdf_ba_step: the parameters after the step x [V][6] -> pose_out, xyz_out; a rotation beyond the bound sets MVSDF_BA_H_ITER to 1 (else 0) and
 * copies the poses.  mvsdf_ba_adjust: `iterations` rounds -> pose_out, xyz_out, r [nnz][2], terms [nnz] and every header word. */
enum {
    MVSDF_BA_MAX_VIEWS = 341,           /* 6 * 341 <= 2048, one chunk of the sum tree */
    MVSDF_BA_MAX_OBS = 1 << 22,         /* observations of one call: a view's sums take at most 2048 chunks */
    MVSDF_BA_MAX_THETA = 1,             /* radians: the bound of a rotation step and of the polynomials' table */
    MVSDF_BA_ROD_TERMS = 10,            /* terms of each polynomial */
    MVSDF_BA_ROD_WORDS = 20,
    MVSDF_BA_MAX_ITERATIONS = 1000,
    MVSDF_BA_MAX_CG = 10000
};
enum {
    MVSDF_BA_H_ERR = 0,                 /* error bits */
    MVSDF_BA_H_ITER = 1,                /* iterations run (those before convergence) */
    MVSDF_BA_H_ACCEPTED = 2,            /* steps accepted */
    MVSDF_BA_H_CG = 3,                  /* conjugate-gradient iterations in total */
    MVSDF_BA_H_COST0 = 4,               /* the initial cost, fp64 bits */
    MVSDF_BA_H_COST = 5,                /* the final cost, fp64 bits */
    MVSDF_BA_H_LAMBDA = 6,              /* the final damping, fp64 bits */
    MVSDF_BA_H_WORDS = 7
};
size_t mvsdf_ba_workspace_bytes(int64_t V, int64_t P, int64_t nnz);
int mvsdf_ba_residuals(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                       int64_t V, int64_t P, int64_t nnz, double loss_scale, int32_t trial, void* ws, size_t ws_bytes, double* r, double* terms,
                       void* stream);
int mvsdf_ba_blocks(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                    const uint8_t* fixed, int64_t V, int64_t P, int64_t nnz, double loss_scale, double lambda, double floor_diag, void* ws,
                    size_t ws_bytes, double* U, double* gc, double* Vb, double* gp, double* bvec, void* stream);
int mvsdf_ba_schur(int64_t V, int64_t P, int64_t nnz, void* ws, size_t ws_bytes, const double* x, double* out, void* stream);
int mvsdf_ba_solve(int64_t V, int64_t P, int64_t nnz, const double* b, int32_t cg_iters, double cg_tol, void* ws, size_t ws_bytes, double* x,
                   void* stream);
int mvsdf_ba_step(int64_t V, int64_t P, int64_t nnz, const double* rod, void* ws, size_t ws_bytes, const double* x, double* pose_out,
                  double* xyz_out, void* stream);
int mvsdf_ba_adjust(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                    const uint8_t* fixed, int64_t V, int64_t P, int64_t nnz, const double* rod, double loss_scale, int32_t iterations, double lambda0,
                    double lambda_min, double lambda_max, double floor_diag, int32_t cg_iters, double cg_tol, double ftol, void* ws, size_t ws_bytes,
                    double* pose_out, double* xyz_out, double* r, double* terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif
