/*
 * ctpvae_radon.h -- C ABI of the MI355X-native Radon projector that replaces CT_PVAE's physics
 * decoder operators.  Plain pointers and sizes only; every pointer named *_dev is a DEVICE pointer
 * (HIP, gfx950), everything else is host memory.  No allocation of outputs, no host synchronisation,
 * no global state except a thread-local last-error string.  `stream` is a hipStream_t passed as
 * void* (NULL = the default stream).
 *
 * Batches may be of any length: entry points whose kernels index slices with a grid dimension (<= 65535) launch longer
 * batches in chunks, back to back on `stream`.
 *
 * All functions return 0 on success and a negative CTPVAE_E* code otherwise; the message is
 * available from ctpvae_last_error().  Nothing is thrown across this boundary.
 *
 * Reference interfaces each entry point replaces (paths relative to the vganapati/CT_PVAE root):
 *   ctpvae_num_proj_pix / ctpvae_pad_amounts   ctvae/forward_functions.py:29-36   (pad_phantom size rule)
 *   ctpvae_rotate_transforms_f32               tfa.image.rotate's transform table, call sites
 *                                              ctvae/forward_functions.py:70-74,113; inverse used by
 *                                              TF's gradient, reached from ctvae/main_ct_vae.py:471-481
 *   ctpvae_rotate_fwd_f32                      project_tf_fast  ctvae/forward_functions.py:80-123
 *                                              project_tf_low_mem ctvae/forward_functions.py:49-78
 *   ctpvae_rotate_fwd_tiled_f32                the same operator for slices larger than LDS (config 5, 512 x 512)
 *   ctpvae_rotate_bwd_f32                      autodiff of the above (tf.GradientTape,
 *                                              ctvae/main_ct_vae.py:471-481) and its exact transpose
 *   ctpvae_rotate_{fwd,bwd}_f64                the same pair on float64 images (ctvae/tomopy_forward_compare.py:52,56)
 *   ctpvae_rotate_plan_* / _planned_f32        the same two operators, batched: index arithmetic hoisted
 *                                              out of the per-object work (no counterpart in the reference)
 *   ctpvae_rotate_cplan_* / _fwd_compact_f32   the planned forward with step-coded (2 bits per sample) plans
 *   ctpvae_rotate_transforms_host_f32          the same table for a host-resident theta (the dataset's angle list,
 *                                              ctvae/main_ct_vae.py:152), evaluated on the host
 *   ctpvae_rotate_*_sel_*                      the per-step angle subset of calculate_log_prob_M_given_R,
 *                                              ctvae/helper_functions.py:350-357 (tf.gather of theta / mask / proj_sample)
 *   ctpvae_rotate_fwd_planned_loglik_f32       project_tf_fast + the Normal log_prob of calculate_log_prob_M_given_R
 *                                              ctvae/helper_functions.py:359-368, one launch
 *   ctpvae_rotate_bwd{,_planned}_scaled_f32    the gradient of the same caller w.r.t. the reconstruction (autodiff of
 *                                              ctvae/helper_functions.py:359-368 under the per-object sum of
 *                                              :305-312), one launch
 *   ctpvae_siddon_tables_f32 / _fwd_f32        create_sinogram -> tomopy.project
 *                                              ctvae/helper_functions.py:33-38
 *   ctpvae_siddon_bwd_f32 / _rownorm_f32       tomopy.recon(algorithm='fbp' | 'sirt') behind iradon_all / evaluate_sinogram
 *                                              ctvae/helper_functions.py:445-457,503,514
 *   ctpvae_siddon_fwd_ratio_f32 / _bwd_sel_mul_f32   tomopy.recon(algorithm='mlem' | 'osem') behind the same two callers
 *   ctpvae_siddon_bwd_sel_pml_f32              tomopy.recon(algorithm='pml_quad' | 'pml_hybrid' | 'ospml_quad' | 'ospml_hybrid'), with
 *                                              _fwd_ratio as its forward
 *   ctpvae_gridrec_*                           tomopy.recon(algorithm='gridrec'), the default of iradon_all / evaluate_sinogram
 *                                              ctvae/helper_functions.py:445-457,503; ctvae/main_ct_vae.py:111-112
 *   ctpvae_fbp_filter_f64 / _backproject{,_bwd}_f64   iradon  ctvae/fbp_tensorflow.py:14-75
 *   ctpvae_loglik_fwd_f32 / _bwd_f32           calculate_log_prob_M_given_R
 *                                              ctvae/helper_functions.py:360-368
 *   ctpvae_poisson_measure_f32                 create_all_masks' noisy sparse sinograms  ctvae/create_masks.py:80-103
 */
#ifndef CTPVAE_RADON_H
#define CTPVAE_RADON_H

#ifdef __cplusplus
extern "C" {
#endif

#define CTPVAE_OK 0
#define CTPVAE_EINVAL (-1)   /* bad argument (shape, enum, null pointer) */
#define CTPVAE_EHIP (-2)     /* a HIP runtime call failed */
#define CTPVAE_ENODEV (-3)   /* no gfx950 device visible */

#define CTPVAE_NOISE_GAUSSIAN 0 /* the likelihood's noise model: Normal(loc, eps + sqrt(loc / pnm + eps)), ctpvae_loglik_fwd_f32 */
#define CTPVAE_NOISE_POISSON 1  /* the exact Poisson(loc * pnm) of ctpvae_poisson_loglik_fwd_f32 */
#define CTPVAE_NEAREST 0     /* tfa.image.rotate default, project_tf_fast */
#define CTPVAE_BILINEAR 1    /* project_tf_low_mem */

#define CTPVAE_BWD_TF_COMPAT 0 /* what TensorFlow's registered gradient computes (gather) */
#define CTPVAE_BWD_EXACT 1     /* true transpose of the forward (scatter) */

typedef void *ctpvae_stream_t;

/* Version of this ABI: major * 1000 + minor.  CTPVAE_ABI_VERSION is what THIS header describes: host code compiled against
 * it (csrc/torch_node.cpp, a maintainer's own binding) compares the macro with ctpvae_abi_version() of the library it loaded
 * and refuses a mismatch -- an entry point called with another version's argument list is a silent wrong-argument call.
 * The rule: the version changes when an EXISTING entry point changes its argument list or what it computes; an ADDED entry point
 * keeps it ("added at ABI 3400" below).  A binding that needs an added symbol therefore also checks that the library has it
 * (ct_pvae_amd/_lib.py resolves every name when it loads: a library without one fails there, not in a call). */
#define CTPVAE_ABI_VERSION 3400
int ctpvae_abi_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char *ctpvae_last_error(void);
/* Number of visible HIP devices, or a negative error code. */
int ctpvae_device_count(void);
/* Developer knobs (tools/ sweeps, tests that force one code path against another); none changes results.  The launch
 * path never reads the environment: the registry is filled once, when the library is loaded, from CTPVAE_TUNE_<NAME>
 * (and CTPVAE_NO_PLAN / CTPVAE_FORCE_GENERIC), and changed afterwards only here.  name: "NS", "G", "WAVES", "BNS",
 * "BW", "SEG_NS", "SEG_CHUNK", "SEG_PPT", "TILED_NS", "TILED_G", "SIDDON_NS", "SIDDON_THREADS", "SIDDON_PPB",
 * "SIDDON_BWD_NS", "SIDDON_BWD_CHUNKS", "MAX_SLICES", "NO_PLAN", "NO_COMPACT", "FORCE_GENERIC", ... (every name: DESIGN.md section 8); value < 0 unsets; name "*" unsets every knob.
 * _active: how many knobs are set (bench.py prints it next to its numbers). */
int ctpvae_tune_set(const char *name, int value);
int ctpvae_tune_active(void);

/* ---- a1: pad_phantom size rule (host arithmetic only) ------------------------------------- */
int ctpvae_num_proj_pix(int nx, int ny);
int ctpvae_pad_amounts(int n, int P, int *lo, int *hi);

/* ---- a3/a4: transform tables ---------------------------------------------------------------
 * theta_dev [A] fp32 radians as the caller of project_tf_fast passes them (the kernel negates).
 * H, W: height (rows) and width (columns) of the image that is rotated (the padded canvas).
 * T8_dev [A][8]: tfa's flat projective rows; Tinv8_dev [A][8] (may be NULL): the rows TensorFlow's
 * gradient uses (fp32 3x3 inverse, divided by its [2][2] element). */
int ctpvae_rotate_transforms_f32(const float *theta_dev, int A, int H, int W, float *T8_dev,
                                 float *Tinv8_dev, ctpvae_stream_t stream);
/* The same tables for a HOST-resident angle set, computed on the host (all pointers are host memory): cos/sin through
 * the C library's fp64 functions rounded once to fp32, then the same unfused fp32 expressions -- the very bits any other
 * host code gets from those expressions ("trig tables are computed by the caller on host in fp32 so CPU and
 * GPU see identical bits").  The device kernel above differs from it only where the device library's cos/sin round a
 * double differently (rare 1-ulp cases); it is kept for angle sets that exist only on the device. */
int ctpvae_rotate_transforms_host_f32(const float *theta, int A, int H, int W, float *T8, float *Tinv8);

/* ---- a2/a5: rotate-and-sum forward ---------------------------------------------------------
 * img_dev  [S][H][W] fp32, contiguous: the UNPADDED slices.  The PH x PW zero canvas with the
 *          slice at (py, px) is never materialised.
 * T8_dev   [A][8] rows applied to the canvas (elements 6, 7 must be 0).
 * sino_dev [S][A][PW]: sino[s][a][j] = sum_{i<PH} sample(canvas_s, T_a(j, i)), rows added in order. */
int ctpvae_rotate_fwd_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                          const float *T8_dev, int A, int interp, float *sino_dev,
                          ctpvae_stream_t stream);

/* The reference's float64 callers (ctvae/tomopy_forward_compare.py:52,56: xdesign's float64 phantoms through both projectors):
 * TensorFlow keeps the coordinates and the interpolation weights in fp32 whatever the image type, casts each weight to the
 * image type and multiplies, adds and row-sums in it.  Same geometry arguments as ctpvae_rotate_fwd_f32; img / sino are
 * double; a correctness-first kernel (one ray per lane, the slice in LDS when 8 H (W + 1) bytes fit).  Round 5, ABI 3400. */
int ctpvae_rotate_fwd_f64(const double *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                          const float *T8_dev, int A, int interp, double *sino_dev, ctpvae_stream_t stream);
/* ... and its backward in double (round 6, ABI 3400: an added entry point).  Arguments and rows as ctpvae_rotate_bwd_f32
 * (CTPVAE_BWD_TF_COMPAT takes the INVERTED rows, CTPVAE_BWD_EXACT the FORWARD rows); gsino / gimg are double.
 * TF_COMPAT: TensorFlow's gradient for T = double -- fp32 coordinates and weights, double taps, products and sums, angles added
 *   in ascending order.
 * EXACT: the transpose of ctpvae_rotate_fwd_f64, gimg[s][r][c] = sum over angles, canvas rows, bins (in that order) of the
 *   samples whose tap is (r, c) of ((double)wy * (double)wx) * gsino[s][a][j] (nearest: 1 * g), wy, wx the forward's own fp32
 *   weights.  A deterministic gather (no atomics, no plan); the rows must be rotations, as ctpvae_rotate_transforms_f32 makes.
 * Both: fixed bits, a correctness-first kernel (the cotangent rows of a chunk of angles in LDS, 8 B per bin). */
int ctpvae_rotate_bwd_f64(const double *gsino_dev, int S, int A, int PH, int PW, const float *T8_dev, int interp, int mode,
                          int H, int W, int py, int px, double *gimg_dev, ctpvae_stream_t stream);

/* ---- a2 for slices larger than LDS (512 x 512): tiled forward, NEAREST -----------------------
 * The slice is cut into tiles 64 wide x tile_h tall, tile_h = ceil(H / ceil(H / 128)) (EQUAL rows of tiles, ABI 3310: 128 for
 * H = 512; up to ABI 3300 it was 96 with a 32-row remainder -- the same taps, another association of the sum);
 * every tile is staged once and serves all angles, the tiles' partial sums (workspace) are then added in ascending tile order
 * (row-major over the slice):
 *     sino[s][a][j] = ((0 + p_0) + p_1) + ...,  p_t = sum over canvas rows i, ascending, of the taps inside tile t.
 * Tap indices are exactly those of ctpvae_rotate_fwd_f32; only the association of the fp32 sum differs.
 * ctpvae_rotate_tile_shape: 1 and the tile shape when (H, W, interp) is a tiled geometry, 0 (and zeros) when it is not --
 * what a checker needs to restate the sum (oracle_rotate_fwd_tiled); a function of its arguments alone, not of the device.
 * _workspace_bytes returns 0 when the slice fits LDS whole (use ctpvae_rotate_fwd_f32),
 * otherwise the size of the caller-owned device workspace (contents undefined on return). */
int ctpvae_rotate_tile_shape(int H, int W, int interp, int *tile_h, int *tile_w);
long long ctpvae_rotate_fwd_tiled_workspace_bytes(int S, int H, int W, int PH, int PW, int A, int interp);
int ctpvae_rotate_fwd_tiled_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                                const float *T8_dev, int A, void *workspace_dev, float *sino_dev,
                                ctpvae_stream_t stream);

/* BILINEAR slices larger than LDS (round 5, ABI 3400; ctvae/forward_functions.py:69-77 at 512 x 512): tiles 64 wide x
 * ceil(H / ceil(H / 96)) tall (86 for H = 512), each staged with a one-pixel halo below and to its right.  A sample's 2 x 2
 * footprint belongs to the tile of its FLOOR tap and is evaluated there exactly as ctpvae_rotate_fwd_f32 evaluates it; a tile's
 * partial sum adds its samples in ascending canvas-row order and the tiles are added in ascending order as above
 * (oracle_rotate_fwd_tiled with interp = 1).  interp = CTPVAE_NEAREST: ctpvae_rotate_fwd_tiled_f32.  Workspace and tile shape:
 * the two functions above with the same interp. */
int ctpvae_rotate_fwd_tiled_interp_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                                       const float *T8_dev, int A, int interp, void *workspace_dev, float *sino_dev,
                                       ctpvae_stream_t stream);

/* ---- a5, precision "fast" (round 8, ABI 3400: two added entry points) -- OPT-IN, BILINEAR only ------------------------------------
 * The bilinear forward above with another blend of the four taps a, b (floor row), c, d (ceil row) of a sample:
 *     t = fma(wx, b - a, a),  u = fma(wx, d - c, c),  v = fma(wy, u - t, t),   wx = x - floor(x), wy = y - floor(y)
 * instead of TensorFlow's unfused wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d): 6 instead of 10 packed operations per slice pair in
 * a kernel bound by the vector unit's issue rate.  The coordinates x, y, their floors, the taps, the zero fill, the tile a sample
 * belongs to and the order of every sum are those of ctpvae_rotate_fwd_f32 / ctpvae_rotate_fwd_tiled_interp_f32 with interp =
 * CTPVAE_BILINEAR, to the bit (the coordinate arithmetic is NOT fused); the result differs from theirs by the rounding of the blend
 * alone (~3e-7 of the sinogram's maximum on white noise; the bar is 1e-5) and is NOT bit-equal to the oracle.  Deterministic: fixed
 * bits for fixed arguments.  Arguments as the exact functions' without `interp`; the workspace and tile shape are those of
 * ctpvae_rotate_fwd_tiled_workspace_bytes / ctpvae_rotate_tile_shape with interp = CTPVAE_BILINEAR; same return codes.
 * ctpvae_rotate_fwd_fast_f32 takes the calls the bilinear LDS kernel takes (the slice and the tables of A angles fit LDS whole) and
 * refuses every other with CTPVAE_EINVAL -- it never runs an exact kernel in silence; the one exception are the NO_PLAN /
 * FORCE_GENERIC knobs of ctpvae_tune_set, which ask for round 1's direct kernels by name: those have no fast form and run as they are.
 * The backward of a fast forward is ctpvae_rotate_bwd_f32 as before: the gradient / transpose of the same interpolant. */
int ctpvae_rotate_fwd_fast_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                               const float *T8_dev, int A, float *sino_dev, ctpvae_stream_t stream);
int ctpvae_rotate_fwd_tiled_fast_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                                     const float *T8_dev, int A, void *workspace_dev, float *sino_dev,
                                     ctpvae_stream_t stream);

/* ... and with the log-likelihood epilogue of ctpvae_rotate_fwd_planned_loglik_f32 (below) in its reduce pass. */
int ctpvae_rotate_fwd_tiled_loglik_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                                       const float *T8_dev, int A, void *workspace_dev, const float *mask_dev,
                                       const float *meas_dev, const float *pnm_dev, float eps, float *sino_dev,
                                       float *lp_dev, float *dlp_dev, ctpvae_stream_t stream);

/* ... through COMPACT tile plans (round 3): the per-sample index arithmetic the tiled kernel is bound by, hoisted into a plan as
 * for slices that fit LDS (ctpvae_rotate_cplan_*): a section per (tile, angle, ray slot) = the ray's first tap inside the tile +
 * 2 bits per row.  Same taps, same order, same partial sums and reduce pass: the bits of ctpvae_rotate_fwd_tiled{,_loglik}_f32.
 * _bytes: 0 if the slice is not tiled (or compact plans are switched off); _overflowed (SYNCHRONISES): 1 = do not use the plan.
 * tplan_dev NULL: the direct tiled kernel (this is then ctpvae_rotate_fwd_tiled{,_loglik}_f32 with the options below).
 * lp_dev NULL: ray-sums only; else the log-likelihood epilogue in the reduce pass (mask, meas, pnm required; dlp_dev optional).
 * lp_sum_dev [S] (with lp_part_dev: ctpvae_loglik_part_floats(S, A, PW, 1) floats, its counters zero): the per-object log-likelihood sums
 * reduced in the reduce pass, as ctpvae_rotate_fwd_compact_f32 does for slices that fit LDS -- the bits of
 * ctpvae_loglik_object_sums_f32(lp, partition 1); sino_dev and lp_dev may then be NULL. */
long long ctpvae_rotate_tplan_bytes(int H, int W, int PH, int PW, int A);
int ctpvae_rotate_tplan_build_f32(const float *T8_dev, int A, int H, int W, int PH, int PW, int py, int px, void *tplan_dev,
                                  ctpvae_stream_t stream);
int ctpvae_rotate_tplan_overflowed(const void *tplan_dev, int H, int W, int PH, int PW, int A, ctpvae_stream_t stream);
int ctpvae_rotate_fwd_tiled_compact_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int py, int px,
                                        const float *T8_dev, int A, const void *tplan_dev, void *workspace_dev,
                                        const float *mask_dev, const float *meas_dev, const float *pnm_dev, float eps,
                                        float *sino_dev, float *lp_dev, float *dlp_dev, float *lp_part_dev, float *lp_sum_dev,
                                        ctpvae_stream_t stream);

/* ---- a4: backward of the above -------------------------------------------------------------
 * gsino_dev [S][A][PW] cotangent.  gimg_dev [S][H][W] (overwritten).
 * mode CTPVAE_BWD_TF_COMPAT: T8_dev must hold the INVERTED rows (Tinv8 above).
 * mode CTPVAE_BWD_EXACT:     T8_dev must hold the FORWARD rows. */
int ctpvae_rotate_bwd_f32(const float *gsino_dev, int S, int A, int PH, int PW, const float *T8_dev,
                          int interp, int mode, int H, int W, int py, int px, float *gimg_dev,
                          ctpvae_stream_t stream);
/* ... with a per-slice factor applied in the kernel's own store: gimg[s] = scale_dev[s * scale_stride] * (the sum).
 * This is the backward half of SURVEY 8 f1: with gsino_dev = the dlp the fused forward wrote and scale = the upstream
 * gradient of sum(lp[s]) (TF's gradient of reduce_sum is a broadcast: stride 0 over angles and bins), the whole
 * backward of calculate_log_prob_M_given_R (ctvae/helper_functions.py:336-368) is this one launch.
 * scale_dev NULL = ctpvae_rotate_bwd_f32; otherwise interp NEAREST and mode TF_COMPAT only. */
int ctpvae_rotate_bwd_scaled_f32(const float *gsino_dev, int S, int A, int PH, int PW, const float *T8_dev,
                                 int interp, int mode, int H, int W, int py, int px, const float *scale_dev,
                                 long long scale_stride, float *gimg_dev, ctpvae_stream_t stream);

/* ---- gather plans (NEAREST): the tap indices of a geometry, computed once, reused for every slice ----------
 * The tap a sample reads depends on (angle, canvas row, detector bin) only, so for batched projection the index
 * arithmetic of a3/a4 is evaluated ONCE by ctpvae_rotate_plan_build_f32 (exactly as the direct kernels do) and
 * stored as u16 LDS indices; ctpvae_rotate_{fwd,bwd}_planned_f32 then compute the SAME sums, bit for bit, as
 * ctpvae_rotate_fwd_f32 / ctpvae_rotate_bwd_f32(mode TF_COMPAT) with interp NEAREST.
 * which: 0 = forward plan, 1 = backward (TF_COMPAT) plan.  _supported returns 1 if the geometry fits the planned
 * kernels (slice / cotangent block must fit LDS), else 0 -- use the direct entry points then.
 * Plan buffers are caller-owned device memory of ctpvae_rotate_plan_bytes() bytes, 256-byte aligned.
 * The backward plan is one 16-byte vector per (group of sixteen angles, row, padded column) -- a byte per angle, 255 = no
 * tap -- and, when A mod 16 is 1 .. 12, behind that array (256-byte aligned) a compact tail section: the last group's
 * live dwords once more, ceil((A mod 16) / 4) = 1 .. 3 per (row, padded column), the column running fastest.  Launches of
 * at most 32 angles read their last group from the section; the array stays complete, every other launch reads it alone. */
int ctpvae_rotate_plan_supported(int H, int W, int PH, int PW, int A, int interp, int which);
long long ctpvae_rotate_plan_bytes(int H, int W, int PH, int PW, int A, int which);
/* T8_dev: forward rows (needed for the forward plan); Tinv8_dev: inverted rows (needed for the backward plan);
 * either plan pointer may be NULL to skip it. */
int ctpvae_rotate_plan_build_f32(const float *T8_dev, const float *Tinv8_dev, int A, int H, int W, int PH, int PW,
                                 int py, int px, void *fwd_plan_dev, void *bwd_plan_dev, ctpvae_stream_t stream);
int ctpvae_rotate_fwd_planned_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A,
                                  const void *fwd_plan_dev, float *sino_dev, ctpvae_stream_t stream);
/* Host only (added at ABI 3400): which form of the kernel ctpvae_rotate_fwd_planned_f32 launches for this shape -- 1 = the lean form
 * for few-task launches of one round of workgroups (rotate_fwd_planned_kernel_few), 0 = the general kernel; negative on bad sizes.
 * Same bits either way.  img_aligned16: whether img_dev is 16-byte aligned.  Honours the developer knobs (FWD_FEW = 0: always 0). */
int ctpvae_rotate_fwd_planned_form(int S, int H, int W, int PH, int PW, int A, int img_aligned16);
/* a8 fused into a2: the planned forward that also writes, for every ray-sum, the log-probability of the
 * measured sample under it -- lp[s][a][j] = ctpvae_loglik_fwd_f32's expression on (sino[s][a][j], mask[s][a],
 * meas[s][a][j]) -- in the same launch.  sino_dev is still written.  dlp_dev (may be NULL) receives
 * d lp / d sino [S][A][PW], i.e. what ctpvae_loglik_bwd_f32 multiplies the upstream gradient by, so that the backward
 * needs no elementwise pass: see ctpvae_rotate_bwd_planned_scaled_f32. */
int ctpvae_rotate_fwd_planned_loglik_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A,
                                         const void *fwd_plan_dev, const float *mask_dev, const float *meas_dev,
                                         const float *pnm_dev, float eps, float *sino_dev, float *lp_dev,
                                         float *dlp_dev, ctpvae_stream_t stream);
/* Angle subsets of a DENSE plan (the training loop projects `api` random angles of the dataset's 180 per step,
 * ctvae/helper_functions.py:350-357): the plan and tables are built ONCE for all A angles; angle_idx_dev [n_idx] int32 on
 * the device (1 <= n_idx <= 256; values are clamped into [0, A)) selects the plan angles a launch projects, in that
 * order: sino / lp / dlp are [S][n_idx][PW].  No plan or table kernel runs per step.  dense_inputs != 0: mask_dev and
 * meas_dev are the DENSE [S][A] / [S][A][PW] arrays and are read at the selected plan angles (the caller's gathers
 * mask[:, angles_i], proj_sample[:, angles_i] folded into the load); 0: they are [S][n_idx] / [S][n_idx][PW]. */
int ctpvae_rotate_fwd_planned_sel_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A,
                                      const void *fwd_plan_dev, const int *angle_idx_dev, int n_idx, float *sino_dev,
                                      ctpvae_stream_t stream);
int ctpvae_rotate_fwd_planned_loglik_sel_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A,
                                             const void *fwd_plan_dev, const int *angle_idx_dev, int n_idx,
                                             const float *mask_dev, const float *meas_dev, int dense_inputs,
                                             const float *pnm_dev, float eps, float *sino_dev, float *lp_dev,
                                             float *dlp_dev, ctpvae_stream_t stream);
/* COMPACT forward plans (round 3): the same taps as the u16 plan above, stored as the ray's first tap + 2 bits per canvas
 * row (does the source column step? does the source row step? -- x_in and y_in of ImageProjectiveTransformV3 are monotone in
 * the row number with slope <= 1, so their rounded values stay or step by one): 1/3 B instead of 2 B per sample (three rows
 * per code byte), 2.4 MB instead of 17 MB at the dataset's 180 angles, L2-resident on every XCD.  The plan kernel evaluates the reference
 * arithmetic exactly as the u16 plan's does; ctpvae_rotate_fwd_compact_f32 computes the SAME sums, bit for bit, as
 * ctpvae_rotate_fwd_planned{,_sel,_loglik,_loglik_sel}_f32 -- one entry point, optional operands:
 *   angle_idx      NULL = all A plan angles; else the n_idx (1..256) plan angles to project, outputs [S][n_idx][PW];
 *                  idx_on_host = 0: a DEVICE int32 vector; != 0: HOST memory (the training loop draws its subset on the
 *                  host, ctvae/helper_functions.py:104-107) -- the indices then travel in the kernel arguments: no upload,
 *                  no device copy for the kernel to wait on; the array may be reused as soon as the call returns
 *   lp_dev         NULL = ray-sums only; else the log-likelihood epilogue of ctpvae_rotate_fwd_planned_loglik_f32
 *                  (mask_dev, meas_dev, pnm_dev required; dense_inputs as in the _sel entry point; dlp_dev may be NULL)
 *   lp_sum_dev     NULL, or [S]: the PER-OBJECT log-likelihood sums the loss takes (ctvae/helper_functions.py:305-312),
 *                  reduced inside the launch: every (angle, 64-bin) task adds its log-probabilities by a
 *                  fixed xor butterfly and writes one partial into lp_part_dev (workspace of
 *                  ctpvae_loglik_part_floats(S, angles, PW, 0) floats, its arrival counters zero), a second tiny launch adds a
 *                  slice's partials in the fixed order stated at ctpvae_loglik_object_sums_f32 -- its bits (partition 0).  sino_dev and lp_dev
 *                  may then be NULL (nothing but dlp [S][n][PW] and the sums leaves the kernel).
 * _supported: 1 if the slice with its one-cell zero border fits LDS (interp NEAREST).  _overflowed (SYNCHRONISES): 1 if some
 * ray's steps do not fit the code (rows that are not a rotation, a ray still inside the slice at the canvas' last row, a
 * rounding tie that makes a coordinate jump by two) -- the plan must then not be used: keep the u16 plan. */
int ctpvae_rotate_cplan_supported(int H, int W, int PH, int PW, int A, int interp);
long long ctpvae_rotate_cplan_bytes(int H, int W, int PH, int PW, int A);
int ctpvae_rotate_cplan_build_f32(const float *T8_dev, int A, int H, int W, int PH, int PW, int py, int px, void *cplan_dev,
                                  ctpvae_stream_t stream);
int ctpvae_rotate_cplan_overflowed(const void *cplan_dev, int H, int W, int PH, int PW, int A, ctpvae_stream_t stream);
int ctpvae_rotate_fwd_compact_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A, const void *cplan_dev,
                                  const int *angle_idx, int n_idx, int idx_on_host, const float *mask_dev,
                                  const float *meas_dev, int dense_inputs, const float *pnm_dev, float eps, float *sino_dev,
                                  float *lp_dev, float *dlp_dev, float *lp_part_dev, float *lp_sum_dev, ctpvae_stream_t stream);
/* The same call with the likelihood's noise model as an operand (added at ABI 3400): noise = CTPVAE_NOISE_GAUSSIAN is the call
 * above, bit for bit; CTPVAE_NOISE_POISSON stores / reduces the exact Poisson log-probability of ctpvae_poisson_loglik_fwd_f32 (its
 * bits) and, in dlp_dev, d lp / d ray-sum as ctpvae_poisson_loglik_bwd_f32 forms it -- the operand of the unchanged scaled backward.
 * eps is ignored under POISSON; the per-object sums keep their fixed order.  Without lp_dev / lp_sum_dev noise selects nothing. */
int ctpvae_rotate_fwd_compact_noise_f32(const float *img_dev, int S, int H, int W, int PH, int PW, int A, const void *cplan_dev,
                                        const int *angle_idx, int n_idx, int idx_on_host, const float *mask_dev,
                                        const float *meas_dev, int dense_inputs, const float *pnm_dev, float eps, int noise,
                                        float *sino_dev, float *lp_dev, float *dlp_dev, float *lp_part_dev, float *lp_sum_dev,
                                        ctpvae_stream_t stream);

/* ... and the TF_COMPAT / NEAREST backward of such a subset: gsino_dev [S][n_idx][PW], Tinv8_dev the DENSE inverted table
 * [A_plan][8]; row k of a cotangent uses table row angle_idx_dev[k].  Same bits as ctpvae_rotate_bwd_scaled_f32 on the
 * gathered table (scale_dev may be NULL). */
int ctpvae_rotate_bwd_sel_scaled_f32(const float *gsino_dev, int S, int A_plan, int PH, int PW, const float *Tinv8_dev,
                                     const int *angle_idx_dev, int n_idx, int H, int W, int py, int px,
                                     const float *scale_dev, long long scale_stride, float *gimg_dev,
                                     ctpvae_stream_t stream);

/* ... through a plan: the "bwd4" layout stores the byte taps of the backward plan as one dword per (angle, four consecutive rows,
 * column), so a launch can take any subset of the plan's angles (the 16-angles-per-vector layout of the plan above
 * cannot).  Same bits as ctpvae_rotate_bwd_sel_scaled_f32 (sum over subset rows k ascending), no per-sample index
 * arithmetic.  angle_idx / idx_on_host as in ctpvae_rotate_fwd_compact_f32 (host indices: n_idx <= 256).  _bytes: 0 if the geometry does not fit byte taps (PW > 255: keep ctpvae_rotate_bwd_sel_scaled_f32). */
long long ctpvae_rotate_bwd4_plan_bytes(int H, int W, int PH, int PW, int A);
int ctpvae_rotate_bwd4_plan_build_f32(const float *Tinv8_dev, int A, int H, int W, int PH, int PW, int py, int px,
                                      void *plan_dev, ctpvae_stream_t stream);
int ctpvae_rotate_bwd_planned_sel_scaled_f32(const float *gsino_dev, int S, int H, int W, int PH, int PW, int A,
                                             const void *bwd4_plan_dev, const int *angle_idx, int n_idx, int idx_on_host,
                                             const float *scale_dev, long long scale_stride, float *gimg_dev,
                                             ctpvae_stream_t stream);

/* STEP PLAN of the direct (segment) backward, for slices too large for the planned backward above (512 x 512; round 3):
 * down a column of pixels the tap of an angle stays or steps by one per row (|t1| <= 1), always the same way, so a lane that
 * owns eight consecutive rows needs its first row's tap (7 bits, relative to the 80-bin segment its 64 x 32 tile stages for
 * the angle) and seven bits: one u16 per (angle, row octet, column), written by a kernel that evaluates the reference
 * arithmetic exactly as ctpvae_rotate_bwd_f32's kernel does.  Same taps, same order: the same bits as ctpvae_rotate_bwd_scaled_f32
 * (mode TF_COMPAT, NEAREST), with two index operations per tap instead of five.  _overflowed (SYNCHRONISES): 1 if the geometry
 * does not fit the code (a tile that leaves the canvas at some angle -- unpadded canvases --, rows that are not a rotation):
 * the plan must then not be used.  Small launches (fewer than 512 tiles of 64 x 32) run ctpvae_rotate_bwd_scaled_f32's kernel. */
long long ctpvae_rotate_bwd_step_plan_bytes(int H, int W, int A);
int ctpvae_rotate_bwd_step_plan_build_f32(const float *Tinv8_dev, int A, int H, int W, int PH, int PW, int py, int px, void *plan_dev,
                                          ctpvae_stream_t stream);
int ctpvae_rotate_bwd_step_plan_overflowed(const void *plan_dev, int H, int W, int A, ctpvae_stream_t stream);
int ctpvae_rotate_bwd_stepped_scaled_f32(const float *gsino_dev, int S, int A, int PH, int PW, const float *Tinv8_dev, int H, int W,
                                         int py, int px, const void *step_plan_dev, const float *scale_dev, long long scale_stride,
                                         float *gimg_dev, ctpvae_stream_t stream);

/* (Which backward: both give the same bits.  The planned one wins except for large batches at few angles -- S >= 80
 * and A <= 64 -- where ctpvae_rotate_bwd_f32's segment kernel, which streams no indices, is up to 25 % faster.) */
int ctpvae_rotate_bwd_planned_f32(const float *gsino_dev, int S, int H, int W, int PH, int PW, int A,
                                  const void *bwd_plan_dev, float *gimg_dev, ctpvae_stream_t stream);
/* ... with the per-slice factor of ctpvae_rotate_bwd_scaled_f32 (scale_dev NULL = no factor). */
int ctpvae_rotate_bwd_planned_scaled_f32(const float *gsino_dev, int S, int H, int W, int PH, int PW, int A,
                                         const void *bwd_plan_dev, const float *scale_dev, long long scale_stride,
                                         float *gimg_dev, ctpvae_stream_t stream);

/* Exact transpose of the NEAREST forward as a deterministic gather (no atomics, bit-reproducible): a rotation followed by
 * rounding sends at most two canvas samples of an angle to one pixel, so the plan stores, per (angle, pixel), the <= 2
 * detector bins whose cotangent the scatter would have added, in the scatter's order (canvas row, then bin), and the
 * planned backward kernel gathers them -- the same sums, bit for bit, as ctpvae_rotate_bwd_f32(mode EXACT) would produce
 * if its atomic adds arrived in order.  _bytes: size of the caller-owned plan buffer (256-byte aligned), 0 if the geometry
 * does not fit (PW > 255: keep ctpvae_rotate_bwd_f32).  _build needs both tables.  _overflowed (synchronises): 1 if
 * some pixel had more than two hits -- the rows were not a rotation -- and the plan must not be used. */
long long ctpvae_rotate_exact_plan_bytes(int H, int W, int PH, int PW, int A);
int ctpvae_rotate_exact_plan_build_f32(const float *T8_dev, const float *Tinv8_dev, int A, int H, int W, int PH, int PW,
                                       int py, int px, void *plan_dev, ctpvae_stream_t stream);
int ctpvae_rotate_exact_plan_overflowed(const void *plan_dev, int H, int W, int PH, int PW, int A, ctpvae_stream_t stream);
int ctpvae_rotate_bwd_exact_planned_f32(const float *gsino_dev, int S, int H, int W, int PH, int PW, int A,
                                        const void *exact_plan_dev, float *gimg_dev, ctpvae_stream_t stream);

/* Exact transpose as a deterministic gather through a plan of SUMMED WEIGHTS (round 5, ABI 3400; north_star: "bilinear
 * sample/scatter").  For a rotation the canvas samples that touch a pixel lie in at most three consecutive detector bins; the
 * plan holds, per (angle, pixel), the first of them and the pixel's summed fp32 weight in each (the forward's own weights,
 * summed over canvas rows in ascending order; interp = NEAREST: the number of samples whose tap the pixel is): 16 bytes per
 * (angle, pixel).  The backward adds ((W0 g[first] + W1 g[first+1]) + W2 g[first+2]) over the angles in ascending order: no
 * atomics at any size, equal bits run to run, <= 1e-5 (of the largest value) from ctpvae_rotate_bwd_f32(mode EXACT) / the
 * oracle's in-order scatter.  BILINEAR: the exact adjoint at every size; NEAREST: for geometries the byte plan above does not
 * hold (PW > 255: 512 x 512).  _bytes: the caller-owned plan buffer (16-byte aligned); _build needs both tables; _overflowed
 * (SYNCHRONISES): 1 if some pixel's samples span more than three bins (the rows are not a rotation) -- keep
 * ctpvae_rotate_bwd_f32 then.  Tinv8_dev places the cotangent segments a pixel tile stages. */
long long ctpvae_rotate_exact_wplan_bytes(int H, int W, int A);
int ctpvae_rotate_exact_wplan_build_f32(const float *T8_dev, const float *Tinv8_dev, int A, int H, int W, int PH, int PW,
                                        int py, int px, int interp, void *plan_dev, ctpvae_stream_t stream);
int ctpvae_rotate_exact_wplan_overflowed(const void *plan_dev, int H, int W, int A, ctpvae_stream_t stream);
int ctpvae_rotate_bwd_exact_wplan_f32(const float *gsino_dev, int S, int A, int PH, int PW, const float *Tinv8_dev,
                                      int H, int W, int py, int px, const void *plan_dev, float *gimg_dev,
                                      ctpvae_stream_t stream);

/* ---- a7: TomoPy-style ray-driven projector --------------------------------------------------
 * Tables (host side, fp32): theta [dt] -> sin, cos of fmodf(theta, 2*pi) and libtomo's quadrant flag. */
int ctpvae_siddon_dx(int ox, int oz, int pad);
int ctpvae_siddon_tables_f32(const float *theta, int dt, float *sin_out, float *cos_out, int *quadrant_out);
/* obj_dev [oy][ox][oz]; sin_dev/cos_dev [dt] fp32, quad_dev [dt] int32; data_dev [oy][dt][dx]
 * (libtomo's order; tomopy.project(sinogram_order=False) returns it with axes 0,1 swapped). */
int ctpvae_siddon_fwd_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev,
                          const float *cos_dev, const int *quad_dev, int dt, int dx, float center,
                          float *data_dev, ctpvae_stream_t stream);

/* The transpose of ctpvae_siddon_fwd_f32 -- what libtomo's fbp.c accumulates (recon[indi[n]] += data * dist[n]; with
 * filter_name 'none', as ctvae/helper_functions.py:514 asks for the mask channel, that IS tomopy.recon(algorithm='fbp')) and
 * the A^T of its sirt.c (helper_functions.py:503 with algorithm='sirt').  data_dev [oy][dt][dx] -> recon_dev [oy][ox][oz].
 * Pixel-driven (round 3): a lane owns a pixel and asks the two rays per angle that can cross it for their segment in it,
 * found with libtomo's own fp32 expressions (the crossings around the pixel, trim_coords' 0.01 rule, the midpoint's pixel);
 * a pixel's terms arrive in libtomo's order (angles, then rays, ascending), so the result equals the ray-driven accumulation
 * bit for bit except for the corner-cutting slivers of rays that pass within fp32 rounding of a grid corner (~1e-6 of the
 * image's range, about one pixel per angle).  No atomics: bit-reproducible.  <A x, y> = <x, A^T y> to rounding.
 *   _workspace_bytes  device memory the calls below need (ray table, flags, one scratch image per slice); 256-byte aligned
 *   _prepare          geometry only: fills the workspace's ray table; once per (grid, angles, dx, center)
 *   _prepared         colsum_dev NULL:  recon = A^T data  (overwritten)
 *                     colsum_dev [ox][oz]:  recon += (A^T data) / colsum where colsum != 0 -- sirt.c's update, in place
 *   _bwd_f32          _prepare + _prepared(colsum NULL)
 *   ctpvae_siddon_fwd_resid_f32   the forward with sirt.c's per-ray factor as its store: upd = (meas - A obj) / rn2 where
 *                     rn2 != 0, else 0 (meas_dev [oy][dt][dx], rn2_dev [dt][dx] from _rownorm) -- a SIRT iteration is this
 *                     launch and one _prepared(colsum) launch.
 * _rownorm: rn2_dev [dt][dx] = sum of squared segment lengths of every ray (sirt.c's sum_dist2; geometry only). */
long long ctpvae_siddon_bwd_workspace_bytes(int oy, int ox, int oz, int dt, int dx);
int ctpvae_siddon_bwd_prepare_f32(int ox, int oz, const float *sin_dev, const float *cos_dev, const int *quad_dev, int dt, int dx,
                                  float center, void *workspace_dev, ctpvae_stream_t stream);
int ctpvae_siddon_bwd_prepared_f32(const float *data_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                   const int *quad_dev, int dt, int dx, float center, const void *workspace_dev,
                                   const float *colsum_dev, float *recon_dev, ctpvae_stream_t stream);
int ctpvae_siddon_bwd_f32(const float *data_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                          const int *quad_dev, int dt, int dx, float center, void *workspace_dev, float *recon_dev,
                          ctpvae_stream_t stream);
int ctpvae_siddon_fwd_resid_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                const int *quad_dev, int dt, int dx, float center, const float *meas_dev,
                                const float *rn2_dev, float *upd_dev, ctpvae_stream_t stream);
/* The forward with a workspace (round 3): with >= 3 slices the slices are interleaved per pixel in workspace_dev
 * (_fwd_workspace_bytes() bytes, 16-byte aligned) and one walk of a ray serves 4 or 8 of them from L2 -- the same bits as ctpvae_siddon_fwd_f32,
 * 2-5x faster on grids whose slice pairs do not fit LDS.  meas_dev / rn2_dev both NULL: ray-sums; both given: the store of
 * ctpvae_siddon_fwd_resid_f32.  _fwd_workspace_bytes() == 0: no workspace needed (the LDS kernels are taken). */
long long ctpvae_siddon_fwd_workspace_bytes(int oy, int ox, int oz);
int ctpvae_siddon_fwd_ws_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                             const int *quad_dev, int dt, int dx, float center, const float *meas_dev, const float *rn2_dev,
                             void *workspace_dev, float *data_dev, ctpvae_stream_t stream);
int ctpvae_siddon_rownorm_f32(int ox, int oz, const float *sin_dev, const float *cos_dev, const int *quad_dev, int dt,
                              int dx, float center, float *rn2_dev, ctpvae_stream_t stream);
/* Host only (added at ABI 3400): which form of the forward kernel a call of the entry points that take a workspace
 * (ctpvae_siddon_fwd_ws_f32, _fwd_ws_tv_dual, _fwd_loglik, _fwd_loglik_noise, _fwd_ratio) launches for these sizes and the current
 * developer knobs -- 0 = one slice per workgroup read from global memory (a slice does not fit LDS), 1 = one slice in LDS, 2 = a
 * slice pair in LDS, 4 / 8 = the packed walk with that many slices behind a ray (the workspace); negative on bad sizes or an
 * unknown store.  dt: the rows the launch writes (n_sel with an angle subset).  store: CTPVAE_SIDDON_STORE_*; only _POISSON changes
 * the answer (it has no packed form: never 4 or 8).  A batch longer than a launch takes (knob MAX_SLICES) goes in chunks: the
 * answer is the first chunk's form (a shorter last chunk decides for its own size).  Same bits in every form.  The launches and
 * ctpvae_siddon_fwd_workspace_bytes ask the same function (csrc/siddon.hip siddon_fwd_form_rule): the size rule is non-zero
 * whenever the answer here is 4 or 8. */
#define CTPVAE_SIDDON_STORE_RAYSUM 0   /* ctpvae_siddon_fwd_ws_f32 without meas */
#define CTPVAE_SIDDON_STORE_SIRT 1     /* ctpvae_siddon_fwd_ws_f32 with meas / rn2: (meas - A x) / rn2 */
#define CTPVAE_SIDDON_STORE_TV_DUAL 2  /* ctpvae_siddon_fwd_ws_tv_dual_f32 */
#define CTPVAE_SIDDON_STORE_GAUSSIAN 3 /* ctpvae_siddon_fwd_loglik_f32, _noise with CTPVAE_NOISE_GAUSSIAN */
#define CTPVAE_SIDDON_STORE_POISSON 4  /* ctpvae_siddon_fwd_loglik_noise_f32 with CTPVAE_NOISE_POISSON */
#define CTPVAE_SIDDON_STORE_RATIO 5    /* ctpvae_siddon_fwd_ratio_f32 */
int ctpvae_siddon_fwd_form(int oy, int ox, int oz, int dt, int dx, int store);
/* The likelihood training call on the ray-driven projector (calculate_log_prob_M_given_R(model="siddon"),
 * ctvae/helper_functions.py:336-368), for the forward model the reference's data were made with.
 *   _fwd_loglik:  the forward of ctpvae_siddon_fwd_ws_f32 (same dispatch, same workspace rule, same ray-sums) whose store is the
 *       Gaussian-Poisson log-probability of every ray-sum and, with dlp_dev, d lp / d ray-sum -- the expressions of
 *       ctpvae_loglik_fwd_f32 in its order: the two-step path's bits.  The tables sin_dev / cos_dev / quad_dev hold dt_all angles;
 *       sel_dev (int32 [n_sel], device; an index outside the table is clamped into it) picks the step's angles: output row k of
 *       every slice is table angle sel[k], in any order, repeats allowed; NULL: all dt_all angles (n_sel 0 or dt_all).  With
 *       rows = n_sel (or dt_all): lp_dev, dlp_dev (or NULL), sino_dev (or NULL: the ray-sums are not stored) [oy][rows][dx];
 *       dense = 1: mask_dev [oy][dt_all], meas_dev [oy][dt_all][dx] are read at the table angle; dense = 0: [oy][rows],
 *       [oy][rows][dx].  pnm_dev: one float on the device.  workspace_dev: ctpvae_siddon_fwd_workspace_bytes(oy, ox, oz) bytes
 *       (NULL when that is 0).
 *   _bwd_sel_scaled:  recon[s] = scale[s * scale_stride] * (A_sel^T data[s]), data_dev [oy][rows][dx], the transpose of the rows
 *       above as ctpvae_siddon_bwd_prepared_f32's gather: a pixel's terms arrive in libtomo's order over sel[0 .. n_sel), the
 *       factor multiplies once, in the store (scale_dev NULL: no factor; stride 0: one factor for the batch).  workspace_dev:
 *       ctpvae_siddon_bwd_workspace_bytes(>= oy, ox, oz, dt_all, dx) bytes PREPARED for the dense tables (_bwd_prepare, once per
 *       geometry): a step's subset costs no _prepare.  No atomics: equal bits run to run and to a call on the gathered tables.
 * oy == 0 returns without a launch; longer batches than a launch takes go in chunks, as in the calls above. */
int ctpvae_siddon_fwd_loglik_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                 const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                 const float *mask_dev, const float *meas_dev, int dense, const float *pnm_dev, float eps,
                                 void *workspace_dev, float *sino_dev, float *lp_dev, float *dlp_dev, ctpvae_stream_t stream);
/* _fwd_loglik with the noise model as an operand (CTPVAE_NOISE_GAUSSIAN: the call above, bit for bit; CTPVAE_NOISE_POISSON: the
 * expressions of ctpvae_poisson_loglik_fwd_f32 / _bwd_f32 on every ray-sum, eps ignored).  _bwd_sel_scaled serves both. */
int ctpvae_siddon_fwd_loglik_noise_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                       const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                       const float *mask_dev, const float *meas_dev, int dense, const float *pnm_dev, float eps,
                                       int noise, void *workspace_dev, float *sino_dev, float *lp_dev, float *dlp_dev,
                                       ctpvae_stream_t stream);
int ctpvae_siddon_bwd_sel_scaled_f32(const float *data_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                     const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                     const void *workspace_dev, const float *scale_dev, long long scale_stride, float *recon_dev,
                                     ctpvae_stream_t stream);
/* MLEM / OSEM (tomopy.recon(algorithm='mlem' | 'osem'); libtomo mlem.c / osem.c restated [3P-recalled: TomoPy 1.11.0]) as TWO
 * projector launches per block and iteration, with nothing elementwise in between (ct_pvae_amd/recon.py _mlem):
 *   _fwd_ratio:    the forward of ctpvae_siddon_fwd_ws_f32 (same dispatch, same workspace rule, same ray-sums) whose store is
 *       ratio = meas / (A obj) where the ray-sum != 0, else 0.  sel_dev / n_sel / dt_all as in _fwd_loglik: output row k of
 *       ratio_dev [oy][rows][dx] is table angle sel[k]; meas_dev [oy][dt_all][dx] is always read DENSE, at the table angle, so
 *       an OSEM block needs no gathered copy of the data.
 *   _bwd_sel_mul:  x <- x * ((A_sel^T ratio) / colsum) where colsum != 0, else x unchanged, in place: x_dev [oy][ox][oz],
 *       ratio_dev [oy][rows][dx], colsum_dev [ox][oz] the block's sum_dist = A_sel^T 1 (_bwd_sel_scaled of ones).  The gather
 *       and the workspace of _bwd_sel_scaled: PREPARED once for the dense tables, a block costs no _prepare; no atomics:
 *       equal bits run to run and to a call on the gathered tables.
 * ONE DEVIATION from libtomo: mlem.c skips only rays without segments and divides by a ray-sum of 0 on rays that do cross pixels
 * (inf / NaN, which an OSEM block that drives the background to exactly 0 does produce); here such a ratio is 0.  On rays
 * without segments the two rules agree.  oy == 0 returns without a launch; long batches go in chunks. */
int ctpvae_siddon_fwd_ratio_f32(const float *obj_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                const float *meas_dev, void *workspace_dev, float *ratio_dev, ctpvae_stream_t stream);
int ctpvae_siddon_bwd_sel_mul_f32(const float *ratio_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                  const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                  const void *workspace_dev, const float *colsum_dev, float *x_dev, ctpvae_stream_t stream);
/* Penalized likelihood (tomopy.recon(algorithm='pml_quad' | 'pml_hybrid' | 'ospml_quad' | 'ospml_hybrid'); libtomo pml_quad.c /
 * pml_hybrid.c / ospml_quad.c / ospml_hybrid.c restated [3P-recalled: TomoPy 1.11.0], the recollection checked by re-deriving the
 * update as De Pierro's separable surrogate): per block and iteration _fwd_ratio above, then this call -- again TWO launches with
 * nothing elementwise in between (ct_pvae_amd/recon.py _pml).  _bwd_sel_mul's gather, operands and workspace; its store is, per
 * pixel c = i * oz + j of every slice, in float32 and in this order, with u = (A_sel^T ratio)[c] and x = x_in[c]:
 *     E     = -(x * u)
 *     F = 0 ; P = 0 ; for q in the neighbour order below, skipping neighbours outside the grid:
 *             r   = x - x_in[k_q]
 *             gam = 1                                    (hybrid == 0: quadratic penalty)
 *                 = 1 / (1 + fabs(r / delta))            (hybrid != 0)
 *             t   = ((2 * beta) * w_q) * gam             (quadratic: (2 * beta) * w_q)
 *             F  += t ;  P -= t * (x + x_in[k_q])
 *     G     = P + colsum[c]
 *     S     = sqrtf(G * G - (8 * E) * F)
 *     x_out[c] = (-2 * E) / (G + S)        where G > 0
 *              = (-G + S) / (4 * F)        where G <= 0 and F != 0        (libtomo's form, which libtomo uses everywhere)
 *              = x                         where G <= 0 and F == 0        (only with beta == 0: a pixel no ray of the block crosses)
 *   Neighbour order (di, dj): (0,+1) (0,-1) (+1,0) (-1,0) (+1,+1) (+1,-1) (-1,+1) (-1,-1) -- libtomo's ind0 + 1, - 1, + ngridy,
 *   - ngridy, + ngridy + 1, + ngridy - 1, - ngridy + 1, - ngridy - 1.  Weights: direct a, diagonal a / sqrt(2), a = 1 / (n_direct +
 *   n_diag / sqrt(2)) over the neighbours that exist, libtomo's tables as float32 literals: interior 0.1464466094 / 0.1035533906,
 *   edge 0.2265409197 / 0.1601886205, corner 0.3693980625 / 0.2612038750.  Every neighbour is read from x_in_dev (Jacobi), so
 *   x_in_dev and x_out_dev [oy][ox][oz] are distinct buffers the caller swaps; x_in_dev is not written.  colsum_dev [ox][oz]: the
 *   block's sum_dist.  delta is read only with hybrid != 0.
 * THE SECOND FLAGGED DEVIATION (beside _fwd_ratio's guarded ratio): where G > 0 the positive root of 2 F x^2 + G x + E = 0 is taken
 * in its cancellation-free form; libtomo's form subtracts two nearly equal numbers there (beta = 0.01, 20 float32 iterations against
 * the same iteration in float64: 2.6e-4 to 5.7e-4 of the image's maximum, against 8.7e-7 for this form; tests/test_pml_cpu.py).
 * EINVAL before any HIP call: a null pointer, x_in_dev == x_out_dev, ox < 2 or oz < 2, beta negative or not finite, hybrid with
 * delta not > 0.  oy == 0 returns without a launch; long batches go in chunks. */
int ctpvae_siddon_bwd_sel_pml_f32(const float *ratio_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                  const int *quad_dev, int dt_all, int dx, float center, const int *sel_dev, int n_sel,
                                  const void *workspace_dev, const float *colsum_dev, float beta, float delta, int hybrid,
                                  const float *x_in_dev, float *x_out_dev, ctpvae_stream_t stream);
/* Round 4: an iteration of the TV STAND-IN of tomopy.recon(algorithm='tv') (README.md:221 of the reference asks for 'tv';
 * libtomo's tv.c is NOT restated -- ct_pvae_amd/recon.py says so on every call) as TWO projector launches instead of ~15 torch
 * ops around them: the diagonally preconditioned Chambolle-Pock iteration for min 1/2 |A x - b|^2 + lam TV(x) on K = (A; grad),
 *   _fwd_ws_tv_dual:  p <- (p + sigma (A xbar - b)) / (1 + sigma)         sigma_dev [dt][dx] = 1 / (row sums of A), p in place
 *   _bwd_tv_primal:   q' = q + 0.5 grad xbar; q <- q' / (max(|q'|, lam) / lam); x <- x - tau (A^T p - div q); xbar <- 2 x - x_old
 *                     tau_dev [ox][oz] = 1 / (column sums of A + 4); x in place; xbar / qx / qy read at neighbouring pixels:
 *                     *_in and *_out must be distinct buffers (the caller swaps them every iteration)
 * with forward differences (zero at the far edges) and their negative transpose, every operation in the order
 * oracle/radon_oracle.py tv_standin() states: the kernels give its bits. */
int ctpvae_siddon_fwd_ws_tv_dual_f32(const float *xbar_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                     const int *quad_dev, int dt, int dx, float center, const float *meas_dev,
                                     const float *sigma_dev, void *workspace_dev, float *p_dev, ctpvae_stream_t stream);
int ctpvae_siddon_bwd_tv_primal_f32(const float *p_dev, int oy, int ox, int oz, const float *sin_dev, const float *cos_dev,
                                    const int *quad_dev, int dt, int dx, float center, const void *workspace_dev,
                                    const float *tau_dev, float lam, float *x_dev, const float *xbar_in_dev, float *xbar_out_dev,
                                    const float *qx_in_dev, const float *qy_in_dev, float *qx_out_dev, float *qy_out_dev,
                                    ctpvae_stream_t stream);

/* ---- a6: filtered back-projection (float64, as the reference runs it) -----------------------
 * filter: circular convolution of every sinogram row with hker_dev [P] = Re(ifft(filter_1d)), which
 * equals Re(ifft(fft(row) * filter_1d)).  sino_dev, out_dev [R][P].
 * backproject: filt_dev [B][A][P], cos_dev/sin_dev [A] fp64 of theta, recon_dev [B][X][Y]. */
int ctpvae_fbp_filter_f64(const double *sino_dev, int R, int P, const double *hker_dev, double *out_dev,
                          ctpvae_stream_t stream);
int ctpvae_fbp_backproject_f64(const double *filt_dev, int B, int A, int P, const double *cos_dev,
                               const double *sin_dev, int X, int Y, double *recon_dev,
                               ctpvae_stream_t stream);
/* ... with the sampling geometry spelled out: pixel (i, j) at (i - x0, j - y0), detector sample k at k - t0.  The reference's
 * iradon is x0 = X / 2, y0 = Y / 2, t0 = P / 2 (the entry point above); tomopy's ray-driven grid -- pixel centres at half-
 * integers, bin d at d - (P - 1) / 2 (libtomo utils.c preprocessing / calc_coords) -- is x0 = (X - 1) / 2, y0 = (Y - 1) / 2,
 * t0 = (P - 1) / 2: what the gridrec stand-in of ct_pvae_amd/recon.py uses on sinograms made by create_sinogram. */
int ctpvae_fbp_backproject_geom_f64(const double *filt_dev, int B, int A, int P, const double *cos_dev,
                                    const double *sin_dev, int X, int Y, double x0, double y0, double t0,
                                    double *recon_dev, ctpvae_stream_t stream);

/* The transpose of ctpvae_fbp_backproject_geom_f64 (iradon's gradient; the reference's iradon, ctvae/fbp_tensorflow.py:14-75, is
 * TF ops and so differentiable): grecon_dev [B][X][Y] -> gfilt_dev [B][A][P], every output one ordered fp64 sum over pixels.
 * The transpose of ctpvae_fbp_filter_f64 is the same entry point with the kernel reversed, hker[(P - n) % P]. */
int ctpvae_fbp_backproject_bwd_f64(const double *grecon_dev, int B, int A, int P, const double *cos_dev,
                                   const double *sin_dev, int X, int Y, double x0, double y0, double t0,
                                   double *gfilt_dev, ctpvae_stream_t stream);

/* ---- f3: TomoPy's gridrec (the encoder's default input channel: tomopy.recon(..., algorithm='gridrec') at
 * ctvae/helper_functions.py:503, defaults ctvae/main_ct_vae.py:111-112; evaluate_sinogram ctvae/helper_functions.py:445-457;
 * bin/final_merit.py:58,81) -- TomoPy 1.11.0 libtomo/gridrec/gridrec.c [recalled, see oracle/gridrec_oracle.c]: zero-padded
 * 1-D FFT of every projection (two slices per complex transform), filter x centre phase, convolution onto a pdim x pdim
 * frequency grid with the separable prolate-spheroidal window, 2-D FFT, window correction.  pdim = the power of two >= dx.
 * _tables_host_f32 fills a HOST buffer of _tables_bytes() bytes (twiddles, window, correction, trig, filter x phase; every
 * pointer host memory; filter_name 0 none, 1 shepp, 2 cosine, 3 hann, 4 hamming, 5 ramlak, 6 parzen = tomopy's default for
 * gridrec, 7 butterworth with filter_par = {cutoff, order}); the caller uploads it.  _f32: data_dev [dy][dt][dx] (sinogram
 * order) -> recon_dev [dy][ngridx][ngridy]; deterministic (the convolution is a gather in gridrec.c's order, no atomics);
 * workspace_dev: _workspace_bytes() bytes of device memory, contents undefined. */
long long ctpvae_gridrec_tables_bytes(int dt, int dx);
int ctpvae_gridrec_tables_host_f32(int dt, int dx, float center, const float *theta, int filter_name, const float *filter_par,
                                   void *tables);
long long ctpvae_gridrec_workspace_bytes(int dy, int dt, int dx);
int ctpvae_gridrec_f32(const float *data_dev, int dy, int dt, int dx, const void *tables_dev, int ngridx, int ngridy,
                       void *workspace_dev, float *recon_dev, ctpvae_stream_t stream);

/* Per-object sums of a log-probability array lp_dev [S][A][PW] -> out_dev [S] (reduce_sum over angles and bins,
 * ctvae/helper_functions.py:305-306), in a FIXED order so that every path gives the same bits: the [A][PW] values of a slice
 * are cut into 64-lane tasks (partition 0: the planned kernels' tasks -- angle a, bin block jb = the two 32-bin bands
 * [c - 32 (jb + 1), c - 32 jb) and [c + 32 jb, c + 32 (jb + 1)), c = PW / 2, lanes 0..31 and 32..63; partition 1: the tiled
 * reduce pass's contiguous 64-bin blocks), a task's values are added by the xor butterfly 32, 16, 8, 4, 2, 1 (lanes
 * without a bin add +0.0f); an angle's task sums are added in ascending order (S_a), and the object's sum is
 * ((0 + B_0) + B_1) + ... with B_g = the same butterfly over S_(64 g) .. S_(64 g + 63) (angles past A add +0.0f).
 * _tasks_per_row: tasks per angle.
 * _part_floats (round 4, ABI 3300): the floats of the `lp_part_dev` workspace the fused per-object sums of
 * ctpvae_rotate_fwd_compact_f32 (partition 0) / ctpvae_rotate_fwd_tiled_compact_f32 (partition 1) take for S slices and
 * n_angles projected angles: one partial sum per (slice, angle, task) and, behind them, ONE ARRIVAL COUNTER PER SLICE, which
 * must be ZERO before the workspace's first use (hipMemset once, when it is allocated); every launch leaves them zero.  The
 * counters serve the developer knob FOLD_SUMS = 1 (the ordered sum of a slice's partials inside the projector launch, by the
 * workgroup that finishes the slice last: same bits, one launch less, measured 0.3-2 us SLOWER than the default's second
 * launch); the default does not touch them.  One workspace serves one launch at a time (launches on ONE
 * stream, as every other caller-owned workspace of this header). */
int ctpvae_loglik_tasks_per_row(int PW, int partition);
long long ctpvae_loglik_part_floats(int S, int n_angles, int PW, int partition);
int ctpvae_loglik_object_sums_f32(const float *lp_dev, int S, int A, int PW, int partition, float *out_dev,
                                  ctpvae_stream_t stream);

/* ---- a8: Gaussian-approximated Poisson log-likelihood epilogue ------------------------------
 * proj_dev, x_dev, out_dev [B][A][P]; mask_dev [B][A]; pnm_dev points at ONE fp32 on the device (the
 * reference keeps poisson_noise_multiplier in a Variable).
 *   loc = proj*mask ; scale = eps + sqrt(loc/pnm + eps) ; out = Normal(loc, scale).log_prob(x)
 * bwd: gproj = gout * d out / d proj  (gpnm_dev, if not NULL, receives sum gout * d out / d pnm). */
int ctpvae_loglik_fwd_f32(const float *proj_dev, const float *mask_dev, const float *x_dev, int B, int A,
                          int P, const float *pnm_dev, float eps, float *out_dev, ctpvae_stream_t stream);
int ctpvae_loglik_bwd_f32(const float *proj_dev, const float *mask_dev, const float *x_dev,
                          const float *gout_dev, int B, int A, int P, const float *pnm_dev, float eps,
                          float *gproj_dev, float *gpnm_dev, ctpvae_stream_t stream);

/* ---- a8, noise = poisson: the exact model of the measurements (ctvae/toy_mcmc_v2_functions.py:30-64,
 * tfd.Poisson(proj * mask * pnm, force_probs_to_zero_outside_support=False).log_prob(x * pnm); TFP 0.14 Poisson._log_prob).
 * Shapes as above.  With k = x * pnm and lam = (proj * mask) * pnm:
 *   out = multiply_no_nan(log lam, k) - lgamma(k + 1) - lam
 * evaluated in fp32 as  k (log1p(u) - u) - r(k),  u = (lam - k) / k,  r(k) = lgamma(k + 1) - (k log k - k)  (the Stirling
 * remainder: 0.5 log(2 pi k) + 1/12k - 1/360k^3 + 1/1260k^5 from k = 8 on, lgammaf below) -- the textbook form's three terms are
 * 1e5 .. 1e7 at pnm = 1e4 and cancel to a value of order 1 .. 10 (max error against float64 on 200,000 draws from the model: 0.09;
 * this form: 2.0e-6 / 1.3e-5 / 1.0e-4 at pnm 1 / 1e2 / 1e4).  What is left is not r(k) but the rounding of lam and k themselves,
 * ~ 2^-23 |k - lam|, and the cancellation in log1p(u) - u at small u.
 *   k == 0:           out = -lam; lam == 0 and k == 0 (a masked-out angle: mask and measurement are 0): out = 0
 *   lam == 0, k > 0:  out = -inf          lam < 0: NaN, as TFP; nothing traps          k < 0: -inf (outside the support)
 *   k need not be an integer.
 * bwd: gproj = gout * mask * pnm * (k - lam) / lam; k == 0: gout * (-mask * pnm), so 0 at a masked angle.  The derivative is that
 * of the formula wherever the formula can be differentiated, as TFP's autograd gives it: it stays finite where out is NaN
 * (lam < 0: d log lam = 1 / lam) or -inf (k < 0), and is +inf at lam == 0, k > 0.  pnm is DATA in this
 * model: there is no d / d pnm.  Parity with TFP's own bits is not pinned (different log / lgamma implementations). */
int ctpvae_poisson_loglik_fwd_f32(const float *proj_dev, const float *mask_dev, const float *x_dev, int B, int A, int P,
                                  const float *pnm_dev, float *out_dev, ctpvae_stream_t stream);
int ctpvae_poisson_loglik_bwd_f32(const float *proj_dev, const float *mask_dev, const float *x_dev, const float *gout_dev,
                                  int B, int A, int P, const float *pnm_dev, float *gproj_dev, ctpvae_stream_t stream);

/* ---- f2: sparse noisy measurements (the step that feeds the training loop) -------------------------------------
 * ctvae/create_masks.py:80-103 in one launch: out[s][a][j] = Poisson(max(sino[s][a][j], 0) * mask[s][a] * pnm) / pnm.
 * sino_dev, out_dev [S][A][P]; mask_dev [S][A].  Counter-based and fully specified (csrc/poisson.hip): element e draws
 * from Philox4x32-10(counter = (e, block), key = seed), multiplication method below rate 10, transformed rejection
 * (PTRS) from there, exp / log by fixed double-precision series -- the same counts on any device or host for a seed,
 * whatever the launch shape.  The reference draws with tfd.Poisson(...).sample(): same distribution, other bits. */
int ctpvae_poisson_measure_f32(const float *sino_dev, const float *mask_dev, int S, int A, int P, float pnm,
                               unsigned long long seed, float *out_dev, ctpvae_stream_t stream);
/* Host-side known-answer hook for the generator: the four words of Philox4x32-10(counter4, key2) (host pointers). */
int ctpvae_philox4x32_10(const unsigned *counter4, const unsigned *key2, unsigned *out4);

/* ---- HMC posterior sampler for small objects (bin/toy_mcmc_v2.py, ctvae/toy_mcmc_v2_functions.py:66-95): one 64-lane wave per chain,
 * n_steps whole transitions per launch (csrc/hmc.hip states the target density, the orders of its sums and the layout of the random
 * numbers).  Square objects of K = N * N <= 64 pixels, the rotate model with NEAREST sampling on the unpadded canvas (P = N), at most
 * CTPVAE_HMC_MAX_ANGLES angles, fp32.  T8_dev / Tinv8_dev [A][8]: the tables of ctpvae_rotate_transforms(_host)_f32 for H = W = N.
 * C chains; chain c samples the posterior of object c / chains_per_object: mask_dev [B][A], meas_dev [B][A][N], B = C /
 * chains_per_object.  The prior is a mixture of M <= CTPVAE_HMC_MAX_COMPONENTS Dirichlets: logw_dev [M] (log weights), alpha_dev
 * [M][K] (concentrations), lbeta_dev [M] (log of the multivariate beta function of each row), all fp32 on the device, computed by
 * the caller (in float64, rounded once).
 *   _state_floats(K): floats of one chain's carried state -- x [K-1], dT/dx [K-1], T, the step size, and the BITS of the unsigned
 *     32-bit index of the chain's next step: 2K + 1.
 *   _init_f32: state_dev [C][2K + 1] from simplex starting points start_dev [C][K] (the inverse bijector; every entry > 0), or from
 *     x = 0 when start_dev is NULL; evaluates T and dT/dx there; step index 0.
 *   _run_f32: n_steps (1 .. CTPVAE_HMC_MAX_STEPS) transitions of every chain from its state's step index t0, with L
 *     (1 .. CTPVAE_HMC_MAX_LEAPFROGS) leapfrog steps each; the step size adapts (x 1.01f if min(log accept ratio, 0) > log 0.75, else
 *     / 1.01f, a NaN ratio included) while the step's index < num_adaptation_steps.  The draws of chain c at step t depend on (seed,
 *     first_chain + c, t) alone, so a run may be cut into launches, and its chains into calls, in any way.  Steps with index >=
 *     n_keep_from are stored: the first such step of THIS launch is row 0 of samples_out_dev [rows][C][K] (points of the simplex),
 *     lar_out_dev, accepted_out_dev (0.0f / 1.0f), target_out_dev [rows][C] (log accept ratio, decision, T after the decision);
 *     rows <= n_steps.  CTPVAE_HMC_MAX_STEPS bounds the time of one launch: the largest power of two that keeps a launch of
 *     the slowest shape measured with 5 leapfrog steps (8 x 8, 180 angles: 149 us per transition) under 100 ms on the MI355X.  At
 *     the extremes this entry point admits (256 angles, 32 leapfrog steps) a full launch takes about 644 ms
 *     (profiles/hmc_timing.txt). */
#define CTPVAE_HMC_MAX_ANGLES 256
#define CTPVAE_HMC_MAX_COMPONENTS 4
#define CTPVAE_HMC_MAX_LEAPFROGS 32
#define CTPVAE_HMC_MAX_STEPS 512
int ctpvae_hmc_state_floats(int K);
int ctpvae_hmc_init_f32(float *state_dev, int C, int chains_per_object, int N, const float *T8_dev, const float *Tinv8_dev, int A,
                        const float *mask_dev, const float *meas_dev, float pnm, int M, const float *logw_dev, const float *alpha_dev,
                        const float *lbeta_dev, const float *start_dev, float step_size, ctpvae_stream_t stream);
int ctpvae_hmc_run_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                       const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                       const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps, unsigned n_keep_from,
                       unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev, float *lar_out_dev,
                       float *accepted_out_dev, float *target_out_dev, ctpvae_stream_t stream);

/* ---- the same sampler for objects beyond 64 pixels: one workgroup of W = ceil(K / 64) waves per chain, one pixel per thread, 2 <= N <= 32
 * (csrc/hmc_wg.hip states how the orders of the sums generalise; everything else -- target, transition, random numbers, state -- is
 * csrc/hmc.hip's).  _wg_init_f32 and _wg_run_f32 take the arguments of ctpvae_hmc_init_f32 and ctpvae_hmc_run_f32 with their meaning and
 * limits, except 2 <= N <= 32; for N <= 8 (one wave) they give those entry points' bits.  The tap tables of a launch sit in LDS: an
 * (N, A) whose request exceeds the 163,840 bytes a workgroup has on gfx950 is refused before any launch (32 x 32 admits 46 angles, 23 x 23
 * 86, 16 x 16 168, 12 x 12 and smaller all 256).  One launch should hold no more chains than the device keeps resident (_wg_resident_chains); the caller
 * cuts C into launches -- state_dev, start_dev and the outputs of a launch are those of ITS chains, first_chain the id of its first.
 *   _wg_state_floats(K): 2K + 1 for 4 <= K <= 1024.
 *   _wg_lds_bytes(N, A): dynamic LDS of one workgroup (host only), also where it exceeds what a workgroup has.
 *   _wg_resident_chains(N, A, chains_out): multiprocessors of the current device x the occupancy query of the run kernel at this block size
 *     and LDS request (at least 1 per multiprocessor).
 * CTPVAE_HMC_MAX_STEPS bounds n_steps here too; ct_pvae_amd/mcmc.py's MAX_STEPS_PER_LAUNCH_WG is the measured cap of this form
 * (profiles/hmc_wg_timing.txt). */
int ctpvae_hmc_wg_state_floats(int K);
long long ctpvae_hmc_wg_lds_bytes(int N, int A);
int ctpvae_hmc_wg_resident_chains(int N, int A, int *chains_out);
int ctpvae_hmc_wg_init_f32(float *state_dev, int C, int chains_per_object, int N, const float *T8_dev, const float *Tinv8_dev, int A,
                           const float *mask_dev, const float *meas_dev, float pnm, int M, const float *logw_dev, const float *alpha_dev,
                           const float *lbeta_dev, const float *start_dev, float step_size, ctpvae_stream_t stream);
int ctpvae_hmc_wg_run_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                          const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                          const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps, unsigned n_keep_from,
                          unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev, float *lar_out_dev,
                          float *accepted_out_dev, float *target_out_dev, ctpvae_stream_t stream);

/* ---- the HMC sampler with the chains' per-pixel marginals accumulated inside the launch (csrc/hmc_marginals.hip states the layout and
 * the orders): the transitions of ctpvae_hmc_run_f32 bit for bit -- same arguments, same state (ctpvae_hmc_init_f32 starts it), same
 * random numbers -- and, for every kept step (index >= n_keep_from) and pixel k < K, with O the sample _run_f32 would store:
 *   hist_dev [B][K][bins + 2] int64: + 1 in the column of O under the bin rule of ctpvae_tn_marginals_f32 (t = (O - lo) / width in
 *     fp32; column 0 if !(t >= 0), NaN too; bins + 1 if t >= bins; else 1 + (int)t), pooled over the chains of object c /
 *     chains_per_object; rows as in the P-VAE's marginals, 1 <= bins <= CTPVAE_MARGINALS_MAX_BINS.  Integer atomics: any order, same bits.
 *   mom_dev [2][2][C][K] float64: [h][0] += (double)O and [h][1] += (double)O * (double)O, h = 0 for steps with index < n_half_from
 *     and 1 from there on.  Each sum is strictly sequential over the chain's own steps in ascending order, however the run is cut into
 *     launches; a chain's sums do not depend on the other chains.
 *   accepted_dev [C] int64: + 1 per accepted kept step.
 * A launch ADDS to the three arrays: zero them before the first (8-byte aligned, never NULL).  samples_out_dev, lar_out_dev,
 * accepted_out_dev, target_out_dev: all four as in _run_f32, or all four NULL -- then nothing is stored per step and no argument's
 * size depends on the number of steps; any other mix is refused.  n_steps is 1 .. CTPVAE_HMC_MAX_STEPS here too: the longest launch
 * of the shape that sizes that cap (8 x 8, 180 angles, 512 steps) with bins = 254 takes 78.9 ms on the MI355X, under 100 ms
 * (profiles/hmc_marginals_timing.txt; _run_f32's: 76.4 ms).
 *   _marginals_lds_bytes(N, A, bins): dynamic LDS of one workgroup (host only): the sampler's tables plus K * (bins + 2) * 4 bytes of
 *     counts, at most 121 KiB (8 x 8, 256 angles, 254 bins); the entry point raises the kernel's limit above the default 64 KiB. */
long long ctpvae_hmc_marginals_lds_bytes(int N, int A, int bins);
int ctpvae_hmc_run_marginals_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                                 const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                                 const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps,
                                 unsigned n_keep_from, unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev,
                                 float *lar_out_dev, float *accepted_out_dev, float *target_out_dev, unsigned n_half_from, float lo,
                                 float width, int bins, long long *hist_dev, double *mom_dev, long long *accepted_dev,
                                 ctpvae_stream_t stream);

/* ---- ctpvae_hmc_run_marginals_f32 with the raw sums of the chains' autocovariance and of the covariance between pixels accumulated in
 * the same launch (csrc/hmc_diagnostics.hip states the layout and the orders).  Every argument of _run_marginals_f32 with its meaning;
 * with max_lag = 0 and xx_dev NULL the three arrays get _run_marginals_f32's bits.  For kept step j (index n_keep_from + j), pixel
 * k < K and x = O_k, after the marginals' updates:
 *   max_lag = Lm, 1 .. CTPVAE_HMC_MAX_LAG:  ring_dev [C][Lm + 1][K] fp32 slot j mod (Lm + 1) = x;  head_dev [C][Lm][K] fp32 row j = x while
 *     j < Lm;  lag_dev [C][Lm + 1][K] float64 row l += (double)x * (double)(the chain's kept value of pixel k at step j - l), l = 0 ..
 *     min(j, Lm) ascending.  Lm = 0: the three pointers are NULL.
 *   xx_dev [C][K][K] float64 (or NULL: off):  [k][i] += (double)O_k * (double)O_i, i ascending; [k][i] and [i][k] are equal by bits.
 * Every sum is strictly sequential over the chain's own kept steps in ascending order, one rounding per step (the products are exact),
 * however the run is cut into launches and its chains into calls.  A launch ADDS: zero all arrays before the first (lag and xx 8-byte
 * aligned).
 *   _diagnostics_lds_bytes(N, A, bins, max_lag, cov): dynamic LDS of one workgroup (host only): _marginals_lds_bytes rounded up to 8, then
 *     (Lm + 1) * K * 4 (rounded up to 8) + (Lm + 1) * K * 8 bytes when Lm > 0 and K * K * 8 when cov != 0.  _run_diagnostics_f32 refuses a
 *     request above the 163,840 bytes a workgroup has on gfx950 (8 x 8, 256 angles, 254 bins, 64 lags and cov: 205,856) before any
 *     launch; lower bins or max_lag, or turn cov off. */
#define CTPVAE_HMC_MAX_LAG 64
long long ctpvae_hmc_diagnostics_lds_bytes(int N, int A, int bins, int max_lag, int cov);
int ctpvae_hmc_run_diagnostics_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                                   const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                                   const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps,
                                   unsigned n_keep_from, unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev,
                                   float *lar_out_dev, float *accepted_out_dev, float *target_out_dev, unsigned n_half_from, float lo,
                                   float width, int bins, long long *hist_dev, double *mom_dev, long long *accepted_dev, int max_lag,
                                   double *lag_dev, float *ring_dev, float *head_dev, double *xx_dev, ctpvae_stream_t stream);

/* ---- the P-VAE decoder's TruncatedNormal output head (ctvae/helper_functions.py:198-201, :273): sample, log-density and its
 * per-object sum in ONE launch, their gradients in one more (csrc/head.hip states the function, the order of the sum and the layout
 * of the random numbers).  alpha_dev, beta_dev [n][pix]: the decoder's raw outputs, pix = X * Y pixels per object, fp32.
 *   loc = pr(alpha), scale = pr(beta), pr(t) = t >= 1 ? t : exp(t - 1) + FLT_EPSILON;  TruncatedNormal(loc, scale, low 0, high 1e10)
 *   x = max(loc + scale ndtri(clamp(Pa + u Z, 1e-7, 1 - 1e-7)), 0),  Pa = Phi(-loc / scale), Z = 1 - Pa
 *   lp = -zeta^2 / 2 - log(2 pi) / 2 - log scale - log Z,  zeta = (x - loc) / scale
 * u of pixel `pixel` of object o is word e & 3 of Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), draw, 0x544E48), key = seed)
 * with the flat 64-bit index e = (first_object + o) * pix + pixel, u = ((w >> 8) + 0.5f) * 2^-24: a batch cut into calls with
 * first_object draws what the whole batch draws.  A non-null u_dev [n][pix] replaces the generator (tests: the clamps cannot be
 * reached otherwise).
 *   _fwd_f32: x_out_dev [n][pix], lp_sum_out_dev [n] (the sum of an object's lp in the fixed order of csrc/head.hip: the same bits
 *     whatever n and first_object), lp_elem_out_dev [n][pix] or NULL.
 *   _bwd_f32: g_alpha_out_dev, g_beta_out_dev [n][pix] for the cotangents g_x_dev [n][pix] and g_lp_dev [n] (either may be NULL: zero),
 *     as autograd gives them on the composition above, lp's path through x included.  Nothing is saved by the forward: the backward
 *     takes the same alpha, beta, first_object, seed, draw (and u_dev) and re-evaluates the pixel.
 *   _uniforms_host_f32: the generator's u for the same arguments into HOST memory u_out_host [n][pix]; needs no GPU.
 * n * pix <= 2^31 - 1; first_object >= 0. */
int ctpvae_tn_head_fwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                           unsigned long long seed, unsigned draw, const float *u_dev, float *x_out_dev, float *lp_sum_out_dev,
                           float *lp_elem_out_dev, ctpvae_stream_t stream);
int ctpvae_tn_head_bwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                           unsigned long long seed, unsigned draw, const float *u_dev, const float *g_x_dev, const float *g_lp_dev,
                           float *g_alpha_out_dev, float *g_beta_out_dev, ctpvae_stream_t stream);
int ctpvae_tn_head_uniforms_host_f32(int n, int pix, long long first_object, unsigned long long seed, unsigned draw, float *u_out_host);

/* ---- the Beta output head (added at ABI 3400): the P-VAE decoder's default output distribution, Beta(pr(alpha), pr(beta)), as one
 * forward and one backward launch (csrc/beta_head.hip states the function, the stream, the order of the per-object sum and the
 * backward's arithmetic).  alpha_dev, beta_dev [n][pix] fp32, the decoder's raw outputs; 0 < sqrt_reg < 0.5 is the clamp of the sample
 * inside the log-density.  The draws of pixel `pixel` of object o are words 0 .. 2 of the blocks
 *   Philox4x32-10((lo32(e), hi32(e), draw, 0x42000000 | gamma << 8 | attempt), key = seed),  e = (first_object + o) * pix + pixel,
 * one block per (pixel, gamma, attempt), attempt < 16.
 *   _fwd_f32: x_out_dev [n][pix] the sample (not clamped), lp_sum_out_dev [n] the per-object sum of the log-densities (fixed order),
 *     lp_elem_out_dev [n][pix] or NULL, aux_out_dev [n][pix][2][4] or NULL: (zn, ub, attempt, lg) of the accepted attempt of each gamma
 *     (tests only).
 *   _bwd_f32: g_alpha_out_dev, g_beta_out_dev [n][pix] for the cotangents g_x_dev [n][pix] and g_lp_dev [n] (either may be NULL: zero):
 *     the implicit reparameterisation gradient of each gamma.  Nothing is saved by the forward: the backward redraws.
 *   _words_host_u32: the Philox words of one (gamma, attempt) into HOST memory out_host [n][pix][4]; needs no GPU.
 * n * pix <= 2^31 - 1; first_object >= 0. */
int ctpvae_beta_head_fwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                             unsigned long long seed, unsigned draw, float sqrt_reg, float *x_out_dev, float *lp_sum_out_dev,
                             float *lp_elem_out_dev, float *aux_out_dev, ctpvae_stream_t stream);
int ctpvae_beta_head_bwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                             unsigned long long seed, unsigned draw, float sqrt_reg, const float *g_x_dev, const float *g_lp_dev,
                             float *g_alpha_out_dev, float *g_beta_out_dev, ctpvae_stream_t stream);
int ctpvae_beta_head_words_host_u32(int n, int pix, long long first_object, unsigned long long seed, unsigned draw, int gamma,
                                    int attempt, unsigned *out_host);

/* ---- per-pixel marginals of the TruncatedNormal output head (the reference's CT_VAE.pixel_dist, ctvae/main_ct_vae.py:648-731): the
 * histogram, the sum and the sum of squares of the samples of every pixel, with no sample written to memory (csrc/marginals.hip
 * states the layout and the fixed order of the float64 sums).  alpha_dev, beta_dev [n][pix] as for ctpvae_tn_head_fwd_f32.  The launch
 * covers the n * pix * draws samples (o, pixel, k), k < draws: each IS, bit for bit, the x that ctpvae_tn_head_fwd_f32 writes for that
 * object and pixel with draw = draw0 + k and the same seed and first_object.  All n objects are samples of the SAME pix pixels.
 *   Bin of a sample x, in fp32: t = (x - lo) / width (one subtraction, one correctly rounded division); column 0 if !(t >= 0) (NaN
 *   too), column bins + 1 if t >= bins, otherwise column 1 + (int)t.
 *   State, caller-owned, on the device, ADDED to (zero it first; any number of launches on one stream is well defined):
 *     hist_dev [pix][bins + 2] int64 counts;  s1_dev, s2_dev [pix] float64: the sum of the samples and of their squares, each fp32
 *     sample widened to double first.  Counts are combined with integer atomics; the float64 sums use no floating-point atomics and a
 *     fixed order, so one sequence of calls gives one set of bits in all three.
 *   _workspace_bytes: bytes of workspace_dev for (n, pix, draws): at most 1024 * pix, whatever draws is.  The workspace carries
 *     nothing between calls.
 *   _bin_host_f32: the bin rule applied to count values in HOST memory, columns into col_out_host [count]; needs no GPU.
 * 1 <= bins <= CTPVAE_MARGINALS_MAX_BINS; width > 0, lo and width finite; draws >= 1, draw0 + draws <= 2^32, n * draws < 2^32;
 * n * pix <= 2^31 - 1; first_object >= 0; state and workspace 8-byte aligned. */
#define CTPVAE_MARGINALS_MAX_BINS 254
long long ctpvae_tn_marginals_workspace_bytes(int n, int pix, unsigned draws);
int ctpvae_tn_marginals_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                            unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                            long long *hist_dev, double *s1_dev, double *s2_dev, void *workspace_dev, ctpvae_stream_t stream);
int ctpvae_tn_marginals_bin_host_f32(const float *x_host, long long count, float lo, float width, int bins, int *col_out_host);

/* ---- per-pixel marginals of the Beta output head, the reference's default output distribution (backward compatible additions at
 * ABI 3400; csrc/beta_marginals.hip): ctpvae_tn_marginals_f32 with the other head's samples.  alpha_dev, beta_dev [n][pix] as for
 * ctpvae_beta_head_fwd_f32; sample (o, pixel, k), k < draws, IS, bit for bit, the x that ctpvae_beta_head_fwd_f32 writes for that object
 * and pixel with draw = draw0 + k and the same seed and first_object (x is not clamped: sqrt_reg plays no part in it).  A NaN alpha or
 * beta gives NaN samples for that pixel: they count in column 0 and make its s1, s2 NaN; no other pixel is touched.  The state, the bin
 * rule (on the host: ctpvae_tn_marginals_bin_host_f32, which does not depend on the head), the workspace rule, the order of the float64
 * sums, the argument rules and the refusals are ctpvae_tn_marginals_f32's; every check is made before any launch. */
long long ctpvae_beta_marginals_workspace_bytes(int n, int pix, unsigned draws);
int ctpvae_beta_marginals_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                              unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                              long long *hist_dev, double *s1_dev, double *s2_dev, void *workspace_dev, ctpvae_stream_t stream);

/* ---- the P-VAE's Normal latent block at one skip level (ctvae/helper_functions.py:247-252, :267, :325-327): the ns reparameterised
 * samples, the KL term against N(0, 1) and its per-object sum in ONE launch, their gradients in one more (csrc/latent.hip states the
 * function, the order of the sum and the layout of the random numbers).  skip_dev [B][2][len]: the encoder's output at the level,
 * len = C * H * W; the first half of an object is loc, the second log_scale, fp32.
 *   scale = pr(log_scale) + sqrt_reg, pr(t) = t >= 1 ? t : exp(t - 1) + FLT_EPSILON
 *   z[s * B + b][i] = loc + scale * eps(s, b, i);   kl[b][i] = 0.5 (scale^2 + loc^2 - 1) - log scale;   KL[b] = sum_i kl[b][i]
 * eps of element i of object b, sample s, comes from word e & 3 of Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), draw,
 * 0x4C000000 | level << 16 | s), key = seed), e = (first_object + b) * len + i:  t = (((w >> 7) & 0xFFFFFF) + 0.5f) * 2^-25,
 * eps = bit 31 of w ? ndtri(t) : -ndtri(t).  A batch cut into calls with first_object draws what the whole batch draws.  A non-null
 * eps_dev [ns * B][len] replaces the generator (tests).
 *   _fwd_f32: z_out_dev [ns * B][len], kl_sum_out_dev [B] (the sum of an object's kl in the fixed order of csrc/latent.hip: the same
 *     bits whatever B and first_object), kl_elem_out_dev [B][len] or NULL, eps_out_dev [ns * B][len] or NULL (the draws used).
 *   _bwd_f32: g_skip_out_dev [B][2][len] for the cotangents g_z_dev [ns * B][len] and g_kl_dev [B] (either may be NULL: zero).  Nothing
 *     is saved by the forward: the backward takes the same skip, sqrt_reg, first_object, seed, draw, level (and eps_dev).
 *   _draws_host_f32: the signed tail probability v = bit 31 ? -t : +t of the same arguments into HOST memory v_out_host [ns][n][len]
 *     (eps = copysign(-ndtri(|v|), v)); needs no GPU and evaluates no quantile.
 * ns * B * len <= 2^31 - 1; 1 <= ns <= 65535; level <= 255; first_object >= 0. */
int ctpvae_latent_fwd_f32(const float *skip_dev, int B, int len, int ns, float sqrt_reg, long long first_object, unsigned long long seed,
                          unsigned draw, unsigned level, const float *eps_dev, float *z_out_dev, float *kl_sum_out_dev,
                          float *kl_elem_out_dev, float *eps_out_dev, ctpvae_stream_t stream);
int ctpvae_latent_bwd_f32(const float *skip_dev, int B, int len, int ns, float sqrt_reg, long long first_object, unsigned long long seed,
                          unsigned draw, unsigned level, const float *eps_dev, const float *g_z_dev, const float *g_kl_dev,
                          float *g_skip_out_dev, ctpvae_stream_t stream);
int ctpvae_latent_draws_host_f32(int n, int len, int ns, long long first_object, unsigned long long seed, unsigned draw, unsigned level,
                                 float *v_out_host);

/* ---- the P-VAE's DEFAULT (Beta) latent block at one skip level (ctvae/helper_functions.py:249-254, :267, :325-327; backward
 * compatible additions at ABI 3400): the ns reparameterised samples of Beta(pr(loc), pr(log_scale)), the KL term against the
 * Beta(0.5, 0.5) prior and its per-object sum in ONE launch, their gradients in one more (csrc/beta_latent.hip states the function, the
 * work split, the order of the sum and the backward's arithmetic).  skip_dev [B][2][len] as for ctpvae_latent_fwd_f32; there is no
 * sqrt_reg.  a = pr(loc), b1 = pr(log_scale);
 *   z[s * B + b][i] = 1 / (1 + exp(lg_1 - lg_0)), lg_j the log-space gammas of the Beta head's sampler (csrc/beta_head.hip);
 *   kl[b][i] = ln pi - lbeta(a, b1) + (a - 1/2) psi(a) + (b1 - 1/2) psi(b1) + (1 - a - b1) psi(a + b1), float64 on the fp32 a, b1, rounded once.
 * The draws of element i of object b, sample s, are words 0 .. 2 of the blocks
 *   Philox4x32-10((lo32(e), hi32(e), draw, 0x51000000 | level << 16 | s << 5 | gamma << 4 | attempt), key = seed),  e = (first_object + b) * len + i,
 * one block per (element, sample, gamma, attempt), attempt < 16.  Top bytes of the fourth counter word in use: 0x51 (here), 0x42 (the
 * Beta head), 0x44 (dropout), 0x4C (the Normal latents); whole words 0x00544E48 (the TruncatedNormal head), 0x00484D43 (HMC), 0 (Poisson).
 *   _fwd_f32: z_out_dev [ns * B][len]; kl_sum_out_dev [B] or NULL (the sum of an object's kl in the fixed order of csrc/beta_latent.hip:
 *     the same bits whatever B and first_object), kl_elem_out_dev [B][len] or NULL -- with both NULL no KL is computed at all;
 *     aux_out_dev [ns * B][len][2][4] or NULL: (zn, ub, attempt, lg) of the accepted attempt of each gamma (tests only).
 *   _bwd_f32: g_skip_out_dev [B][2][len] for the cotangents g_z_dev [ns * B][len] and g_kl_dev [B] (either may be NULL: zero): the
 *     implicit reparameterisation gradient of each gamma and the closed-form gradient of the KL term, float64, rounded once.  Nothing
 *     is saved by the forward: the backward redraws.
 *   _words_host_u32: the Philox words of one (level, s, gamma, attempt) into HOST memory out_host [n][len][4]; needs no GPU.
 * ns * B * len <= 2^31 - 1; 1 <= ns <= 2048 (s < 2048); level <= 255; first_object >= 0. */
int ctpvae_beta_latent_fwd_f32(const float *skip_dev, int B, int len, int ns, long long first_object, unsigned long long seed, unsigned draw,
                               unsigned level, float *z_out_dev, float *kl_sum_out_dev, float *kl_elem_out_dev, float *aux_out_dev,
                               ctpvae_stream_t stream);
int ctpvae_beta_latent_bwd_f32(const float *skip_dev, int B, int len, int ns, long long first_object, unsigned long long seed, unsigned draw,
                               unsigned level, const float *g_z_dev, const float *g_kl_dev, float *g_skip_out_dev, ctpvae_stream_t stream);
int ctpvae_beta_latent_words_host_u32(int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned level, int s,
                                      int gamma, int attempt, unsigned *out_host);

/* ---- the glue around every convolution of the P-VAE's ConvBlock (ctvae/models.py:219-263, :330-341) as one launch each way
 * (csrc/convblock.hip states the functions and the backward's order of addition).  All tensors fp32, contiguous [N][C][H][W].
 * Periodic pad, planes = N * C, OH = H + hl + hr, OW = W + wl + wr (a pad may exceed the extent):
 *   _pad_fwd_f32: out_dev [planes][OH][OW], out[p][r][q] = x[p][(r - hl) mod H][(q - wl) mod W].
 *   _pad_bwd_f32: gx_out_dev [planes][H][W] for the cotangent g_dev [planes][OH][OW]: per padded row the copies of a column added in
 *     ascending q, then the rows of a source row in ascending r, each sum starting from its first term; no atomics.
 * Maxout, y_dev [n][2][len] (len = C * H * W; the two channel halves of an object):
 *   _maxout_fwd_f32: first = y[n][0][i] >= y[n][1][i] (a tie takes the first half, a NaN in either the second);
 *     out_dev [n][len] = first ? first half : second half, first_out_dev [n][len] one byte per element (0 or 1), all the backward needs.
 *   _maxout_bwd_f32: gy_out_dev [n][2][len] = (first ? g : 0, first ? 0 : g) for the cotangent g_dev [n][len]; every element is written.
 * Every extent >= 1, every pad >= 0, every element count (planes * OH * OW, 2 * n * len) <= 2^31 - 1. */
int ctpvae_periodic_pad_fwd_f32(const float *x_dev, int planes, int H, int W, int wl, int wr, int hl, int hr, float *out_dev,
                                ctpvae_stream_t stream);
int ctpvae_periodic_pad_bwd_f32(const float *g_dev, int planes, int H, int W, int wl, int wr, int hl, int hr, float *gx_out_dev,
                                ctpvae_stream_t stream);
int ctpvae_maxout_fwd_f32(const float *y_dev, int n, int len, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream);
int ctpvae_maxout_bwd_f32(const float *g_dev, const unsigned char *first_dev, int n, int len, float *gy_out_dev, ctpvae_stream_t stream);

/* ---- the ConvBlock's dropout (ctvae/models.py:58-61, :141-144, :283-284: on the block's input, before the padding), alone and inside
 * the periodic pad's launches; all five added at ABI 3400 (csrc/convblock.hip states the layout).  The stream is part of the
 * definition: Philox4x32-10, key = seed.  The block input is [n][len] (len = C * H * W); element i of object b has the 64-bit flat
 * index e = (first_object + b) * len + i and takes word w = e & 3 of the block with counter (lo32(e >> 2), hi32(e >> 2), draw,
 * 0x44000000 | layer), layer < 2^24 (the top byte 0x44 keeps the fourth counter word apart from the latents' 0x4C......, the head's
 * 0x544E48, the HMC sampler's 0x484D43 and the Poisson sampler's 0).
 *   keep   k = w >> 8, u = k * 2^-24 (exact in float32); keep iff u >= float32(rate), i.e. k >= T with T = ceil(float32(rate) * 2^24),
 *          which the HOST computes and passes: 1 <= T <= 2^24 - 1 for 0 < float32(rate) < 1
 *   value  keep ? x * scale : +0.0f, scale = float32(1 / (1 - rate)) computed in double by the host (1 <= scale <= 2^24): one float32
 *          multiply.  A dropped element is a selection, not a product with 0: a dropped inf or NaN gives +0, where TensorFlow's
 *          x * scale * mask gives NaN (the maxout's backward selects the same way).
 *   _dropout_fwd_f32: out_dev [n][len] of x_dev [n][len].
 *   _dropout_bwd_f32: gx_out_dev [n][len] = keep ? scale * g : +0.0f of the cotangent g_dev [n][len].
 *   _dropout_pad_fwd_f32: out_dev [n * channels][OH][OW], out[p][r][q] = drop(x)[p][(r - hl) mod H][(q - wl) mod W], len = channels * H * W:
 *     the decision belongs to the SOURCE element, every wrapped copy of it shares it; the bits of _periodic_pad_fwd_f32 of _dropout_fwd_f32.
 *   _dropout_pad_bwd_f32: gx_out_dev [n * channels][H][W] = keep ? scale * acc : +0.0f, acc the two ascending folds of
 *     _periodic_pad_bwd_f32 in their order.
 *   The backwards draw the mask again from the same (first_object, seed, draw, layer, T): the forwards keep nothing for them.
 *   _dropout_keep_host_u8: the keep decisions (1 = kept) of the same arguments into HOST memory out_host [n][len]; needs no GPU.
 * A batch cut into calls with first_object drops what the whole batch drops.  Every extent >= 1, every pad >= 0, the element counts of
 * the device calls (n * len, n * channels * OH * OW) <= 2^31 - 1, first_object >= 0 and (first_object + n) * len <= 2^63 - 1. */
int ctpvae_dropout_fwd_f32(const float *x_dev, int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer,
                           unsigned T, float scale, float *out_dev, ctpvae_stream_t stream);
int ctpvae_dropout_bwd_f32(const float *g_dev, int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer,
                           unsigned T, float scale, float *gx_out_dev, ctpvae_stream_t stream);
int ctpvae_dropout_pad_fwd_f32(const float *x_dev, int n, int channels, int H, int W, int wl, int wr, int hl, int hr, long long first_object,
                               unsigned long long seed, unsigned draw, unsigned layer, unsigned T, float scale, float *out_dev,
                               ctpvae_stream_t stream);
int ctpvae_dropout_pad_bwd_f32(const float *g_dev, int n, int channels, int H, int W, int wl, int wr, int hl, int hr, long long first_object,
                               unsigned long long seed, unsigned draw, unsigned layer, unsigned T, float scale, float *gx_out_dev,
                               ctpvae_stream_t stream);
int ctpvae_dropout_keep_host_u8(int n, int len, long long first_object, unsigned long long seed, unsigned draw, unsigned layer, unsigned T,
                                unsigned char *out_host);

/* ---- (MSE, SSIM, PSNR) of a batch of image pairs in float64 (the reference's compare, ctvae/helper_functions.py:394-418, with
 * scikit-image 0.18's structural_similarity: uniform window, K1 0.01, K2 0.03, sample covariance, the data range taken from the
 * reference image); added at ABI 3400.  ref_dev, test_dev [n][X][Y] contiguous, both float (_f32; widened to double first) or both
 * double (_f64); out_dev [n][3] float64 = (mse, ssim, psnr) of test[k] against ref[k].  csrc/merit.hip states every operation and the
 * one order of every sum: three launches whatever n, X, Y are, no floating-point atomics, no S map in memory; the same call gives the
 * same bits on every run and pair k's numbers do not depend on n or k.  win = 7 if min(X, Y) >= 7, else the largest odd number
 * <= min(X, Y); psnr = +inf where mse == 0; non-finite pixels propagate as in numpy's formula.
 *   _tile: the edge of a tile of window positions (a workgroup of the SSIM launch covers tile x tile positions; host only).
 *   _workspace_bytes: bytes of workspace_dev (8-byte aligned) for (n, X, Y): at most 32 * n * ceil((X - win + 1) / tile) *
 *     ceil((Y - win + 1) / tile); 0 for n = 0.  The workspace carries nothing between calls.
 * Every check is made before any launch: n >= 0 (n = 0: nothing is launched, CTPVAE_OK); X, Y >= 3; n * X * Y <= 2^31 - 1. */
int ctpvae_merit_tile(void);
long long ctpvae_merit_workspace_bytes(int n, int X, int Y);
int ctpvae_merit_f32(const float *ref_dev, const float *test_dev, int n, int X, int Y, void *workspace_dev, double *out_dev,
                     ctpvae_stream_t stream);
int ctpvae_merit_f64(const double *ref_dev, const double *test_dev, int n, int X, int Y, void *workspace_dev, double *out_dev,
                     ctpvae_stream_t stream);

/* ---- the update stage of a P-VAE training step (ctvae/main_ct_vae.py:353, :482-485): tf.where(is_nan, 0, g), tf.clip_by_norm per
 * tensor and Keras's Adam (epsilon outside the bias correction) as TWO launches over the flat gradient buffer, whatever the number of
 * tensors; csrc/update.hip states every operation, the order of the float64 sum of squares and the two deviations from TensorFlow.
 * Added without a new ABI version: nothing that existed changes.  T tensors of lens_host[k] >= 1 elements lie back to back in
 * grad_dev / m_dev / v_dev (float32, 4-byte aligned, any offsets); the parameters stay where they are, params_host[k] is tensor k's
 * DEVICE address (4-byte aligned), held in host memory.
 *   _chunk_len: C, the longest chunk (host only).
 *   _plan_bytes: bytes of the chunk table for these lengths = 32 * the number of chunks, sum of ceil(len / C) (host only).
 *   _plan_host: the table into HOST memory plan_out_host (8-byte aligned): per chunk {int64 flat offset, address of the parameter's
 *     element there, int32 length, tensor, index of the tensor's first chunk, chunks of the tensor}; tensor after tensor, ascending in
 *     offset, no chunk across a tensor boundary or longer than C.  The caller copies it to the device.
 *   _update_f32: launch 1 writes one float64 per chunk into partials_dev [n_chunks]; launch 2 adds each tensor's partials in ascending
 *     order, stores l2 = (float)sqrt(sum) into norms_out_dev [T] and updates m_dev, v_dev and the parameters in place; grad_dev is read
 *     only (it keeps its NaNs).  t >= 1 is the step this call takes (for the record: the device keeps no counter), alpha the caller's
 *     float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t)) evaluated in float64; clip > 0; 0 <= b1, b2 < 1; eps >= 0.  plan_dev must be the
 *     table _plan_host built for exactly these buffers: the kernels trust it.  No synchronisation, nothing read back. */
int ctpvae_update_chunk_len(void);
long long ctpvae_update_plan_bytes(const long long *lens_host, int T);
int ctpvae_update_plan_host(const long long *lens_host, const void *const *params_host, int T, void *plan_out_host);
int ctpvae_update_f32(const void *plan_dev, int n_chunks, int T, const float *grad_dev, float *m_dev, float *v_dev, double *partials_dev,
                      float *norms_out_dev, long long t, float alpha, float clip, float b1, float b2, float eps, ctpvae_stream_t stream);

/* ---- the convolution of a padded (non-transposed) ConvBlock with its periodic padding in front and its maxout behind, on the matrix
 * cores with fp32 operands (csrc/conv.hip states every sum's one order, the tail rule, the chunk rule and how invalid taps enter);
 * added without a new ABI version: nothing that existed changes.  All tensors fp32, contiguous NCHW: x_dev [N][Cin][H][W], w_dev
 * [2C][Cin][k][k], b_dev [2C]; stride s; pads (wl, wr, hl, hr) >= 0; PH = H + hl + hr, PW = W + wl + wr, OH = (PH - k) / s + 1,
 * OW = (PW - k) / s + 1; the padded input xp[n][ci][r][q] = x[n][ci][(r - hl) mod H][(q - wl) mod W] is never written to memory.
 *   _fwd_f32: ONE launch.  y[n][c2][oh][ow] = one fmaf chain from b[c2] over ci, kh, kw ascending; out_dev [N][C][OH][OW] =
 *     first ? y[c] : y[C + c] with first = y[c] >= y[C + c] (a tie takes the first half, a NaN the second), first_out_dev one byte
 *     (0 or 1) per output element; y is not written.
 *   _wgrad_chunk_len: the chunk length of the weight gradient's sum over m = (n * OH + oh) * OW + ow (host only).
 *   _wgrad_workspace_bytes: 4 * ceil(N * OH * OW / chunk_len) * 2C * (Cin * k * k + 1), a function of the shapes alone (host only).
 *   _bwd_weight_f32: TWO launches.  gw_out_dev [2C][Cin][k][k] and gb_out_dev [2C] of the cotangent g_dev [N][C][OH][OW] and
 *     first_dev: per chunk one fmaf chain from +0 ascending in m, then the chunks' partials added in ascending order in fp32.
 *   _bwd_input_f32: ONE launch.  gp_out_dev [N][Cin][PH][PW], the cotangent of the padded input: one fmaf chain from +0 over c2, kh,
 *     kw ascending; ctpvae_periodic_pad_bwd_f32(gp, N * Cin, H, W, wl, wr, hl, hr, gx) folds it into the input's gradient.
 * 1 <= k <= 8, 1 <= s <= k, k <= PH, k <= PW, every extent >= 1, every element count (the tensors, gp, the workspace) <= 2^31 - 1;
 * every check is made before any launch. */
int ctpvae_conv_wgrad_chunk_len(void);
long long ctpvae_conv_wgrad_workspace_bytes(int N, int Cin, int H, int W, int C, int k, int s, int wl, int wr, int hl, int hr);
int ctpvae_conv_fwd_f32(const float *x_dev, const float *w_dev, const float *b_dev, int N, int Cin, int H, int W, int C, int k, int s, int wl,
                        int wr, int hl, int hr, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream);
int ctpvae_conv_bwd_weight_f32(const float *x_dev, const float *g_dev, const unsigned char *first_dev, int N, int Cin, int H, int W, int C,
                               int k, int s, int wl, int wr, int hl, int hr, void *workspace_dev, float *gw_out_dev, float *gb_out_dev,
                               ctpvae_stream_t stream);
int ctpvae_conv_bwd_input_f32(const float *g_dev, const unsigned char *first_dev, const float *w_dev, int N, int Cin, int H, int W, int C,
                              int k, int s, int wl, int wr, int hl, int hr, float *gp_out_dev, ctpvae_stream_t stream);

/* ---- the transposed convolution of an up-sampling ConvBlock with its maxout behind, on the matrix cores with fp32 operands
 * (csrc/conv_transpose.hip states every sum's one order, the phase taps, the tail rule, the two chunk rules and how invalid taps
 * enter); added without a new ABI version: nothing that existed changes.  All tensors fp32, contiguous: x_dev [N][Cin][H][W], w_dev
 * [Cin][2C][k][k] (nn.ConvTranspose2d's weight; the maxout's halves are [0, C) and [C, 2C) of axis 1), b_dev [2C]; stride s, padding
 * pad, output padding opad; OH = (H - 1) * s - 2 * pad + k + opad, OW likewise.
 *   _fwd_f32: ONE launch.  y[n][c2][oy][ox] = one fmaf chain from b[c2] over ci, the pixel's phase kh, its phase kw ascending (a phase
 *     tap outside the image enters as +0, taps of other phases not at all); out_dev [N][C][OH][OW] = first ? y[c] : y[C + c] with
 *     first = y[c] >= y[C + c] (a tie takes the first half, a NaN the second), first_out_dev one byte (0 or 1) per output element; y
 *     is not written.
 *   _wgrad_workspace_bytes: 4 * (ceil(N * H * W / chunk) * Cin * 2C * k * k + ceil(N * OH * OW / chunk) * 2C) with chunk =
 *     ctpvae_conv_wgrad_chunk_len(), a function of the shapes alone (host only).
 *   _bwd_weight_f32: TWO launches.  gw_out_dev [Cin][2C][k][k] and gb_out_dev [2C] of the cotangent g_dev [N][C][OH][OW] and
 *     first_dev: gw per chunk of m = (n * H + iy) * W + ix one fmaf chain from +0 ascending in m, gb per chunk of
 *     mo = (n * OH + oy) * OW + ox one chain of additions from +0 ascending in mo, then the partials added in ascending chunk order.
 *   _bwd_input_f32: ONE launch.  gx_out_dev [N][Cin][H][W]: one fmaf chain from +0 over c2, kh, kw ascending.
 * 1 <= k <= 8, 1 <= s <= k, 0 <= pad < k, 0 <= opad < s, OH >= 1, OW >= 1, every extent >= 1, every element count (the tensors, the
 * workspace, the launches' workgroups) <= 2^31 - 1; every check is made before any launch. */
long long ctpvae_convt_wgrad_workspace_bytes(int N, int Cin, int H, int W, int C, int k, int s, int pad, int opad);
int ctpvae_convt_fwd_f32(const float *x_dev, const float *w_dev, const float *b_dev, int N, int Cin, int H, int W, int C, int k, int s, int pad,
                         int opad, float *out_dev, unsigned char *first_out_dev, ctpvae_stream_t stream);
int ctpvae_convt_bwd_weight_f32(const float *x_dev, const float *g_dev, const unsigned char *first_dev, int N, int Cin, int H, int W, int C,
                                int k, int s, int pad, int opad, void *workspace_dev, float *gw_out_dev, float *gb_out_dev,
                                ctpvae_stream_t stream);
int ctpvae_convt_bwd_input_f32(const float *g_dev, const unsigned char *first_dev, const float *w_dev, int N, int Cin, int H, int W, int C,
                               int k, int s, int pad, int opad, float *gx_out_dev, ctpvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CTPVAE_RADON_H */
