/*
 * gisnav_amd.h -- C ABI of the MI355X-native PoseNode hot path (libgisnav_amd.so).
 *
 * GISNav has no formal plugin interface; PoseNode hard-codes three seams.
 * Each entry point below names the reference code it stands in for
 * (paths relative to the reference tree, ros/gisnav/gisnav/core/):
 *
 *   gn_create / gn_load_tensor   LightGlueMatcher("sift", params={n_layers:9, filter_threshold:.5,
 *                                depth_confidence:-1, width_confidence:-1}).to(device).eval()
 *                                                                       pose_node.py:109-121
 *   gn_match                     RootSIFT + self._matcher(desc_q, desc_r, laf_q, laf_r)
 *                                                                       pose_node.py:278-287
 *   gn_gather_points             kp[idx] gathers, MIN_MATCHES gate, _compute_3d_points
 *                                                 pose_node.py:289-303, _shared.py:95-102
 *   gn_pnp_ransac                cv2.solvePnPRansac(..., iterationsCount=10) + cv2.Rodrigues
 *   gn_set_ransac                iterationsCount / reprojectionError / confidence of the pose stage inside gn_estimate and gn_vo_estimate
 *                                (1 .. GN_RANSAC_MAX_ITERATIONS hypotheses; the default stays the reference's 10, 8.0, 0.99)
 *                                                                       _shared.py:104-117
 *   gn_estimate                  the whole of PoseNode._pose lines 246-308 for a batch of pairs
 *                                (gn_set_active_kpts: padded size per call, for batches well below max_kpts)
 *   gn_pose_to_earth (+ gn_proj_to_affine, gn_wgs84_to_ecef)   the georeferencing after the pose
 *                                                 pose_node.py:333-381, _transformations.py:298-393
 *   gn_*_cov, gn_pose_cov_to_camera / _to_earth  the covariance the reference leaves at zero (pose_node.py:477)
 * and, widening to the feeders of that path:
 *   gn_sift_detect_and_compute(_batch)   cv2.SIFT_create().detectAndCompute(img, None)
 *                                                 pose_node.py:122,230-232; twist_node.py:93,227-245
 *   gn_rotate_crop_center / gn_stereo_reference   StereoNode reference raster   stereo_node.py:229-262,292-335
 *   gn_vo_match / gn_vo_estimate cv2.BFMatcher.knnMatch(k=2) + ratio test + compute_pose   twist_node.py:95,248-289
 *
 * Conventions: plain C, no torch types.  Every data pointer is a DEVICE pointer unless the
 * parameter is marked "host".  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  All work is stream-ordered; no entry point synchronises except gn_debug_read and
 * gn_sift_detect_and_compute(_batch) (one sync at the end, to return the keypoint counts).
 * Return value: 0 on success, negative gn_status on failure; nothing throws.  One context
 * per GPU; a context is thread-compatible, not thread-safe (PoseNode calls from one executor
 * thread at a time, gisnav/__init__.py:140-154).  DIFFERENT contexts (gn_ctx and gn_loftr alike)
 * may be driven from different host threads at the same time: nothing the launch paths consult
 * is process-wide.  gn_last_error(NULL) reports the calling thread's last error.
 */
#ifndef GISNAV_AMD_H
#define GISNAV_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gn_ctx gn_ctx;

enum gn_status {
  GN_OK = 0,
  GN_ERR_ARG = -1,       /* bad argument (NULL, out of range, B > max_batch, n > max_kpts) */
  GN_ERR_HIP = -2,       /* a HIP runtime call failed; see gn_last_error */
  GN_ERR_NAME = -3,      /* unknown tensor name */
  GN_ERR_SHAPE = -4,     /* tensor shape mismatch */
  GN_ERR_WEIGHTS = -5,   /* forward called before every required tensor was loaded */
  GN_ERR_ARCH = -6       /* device is not gfx950 */
};

enum gn_precision {
  GN_PREC_F32 = 0,       /* every contraction on f32 MFMA (parity mode) */
  GN_PREC_BF16_ATTN = 1, /* QK^T / PV on bf16 MFMA with f32 softmax+accumulate (what kornia's
                            Attention does in fp16 on CUDA when flash=True); projections,
                            FFN and the match head stay on the exact-f32 MFMA */
  GN_PREC_F32X3_BF16_ATTN = 2, /* as 1, but projections / FFN / match-head GEMMs run f32-ACCURATE on the bf16
                            matrix pipe: every f32 operand is split exactly into three bf16 terms and six
                            partial products are accumulated in f32 (error vs fp64 at or below the exact-f32
                            MFMA path's; see tests) */
  GN_PREC_F16X2_BF16_ATTN = 3, /* as 2 at half the matrix-pipe work: every f32 operand is split into two fp16
                            terms (round to nearest, 22 significant bits, subnormals honoured by the gfx950
                            matrix pipe) and three partial products are accumulated in f32; weight planes are
                            pre-scaled by a power of two.  Domain |activation| < 65504 (the reference's fp32
                            nn.Linear has no such limit): GUARDED -- every kernel that writes an activation in
                            this format raises a context word when a value leaves the range, a tripped call
                            reports ZERO matches instead of inf / NaN, and gn_set_guard(ctx, 2) re-runs it in
                            mode 2 (see gn_set_guard).  Error vs fp64 at the level of an f32 accumulation
                            (see tests) */
  GN_PREC_F16X2_F16_ATTN = 4  /* as 3, with QK^T / PV on the FP16 matrix instruction (v_mfma_f32_32x32x16_f16): q, k, v and
                            the probabilities are rounded to fp16 (11 significant bits) instead of bf16 (8), f32 softmax
                            and accumulation as before -- the arithmetic of the reference's own CUDA path (kornia casts
                            q, k, v to half for F.scaled_dot_product_attention when flash=True; pose_node.py:285-287 via
                            SURVEY.md:314), at the same matrix-pipe rate as bf16.  q / k / v share the guarded fp16 domain
                            of the activations (|value| < 65504, else the guard word is raised; the guard-2 re-run uses bf16
                            attention operands, which have f32's range) */,
  GN_PREC_F16X2_F16X2_ATTN = 5 /* as 3 with an f32-accurate attention on the FP16 matrix instruction: the q | k | v projections leave f32 rows
                            (the f16x2 GEMMs, three products), and k_attn_f16x2 splits q, k, v and the probabilities into two fp16 terms
                            each under power-of-two scales (S = qh kh + qh kl + ql kh, O = ph vh + ph vl + pl vh, f32 softmax with the
                            exact running maximum, f32 accumulation); the block tail on three products.  Every contraction is
                            f32-accurate and all of them run on the 16-bit matrix pipe.  Guarded like 3 (a high term or an hm16 output
                            that leaves the fp16 range raises the guard word).  SIFT contexts only (GN_FEATURE_SUPERPOINT: GN_ERR_ARG).
                            Also the middle level of the certificate's re-run ladder (gn_set_certify_ladder). */
};

enum gn_kpt_format {
  GN_KPT_LAF = 0,        /* 6 floats/keypoint: kornia LAF (2x3 row-major) -- the B1 seam's argument */
  GN_KPT_XYSA = 1,       /* 4 floats/keypoint: x, y, size, angle_deg (cv2.KeyPoint fields,
                            KEYPOINT_DTYPE in _shared.py:26-35); the LAF of pose_node.py:267-276
                            is formed in registers */
  GN_KPT_RECORD = 2      /* 133 floats/keypoint = the RAW 532-byte wire record of KEYPOINT_DTYPE
                            (_shared.py:26-35: x, y, z, size, angle, descriptor[128]; all float32,
                            little endian) exactly as OrthoStereoImage.query_sift
                            carries it (pose_node.py:207-213): kpt_* point at [B][stride] records, the
                            descriptor is read from the record itself and the desc_* arguments are
                            ignored (may be NULL).  The message bytes go to the device as they are --
                            no host-side unpacking (np.frombuffer + column_stack).  SIFT contexts only. */
};
/* OR into kpt_format when the descriptors are ALREADY RootSIFT-normalised (the B1 seam: PoseNode
 * normalises at pose_node.py:278-284 before calling the matcher object); otherwise gn_match applies
 * RootSIFT itself to raw SIFT descriptors. */
#define GN_DESC_ROOTSIFT 0x100

/* Library / build info: "gisnav_amd <ver> gfx950 src:<source digest>". */
const char* gn_version(void);
/* Human-readable text for the last failure on this context (or global if ctx is NULL). */
const char* gn_last_error(const gn_ctx* ctx);

/* The fp16-range guard of GN_PREC_F16X2_BF16_ATTN (no effect in the other modes):
 *   0  off (no checks; an out-of-range activation silently becomes inf / NaN -- for kernel experiments only);
 *   1  (default) flag: stream-ordered, no host sync.  A call in which any activation reached |x| >= 65504 returns
 *      n_match = 0 for every pair (and therefore ok = 0 from gn_estimate); gn_get_guard_status tells the host.  With
 *      gn_set_substreams(n > 1) every sub-batch group has its own guard word: a trip zeroes the matches of the pairs of
 *      THAT group only, and gn_get_guard_status reports the OR over the groups of the last call;
 *   2  flag + fallback: gn_match / gn_estimate synchronise the stream once after the matcher, and a tripped call is
 *      re-run transparently with every operand split exactly into three bf16 terms (the arithmetic of mode
 *      GN_PREC_F32X3_BF16_ATTN: f32 range and accuracy, ~1.5x slower) before the call returns.  The Python mirrors of
 *      the reference's objects (LightGlueMatcher, PoseNode) use this: they synchronise after the matcher anyway. */
int gn_set_guard(gn_ctx* ctx, int mode);
/* Synchronises `stream`; *last_call_tripped = 1 if the most recent matcher run on this context left the fp16 range,
 * *trips_total = number of tripped calls observed so far (either pointer may be NULL). */
int gn_get_guard_status(gn_ctx* ctx, void* stream, int32_t* last_call_tripped, int64_t* trips_total);

/* The margin certificate of the correspondence indices.  kornia's LightGlueMatcher returns `match_indices` that PoseNode uses as exact
 * integers (ros/gisnav/gisnav/core/pose_node.py:285-297); the fast precision modes compute the assignment scores P with an arithmetic
 * error, so a decision whose margin is smaller than that error may come out differently from the exact-f32 arithmetic.  With the certificate
 * on, the match head keeps the runner-up of every row / column maximum of P and reports, per PAIR, whether every decision of that pair
 * is safe: (a) every row whose best score is >= log(filter_threshold) - eps leads its runner-up by more than 2 eps, (b) the same for every
 * column, (c) no row's best score lies within eps of log(filter_threshold).  eps is the stated bound on |P_mode - P_exact| for the
 * entries that decide (measured per weight set by tools/certify_eps.py / PoseEngine.calibrate_certify; pass < 0 to keep the current
 * value).  A pair that satisfies (a)-(c) has exactly the exact arithmetic's match list (proof in DESIGN.md).
 *   mode 0  off (default): no flags are written;
 *   mode 1  flags only, stream-ordered, no host synchronisation: gn_get_uncertain reads them;
 *   mode 3  as mode 2, but gn_estimate with sub-batch streams resolves call n's flags after call n + 1 has been enqueued (or in gn_flush): the caller keeps
 *           the inputs AND outputs of call n untouched until then (two alternating output sets); no host wait on an idle GPU.
 *           When such a gn_estimate returns, `stream` is behind the call's match heads only: its gather and PnP are still in flight on the
 *           library's own streams.  A later gn_estimate orders itself behind them; every OTHER entry point that uses the context's match or
 *           PnP workspaces (gn_match, gn_gather_points, gn_pnp_ransac, ...) needs a gn_flush first;
 *   mode 2  certified results: gn_match / gn_estimate synchronise the stream once per call, read the flags and run every flagged pair
 *           again -- matcher, and for gn_estimate also gather + PnP -- on GN_PREC_F32's kernels (the context keeps f32 weights and f32
 *           workspaces in every mode).  A call whose activations left the fp16 range is flagged as a whole (flag value 2), so this mode
 *           also takes over gn_set_guard(2)'s fallback.  In a GN_PREC_F32 context nothing is re-run: the flags (for eps_f32) are counted.
 * Results of a pair do not depend on which other pairs were re-run.
 * A calibration belongs to the weights it was measured on: gn_load_tensor marks an eps measured by gn_calibrate_certify as discarded, and
 * until gn_calibrate_certify runs again or an eps is stated here, modes 2 and 3 send every pair to exact f32.  An eps stated here (or the
 * built-in default) is the caller's and survives a load. */
int gn_set_certify(gn_ctx* ctx, int mode, float eps, float eps_f32);
/* Arithmetic of the block tail (ffn.0 -> LayerNorm -> GELU -> ffn.3 with out_proj folded in; kornia `x + ffn(cat[x, msg])`) on bulk grids in the f16x2
 * modes: 3 (default) = every operand as two fp16 terms, three partial products, f32-accurate; 2 = the activations' fp16 HIGH term only (22-bit weights x
 * 11-bit activations, f32 accumulation: the arithmetic of the attention input projections, and the rounding the fp16 attention applies to q, k, v anyway) --
 * a third less matrix-pipe work.  On this level the GELU's erf is a degree-4 polynomial inside exp2 (6.7e-7 absolute; GELU error <= 3.7e-7 |y|, far
 * below the fp16 rounding step, 2^-12 |h|, applied to the same value in the next instruction) instead of level 3's degree-7 one (2.2e-8): 12 instead of 17
 * vector instructions per hidden value.  The error of the assignment scores grows (gn_calibrate_certify measures it), so this setting is meant to run under the
 * margin certificate (gn_set_certify(2 / 3)), which makes the returned correspondence indices independent of the fast pass's arithmetic.  Small grids
 * (fewer than 256 tiles of 128 tokens) keep three products.
 * 1 = the weights' fp16 HIGH term only as well (W_h X_h: one product per k-step, 11-bit weights x 11-bit activations -- a second, independent rounding of the
 * size of the activations'; half of level 2's matrix-pipe work and weight bytes in both GEMMs; LayerNorm, the degree-4 erf, the fp16-range guard and the fused
 * next-block projection, which stays on two products, are level 2's).  Composed form on bulk grids only, and under the certificate, as 2.
 * 0 = the level FOLLOWS THE CERTIFICATE (needs gn_set_certify(2 / 3) and a gn_calibrate_certify made under this setting, which measures eps for both
 * levels; three products otherwise): every matcher call also evaluates the other level's certificate on its scores, the context counts over windows
 * of >= 64 certified pairs how many pairs each level flags, and runs the next window on two products only when that would flag at most 1 pair in 64
 * more than three products (a flagged pair costs an exact-f32 re-run, ~4 fast passes; the two-product pass saves ~7 % of one).  Starts on three
 * products.  The returned indices do not depend on the level (both are certified against the same exact arithmetic); scores differ within eps.
 * Under 0 gn_calibrate_certify also measures eps_one_product (same passes, same extra grids; stored so that eps_one >= eps_two >= eps_three) and every call
 * evaluates all three certificates.  From two products the context goes down to one only after TWO consecutive windows on level 2 in each of which one product
 * would have flagged at most 1 pair in 64 more than three products; on level 1 a single window that fails that test goes back to 2 (to 3 when level 2 fails
 * its own test as well).  The first 128 certified pairs of a context therefore behave as before the third level existed.
 * gn_load_tensor discards the levels' calibration (three products until gn_calibrate_certify / gn_set_ffn_level_eps is called again). */
int gn_set_ffn_products(gn_ctx* ctx, int products);
/* The level the next call runs on (1 / 2 / 3), the eps calibrated for each (< 0: not calibrated), and out4 = {certified calls that ran on two products, on three
 * products, level switches, 1 when the automatic setting is in effect} since gn_reset_certify_stats.  Any pointer may be NULL. */
int gn_get_ffn_level(gn_ctx* ctx, int32_t* level, float* eps2, float* eps3, int64_t* out4);
/* The two levels' eps and the level to start on, stated by the caller instead of measured (values a gn_calibrate_certify of the same weights and
 * batch size returned earlier: a process that restarts need not repeat the calibration's exact-f32 pass). */
int gn_set_ffn_level_eps(gn_ctx* ctx, float eps2, float eps3, int level);
/* The one-product level's share of the two calls above (their ABI is unchanged): its eps (< 0: not calibrated -- the level is then never selected) and the
 * certified calls that ran on it.  gn_set_ffn_level_eps1 states eps_one (stored as max(eps_one, eps_two)); call it BEFORE gn_set_ffn_level_eps when the
 * context is to start on level 1: gn_set_ffn_level_eps(e2, e3, 1) without a stated eps_one starts on level 2. */
int gn_get_ffn_level1(gn_ctx* ctx, float* eps1, int64_t* calls1);
int gn_set_ffn_level_eps1(gn_ctx* ctx, float eps1);
/* Developer / test entry, no device: the automatic level's rule run over n_calls synthetic calls of B pairs, starting on three products.  f1, f2, f3:
 * [n_calls][B] flags (0 / 1) the one-, two- and three-product certificates would raise on each call's scores; have1: level 1 has an eps.  levels_out
 * [n_calls] (may be NULL): the level each call ran on; out4 (may be NULL) = {level after the last call, switches, calls on two products, calls on one}. */
int gn_debug_ffn_level_sim(int n_calls, int B, const int32_t* f1, const int32_t* f2, const int32_t* f3, int have1, int32_t* levels_out, int64_t* out4);
/* Partial products of the attention input projections on bulk grids (k_qkv, and the projection fused behind the block tail):
 * 2 = two (W_m X_h + W_h X_h), as before.
 * 1 = ONE (W_h X_h: half the matrix-pipe work and weight bytes of the projection; its outputs are rounded to fp16 in any case) wherever the block tail runs on
 *     level 1 and the bulk kernels are selected -- GN_PREC_F16X2_F16_ATTN only; small grids, the three-product levels and every other mode keep two.
 * 0 (default) = automatic: a rung of the automatic ladder (gn_set_ffn_products(0)) below level 1.  gn_calibrate_certify then measures a fourth arithmetic,
 *     level 1 + one-product projections (stored so that eps_proj1 >= eps_one), every automatic call evaluates that eps too, and a context on level 1 steps onto
 *     the rung after ONE window of >= 64 certified pairs on level 1 in which the rung would have flagged at most 1 pair in 64 more than three products; on the
 *     rung one window that fails that test goes back to level 1 (further when level 1 fails its own test).  192 clean pairs still end on level 1 after two
 *     switches; the rung is first possible after 256.  gn_set_ffn_products(1) alone never selects it.
 * The level reported by gn_get_ffn_level stays 1 on the rung; gn_get_qkv_level says whether the next call's projections run on one product (on_rung), the
 * rung's eps (< 0: not calibrated -- never selected automatically) and the certified calls that ran on it.  gn_set_qkv_level_eps states that eps instead of
 * measuring it (after gn_set_ffn_level_eps1 / gn_set_ffn_level_eps; stored as max(eps_proj1, eps_one)).  The fused forms are proved against the separate
 * launches like every other (gn_fused_projection_status).  Any pointer may be NULL. */
int gn_set_qkv_products(gn_ctx* ctx, int products);
int gn_get_qkv_level(gn_ctx* ctx, int32_t* setting, int32_t* on_rung, float* eps_proj1, int64_t* calls_proj1);
int gn_set_qkv_level_eps(gn_ctx* ctx, float eps_proj1);
/* gn_debug_ffn_level_sim with the rung: f0 = the flags the rung's certificate would raise, have0: the rung has an eps.  rung_out [n_calls] (may be NULL): 1 where
 * the call ran on the rung (levels_out is then 1); out5 (may be NULL) = {level after, switches, calls on two products, calls on one (rung included), on the rung after}.
 * With have0 == 0 every answer is gn_debug_ffn_level_sim's. */
int gn_debug_ffn_level_sim_rung(int n_calls, int B, const int32_t* f0, const int32_t* f1, const int32_t* f2, const int32_t* f3, int have1, int have0,
                                int32_t* levels_out, int32_t* rung_out, int64_t* out5);
/* On bulk grids the block-tail kernel also computes the next block's attention input projection (one launch and one pass over the residual rows
 * less).  Every context proves that fused form against the separate launches on its own weights before using it: at the first forward call after
 * a weight (re)load or a change of gn_set_ffn_products both forms run on pseudo-random rows, at the full padded size whatever gn_set_active_kpts
 * has set, on every block-tail level the setting can select (three products; also two under 2 or 0, one under 1 or 0), and their outputs are compared bit for bit
 * (~60 ms per level, once); a difference switches the fusion off for the context until the next check passes.  Returns 1 = checked equal, 0 = differed (fusion off), -1 = not run yet / not applicable (small contexts, other modes). */
int gn_fused_projection_status(const gn_ctx* ctx);
/* NUMA node of HIP device `device` (its PCI function's /sys/bus/pci/devices/<bus id>/numa_node), or -1 when the platform does not say.  The host side pins
 * the staging threads of a rank to that node's cores (gisnav_amd.engine.RecordStager): with one rank per GPU, eight staging pools otherwise share whatever
 * cores the scheduler picks. */
int gn_device_numa_node(int device);
/* out8: calls certified, pairs certified, pairs flagged for margin, pairs flagged for fp16 range, pairs re-run in exact f32,
 * re-run (or, in an f32 context, original) pairs that are marginal even for eps_f32, current mode, and where eps comes from: 0 the built-in
 * default, 1 stated through gn_set_certify, 2 measured by gn_calibrate_certify, 3 measured on weights that gn_load_tensor has since replaced. */
int gn_get_certify_stats(gn_ctx* ctx, int64_t* out8);
int gn_reset_certify_stats(gn_ctx* ctx);
/* The certificate's re-run ladder (off by default; contexts of GN_PREC_F16X2_BF16_ATTN / GN_PREC_F16X2_F16_ATTN with SIFT features only, else
 * GN_ERR_ARG when enabling).  With it on and eps_mid calibrated, gn_set_certify(2 / 3) re-runs the pairs flagged for margin (flag 1) first in
 * GN_PREC_F16X2_F16X2_ATTN's arithmetic on this context's weights and workspaces, and the match head certifies them there against eps_mid; only
 * the pairs still flagged -- together with every pair flagged for range (flag 2) and every pair whose middle pass left the fp16 range -- go on to
 * the exact-f32 re-run.  eps_mid < 0 keeps the current value.  gn_calibrate_certify, with the ladder on, adds a mode-5 pass (on the sample and on
 * its first pair alone) and sets eps_mid = max(floor_eps, safety * max |P_mid - P_f32|) over the best score and runner-up of every row AND column
 * that come within 1 of log(filter_threshold); gn_load_tensor discards eps_mid (flagged pairs then go straight to exact f32 until the next
 * calibration).  With the ladder off nothing of the certified path changes. */
int gn_set_certify_ladder(gn_ctx* ctx, int enable, float eps_mid);
/* out4: pairs re-run on the middle level, of those certified there, of those passed on to exact f32 (since gn_reset_certify_stats), and eps_mid
 * as the IEEE-754 bits of the float (an unsigned 32-bit value), or -1 when eps_mid is not calibrated.  gn_get_certify_stats' re-run count stays
 * "re-run in exact f32". */
int gn_get_certify_ladder_stats(gn_ctx* ctx, int64_t* out4);
/* Measure eps for THIS context's weights and precision mode on a sample batch (arguments as gn_match): the batch is matched twice -- in the
 * context's arithmetic and on the exact-f32 kernels -- and eps = max(floor_eps, safety * max |P_mode - P_f32|) over the best score and the
 * runner-up of every valid row that comes within 1 of log(filter_threshold) in either arithmetic (all rows when the threshold is 0, or when no row
 * of the sample comes that close) -- over the batch, and over three one-pair passes on its first pair: as it is, and with its reference side
 * cut to 128 and to 2 keypoints (the one-pair grid of bucket remainders; few-keypoint sides, where the fp16 attention's error is larger), and
 * over the batch once more with every 128-d descriptor cut to its three largest bins (the error follows the descriptors' statistics: a sample of
 * dense descriptors understates it for sparse ones; not for GN_DESC_ROOTSIFT input or 256-d features, which are used as they come).
 * Synchronises; sets the context's eps and returns the measured maximum and eps through the two host pointers (either may be NULL).  Call
 * it once after loading a checkpoint, on representative pairs, IN A BATCH OF THE SIZE THE REAL CALLS HAVE (the kernel family -- and with it the arithmetic
 * whose error is being measured -- follows the grid size); safety >= 1 is the stated safety factor (the Python mirror uses 4). */
int gn_calibrate_certify(gn_ctx* ctx, int B, int kpt_format,
                         const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                         const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                         float safety, float floor_eps, float* measured_host, float* eps_host, void* stream);
/* Synchronises `stream`; host_flags[b] of the most recent matcher call: 0 certified, 1 a decision inside the margin, 2 fp16 range left. */
int gn_get_uncertain(gn_ctx* ctx, int B, int32_t* host_flags, void* stream);
/* 16 hex digits over every source file and compile flag the loaded binary was built from (gisnav_amd.build.source_digest() computes the
 * same value from the tree; gisnav_amd._lib.load refuses a library whose digest differs from its tree's). */
const char* gn_source_digest(void);

/* Create a context on HIP device `device` sized for batches of up to max_batch pairs with up
 * to max_kpts keypoints per side (rounded up to a multiple of 128 internally). */
int gn_create(int device, int max_batch, int max_kpts, int precision, gn_ctx** out);
/* The same for another local-feature type.  The reference instantiates LightGlueMatcher("sift") only (pose_node.py:109-121);
 * BASELINE.json configs[4] names the SuperPoint + LightGlue path, i.e. kornia's LightGlue(features = "superpoint"):
 * input_dim 256 = descriptor_dim (no input_proj), add_scale_ori False (posenc.Wr is [32][2] on the normalised (x, y)),
 * everything else -- 9 layers, shared to_qk, match head -- as for SIFT.  With GN_FEATURE_SUPERPOINT the descriptor arguments
 * of gn_match / gn_estimate are [B][stride][256] (used as they are: L2-normalised by the extractor), the keypoint records
 * keep their format (size / angle fields ignored), and the state dict has no input_proj.* entries. */
enum gn_feature { GN_FEATURE_SIFT = 0, GN_FEATURE_SUPERPOINT = 1 };
int gn_create_ex(int device, int max_batch, int max_kpts, int precision, int feature, gn_ctx** out);
/* kornia's LightGlueMatcher.forward(..., hw1, hw2): image sizes (w, h) used by normalize_keypoints for the query / reference
 * side; a non-positive value selects the keypoint extent (max_x, max_y) of that side, which is what PoseNode gets because it
 * passes hw1 = hw2 = None (pose_node.py:285-287).  Sticky host-side state, (0, 0, 0, 0) by default. */
int gn_set_image_size(gn_ctx* ctx, float w_q, float h_q, float w_r, float h_r);
/* Re-size the context for up to max_kpts keypoints per side: synchronises the device, replaces the max_kpts-dependent workspaces and keeps every
 * weight (and its pre-split planes / fragment layouts) where it is -- the reference accepts any keypoint count (cv2.SIFT_create() is unbounded,
 * pose_node.py:122), so the mirrors grow a context instead of failing, and a grow costs a few allocations, not a weight reload.  gn_kmax
 * changes; gn_set_active_kpts is reset to the new size; every other setting stays. */
int gn_resize(gn_ctx* ctx, int max_kpts);
void gn_destroy(gn_ctx* ctx);

/* Load one tensor of the kornia LightGlue("sift") state dict from HOST
 * memory, float32, row-major [out,in].  Both spellings `transformers.{i}.self_attn.*` and the
 * checkpoint's `self_attn.{i}.*` are accepted.  token_confidence.* and confidence_thresholds
 * are accepted and ignored (dead in PoseNode's live configuration, pose_node.py:113-116). */
int gn_load_tensor(gn_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* Number of required tensors still missing (0 = ready). */
int gn_missing_tensors(const gn_ctx* ctx);

/* Matcher options (defaults = PoseNode's: 9 layers, threshold 0.5). */
int gn_set_num_layers(gn_ctx* ctx, int n_layers);
int gn_set_filter_threshold(gn_ctx* ctx, float th);

/* LightGlue point pruning (kornia's width_confidence with early exit off; adaptive depth is not built).  After the cross block of every layer
 * but the last, each side of each pair whose CURRENT keypoint count is > min_kpts keeps the keypoints with
 * sigmoid(log_assignment.{i}.matchability(x)) > 1 - width_confidence (f32), compacted in ascending order; the count shrinks on the device, the work
 * lists are rebuilt, and every later kernel of the call runs on what is left.  Match indices are mapped back to the ORIGINAL keypoint indices
 * (a pruned query simply has no match), so every output keeps its meaning and the match list stays in ascending query index.
 *   width_confidence <= 0     off (the default): no extra launch, no extra buffer read, the same bits as a build without the feature
 *   width_confidence >= 1, or not finite: GN_ERR_ARG, the previous setting stays
 *   min_kpts < 0              the default, 1536
 * Restated from the public kornia 0.7.2 / cvg LightGlue source; kornia is not in this project's oracle environment, so parity with it is UNPINNED.
 * min_kpts' default is RECALLED from that source (pruning_keypoint_thresholds: 1536 for CUDA with flash attention, 1024 without), not verified.
 * This build's own behaviour: a side left with NO keypoint makes its pair report n_match = 0 (kornia would raise in a max over an empty dimension).
 * A side left with one keypoint runs on, as in kornia: gn_match's fewer-than-two rule looks at the call's input counts.
 * Pruning and the margin certificate exclude each other: the calibrated eps bounds |P - P_f32| on the SAME token set, and a fast mode may prune a
 * different set.  With gn_set_certify mode > 0 this call returns GN_ERR_ARG; with pruning on, gn_set_certify(mode > 0) and gn_calibrate_certify do.
 * Works through gn_match / gn_estimate / gn_estimate_cov / gn_estimate_report, both feature types, every precision, sub-batch streams, deferred
 * joins and the overlapped pose stage (the new per-slot buffers are sliced like the others). */
int gn_set_width_pruning(gn_ctx* ctx, float width_confidence, int min_kpts);
int gn_get_width_pruning(const gn_ctx* ctx, float* width_confidence, int* min_kpts);
/* kornia's prune0 / prune1 of the most recent matcher call, into HOST buffers [B][gn_kmax] each, after a device synchronisation: how many layers
 * every original keypoint took part in.  Pruning off: n_layers for every keypoint; on but never fired: 1.  Rows past a side's count are 0.
 * B may not exceed the pairs of that call (GN_ERR_ARG; also before the first call on the context's current workspaces).
 * (With deferred joins or deferred certificates open, gn_flush first.) */
int gn_get_prune(gn_ctx* ctx, int B, int32_t* prune_q, int32_t* prune_r);

/* Batched LightGlueMatcher.forward on RAW (un-normalised) SIFT descriptors.
 *   desc_q  [B][stride_q][128] f32     kpt_q [B][stride_q][6 or 4] f32     n_q [B] int32
 *   desc_r  [B][stride_r][128] f32     kpt_r [B][stride_r][6 or 4] f32     n_r [B] int32
 * Outputs (device): idx [B][kmax][2] int64 (col0 query index, col1 reference index, rows in
 * ascending query index), score [B][kmax] f32, n_match [B] int32; kmax = gn_kmax(ctx).
 * A pair with n_q < 2 or n_r < 2 yields n_match = 0 (kornia's _no_match). */
int gn_match(gn_ctx* ctx, int B, int kpt_format,
             const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
             const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
             int64_t* idx, float* score, int32_t* n_match, void* stream);
int gn_kmax(const gn_ctx* ctx);

/* Gather matched points and lift the reference side to 3-D with the DEM.
 *   mkp_q [B][kmax][2] f32, obj [B][kmax][3] f32 = (x_r, y_r, dem[floor(y_r)][floor(x_r)])
 *   dem   [B][H][W] u8 or NULL (z = 0).  `const uint8_t* dem` here and in gn_estimate* points at elements of the context's DEM type
 *         (gn_set_dem_format below; uint8 by default), densely packed.  While that format states a void value, a match on a void cell is
 *         removed: idx and n_match are then rewritten in place (the shorter list), whatever their const qualifier says. */
int gn_gather_points(gn_ctx* ctx, int B, int kpt_format,
                     const float* kpt_q, int stride_q, const float* kpt_r, int stride_r,
                     const int64_t* idx, const int32_t* n_match,
                     const uint8_t* dem, int H, int W,
                     float* mkp_q, float* obj, void* stream);
/* gn_gather_points for a match list that carries scores: score [B][kmax] f32 (may be NULL) is compacted beside idx when voids are removed.
 * Without a void value in the format it is gn_gather_points and idx / score / n_match are only read. */
int gn_gather_points_scored(gn_ctx* ctx, int B, int kpt_format,
                            const float* kpt_q, int stride_q, const float* kpt_r, int stride_r,
                            int64_t* idx, float* score, int32_t* n_match,
                            const uint8_t* dem, int H, int W,
                            float* mkp_q, float* obj, void* stream);

/* Elevation rasters beyond 8 bits (DESIGN.md "Elevation rasters: element types, scale, offset, voids"; the reference's own TODOs:
 * pose_node.py:220 "Support 16-bit elevation", gis_node.py:691).  The element type of every `dem` argument of gn_gather_points and
 * gn_estimate*, an affine map from the raw cell to z, and a void value.  Rasters stay [B][H][W], densely packed in elements of the type.
 *   lift    the cell is chosen as always (floorf, clamped to the raster); z = (float)(raw * scale + offset), the product and the sum taken in
 *           f64 and rounded once each, then rounded to f32.  With scale = 1, offset = 0 this is (float)raw.
 *   voids   with has_nodata, a cell whose raw value equals nodata is void; for GN_DEM_F32 every non-finite cell is void too (nodata = NaN:
 *           those alone).  A match whose reference keypoint lands on a void cell is removed from the call's match list before PnP and the
 *           list is compacted stably: n_match, idx, score, mkp_q and obj all describe the shorter list (the caller's arrays in
 *           gn_estimate_report, the workspaces otherwise), so min_matches, PnP, the covariance and the report need no mask.  A pair whose
 *           matches are all void reports n_match = 0, ok = 0.  gn_match never sees a DEM and is unchanged.
 * Sticky host-side state like gn_set_ransac, captured by value when a call is issued.  The default (GN_DEM_U8, 1, 0, no voids) launches the
 * uint8 gather it always did: same bits, no launch more, no buffer more.  GN_ERR_ARG, with gn_last_error naming this function and the state
 * left alone: unknown type; scale zero or not finite; offset not finite; nodata not representable in an integer type (non-integral or out
 * of its range; ignored when has_nodata = 0). */
enum { GN_DEM_U8 = 0, GN_DEM_U16 = 1, GN_DEM_I16 = 2, GN_DEM_F32 = 3 };
int gn_set_dem_format(gn_ctx* ctx, int type, double scale, double offset, int has_nodata, double nodata);
/* The values in effect (each pointer may be NULL). */
int gn_get_dem_format(const gn_ctx* ctx, int* type, double* scale, double* offset, int* has_nodata, double* nodata);
/* Matches removed as void from pairs 0 .. B-1 of the most recent call that ran with a void value (gn_estimate*, gn_gather_points*);
 * zeros before the first.  dropped_host: HOST [B] int32.  Synchronises the device (the call may sit on the library's own streams). */
int gn_dem_last_dropped(gn_ctx* ctx, int B, int32_t* dropped_host, void* stream);

/* Batched solvePnPRansac + Rodrigues.
 *   obj [B][kstride][3] f32, img [B][kstride][2] f32, n_pts [B] int32, K9: HOST 3x3 row-major f64.
 * Outputs (device): R [B][9] f64 row-major, t [B][3] f64, n_inliers [B] int32,
 * ok [B] u8 (0 when n_pts < min_pts or RANSAC found no model with > 4 inliers).  n_pts == 4 with min_pts <= 4 takes OpenCV's
 * `npoints == 4` branch: one P3P solve (Gao) on the first three points, the fourth picks the pose, all four are inliers, no refinement.
 * iterations_count: 1 .. GN_RANSAC_MAX_ITERATIONS (GN_ERR_ARG outside; gn_last_error names the range).  For every count the result is that
 * of OpenCV's sequential loop: the same cv::RNG stream and subsets, `good > max(maxGood, 4)`, RANSACUpdateNumIters after every improvement,
 * hypotheses at or past the adapted count never counted, the same refinement on the winner's inliers.  Counts up to 16 evaluate all their
 * hypotheses in one launch; above 16 they run in rounds of 64 with the adapted count checked between rounds, so a pair that stops early
 * costs at most one round more than it needed, and the workspace does not grow with the count (DESIGN.md "RANSAC beyond 16 hypotheses"). */
#define GN_RANSAC_MAX_ITERATIONS 4096
int gn_pnp_ransac(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                  const double* K9_host, int iterations_count, float reproj_error_px, double confidence,
                  int min_pts, double* R, double* t, int32_t* n_inliers, uint8_t* ok, void* stream);

/* gn_pnp_ransac + the first-order covariance of the returned pose (DESIGN.md "Pose covariance"; the reference publishes all zeros:
 * pose_node.py:477 "TODO: re-enable covariance/implement error model").  R / t / n_inliers / ok are bit for bit gn_pnp_ransac's.  Per pair
 * with ok = 1: I = the inliers of the winning RANSAC hypothesis (all points when n_pts is 4 or 5), e_i = project(rvec, tvec; X_i) - u_i in
 * f64 on the widened f32 inputs, J = de / d(rvec, tvec), N = J^T J, dof = 2 |I| - 6,
 *   sigma_hat [B] f64 = sqrt(sum |e_i|^2 / dof)             the a-posteriori pixel sigma
 *   cov_rt [B][36] f64 = s^2 N^-1, row-major, symmetric, order (r0, r1, r2, t0, t1, t2); s = sigma_px when sigma_px > 0 (the caller states
 *                        the pixel noise), else sigma_hat
 *   cov_ok [B] u8      = 1 iff ok, dof > 0, every LDL^T pivot of N exceeds 1e-12 of its diagonal entry, and every output is finite;
 *                        otherwise 0, with cov_rt all zeros and sigma_hat 0.
 * Not modelled: DEM height error, match-score weighting, the discreteness of the inlier selection. */
int gn_pnp_ransac_cov(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                      const double* K9_host, int iterations_count, float reproj_error_px, double confidence,
                      int min_pts, double* R, double* t, int32_t* n_inliers, uint8_t* ok,
                      double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream);

/* gn_pnp_ransac(_cov) + a report of the stage: cv2.solvePnPRansac's fourth return value `inliers`, and a per-point residual (DESIGN.md "Report
 * of the pose stage").  R / t / n_inliers / ok are bit for bit gn_pnp_ransac's.  cov_rt / sigma_hat / cov_ok: all three given (then as
 * gn_pnp_ransac_cov) or all three NULL.  The report arrays are device outputs, row stride kstride, each may be NULL on its own; with all three
 * NULL nothing more is launched than without this call.
 *   inlier_mask [B][kstride] u8     1 where point i is an inlier of the winning RANSAC hypothesis -- the set the refinement and the covariance
 *                                   sum over; every point when n_pts is 4 or 5 --, 0 elsewhere: slots >= n_pts, and the whole row when ok = 0
 *   inlier_idx  [B][kstride] int32  the indices of the inliers, ascending (cv2's `inliers`): the first n_inliers[b] entries, the rest -1;
 *                                   the whole row -1 when ok = 0
 *   reproj_err  [B][kstride] f32    |project(R, t; X_i) - u_i| in pixels at the RETURNED (refined) pose for every i < n_pts, inlier or not,
 *                                   through the forward model the stage uses (lens distortion included when gn_set_distortion is on), in f64
 *                                   on the widened f32 inputs, stored as f32; -1 in slots >= n_pts, and in every slot when ok = 0
 * As in OpenCV the mask comes from the hypothesis model (f32 squared error <= reproj_error_px^2 at the minimal solver's pose) and reproj_err
 * from the refined pose: an inlier may sit above reproj_error_px in reproj_err, and a point below it may be no inlier. */
int gn_pnp_ransac_report(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                         const double* K9_host, int iterations_count, float reproj_error_px, double confidence,
                         int min_pts, double* R, double* t, int32_t* n_inliers, uint8_t* ok,
                         double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                         uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream);

/* cv2.solvePnPRansac's iterationsCount, reprojectionError and confidence for the PnP stage that gn_estimate(_cov), gn_vo_estimate(_cov) and
 * the certificate's re-runs issue themselves (gn_pnp_ransac(_cov) take theirs as arguments).  Sticky host-side state like gn_set_distortion;
 * the default (10, 8.0, 0.99) is what the reference passes (_shared.py:115), and a context that is never told, or told the default, computes
 * bit for bit what it always did.  Captured when a call is issued, as K9_host and the distortion coefficients are.  iterations_count outside
 * 1 .. GN_RANSAC_MAX_ITERATIONS, reproj_error_px <= 0 or confidence outside (0, 1): GN_ERR_ARG, state unchanged. */
int gn_set_ransac(gn_ctx* ctx, int iterations_count, float reproj_error_px, double confidence);
/* The values in effect (each pointer may be NULL). */
int gn_get_ransac(const gn_ctx* ctx, int* iterations_count, float* reproj_error_px, double* confidence);
/* "How hard was this frame": for pairs 0 .. B-1 of the most recent PnP stage of this context, the final adapted iteration count (what
 * RANSACUpdateNumIters left; 0 where the loop never ran: n_pts < min_pts, or the 4-point branch) and the number of hypotheses that were
 * actually evaluated (above 16 requested: less than one round of 64 past the adapted count; up to 16: all that were requested, they run at
 * once).  Synchronises the device.  niters_host /
 * evaluated_host: HOST [B] int32.  The point counts of that stage (n_pts / n_match, device) must still be alive.  After a call that was split
 * into sub-batch groups (gn_set_substreams) every group's pairs are reported; after a certificate re-run, the re-run's. */
int gn_ransac_last_counts(gn_ctx* ctx, int B, int32_t* niters_host, int32_t* evaluated_host, void* stream);

/* Lens distortion of the PnP stage: cv2.solvePnPRansac's distCoeffs argument (the reference passes zeros, _shared.py:104-116; a real camera
 * publishes CameraInfo.d).  d_host: HOST, n = 4 (k1, k2, p1, p2; k3 = 0) or 5 (k1, k2, p1, p2, k3) plumb-bob coefficients; NULL or n = 0
 * switches it off, and so do coefficients that are all zero: every output is then bit for bit what it was before the call.  n = 8, 12, 14
 * (rational, thin-prism, tilted) and non-finite values return GN_ERR_ARG (gn_last_error says why) and leave the state as it was.  Sticky
 * host-side state like gn_set_image_size, off by default.  It applies to the PnP stage of gn_pnp_ransac(_cov), gn_estimate(_cov) and
 * gn_vo_estimate(_cov) in every mode (gn_set_overlap, gn_set_substreams, gn_set_deferred_join, the certificate's re-runs); the coefficients
 * are captured when a call is issued, as K9_host is: a change between two pipelined calls does not reach the earlier call.
 * Semantics (OpenCV 4.x restated, DESIGN.md "Lens distortion"): the minimal solvers (EPnP, P3P) and the planar / DLT start read image points
 * undistorted by cv::undistortPoints' FIVE fixed-point steps (not run to convergence); hypothesis scoring, the Levenberg-Marquardt residuals
 * and Jacobian, and the covariance's e_i and J use the forward model with distortion against the raw image points. */
int gn_set_distortion(gn_ctx* ctx, const double* d_host, int n);
/* The coefficients in effect into d5_host (HOST, 5 doubles, zeros when off; may be NULL).  Returns 1 when distortion is on, 0 when off. */
int gn_get_distortion(const gn_ctx* ctx, double* d5_host);
/* cv2.undistortPoints(img, K, d) with the context's coefficients (gn_set_distortion) for B point lists.
 *   img [B][kstride][2] f32 pixels, n_pts [B] int32, K9: HOST 3x3 row-major f64, out [B][kstride][2] f32 (device; slots past n_pts untouched).
 * to_pixels = 0: normalised coordinates; 1: K re-applied (cv2's P = K).  Computed in double and stored as f32 (cv2's output takes the
 * input's depth); five fixed-point steps, as above.  With distortion off the result is (float)((u - cx) / fx), (float)((v - cy) / fy). */
int gn_undistort_points(gn_ctx* ctx, int B, const float* img, const int32_t* n_pts, int kstride,
                        const double* K9_host, int to_pixels, float* out, void* stream);

/* Per-pair cameras: one camera per pair of a batch instead of one K9_host (and one gn_set_distortion state) per call -- frames of several
 * vehicles, each with its own CameraInfo, in one call.
 * cams: DEVICE [n][GN_PAIR_CAMERA_DOUBLES] f64, row b = the camera of pair b of every later call.
 * model 0: the pinhole instantiations (coefficient columns ignored); 1: the plumb-bob instantiations for every pair
 * (a row of zero coefficients is a pinhole camera run through them).  cams = NULL or n = 0 switches the table off.
 * Sticky host-side state like gn_set_distortion, off by default; n < 0, n > max_batch or a model outside {0, 1} returns GN_ERR_ARG
 * (gn_last_error names this setter) and leaves the state as it was.  Off, every output is bit for bit what it was and nothing more is
 * launched, copied or read.
 * While a table is set it rules every gn_pnp_ransac(_cov|_report), gn_estimate(_cov|_report), gn_vo_estimate(_cov|_report) and
 * gn_undistort_points call: a call with B > n returns GN_ERR_ARG; K9_host may be NULL and is ignored; the gn_set_distortion state is ignored
 * for those calls (it stays stored and applies again once the table is off).  Every mode works: gn_set_overlap, gn_set_substreams (a group
 * reads its own rows), gn_set_deferred_join, the certificate's re-runs (a re-run pair takes its row with it), more than 16 RANSAC
 * iterations, point pruning, gn_set_active_kpts.
 * Lifetime: the table is an input of the call, like n_q: read in stream order (the overlapped PnP stage reads a copy made in stream order),
 * the pointer and the model captured when the call is issued; the caller keeps it alive and unchanged as long as the call's other inputs --
 * until gn_flush under gn_set_deferred_join or the deferred certificate.  The rows are not validated (they are device memory): fx, fy > 0
 * and finite values are the caller's to ensure (PoseEngine.pair_cameras checks them on the host). */
#define GN_PAIR_CAMERA_DOUBLES 9      /* fx, fy, cx, cy, k1, k2, p1, p2, k3 */
int gn_set_pair_cameras(gn_ctx* ctx, const double* cams, int n, int model);
/* The table in effect: each pointer may be NULL; returns 1 when on, 0 when off (then *cams = NULL, *n = 0, *model = 0). */
int gn_get_pair_cameras(const gn_ctx* ctx, const double** cams, int* n, int* model);

/* PoseNode._pose lines 246-308 for B pairs: match -> gather -> MIN_MATCHES gate -> PnP. */
int gn_estimate(gn_ctx* ctx, int B, int kpt_format,
                const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                const uint8_t* dem, int H, int W, const double* K9_host, int min_matches,
                double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok, void* stream);

/* gn_estimate with gn_pnp_ransac_cov as its last stage.  cov_rt / sigma_hat / cov_ok are per-pair outputs like R / t / ok: complete when those are, in
 * every mode (gn_set_overlap, gn_set_substreams, gn_set_deferred_join, gn_set_certify 2 and 3 -- a re-run pair gets the re-run's covariance). */
int gn_estimate_cov(gn_ctx* ctx, int B, int kpt_format,
                    const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                    const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                    const uint8_t* dem, int H, int W, const double* K9_host, int min_matches,
                    double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                    double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream);

/* gn_estimate(_cov) + the match list the pose was computed from and gn_pnp_ransac_report's report of its PnP stage.  cov_rt / sigma_hat / cov_ok:
 * all three or none.  idx [B][kmax][2] int64 and score [B][kmax] f32 are exactly gn_match's outputs (with idx given the matcher writes into it
 * and the gather reads it there); inlier_mask / inlier_idx / reproj_err are [B][kmax], kmax = gn_kmax(ctx), and their row k refers to row k of
 * idx (the gather keeps row order); a pair below min_matches has an all-sentinel report.  Each of the five may be NULL on its own; with all
 * NULL this is gn_estimate(_cov).  They are per-pair outputs like R / t / ok: complete when those are, in every mode (gn_set_overlap,
 * gn_set_substreams, gn_set_deferred_join, gn_set_certify 2 and 3 and the ladder -- a re-run pair gets the re-run's matches and report). */
int gn_estimate_report(gn_ctx* ctx, int B, int kpt_format,
                       const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                       const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                       const uint8_t* dem, int H, int W, const double* K9_host, int min_matches,
                       double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                       double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                       int64_t* idx, float* score, uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream);

/* Throughput option for back-to-back gn_estimate calls (batch serving): with overlap enabled the PnP stage of a call
 * runs on an internal stream beside the matcher of the NEXT call (its inputs are double-buffered).  R / t /
 * n_inliers / ok of a call are then complete only after gn_flush(ctx, stream) has been issued behind it (it makes
 * `stream` wait for every outstanding PnP stage); n_match is complete in stream order as before.  Off by default:
 * without it everything is complete in stream order when gn_estimate returns. */
int gn_set_overlap(gn_ctx* ctx, int enable);
/* Throughput option for back-to-back calls: split the B pairs of every gn_estimate call into n groups (1..8) that run
 * the whole path on n internal streams, forked from the caller's stream; consecutive calls pipeline inside each
 * group's stream and one group's memory-bound kernels overlap another's matrix-bound ones.  By default the caller's stream
 * is made to wait for every group before gn_estimate returns: inputs and outputs obey plain stream order, as without the
 * option.  Measured on the 32-pair bench with the round-2 kernels: +7..10 % with n = 2 (bench.py times `value` that way), slower with
 * n >= 3 (smaller launches); off (n = 1) by default. */
int gn_set_substreams(gn_ctx* ctx, int n);
/* Opt-in companion of gn_set_substreams: leave the join to gn_flush, so that the groups of consecutive calls drift out of
 * phase.  Then ALL outputs of a call (n_match included) are complete only after gn_flush(ctx, stream), and the caller must
 * keep the INPUT buffers of a call alive (and unmodified) until it has flushed -- they are read off the caller's stream.
 * A call whose B or active padded size differs from the previous unflushed call joins first, by itself. */
int gn_set_deferred_join(gn_ctx* ctx, int enable);
/* The matcher pads every image to a multiple of 128 keypoints; by default that is max_kpts of gn_create.  When the caller
 * knows an upper bound of the keypoint counts of the coming calls (the SIFT entry points return them), this sets the padded
 * size those calls run at -- attention cost falls with its square, the GEMMs linearly.  Keypoints beyond it are ignored.
 * Results do not depend on the padded size (padding is masked out exactly).  Returns the padded size now in effect
 * (min(round_up(max_kpts_per_side, 128), padded max_kpts of the context)) or a negative status.  Output strides (gn_kmax)
 * do not change.  Host-side, STICKY state: it stays in effect for every later gn_match / gn_estimate on this context until
 * it is set again -- a caller that shrinks it for one batch restores it afterwards (gn_set_active_kpts(ctx, max_kpts));
 * the Python mirrors (PoseEngine.estimate_images, PoseNode.estimate) do. */
int gn_set_active_kpts(gn_ctx* ctx, int max_kpts_per_side);
int gn_flush(gn_ctx* ctx, void* stream);

/* ---- visual-odometry path of TwistNode ---------------------------- */
/* cv2.BFMatcher(crossCheck=False).knnMatch(desc_qry, desc_ref, k=2) + Lowe ratio test for B frame pairs --
 * ros/gisnav/gisnav/core/twist_node.py:95,248-267.  Descriptors [B][stride][128] f32 (cv2.SIFT output:
 * integer-valued, for which distances are bit-identical to OpenCV's; f32 rounding of d^2 otherwise).
 *   idx  [B][kmax][2] int64 (queryIdx, trainIdx) of the matches with m.distance < ratio * n.distance, in query
 *        order; dist [B][kmax] f32 = m.distance; n_good [B] (0 when a pair has fewer than 2 train descriptors)
 *   nn_idx / nn_dist: optional [B][kmax][2] best and second-best train index (int32, -1 = none) / distance
 *        per query keypoint (the raw knnMatch result), may be NULL. */
int gn_vo_match(gn_ctx* ctx, int B, const float* desc_q, const int32_t* n_q, int stride_q,
                const float* desc_r, const int32_t* n_r, int stride_r, double ratio,
                int64_t* idx, float* dist, int32_t* n_good, int32_t* nn_idx, float* nn_dist, void* stream);

/* TwistNode._pose lines 227-289 for B frame pairs: knnMatch -> ratio test -> MIN_MATCHES gate ->
 * compute_pose(camera_info, mkp_qry, mkp_ref, zeros) (planar PnP-RANSAC + Rodrigues); outputs as gn_estimate. */
int gn_vo_estimate(gn_ctx* ctx, int B, int kpt_format,
                   const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                   const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                   const double* K9_host, double ratio, int min_matches,
                   double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok, void* stream);

/* gn_vo_estimate with gn_pnp_ransac_cov as its last stage. */
int gn_vo_estimate_cov(gn_ctx* ctx, int B, int kpt_format,
                       const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                       const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                       const double* K9_host, double ratio, int min_matches,
                       double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                       double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream);

/* gn_vo_estimate(_cov) + the match list (gn_vo_match's idx and dist, as `score`) and the report, as gn_estimate_report. */
int gn_vo_estimate_report(gn_ctx* ctx, int B, int kpt_format,
                          const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                          const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                          const double* K9_host, double ratio, int min_matches,
                          double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                          double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                          int64_t* idx, float* score, uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream);

/* ---- StereoNode reference-raster preparation ----------------------- */
/* StereoNode._rotate_and_crop_center(image, angle_degrees, shape) -- ros/gisnav/gisnav/core/stereo_node.py:292-335:
 * cv2.getRotationMatrix2D((W//2, H//2), angle, 1.0) + cv2.warpAffine(image, M, (W, H)) [INTER_LINEAR, constant 0
 * border] + centre crop, on a 2-channel u8 stack [H][W][2] (device).  out_stack [crop_h][crop_w][2] (device);
 * back9_host: optional HOST 3x3 f64 = the returned matrix (rotated-and-cropped frame -> original frame). */
int gn_rotate_crop_center(gn_ctx* ctx, const uint8_t* stack, int H, int W, double angle_degrees, int crop_h, int crop_w,
                          uint8_t* out_stack, double* back9_host, void* stream);
/* stereo_node.py:229-262 fused: cv2.cvtColor(BGR2GRAY) + np.dstack((gray, dem)) + _rotate_and_crop_center.
 * bgr [H][W][3] u8, dem [H][W] u8 (device) -> out_ref, out_dem [crop_h][crop_w] u8 (device). */
int gn_stereo_reference(gn_ctx* ctx, const uint8_t* bgr, const uint8_t* dem, int H, int W, double angle_degrees,
                        int crop_h, int crop_w, uint8_t* out_ref, uint8_t* out_dem, double* back9_host, void* stream);
/* gn_stereo_reference for a DEM of any element type (GN_DEM_*): dem [H][W] and out_dem [crop_h][crop_w] hold elements of dem_type.  The type
 * and the void value are arguments, not context state (StereoNode and PoseNode are different processes).  out_ref is byte for byte
 * gn_stereo_reference's, as if the two rasters were warped separately.  A GN_DEM_U8 DEM keeps the fixed-point arithmetic.  The other types
 * use the float bilinear form this build defines: source cell and 1/32 fractions fx, fy as for the gray channel; f32 weights
 * (32-fx)(32-fy)/1024, fx(32-fy)/1024, (32-fx)fy/1024, fx fy/1024; v = ((t0 w0 + t1 w1) + t2 w2) + t3 w3, every product and sum rounded
 * to f32; taps outside the source, and taps of zero weight, read 0; integer outputs are rint (half to even) saturated to the type.
 * With has_nodata an output cell stores nodata when any tap of non-zero weight is void (equal to nodata; non-finite for GN_DEM_F32) or
 * outside the source: angle 0 is an exact crop and voids do not dilate.  nodata must be representable in an integer type (GN_ERR_ARG). */
int gn_stereo_reference_dem(gn_ctx* ctx, const uint8_t* bgr, const void* dem, int dem_type, int has_nodata, double nodata, int H, int W,
                            double angle_degrees, int crop_h, int crop_w, uint8_t* out_ref, void* out_dem, double* back9_host, void* stream);

/* ---- post-pose georeferencing (host-side scalar code, no context) ---- */
/* _transformations.py:298-323 proj_to_affine: "+proj=affine +xoff=.. +s11=.. ..." -> 3x4 row-major [s11 s12 s13 xoff; ...]. */
int gn_proj_to_affine(const char* proj_str, double* affine12);
/* _transformations.py:326-345 wgs84_to_ecef (pyproj latlong -> geocent on the WGS 84 datum), degrees / metres. */
int gn_wgs84_to_ecef(double lon_deg, double lat_deg, double alt_m, double* xyz3);
/* pose_node.py:333-381: r [9] row-major, t [3] of compute_pose + the OrthoStereoImage CRS affine ->
 * `earth`-frame camera position (ECEF metres) and orientation quaternion (x, y, z, w) of gisnav_camera_link_optical;
 * lonlatalt3 optional.  Returns GN_OK, or 1 if the camera centre is outside the expected range of the reference
 * raster (the node returns None, pose_node.py:339-341). */
int gn_pose_to_earth(const double* R9, const double* t3, const double* affine12, int ref_h, int ref_w,
                     double* position_ecef3, double* quat_xyzw4, double* lonlatalt3);

/* cov_rt of gn_pnp_ransac_cov (HOST, 6x6 row-major) -> covariance of the camera in the raster frame, order (cx, cy, cz, phi_x, phi_y, phi_z):
 * c = -R^T t [raster px], phi [rad] the increment of R_wc = R^T with R_wc,true = Exp(phi) R_wc.  Closed form: phi = -J_r(rvec) d rvec (J_r the
 * right Jacobian of SO(3)), dc = -R^T dt - [c]x phi. */
int gn_pose_cov_to_camera(const double* R9, const double* t3, const double* cov_rt36, double* cov_cam36);
/* ... and pushed through gn_pose_to_earth's map: order (ECEF x, y, z [m], psi_x, psi_y, psi_z [rad]) with q_true = dq(psi) (x) q_est for the
 * quaternion gn_pose_to_earth returns (rotation about the fixed axes: the layout of geometry_msgs/PoseWithCovariance.covariance).  Returns
 * GN_OK, or 1 exactly where gn_pose_to_earth returns 1 (cov_earth36 is then not written). */
int gn_pose_cov_to_earth(const double* R9, const double* t3, const double* cov_rt36, const double* affine12, int ref_h, int ref_w,
                         double* cov_earth36);

/* ---- SIFT feature extraction ------------------------------------------ */
/* cv2.SIFT_create(nOctaveLayers, contrastThreshold, edgeThreshold, sigma).detectAndCompute(gray, None) with the parameters of
 * gn_sift_set_params (OpenCV's defaults 3, 0.04, 10, 1.6 until it is called) -- the tile extractor of PoseNode
 * (pose_node.py:122,230-232) and the frame extractor of TwistNode (twist_node.py:93,227-245).
 *   gray [H][W] u8 (device).  Outputs (device): kpt_xysa [max_kpts][4] f32 = (x, y, size, angle_deg) -- the
 *   GN_KPT_XYSA keypoint format of gn_match / gn_estimate; response [max_kpts] f32 and octave [max_kpts] int32
 *   (packed as cv2.KeyPoint.octave) may be NULL; desc [max_kpts][128] f32 (integer-valued 0..255, as cv2 emits).
 *   n_out_host: HOST int32, number of keypoints, in OpenCV's order (sorted by x, y, size desc, angle, ...).
 *   More than max_kpts distinct keypoints: the call does NOT fail -- like cv2's `nfeatures` cap (KeyPointsFilter::retainBest,
 *   pose_node.py:108) the max_kpts keypoints of largest response are kept (equal responses: the earlier one in the order
 *   above), still listed in that order (cv2 itself leaves them in nth_element order and keeps every tie of the last
 *   response); gn_sift_last_totals reports how many there were, so the caller can grow its buffers.
 * Everything -- scale space, extrema, refinement, the sort / duplicate removal, descriptors -- runs on the device in
 * stream order; the call synchronises `stream` once, at the end, to hand the keypoint count to the host. */
int gn_sift_detect_and_compute(gn_ctx* ctx, const uint8_t* gray, int H, int W, int max_kpts,
                               float* kpt_xysa, float* response, int32_t* octave, float* desc, int32_t* n_out_host, void* stream);
/* The same for B equally sized images in ONE pass (every kernel launch covers all images): gray [B][H][W]; outputs
 * [B][max_kpts][...] with image b's keypoints in rows [0, n_out_host[b]); n_out_host: HOST int32 [B].  The reference
 * extracts one image per ROS message; batching is this build's addition for the frames -> pose pipeline, whose matcher
 * (gn_estimate) already takes batches of pairs in this keypoint format. */
int gn_sift_detect_and_compute_batch(gn_ctx* ctx, const uint8_t* gray, int B, int H, int W, int max_kpts,
                                     float* kpt_xysa, float* response, int32_t* octave, float* desc, int32_t* n_out_host, void* stream);

/* cv2.SIFT_create's nOctaveLayers, contrastThreshold, edgeThreshold and sigma for the gn_sift_detect_and_compute(_batch) calls that follow:
 * sticky host-side state like gn_set_ransac, (3, 0.04, 10, 1.6) by default -- with those values a context computes exactly what it computes
 * when never told.  Accepted: n_octave_layers 1 .. 5, contrast_threshold finite and >= 0, edge_threshold finite and > 0, sigma in [1.0, 2.4];
 * anything else returns GN_ERR_ARG (gn_last_error names the range) and leaves the state as it was.  The ranges are this build's own (cv2 accepts
 * more): they bound an octave at 8 Gaussian + 7 DoG planes and the widest blur kernel at 135 taps.  A change of n_octave_layers or sigma
 * replaces the SIFT workspace (pyramid planes, blur kernels) at the next call; the thresholds cost nothing to change.  nfeatures is the
 * max_kpts argument of the call (order and tie rule above).  gn_sift_get_params: any pointer may be NULL. */
int gn_sift_set_params(gn_ctx* ctx, int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma);
int gn_sift_get_params(const gn_ctx* ctx, int* n_octave_layers, double* contrast_threshold, double* edge_threshold, double* sigma);

/* Distinct keypoints each image of the LAST gn_sift_detect_and_compute(_batch) call had before the max_kpts cap (HOST int32 [B]). */
int gn_sift_last_totals(gn_ctx* ctx, int B, int32_t* totals_host);

/* ---- SuperPoint extractor (BASELINE.json configs[4] / north_star "conv backbone"; not in the reference tree) ---------- */
/* Load one tensor of the SuperPoint network from HOST memory, float32, torch layout ([out][in][kh][kw] for conv weights), under
 * transformers' SuperPointForKeypointDetection key names: encoder.conv_blocks.{0..3}.conv_{a,b}.{weight,bias},
 * keypoint_decoder.conv_score_{a,b}.*, descriptor_decoder.conv_descriptor_{a,b}.*. */
int gn_sp_load_tensor(gn_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
/* SuperPoint on B grayscale images: gray01 [B][H][W] f32 in [0, 1] (device), H and W multiples of 8.  Outputs (device):
 * kpt_xysa [B][max_kpts][4] = (x, y, 1, 0) keypoint records in the GN_KPT_XYSA format of gn_match / gn_estimate (for a
 * GN_FEATURE_SUPERPOINT context), score [B][max_kpts] (may be NULL), desc [B][max_kpts][256] L2-normalised; n_out_host: HOST
 * int32 [B] keypoints per image, sorted by descending score (raster order on equal scores).  Detector settings of the
 * published model: threshold 0.005, NMS radius 4, border 4, top max_kpts (<= 2048).  The convolutions are exact f32
 * (v_mfma_f32_32x32x2_f32).  Synchronises `stream` once per pass of 4 images to read the counts. */
int gn_sp_detect_and_describe(gn_ctx* ctx, const float* gray01, int B, int H, int W, int max_kpts,
                              float* kpt_xysa, float* score, float* desc, int32_t* n_out_host, void* stream);
/* Arithmetic of the SuperPoint convolutions: GN_SP_EXACT_F32 (v_mfma_f32_32x32x2_f32: every context can), GN_SP_SPLIT_FP16 (f32 operands
 * as two fp16 terms, three products, f32 accumulate: f32-accurate, the default of f16x2 contexts, with the fp16-range guard and exact
 * retry), GN_SP_FP16 (ONE fp16 product per block, f32 accumulate: the 16-bit-operand arithmetic BASELINE.json configs[4] names
 * ("bf16"; fp16 keeps three more mantissa bits) -- NOT f32-accurate: ~99 % of the keypoints of the exact path on the test images;
 * same guard and retry).  The two fp16 modes need a context of the f16x2 precision; elsewhere the call returns GN_ERR_ARG. */
enum { GN_SP_EXACT_F32 = 0, GN_SP_SPLIT_FP16 = 1, GN_SP_FP16 = 2 };
int gn_sp_set_arithmetic(gn_ctx* ctx, int mode);

/* ---- LoFTR (BASELINE.json north_star "LoFTR / SuperPoint+LightGlue", configs[1] "LoFTR matcher ... fp32"; not in the reference tree) ---- */
/* kornia.feature.LoFTR(pretrained = "outdoor").forward({"image0", "image1"}) -> keypoints0 / keypoints1 / confidence for ONE pair of equally
 * sized grayscale images (the detector-free matcher older GISNav releases used; at this tag only the word survives:
 * docs/vitepress/docs/glossary.md:186).  f32 throughout: ResNet-FPN backbone on the exact f32 matrix instruction, 4 x (self, cross)
 * LINEAR-attention encoder layers at 1/8 resolution, dual-softmax coarse matching (temperature 0.1, threshold 0.2, border 2, mutual
 * maxima), and -- when `fine` is set -- the 5x5-window fine level that refines keypoints1 to sub-pixel positions.  Specification:
 * the published architecture as restated in oracle/loftr.py (parity UNPINNED: kornia is not importable in the build image).
 * A context is sized for one image shape (H, W multiples of 8) and at most min(max_matches, H/8 * W/8, 131072) matches per call: a pair has
 * at most one match per coarse cell of image0, so max_matches >= H/8 * W/8 returns all of them, as kornia does (the Python mirror's default);
 * a smaller number keeps the first ones in ascending cell order.  The context is separate from gn_ctx and owns its weights. */
typedef struct gn_loftr gn_loftr;
int gn_loftr_create(int device, int H, int W, int max_matches, int fine, gn_loftr** out);
void gn_loftr_destroy(gn_loftr* ctx);
const char* gn_loftr_last_error(const gn_loftr* ctx);
/* One tensor of kornia's LoFTR state dict from HOST memory (float32, torch layout): backbone.* (convolutions [out][in][k][k], BatchNorm
 * weight / bias / running_mean / running_var), loftr_coarse.layers.{0..7}.* and loftr_fine.layers.{0,1}.* ({q,k,v}_proj, merge, mlp.0,
 * mlp.2 weights; norm1 / norm2 weight + bias), fine_preprocess.{down_proj,merge_feat}.{weight,bias}.  pos_encoding.pe and
 * num_batches_tracked entries are accepted and ignored. */
int gn_loftr_load_tensor(gn_loftr* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int gn_loftr_missing_tensors(const gn_loftr* ctx);
/* image0 / image1: DEVICE f32 [H][W] in [0, 1].  Outputs (device): kpts0 / kpts1 [max_matches][2] (x, y) pixels (kpts0 on the 1/8 grid;
 * kpts1 = coarse cell + fine offset, or the coarse cell without a fine level), conf [max_matches], ij (optional, may be NULL)
 * [max_matches][2] int32 coarse cell indices (i in image0, j in image1); matches in ascending i.  *n_host (HOST): number of matches;
 * the call synchronises `stream` once to return it. */
int gn_loftr_match(gn_loftr* ctx, const float* image0, const float* image1, float* kpts0, float* kpts1, float* conf, int32_t* ij,
                   int32_t* n_host, void* stream);
/* The same matcher on B pairs per call.  gn_loftr_create_batch sizes the context for up to max_pairs pairs of one image shape (device memory
 * grows with max_pairs: one similarity matrix and one set of activations per pair; creation fails with GN_ERR_HIP when it does not fit, and
 * with GN_ERR_ARG when max_pairs x the padded per-pair match slots exceed 131072); gn_loftr_create is the max_pairs = 1 case and
 * gn_loftr_match the B = 1 call of the same code.  gn_loftr_cap: the per-pair segment length cap = min(max_matches, H/8 * W/8, 131072).
 * image0 / image1: DEVICE f32 [B][H][W], 1 <= B <= max_pairs (GN_ERR_ARG otherwise).  Outputs (device) in per-pair segments of cap rows: kpts0 /
 * kpts1 [B][cap][2], conf [B][cap], ij [B][cap][2] (may be NULL); pair b's matches are the first n[b] rows of its segment, in ascending cell of
 * image0 -- the layout gn_gather_points / gn_pnp_ransac take with kstride = cap and n_pts = n_match_dev.  n_match_dev (DEVICE [B], may be NULL)
 * and n_host (HOST [B], may be NULL) receive the counts.  A pair's outputs do not depend on B, on its place in the batch or on the other pairs,
 * bit for bit.  Synchronisation: in exact-f32 arithmetic without n_host the call does not synchronise `stream` (the counts stay on the device
 * for the solver); with n_host it synchronises once for the whole batch; split-fp16 arithmetic always synchronises once to read the per-pair
 * range guards (and once more only when a pair had to be repeated).  One hipGraph is captured lazily per (arithmetic, B). */
int gn_loftr_create_batch(int device, int max_pairs, int H, int W, int max_matches, int fine, gn_loftr** out);
int gn_loftr_match_batch(gn_loftr* ctx, int B, const float* image0, const float* image1, float* kpts0, float* kpts1, float* conf, int32_t* ij,
                         int32_t* n_match_dev, int32_t* n_host, void* stream);
int gn_loftr_cap(const gn_loftr* ctx);
/* 1 (default): the forward's ~190 dependent launches are captured once into a hipGraph (all buffers belong to the context, the match count
 * stays on the device) and replayed with one graph launch per call; 0: plain stream launches (same kernels, same results). */
int gn_loftr_set_graph(gn_loftr* ctx, int enable);
/* Arithmetic of the convolutions and linear layers: 0 (default) exact f32 (v_mfma_f32_32x32x2_f32) -- what configs[1] names; 1 split fp16: every
 * f32 operand as two fp16 terms, three fp16 MFMA products, f32 accumulation (the matcher's f16x2 scheme: f32-accurate, 5 x the matrix-pipe
 * rate).  Mode 1 guards fp16's range PER PAIR: the pairs of a call in whose forward any activation left it are repeated on the exact kernels, as a
 * smaller batch, before the call returns; the other pairs keep their split-arithmetic results. */
int gn_loftr_set_arithmetic(gn_loftr* ctx, int mode);
/* Certified coarse matches: a per-pair certificate that the coarse (i, j) list of this arithmetic is the one exact f32 computes.
 * With eps a bound on |conf - conf_f32| entry-wise, thr = 0.2, border = 2 and a coarse cell INTERIOR when it lies at least `border` cells from every
 * edge, a pair is flagged when (a) an interior row's best confidence is >= thr - eps and leads its runner-up (multiplicity counted: a tie has gap
 * 0) by <= 2 eps, (b) the same for an interior column, or (c) an interior row's best lies within eps of thr.  An unflagged pair's list is f32's.
 * mode 0 (default): off -- outputs, launches and time are those of a library without the certificate.  mode 1: flags only, the results stay the
 * context's arithmetic (on an exact-f32 context: the pairs f32's own rounding decides).  mode 2: flagged pairs are repeated on the exact-f32
 * kernels inside the call, together with the pairs of the fp16-range guard, and overwrite their segments; needs arithmetic 1 (GN_ERR_ARG
 * otherwise, and gn_loftr_set_arithmetic(0) is refused while it is on).  eps: 0 <= eps < 1 states it; eps < 0 means the one
 * gn_loftr_calibrate_certify measured (GN_ERR_ARG when there is none).  A certified call synchronises once (flags, guard words and counts in one
 * read), also in exact-f32 arithmetic; eps may change between calls (the captured graph reads it from device memory). */
int gn_loftr_set_certify(gn_loftr* ctx, int mode, float eps);
/* Measure eps on a sample of B pairs (DEVICE f32 [B][H][W], B <= max_pairs): the sample runs in split-fp16 and in exact-f32 arithmetic,
 * d_max = max over the pairs and all i, j of |conf_split - conf_f32|, eps = max(floor_eps, safety x d_max) becomes the context's calibrated eps.
 * out (HOST): {d_max, eps}.  safety >= 1, 0 <= floor_eps < 1.  Fails (GN_ERR_ARG) when the fp16-range guard trips on the sample.  Holds one more
 * similarity matrix per pair for the duration of the call.  gn_loftr_load_tensor afterwards discards the calibrated eps: it belongs to its weights. */
int gn_loftr_calibrate_certify(gn_loftr* ctx, int B, const float* image0, const float* image1, float safety, float floor_eps, float* out,
                               void* stream);
/* flags_host (HOST int32 [B]): 1 for the pairs of the last certified call (B = its batch size) that the certificate flagged -- in mode 2 the
 * pairs that were repeated for it.  A pair repeated for the fp16-range guard is exact already and not flagged. */
int gn_loftr_get_uncertain(gn_loftr* ctx, int B, int32_t* flags_host);
/* out4 (HOST int64 [4]) since the context was created: pairs seen by certified calls, pairs flagged, pairs repeated for the certificate, pairs
 * repeated for the fp16-range guard. */
int gn_loftr_get_certify_stats(gn_loftr* ctx, int64_t* out4);
/* test hook: internal tensor -> HOST after synchronising.  Names: "x1" "x2" "x3" "x3_out" "x1_out" (NHWC, 196 channels padded to 224),
 * "tok" ([2][Lp][256] coarse features after the transformer), "sim", "crow", "ccol", "ftok"; of the last certified forward "crow2", "ccol2" (the
 * runner-ups) and "unc" (the certificate's words, raw).  Returns the element count or a negative status.
 * After a call with B pairs the buffers are side-major over the pairs: [2][B]... maps and tokens, [B]... "sim" / "crow" / "ccol". */
int64_t gn_loftr_debug_read(gn_loftr* ctx, const char* name, void* host_out, int64_t max_bytes, void* stream);
/* Developer knobs of THIS LoFTR context: the selectors its launches read, with the numbers and values gn_debug_set_variant documents below --
 * 41 and 44 (the exact-f32 GEMM's 64-row and 64 x 64 tile forms) and 42 (bits 8 and up: the overhead term of the convolutions' rows-per-wave cost
 * model x 100; any of bits 0-7 is refused).  Every other knob returns GN_ERR_ARG.  Synchronises the device and drops the context's captured
 * graphs: the next call captures again with the knob in force.  All three select between forms with identical results. */
int gn_loftr_debug_set_variant(gn_loftr* ctx, int which, int value);

/* ---- test / profiling hooks (not part of the drop-in surface) --------------------------- */
/* Copy an internal workspace tensor to HOST memory after synchronising `stream`.
 * Names: "desc" "cos" "sin" "x" "qkv" "ctx" "msg" "h" "md" "ls" "sim" "rowmax" "rowlog"
 * "colmax" "collog" "m0" "m1" "max0" "max0b" "colbest" "col2" (ints are returned bit-cast in float slots; the last two exist after a call that
 * measured columns: gn_calibrate_certify's middle level, gn_debug_match_head). Returns the element
 * count copied, or a negative status.  "sim" exists only after the unfused match head (developer knob 16 = 0), gn_vo_match or a
 * phase-stamp knob allocated it: the matcher itself never materialises the similarity matrix (it returns 0 elements before that).
 * SuperPoint extractor (last pass): "sp_enc" "sp_scores" "sp_nms" "sp_counts" "sp_cand" "sp_x" "sp_y" (raw words of the two activation
 * buffers), "sp_z" (f32: the raw descriptor map [h][w][256]; the logits [h][w][128] when developer knob 39 stopped the pass at layer 9), and
 * "sp_split_trips" (ONE int64, 8 bytes: how many passes of this context the split-fp16 guard repeated on the exact f32 convolutions). */
int64_t gn_debug_read(gn_ctx* ctx, const char* name, void* host_out, int64_t max_bytes, void* stream);
/* Stand-alone kernels for unit tests: Y[M,N] = A[M,K] W[N,K]^T + bias (f32 MFMA path). */
int gn_debug_gemm(gn_ctx* ctx, int M, int N, int K, const float* A, const float* W, const float* bias,
                  float* Y, void* stream);
/* softmax(q k^T * scale) v for [BS][n][heads*64]-strided tensors; nkv [BS] valid key counts. */
int gn_debug_attention(gn_ctx* ctx, int BS, int npad, int cross, float qscale,
                       const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       const int32_t* nkv, float* out, int ldo, void* stream);
/* The match head alone, as gn_match runs it behind the last layer (the same launches: the fused two-sweep form, or the similarity GEMM + five passes
 * under developer knob 16 = 0; gn_set_filter_threshold and gn_set_certify's mode / eps / eps_f32 apply; no weights needed).  md [B][2][np][256] f32
 * projected descriptors (side 0, then side 1), ls [B][2][np] f32 log-sigmoid matchabilities, nvalid [B][2]; np a multiple of 128, at most gn_kmax().
 * The inputs are copied into the context's workspaces laid out at np (an f16x2 context splits md into hm16 rows as the projection's epilogue does), so
 * gn_debug_read serves the first B * np elements of "rowmax" "rowlog" "colmax" "collog" "max0" "max0b" "m0" "m1" -- and, from the fused form, "colbest"
 * "col2": best score and runner-up of every column -- and gn_get_uncertain the flags.  idx [B][gn_kmax()][2], score [B][gn_kmax()], n_match [B]. */
int gn_debug_match_head(gn_ctx* ctx, int B, int np, const float* md, const float* ls, const int32_t* nvalid,
                        int64_t* idx, float* score, int32_t* n_match, void* stream);
/* Milliseconds spent in each stage of the last gn_estimate/gn_match when timing is enabled. */
int gn_set_stage_timing(gn_ctx* ctx, int enable);
int gn_get_stage_ms(gn_ctx* ctx, float* host_ms, int max_stages);
/* HIP-event timing of every launch of the dominant kernel (the f32 MFMA GEMM) on the caller's
 * stream: enable with room for max_launches launches (0 disables), then read
 * out3 = {launches recorded, total milliseconds, total algorithmic flops (2 M N K)}. */
/* Developer knobs: select a kernel variant (which = 0: GEMM) for A/B benchmarking; run a pure
 * v_mfma_f32_32x32x2_f32 issue-rate probe (blocks x 256 threads x iters x 8 MFMAs per wave).
 * Every knob belongs to the context it is set on and to nothing else: a gn_ctx keeps the matcher's and the pose stage's (0-33, 41, 43, 44, 47-49), the SuperPoint
 * extractor's (21, 34, 35, 39, 40, 46) and the SIFT extractor's (50) for the calls made on it; a gn_loftr keeps its own 41, 42 and 44
 * (gn_loftr_debug_set_variant).  Another context, of either type, in the same process is not affected.
 * Knobs added in round 2 (value 0 restores the round-1 path unless noted): 10 block-tail fusion level, 12 block-tail phase stamps
 * (8; k_ffn128 also 136), 13 out_proj folded into the tail, 14 k_ffn_fused workgroup shape (64 / 32 tokens), 15 PnP phase stamps,
 * 16 fused match head (0 = similarity GEMM + five passes), 17 k_head_fused phase stamps, 19 k_qkv projections
 * (0 = tiled GEMM, 2 = force at any batch size), 20 k_qkv phase stamps, 21 SuperPoint split-fp16 convolutions, 23 largest number of key ranges the
 * attention of a small batch is split into (default 1 = never; 4 gives -5 % latency at batch 1 but rounds the probabilities per split), 25 start the guard word of sub-batch group value - 1 raised (tests).  Knob 1 (attention) values: 4 default,
 * 5 k_attn16_v5 always, 56 the exact running maximum in every key tile (the path a workgroup of the default kernel falls back to), 60 the
 * optimistic fp16 form, 70 / 73 k_attn_pw whenever it applies (73 with phase stamps), 80 / 81 k_attn_ks always (eight / four waves).  Knob 8: 0 / 1
 * (the 256 x 256 GEMM k_gemm_p2w off / automatic).  Retired timing ablations and rejected experiments (knob 0 = 51-57, 61-67; knob 1 = 41-46,
 * 48, 51-55, 57, 58, 71, 72, >= 1000; knob 8 >= 2; knob 12 other than 0 / 8 / 136; knob 18; knob 24 and knob 36 with any value, knob 34 other than 0 / 2: SuperPoint's superseded
 * convolution and simple_nms forms; knob 42 with any value: it is a gn_loftr knob and reaches nothing here) return GN_ERR_ARG.  A bench line run with any knob set records it in `debug_variant`.
 * Knobs of late round 5 (the shipped value is 0 unless noted): 41 (gn_ctx and gn_loftr) largest 128 x 128 grid the exact-f32 GEMM leaves to 64-row
 * tiles (320; 0 = never), 42 (gn_loftr only) bits 8 and up: the overhead term of the rows-per-wave cost model of LoFTR's convolutions x 100 (0 = the shipped 0.25; bits
 * 0-7 selected LoFTR's forms of rounds 3-4 and are retired), 43 (gn_ctx) exact-f32 attention of one or two pairs (bits 0-1: 0 = k_attn_f32_ks, 1 = k_attn_f32 always, 2 = k_attn_f32_ks
 * always; bit 2 its eight-wave form), 44 (gn_ctx and gn_loftr) exact-f32 GEMM on 64 x 64 tiles (1 = for grids of at most 128 workgroups on 64 x 128 tiles, 0 = never,
 * 2 = the four-slot-ring kernel on 64 x 128 tiles everywhere).  All of them select between forms with identical results except 43 (f32 rounding).
 * Knob 49: 1 sends iterations_count <= 16 through the round path of the PnP stage as well (same bits; tests). */
int gn_debug_set_variant(gn_ctx* ctx, int which, int value);
int gn_debug_mfma_probe(gn_ctx* ctx, int blocks, int iters, void* stream);
/* LDS-DMA addressing probe (80 KB of LDS per block filled by global_load_lds, verified by ds_read):
 * pattern [8][80][256] f32, out [81] u32 = mismatching words per 1 KB piece + number of blocks run. */
int gn_debug_lds_dma_probe(gn_ctx* ctx, const float* pattern, unsigned int* out, int blocks, int spin, void* stream);
/* EPnP minimal solver on n 5-point sets: pws [n][5][3] f64, us [n][5][2] f64 (normalised image
 * coordinates), out [n][64] f64 = R(9) t(3) candidate errors(3) candidate betas(12) eigenvalues(12) rho(6) L row0(10) ok(1). */
int gn_debug_epnp(gn_ctx* ctx, int n, const double* pws, const double* us, double* out, void* stream);
/* HIP-event timing of individual launches inside gn_match / gn_estimate (on the caller's stream):
 * record up to max_launches launches (0 = off, resets the log); kernel_class 0 = projection / FFN /
 * similarity GEMMs, 1 = attention; out3 = {launches, summed ms, summed algorithmic flops}. */
int gn_set_kernel_timing(gn_ctx* ctx, int max_launches);
int gn_get_kernel_stats(gn_ctx* ctx, int kernel_class, double* out3);
/* summed ALGORITHMIC HBM bytes of the same launches (every operand / result array once: the compulsory traffic). */
int gn_get_kernel_bytes(gn_ctx* ctx, int kernel_class, double* out1);
/* Per-kernel table of the launches recorded since gn_set_kernel_timing, as a JSON array in `json` (capacity bytes):
 * [{"name", "launches", "ms", "flops", "bytes"}, ...] with rocprofv3-style kernel names; returns the length or a negative status. */
int gn_get_kernel_table(gn_ctx* ctx, char* json, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* GISNAV_AMD_H */
