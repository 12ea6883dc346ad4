// C ABI of libgisnav_amd.so: context, weight loading, and the stream-ordered schedule of the
// PoseNode hot path (ros/gisnav/gisnav/core/pose_node.py:246-308, core/_shared.py:89-125).
// See include/gisnav_amd.h for the contract of every entry point.
#include "gn_common.h"

#include <cstdio>
#include <cstring>
#include <cmath>
#include <cctype>
#include <algorithm>
#include <memory>
#include <tuple>

using namespace gn;

namespace {

thread_local std::string g_err;

struct Linear { float* w = nullptr; float* b = nullptr; int out = 0, in = 0; uint16_t* wp = nullptr; float acc_scale = 1.f;
                uint16_t* wf = nullptr; int frag_order = -1;       // frag_order: -1 none, else the k order of build_weight_fragments
                uint16_t* wf2 = nullptr;
                uint16_t* wfn = nullptr; };                         // ffn.3 only: NATURAL k order (gn_skinny.hip reads GELU rows from memory, not from registers)                         // ffn.0 only: order 2 (message half permuted) for the folded out_proj   // wf: the scaled fp16 pair in MFMA fragment order (gn_ffn.hip), same scale as wp
// wp: pre-split planes, [3][out][in] bf16 (f32x3) or [2][out][in] fp16 of w / acc_scale (f16x2; acc_scale a power of two)

struct Block {       // one SelfBlock or CrossBlock
  Linear proj_in;    // self: Wqkv re-ordered to [q|k|v][head][d] (768x256); cross: [to_qk ; to_v] (512x256)
  Linear proj_out;   // out_proj / to_out
  Linear ffn0;       // 512x512
  float* ln_g = nullptr; float* ln_b = nullptr;
  Linear ffn3;       // 256x512
  // out_proj / to_out COMPOSED into ffn.0 (round 4): ffn.0([x | out_proj(ctx)]) = [W1_x | W1_m Wo] [x | ctx] + (b1 + W1_m bo) -- the message tile and
  // its GEMM (14 % of the block tail's matrix work) disappear; built at the first forward call after the tensors were (re)loaded
  uint16_t* wfc = nullptr; float* b1c = nullptr; float wfc_scale = 1.f; bool comp_dirty = true;
};

enum Stage { ST_PREP = 0, ST_PROJ, ST_ATTN, ST_FFN, ST_HEAD, ST_GATHER, ST_PNP, ST_COUNT };

// One matcher / estimate call: its per-pair arrays as pointers to the first pair, the strides that step from pair to pair, and the estimate's
// call-wide inputs.  A per-pair array the call does not own stays null (the estimate path's idx / score live in the e_idx / e_score workspaces
// unless gn_estimate_report was given arrays for them).
struct Call {
  int B = 0, kpt_format = 0, stride_q = 0, stride_r = 0;
  const float *desc_q = nullptr, *kpt_q = nullptr, *desc_r = nullptr, *kpt_r = nullptr; const int32_t *n_q = nullptr, *n_r = nullptr;
  const uint8_t* dem = nullptr; int H = 0, W = 0;      // dem: [B][H][W] elements of demf.type
  // gn_set_dem_format as the context held it when the call was issued, by value; dropped: the call's rows of the dem_dropped workspace while the
  // format states a void value (null otherwise) -- a per-pair output like n_match, so slices, staged re-runs and their scatter carry it
  gn::DemFormat demf; int32_t* dropped = nullptr;
  double *R = nullptr, *t = nullptr; int32_t *n_match = nullptr, *n_inliers = nullptr; uint8_t* ok = nullptr; int64_t* idx = nullptr; float* score = nullptr;
  double *cov = nullptr, *sigma_hat = nullptr; uint8_t* cov_ok = nullptr; double sigma_px = 0.0;   // pose covariance (gn_estimate_cov): null = not asked for
  uint8_t* inlier_mask = nullptr; int32_t* inlier_idx = nullptr; float* reproj_err = nullptr;   // report of the pose stage (gn_estimate_report): each null = not asked for
  const double* K9 = nullptr; int min_matches = 0;
  int dist = 0; double dk[5] = {0, 0, 0, 0, 0};   // lens distortion as the context held it when the call was issued (gn_set_distortion), by value
  int ransac_iters = 10; float ransac_reproj = 8.0f; double ransac_conf = 0.99;   // gn_set_ransac, captured the same way
  // per-pair cameras (gn_set_pair_cameras) as the context held them when the call was issued: DEVICE [B][GN_PAIR_CAMERA_DOUBLES], a per-pair input
  // like n_q (null = off: K9 / dist / dk above); cam_model picks the PnP instantiation for the whole call
  const double* cams = nullptr; int cam_model = 0;
  int kw = 0, in_dim = 0; size_t km = 0;   // floats per keypoint, per descriptor; match-list stride (gn_kmax)
  Call() = default;
  Call(int feature, int npad, int B_, int kpt_format_, const float* desc_q_, const float* kpt_q_, const int32_t* n_q_, int stride_q_,
       const float* desc_r_, const float* kpt_r_, const int32_t* n_r_, int stride_r_)
      : B(B_), kpt_format(kpt_format_), stride_q(stride_q_), stride_r(stride_r_), desc_q(desc_q_), kpt_q(kpt_q_), desc_r(desc_r_), kpt_r(kpt_r_),
        n_q(n_q_), n_r(n_r_), kw((kpt_format_ & 0xff) == GN_KPT_LAF ? 6 : (kpt_format_ & 0xff) == GN_KPT_RECORD ? kRecordFloats : 4),
        in_dim(feature == GN_FEATURE_SIFT ? kInDim : kDim), km((size_t)npad) {}
};

// Every per-pair array of the calls `c...` (all of one shape, that of h), in one fixed order -- inputs, then outputs -- as f(bytes per pair, is output,
// c.array...).  Slicing, the re-run's staging layout, its gather and its scatter all walk this list.
template <typename F, typename... C> void pair_arrays(const Call& h, F&& f, C&... c) {
  f((size_t)h.stride_q * h.in_dim * 4, false, c.desc_q...); f((size_t)h.stride_r * h.in_dim * 4, false, c.desc_r...);
  f((size_t)h.stride_q * h.kw * 4, false, c.kpt_q...); f((size_t)h.stride_r * h.kw * 4, false, c.kpt_r...);
  f((size_t)4, false, c.n_q...); f((size_t)4, false, c.n_r...); f((size_t)h.H * h.W * gn::dem_elem_bytes(h.demf.type), false, c.dem...);
  f((size_t)GN_PAIR_CAMERA_DOUBLES * 8, false, c.cams...);
  f((size_t)72, true, c.R...); f((size_t)24, true, c.t...); f((size_t)4, true, c.n_match...); f((size_t)4, true, c.n_inliers...); f((size_t)1, true, c.ok...);
  f(h.km * 16, true, c.idx...); f(h.km * 4, true, c.score...); f((size_t)4, true, c.dropped...);
  f((size_t)288, true, c.cov...); f((size_t)8, true, c.sigma_hat...); f((size_t)1, true, c.cov_ok...);
  f(h.km, true, c.inlier_mask...); f(h.km * 4, true, c.inlier_idx...); f(h.km * 4, true, c.reproj_err...);
}
// the report arrays of a PnP stage (gn_pnp_ransac_report), each null on its own
struct Report { uint8_t* inlier_mask = nullptr; int32_t* inlier_idx = nullptr; float* reproj_err = nullptr; };
Report report_of(const Call& v) { return {v.inlier_mask, v.inlier_idx, v.reproj_err}; }
template <typename T> T* byte_offset(T* p, size_t bytes) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + bytes); }

// pairs [b0, b0 + n) of a call
Call slice(const Call& v, size_t b0, int n) {
  Call o = v;
  o.B = n;
  pair_arrays(o, [&](size_t bytes, bool, auto*& p) { if (p) p = byte_offset(p, b0 * bytes); }, o);
  return o;
}

// Fields (of the context) restored to their values at construction when the scope ends: the one way this file overrides context state for a while
template <typename... T> struct Restore {
  std::tuple<T&...> ref; std::tuple<T...> val;
  explicit Restore(T&... r) : ref(r...), val(r...) {}
  ~Restore() { ref = val; }
  Restore(const Restore&) = delete;
  Restore& operator=(const Restore&) = delete;
};

// The per-pair device workspaces of the matcher, the PnP stage and point pruning, each declared ONCE, here:
//   X(element type, field, elements per pair, when it exists, gn_debug_read name or nullptr)
// Allocation is max_batch x (elements per pair at np = npad); a view of the pairs from b0 on starts b0 x (elements per pair at np = npad_run)
// into every buffer -- the buffers are laid out per call, at the padded size the call runs at.  Nothing else states a workspace's size.
// T2 = 2 np (tokens per pair); km = npad = gn_kmax(): the match lists, the PnP masks and the work lists are strided by the context's padded
// maximum whatever the active size.  uint16_t buffers count uint16 elements (hm16 rows: 2 T C).  A buffer that is not per pair (attn_part,
// attn_tickets, vo_*, the guard words, tile_feedback, the pinned mirrors, cert_stage) is never sliced and stays a plain member of the context.
enum { kWsAlways = 1, kWsF16x2 = 2 /* f16x2 contexts */, kWsNotF32 = 4 /* every precision but f32 */, kWsFirstUse = 8 /* ensure_sim */, kWsPnpStage = 16 /* ensure_pnp_stage */ };
inline long long lists_stride_of(long long km) { return gn::kTileListBase + 2 * (km / 128) + 8 * ((km + 255) / 256); }   // ints per pair (launch_tile_lists)
#define GN_WORKSPACES(X)                                                                                                         \
  X(float, desc, T2 * kInDim, kWsAlways, "desc") X(float, cos_t, T2 * kFreq, kWsAlways, "cos") X(float, sin_t, T2 * kFreq, kWsAlways, "sin") \
  X(float, extent, 4, kWsAlways, "extent") X(int32_t, nvalid, 2, kWsAlways, "nvalid")                                            \
  X(float, x, T2 * kDim, kWsAlways, "x") X(float, qkv, T2 * 3 * kDim, kWsAlways, "qkv") X(float, ctx, T2 * kDim, kWsAlways, "ctx") \
  X(float, msg, T2 * kDim, kWsAlways, "msg") X(float, h, T2 * 2 * kDim, kWsAlways, "h") X(float, md, T2 * kDim, kWsAlways, "md") \
  X(float, ls, T2, kWsAlways, "ls")                                                                                              \
  /* f16x2 mode: the hm16 rows that shadow the f32 activations feeding GEMMs (planes_of), written by their producers */          \
  X(uint16_t, desc_p, 2 * T2 * kInDim, kWsF16x2, "desc_p") X(uint16_t, x_p, 2 * T2 * kDim, kWsF16x2, "x_p")                      \
  X(uint16_t, ctx_p, 2 * T2 * kDim, kWsF16x2, nullptr) X(uint16_t, msg_p, 2 * T2 * kDim, kWsF16x2, "msg_p")                      \
  X(uint16_t, h_p, 2 * T2 * 2 * kDim, kWsF16x2, nullptr) X(uint16_t, md_p, 2 * T2 * kDim, kWsF16x2, nullptr)                     \
  /* rotary table of k_qkv: [16][Tmax] float4, plane-strided by Tmax (rot_stride) -- a pair is 2 np float4 further on in every plane */ \
  X(float, rot4, slicing ? T2 * 4 : T2 * 2 * kFreq, kWsF16x2, "rot4")                                                            \
  X(uint16_t, qkb, T2 * 2 * kDim, kWsNotF32, "qkb") X(uint16_t, vtb, T2 * kDim, kWsNotF32, "vtb") /* 16-bit q | k rows, V^T panels */ \
  /* match head: per-row / per-column statistics, the certificate's runner-ups and per-pair flags, the calibration's column scores */ \
  X(float, rowmax, np, kWsAlways, "rowmax") X(float, rowlog, np, kWsAlways, "rowlog") X(float, colmax, np, kWsAlways, "colmax")  \
  X(float, collog, np, kWsAlways, "collog") X(float, max0, np, kWsAlways, "max0") X(int32_t, m0, np, kWsAlways, "m0")            \
  X(int32_t, m1, np, kWsAlways, "m1") X(float, max0b, np, kWsAlways, "max0b") X(float, rpart_c, 8 * np, kWsAlways, nullptr)      \
  X(int32_t, uncert, 1, kWsAlways, "uncert") X(int32_t, uncert_alt, 1, kWsAlways, nullptr) X(int32_t, uncert_alt2, 1, kWsAlways, nullptr) \
  X(int32_t, uncert_alt3, 1, kWsAlways, nullptr)                                                                                 \
  X(float, colbest, np, kWsAlways, "colbest") X(float, col2, np, kWsAlways, "col2")                                                 \
  /* fused head: column partials [np / 32][np], row partials [8][np], two arrival counters (zero between calls) */               \
  X(float, cpart_m, (np / 32) * np, kWsAlways, nullptr) X(float, cpart_s, (np / 32) * np, kWsAlways, nullptr)                    \
  X(int32_t, cpart_i, (np / 32) * np, kWsAlways, nullptr) X(float, rpart_a, 8 * np, kWsAlways, nullptr)                          \
  X(float, rpart_b, 8 * np, kWsAlways, nullptr) X(unsigned int, tickets, 2, kWsAlways, nullptr)                                  \
  /* gn_estimate's match list, gathered points and PnP scratch (e_idx has 8-byte elements: gn_debug_read serves it by hand) */   \
  X(int64_t, e_idx, km * 2, kWsAlways, nullptr) X(float, e_score, km, kWsAlways, "e_score") X(float, e_mkp, km * 2, kWsAlways, "e_mkp") \
  X(float, e_obj, km * 3, kWsAlways, "e_obj") X(uint8_t, mask_ws, km * 16, kWsAlways, nullptr) X(float, pts_ws, km * 5, kWsAlways, nullptr) \
  X(gn::HypResult, hyp_ws, 16, kWsAlways, "hyp")                                                                                 \
  /* matches the gather removed as void (gn_set_dem_format with a void value; written and read only then): gn_dem_last_dropped */ \
  X(int32_t, dem_dropped, 1, kWsAlways, "dem_dropped")                                                                           \
  /* round path of the PnP stage: [kRansacRound + 1][km] masks whatever iterations_count, one state */                           \
  X(uint8_t, rmask_ws, km * (gn::kRansacRound + 1), kWsAlways, "ransac_mask") X(gn::RansacState, rstate_ws, 1, kWsAlways, "ransac_state") \
  X(int, lists, lists_stride_of(km), kWsAlways, "lists") /* work lists of the call as they stand ([0] tiles, [1] attention items, ...) */ \
  /* point pruning (gn_prune.hip), [2][np] per pair: original indices, prune counts, move targets, z of the last pruning layer;   \
     pr_counts: [2][kMaxLayers] a slot's count after every layer; pr_nin: [2] the call's input counts (the head's no-match rule) */ \
  X(int32_t, pr_ind, T2, kWsAlways, "prune_ind") X(int32_t, pr_prune, T2, kWsAlways, nullptr) X(int32_t, pr_dst, T2, kWsAlways, nullptr) \
  X(int32_t, pr_counts, 2 * kMaxLayers, kWsAlways, "prune_counts") X(int32_t, pr_nin, 2, kWsAlways, nullptr) X(float, pr_z, T2, kWsAlways, "prune_z") \
  /* [np][np] similarity buffer: TwistNode's brute-force matcher, the unfused developer path and the phase-stamp tools only */   \
  X(float, sim, np * np, kWsFirstUse, "sim")                                                                                     \
  /* PnP inputs of the overlapped pose stage, double-buffered by call parity */                                                  \
  X(float, o_mkp0, km * 2, kWsPnpStage, nullptr) X(float, o_obj0, km * 3, kWsPnpStage, nullptr) X(int32_t, o_nmatch0, 1, kWsPnpStage, nullptr) \
  X(float, o_mkp1, km * 2, kWsPnpStage, nullptr) X(float, o_obj1, km * 3, kWsPnpStage, nullptr) X(int32_t, o_nmatch1, 1, kWsPnpStage, nullptr) \
  /* the call's rows of the per-pair camera table beside them (written and read only while gn_set_pair_cameras is on) */         \
  X(double, o_cams0, GN_PAIR_CAMERA_DOUBLES, kWsPnpStage, nullptr) X(double, o_cams1, GN_PAIR_CAMERA_DOUBLES, kWsPnpStage, nullptr)

struct Workspace {
#define X(type, field, per_pair, when, name) type* field = nullptr;
  GN_WORKSPACES(X)
#undef X
};
// f(field, elements per pair, when it exists, debug name) for every workspace of w, in table order
template <typename F> void for_each_workspace(Workspace& w, long long np, long long km, bool slicing, F&& f) {
  const long long T2 = 2 * np;
#define X(type, field, per_pair, when, name) f(w.field, (long long)(per_pair), (int)(when), (const char*)(name));
  GN_WORKSPACES(X)
#undef X
}
// The workspaces of the pairs from b0 on (view_of): what a sub-batch group, or the certificate's re-run of a run of pairs, works in.  The code
// that enqueues work reads workspaces from the view it is given, never from the context.  g: the sub-batch group, ovf: its guard word.
struct View : Workspace { long long b0 = 0; int g = 0; unsigned int* ovf = nullptr; };

}  // namespace

struct gn_ctx {
  int device = 0, max_batch = 0, npad = 0, precision = 0;
  int x_planes_only = 1;   // f16x2 mode: between layers the residual stream x exists only as hm16 pairs (developer knob 11; 0 = also f32, residual read as f32)
  int qkv_stamps = 0;      // developer knob 20: k_qkv writes s_memtime phase stamps into the sim buffer
  int qkv_fused = 1;       // attention input projections by k_qkv (gn_qkv.hip) instead of the LDS-staged GEMM (developer knob 19)
  int sp_split = 1;        // gn_sp_set_arithmetic (developer knob 21): 0 exact f32, 1 split-fp16 operands (contexts of the f16x2 mode), 2 one fp16 product
  long long sp_split_trips = 0;
  int sp_stop = 0;
  int sp_ts_layer = 0;          // developer knob 35: the layer (1..11) whose k_sp_conv_s launch writes phase stamps into sp_ts (gn_debug_read("sp_ts"))
  long long* sp_ts = nullptr;   // [8192 workgroups][32] s_memtime stamps
  void* sp_allocs_dbg = nullptr;
  bool sp_enc_hm16 = false, sp_enc_fp16 = false;   // the last pass left the encoder output (sp_y) as hm16 records (gn_debug_read("sp_enc") converts)
  int head_fused = 1;      // match head: 1 = two fused sweeps that recompute the similarity tiles (no sim buffer); 0 = sim GEMM + five passes (developer knob 16)
  int head_stamps = 0;     // developer knob 17: k_head_fused writes s_memtime phase stamps into the sim buffer
  int pnp_rounds = 0;      // developer knob 49: iterations_count <= 16 through the round path of the PnP stage too
  int pnp_stamps = 0;      // developer knob 15: k_pnp_* write s_memtime phase stamps into the sim buffer
  int ffn_compose = 1;     // with ffn_fused == 3 and ffn_fold: out_proj / to_out composed into ffn.0's weights (developer knob 28; 0 = the kernel computes the message)
  int ffn_fold = 1;        // with ffn_fused == 3: out_proj / to_out folded into the block-tail kernel (developer knob 13; 0 = separate GEMM launch)
  int ffn_fused = 3;       // f16x2 mode: 3 = the whole block tail in one launch (k_ffn_fused, gn_ffn.hip); 1 = ffn.0 + LayerNorm + GELU in one launch
                           // (k_gemm_p2ln) when the grid fills the chip, 2 = always; 0 = separate k_ln_gelu (developer knob 10)
  // f16x2 domain guard (gn_set_guard): device word raised by any hm16 writer whose value does not fit fp16
  // ovf_base: [0..7] one word per sub-batch group of the matcher (groups run concurrently on their own streams and each clears / reads its own
  // word: View::ovf), [8] the SuperPoint extractor's, [12] selfcheck_fused_projection's counter; ovf_host: pinned mirror of all 16
  unsigned int* ovf_base = nullptr; unsigned int* ovf_host = nullptr;
  int dbg_trip_group = 0;  // developer knob 25: g + 1 = the matcher starts group g's guard word RAISED instead of cleared (tests of the per-group words)
  bool in_group = false;   // gn_estimate is enqueuing one of its sub-batch groups (gn_match then leaves ovf_groups_last alone)
  int ovf_groups_last = 1; // number of group words the most recent matcher call used (gn_get_guard_status ORs exactly those)
  int guard = 1;           // 0 off, 1 flag (a tripped call reports zero matches), 2 flag + synchronous re-run in the f32x3 mode
  long long guard_trips = 0;   // calls that tripped (counted when observed: guard 2, or gn_get_guard_status)
  // margin certificate (gn_set_certify): the match head keeps the runner-up of every row / column maximum and flags, per PAIR, a decision that
  // lies within cert_eps of flipping; mode 2 reads the flags back once per call (one stream synchronisation) and re-runs the flagged pairs in the
  // exact-f32 arithmetic (GN_PREC_F32's kernels on this context's f32 weights and f32 workspaces), which also takes over the fp16-range fallback
  int certify = 0;             // 0 off, 1 flags only (gn_get_uncertain), 2 flags + f32 re-run of the flagged pairs
  float cert_eps = 4.0e-3f;    // stated bound on |P_mode - P_exact| for this context's arithmetic (tools/certify_eps.py measures it)
  int cert_eps_src = 0;        // where cert_eps comes from: 0 the built-in default, 1 stated (gn_set_certify), 2 measured (gn_calibrate_certify),
                               // 3 measured on weights since replaced (gn_load_tensor; cert_eps is then +inf: every pair goes to exact f32)
  float cert_eps_f32 = 1.0e-4f;   // the same for the exact-f32 kernels (GPU f32 against the torch-CPU f32 oracle: summation order only)
  int32_t* uncert_host = nullptr;   // pinned [4 * max_batch] (flags | the three other arithmetics' flags)
  bool cert_inner = false;     // a certificate re-run is being enqueued (no nested certification)
  void* cert_stage = nullptr; size_t cert_stage_bytes = 0;      // staging block of the gathered re-run (certify_rerun), grown on demand
  // mode 3 (deferred): gn_estimate leaves the flags of call n in a pinned slot behind an event and resolves them -- reads them, re-runs the flagged
  // pairs from the SAVED arguments -- after call n + 1 has been enqueued (or in gn_flush), so the host never waits for an idle GPU
  struct CertPending {
    bool active = false; hipEvent_t ev = nullptr; int32_t* flags = nullptr;   // flags: pinned [4 * max_batch] (own level | the three alternates, as uncert_host)
    int npad_run = 0, level = 0;
    Call call; double K9[9] = {0};      // call.K9 points at K9, the saved copy of the caller's matrix
  } cert_pend[2];
  int cert_slot = 0;
  long long cert_calls = 0, cert_pairs = 0, cert_flag_margin = 0, cert_flag_range = 0, cert_rerun = 0, cert_f32_marginal = 0;
  int attn_f16 = 0;        // GN_PREC_F16X2_F16_ATTN: q | k rows, V^T panels and the probabilities are fp16 instead of bf16 (precision itself reads F16X2_BF16_ATTN);
                           // 2 = split: f32 q | k | v rows from the f16x2 projection GEMMs, k_attn_f16x2 (GN_PREC_F16X2_F16X2_ATTN, and the ladder's middle level)
  // the certificate's re-run ladder (gn_set_certify_ladder): flagged pairs are re-run first in mode-5 arithmetic (MidLevel) and certified there against
  // cert_eps_mid (< 0 = not calibrated: straight to exact f32); only the pairs still flagged go on to exact f32
  int ladder = 0; float cert_eps_mid = -1.f, cert_mid_measured = -1.f;
  long long mid_rerun = 0, mid_certified = 0, mid_passed = 0;
  bool cal_cols = false;   // the fused head also writes colbest / col2: best score / runner-up of every column
  int precision_api = 0;   // the gn_precision value gn_create was called with
  int feature = 0;         // GN_FEATURE_SIFT / GN_FEATURE_SUPERPOINT (gn_create_ex)
  int ransac_iters = 10; float ransac_reproj = 8.0f; double ransac_conf = 0.99;   // gn_set_ransac: what gn_estimate / gn_vo_estimate pass to the PnP stage
  gn::DemFormat demf;      // gn_set_dem_format: element type, scale, offset and void value of every `dem` argument (default: uint8, 1, 0, none)
  gn::PnpArgs last_pnp; bool last_pnp_valid = false; const int32_t* last_npts = nullptr;   // the most recent PnP stage (gn_ransac_last_counts)
  int dist_on = 0; double dist[5] = {0, 0, 0, 0, 0};      // gn_set_distortion: plumb-bob (k1, k2, p1, p2, k3) of the PnP stage; off = the pinhole kernels
  // gn_set_pair_cameras: the caller's DEVICE table [pair_cams_n][GN_PAIR_CAMERA_DOUBLES] (null = off) and the model (0 pinhole, 1 plumb-bob) its calls run
  const double* pair_cams = nullptr; int pair_cams_n = 0, pair_cams_model = 0;
  float size_q[2] = {0.f, 0.f}, size_r[2] = {0.f, 0.f};   // gn_set_image_size: (w, h) per side for the keypoint normalisation, 0 = keypoint extent
  int npad_run = 0;        // padded keypoint count the matcher runs at (<= npad, gn_set_active_kpts); buffers are laid out for it per call
  int n_layers = kMaxLayers;
  float threshold = 0.5f;
  // point pruning (gn_set_width_pruning; gn_prune.hip): off unless width_conf > 0 (workspaces: pr_*)
  float width_conf = -1.f; int prune_min_kpts = 1536;
  bool prune_last_on = false; int prune_last_np = 0, prune_last_layers = 0, prune_last_B = 0;                  // the most recent matcher call (gn_get_prune)
  std::string err;
  // weights
  Linear input_proj;
  float* wr = nullptr;
  Block self_blk[kMaxLayers], cross_blk[kMaxLayers];
  Linear final_proj[kMaxLayers], matchability[kMaxLayers];
  std::map<std::string, bool> loaded;
  std::vector<std::string> required;
  Workspace ws;            // the per-pair workspaces as allocated (GN_WORKSPACES): changes in alloc_workspaces only; work is enqueued on a view_of it
  size_t Tmax = 0;         // token slots allocated (max_batch * 2 * npad) = plane stride in rows
  int planes_mode = 0;     // 1: activations travel as fp16 planes and GEMMs run k_gemm_p2 (default in f16x2 mode)
  float* attn_part = nullptr; unsigned int* attn_tickets = nullptr;   // split-keys attention of small batches: <= 256 partial results, their tickets
  int attn_split = 1;      // developer knob 23: largest number of key ranges the attention of a small batch is split into (default 1 = never: the
                           // split changes the rounding of the probabilities, and results would then depend on batch size / padding / sub-streams)
  gn::LaunchKnobs knobs;   // the kernel selectors of this context's launches (gn_debug_set_variant); gn_create sets knobs.gemm_variant from the precision:
                           // 3 f32 MFMA (LDS-DMA), 5 f32x3 (GN_PREC_F32X3_BF16_ATTN), 6 f16x2
  int stop_after = 0;      // developer knob: return from run_matcher after this many GEMM/attention launches
  int launch_count = 0;
  int no_planes = 0;       // developer knob: ignore the pre-split weight planes (f32x3 splits B on the fly)
  int dbg_planes = 0;      // gn_debug_gemm: pre-split W into bf16 planes first (exercises the WP path)
  uint16_t* dbg_wp = nullptr; size_t dbg_wp_n = 0;
  int dbg_out = 0;         // gn_debug_gemm variant 7: 1 = hm16 output only (into scratch), 2 = f32 + hm16 (timing experiments)
  uint16_t* dbg_yp = nullptr; size_t dbg_yp_n = 0;
  int dbg_vt_skip = 0;     // timing probe: projection epilogues skip the V^T panel stores (wrong results)
  int dbg_reuse = 0;       // gn_debug_gemm: keep the operand planes of the previous call (micro-benchmarks time the GEMM alone)
  uint16_t* dbg_ap = nullptr; size_t dbg_ap_n = 0;   // gn_debug_gemm, variant 7: A planes for k_gemm_p2
  // sub-batch streams (gn_set_substreams): the pairs of one call are split into groups that run the whole path on
  // internal streams, out of phase with each other (fork / join events around them on the caller's stream)
  int defer_join = 0, sub_last_B = 0, sub_last_np = 0;   // gn_set_deferred_join; shape of the last unjoined sub-stream call
  int sub_serial = 0;      // developer knob 26: the sub-batch groups run one after the other on ONE stream (a working set the size of the Infinity Cache) instead of concurrently
  int cu_mask_mode = 0;    // developer knob 29
  int use_lists = 1;       // knob 31.  0: every tile.  1 (default): k_qkv / k_attn_pw walk the call's lists of tiles with valid tokens, and the block tail k_ffn128
                           // chooses its form from the padding the SAME group's previous call had (tile_feedback): one workgroup per tile (padding-only tiles leave
                           // at once) while >= 90 % of the tiles hold tokens, else one workgroup per CU walking the list (3 % slower per tile on a batch without
                           // padding, 20 % faster on a ragged one; identical bits).  2: always walk.  3: never walk.
  int ncu = 256;           // compute units of ctx->device (grids of the walking kernels)
  int fused_proj_status = -1;   // self-check of the projection fused behind the block tail (selfcheck_fused_projection): -1 not run / not applicable to this
                                // context, 1 bitwise equal to the separate k_qkv launches, 0 differed -> fused_proj_off for this context
  bool fused_proj_pending = true;   // run the self-check at the next forward call (set by every weight (re)load and block-tail level change)
  int fused_proj_off = 0;  // the self-check saw a difference: the fusion stays off until the next check passes (knob 32 keeps the caller's setting)
  int qkv_in_tail = 1;     // knob 32.  1 (default): on bulk grids the block tail k_ffn128 also computes the NEXT block's attention input projection from the rows
                           // it has just produced (k_ffn128<., ., ., 1 / 2>: no k_qkv launch, no read-back of the residual stream); 0: separate k_qkv launches
  int skinny = 1;          // knob 33.  1 (default): calls of one or two pairs run the attention input projections and the block
                           // tail as CU-split small-grid kernels (gn_skinny.hip); 0: never; 2: whenever the shapes allow; + 4: not the projections; + 8: not the tail;
                           // >> 4: kernel variant (tools/skinny_ab.py)
  // gn_set_ffn_products(0) -- the level follows the certificate: with eps calibrated for both levels (cert_eps_lvl[0 / 1] = two / three products, < 0 = not
  // calibrated) every head launch also evaluates the OTHER level's certificate on the same scores (uncert_alt); over windows of >= 64 certified pairs the
  // context counts the pairs each level flags and runs the next window on two products only when that flags at most 1 pair in 64 more than three products
  // would (a re-run in exact f32 costs ~4 block-tail passes of the pair, the two-product pass saves ~7 % of one).  Starts on three products.
  // Third level (one product, W_h X_h: cert_eps_one): the head evaluates all three eps on every automatic call (own level, uncert_alt, uncert_alt2); from two
  // products the context goes down to one only after two consecutive windows, evaluated on level 2, in each of which one product would have flagged at most
  // 1 pair in 64 more than three; on level 1 one window that fails that test goes back to 2 (or to 3 when level 2 fails its own test too).
  int auto_level = 3; float cert_eps_lvl[2] = {-1.f, -1.f}, cert_eps_one = -1.f; long long auto_pairs = 0, auto_wide = 0, auto_narrow = 0, auto_one = 0, auto_calls_lvl[2] = {0, 0}, auto_calls_one = 0, auto_switches = 0;
  int auto_ok1 = 0;        // consecutive level-2 windows that passed level 1's test
  int ffn_products = 3;    // gn_set_ffn_products: fp16 partial products of the block tail's two GEMMs on bulk grids (k_ffn128, composed form): 3 = f32-accurate split,
                           // 2 = the activations' fp16 high term only (meant to run under the margin certificate)
  int qkv_products = 2;    // knob 27: fp16 partial products of the attention input projections (2 or 3; 1 = gn_set_qkv_products(1)), per context
  // The rung below level 1 (gn_set_qkv_products): the attention input projections on ONE product as well (W_h X_h: k_qkv<., true, 1>, k_ffn128<., ., ., 3 / 4, 1>)
  // wherever the tail runs on level 1 and the bulk kernels are selected.  qkv_set: 2 = never (two products, as before), 1 = always there, 0 = automatic: part
  // of the automatic ladder (gn_set_ffn_products(0)) -- cert_eps_proj1 is the eps of that arithmetic (level 1 + one-product projections, >= cert_eps_one;
  // < 0 = not calibrated), the head evaluates it as a fourth eps on every automatic call (uncert_alt3), and after one window on level 1 in which it flags at
  // most 1 pair in 64 more than three products would the context steps onto the rung (auto_rung); one failing window there goes back to level 1, or further
  // when level 1 fails too.  gn_set_ffn_products(1) alone never selects it.  `level` stays 1 on the rung.
  int qkv_set = 0, auto_rung = 0, qkv_force = 0;      // qkv_force: +1 / -1 = the rung on / off whatever the setting (calibration and self-check passes), 0 = the setting decides
  float cert_eps_proj1 = -1.f; long long auto_proj1 = 0, auto_calls_proj1 = 0;
  unsigned long long* tile_feedback = nullptr;   // pinned host [8]: (all tiles << 32 | valid tiles) written by k_tile_lists of sub-batch group g's last call
  int n_sub = 1; hipStream_t sub_s[8] = {}; hipEvent_t ev_fork = nullptr; hipEvent_t ev_join[8] = {}; bool sub_pending[8] = {};
  // overlapped pose stage (gn_set_overlap): PnP of call n runs on an internal stream beside the matcher of call n+1
  // and the pose stage of the sub-batch groups: every group of call n hands its PnP to the ONE PnP stream and its own stream goes on with call n + 1.
  // The PnP inputs (o_mkp0 / 1 ...) are double-buffered by call parity; [slot][g] = group g's PnP of the call that used that slot (g = 0 without sub-batch groups)
  int overlap = 0; unsigned long long calls = 0;
  hipStream_t s_pnp = nullptr; hipEvent_t ev_gather[2][8] = {}, ev_pnp[2][8] = {}; bool pnp_pending[2][8] = {}, pnp_recorded[2][8] = {};
  hipEvent_t ev_head[8] = {};      // group g's match head is done: the certificate's flags of the call exist (deferred certificate)
  int prep_fused = 1;      // knob 48.  1 (default): k_prep writes the hm16 descriptor rows and the rot4 table itself and k_extent clears the guard word;
                           // 0: the separate k_split_hm16 / k_rot_table launches behind it (same bits; tests)
  // SIFT workspace (gn_sift_detect_and_compute), sized for the last image shape seen
  int sift_h = 0, sift_w = 0; std::vector<void*> sift_allocs; SiftPyramid sift_py; float* sift_tmp = nullptr;
  float* sift_dk = nullptr; std::vector<std::vector<float>> sift_kernels; std::vector<int> sift_koff;   // [0] = initial blur, [1..nOctaveLayers + 2] = layer blurs
  int sift_layers = 3; double sift_contrast = 0.04, sift_edge = 10.0, sift_sigma = 1.6;   // gn_sift_set_params (cv2.SIFT_create's defaults)
  int sift_ws_layers = 0; double sift_ws_sigma = 0.0;                                     // what the workspace above was built for
  int4* sift_cand = nullptr; int* sift_counts = nullptr; SiftKeypoint* sift_kp = nullptr;
  int sift_max_cand = 0, sift_max_kp = 0, sift_raw_cap = 0, sift_batch = 0; long long sift_kp_stride = 0;
  std::vector<int32_t> sift_totals;   // distinct keypoints found per image by the last call (before the max_kpts cap)
  // SuperPoint extractor (gn_sp_*): 12 convolutions in network order, workspace sized for the last (chunk, H, W) seen
  struct SpConv { float* wf = nullptr; float* b = nullptr; int cout = 0, cin = 0, taps = 0, cout_pad = 0; bool have_w = false, have_b = false;
                  uint16_t* wfh = nullptr; float acc_scale = 1.f; };   // wfh: fp16 pairs in fragment order (contexts of the f16x2 mode)
  SpConv sp[12];
  std::vector<void*> sp_allocs; int sp_h = 0, sp_w = 0, sp_chunk = 0, sp_cap = 0, sp_max = 0;
  float *sp_x = nullptr, *sp_y = nullptr, *sp_z = nullptr, *sp_maps[3] = {};      // full-resolution maps: scores, simple_nms output, score sink of callers without a score pointer
  int *sp_cand = nullptr, *sp_counts = nullptr, *sp_index = nullptr;
  // visual-odometry matcher workspace (gn_vo_match)
  float* vo_norm2 = nullptr; int32_t* vo_nn_idx = nullptr; float* vo_nn_dist = nullptr; uint8_t* vo_good = nullptr;
  std::vector<void*> allocs;
  std::vector<void*> ws_allocs;     // the max_kpts-dependent workspaces (alloc_workspace): replaced by gn_resize, weights stay
  // stage timing
  bool timing = false;
  hipEvent_t ev[2 * 128];
  int ev_stage[128]; int n_ev = 0; bool ev_ready = false;
  float stage_ms[ST_COUNT] = {0};
  // per-launch timing of the dominant kernel (f32 MFMA GEMM) for the roofline report
  bool ktiming = false;
  std::vector<hipEvent_t> kev;      // pairs (start, stop)
  std::vector<double> kflops;       // algorithmic flops of each recorded launch
  std::vector<double> kbytes;       // algorithmic HBM bytes of each recorded launch (operands in, results out, each once)
  std::vector<int> kclass;          // 0 = projection/FFN/similarity GEMM, 1 = attention
  std::vector<const char*> kname;   // rocprof-style kernel name of each recorded launch (gn::g_last_kernel)
  size_t kused = 0;
};

namespace {

#define GN_HIP(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      char buf_[512];                                                                             \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      if (ctx) ctx->err = buf_;                                                                   \
      g_err = buf_;                                                                               \
      return GN_ERR_HIP;                                                                          \
    }                                                                                             \
  } while (0)

int fail(gn_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}

template <typename T>
int dalloc(gn_ctx* ctx, T** p, size_t count) {
  void* q = nullptr;
  GN_HIP(hipMalloc(&q, count * sizeof(T)));
  GN_HIP(hipMemset(q, 0, count * sizeof(T)));
  ctx->allocs.push_back(q);
  *p = reinterpret_cast<T*>(q);
  return GN_OK;
}

// Every buffer whose size depends on max_kpts (the per-token / per-pair workspaces), tracked apart from the weights so that gn_resize can
// replace them without touching a weight: ctx->ws_allocs.
template <typename T_>
int ws_alloc(gn_ctx* ctx, T_** p, size_t count) {
  void* q = nullptr;
  GN_HIP(hipMalloc(&q, count * sizeof(T_)));
  GN_HIP(hipMemset(q, 0, count * sizeof(T_)));
  ctx->ws_allocs.push_back(q);
  *p = reinterpret_cast<T_*>(q);
  return GN_OK;
}

std::string canonical(const std::string& k) {
  for (const char* kind : {"self_attn.", "cross_attn."}) {
    const size_t L = strlen(kind);
    if (k.compare(0, L, kind) == 0) {
      const size_t dot = k.find('.', L);
      if (dot == std::string::npos) return k;
      return "transformers." + k.substr(L, dot - L) + "." + std::string(kind) + k.substr(dot + 1);
    }
  }
  return k;
}

struct StageTimer {
  gn_ctx* c; hipStream_t s; int st;
  StageTimer(gn_ctx* c_, hipStream_t s_, int st_) : c(c_), s(s_), st(st_) {
    if (c->timing && c->n_ev < 128) { hipEventRecord(c->ev[2 * c->n_ev], s); }
  }
  ~StageTimer() {
    if (c->timing && c->n_ev < 128) { hipEventRecord(c->ev[2 * c->n_ev + 1], s); c->ev_stage[c->n_ev] = st; ++c->n_ev; }
  }
};

// f16x2 planes mode: the hm16 buffer that shadows an f32 activation buffer.  hm16 rows have the byte pitch of the
// f32 rows, so an element offset into the f32 buffer (whole rows) maps to twice that many fp16 elements.
bool planes_of(const gn_ctx* c, const View& w, const float* p, uint16_t** planes) {
  struct { const float* f; uint16_t* q; size_t cols; } tab[] = {
    {w.desc, w.desc_p, (size_t)kInDim}, {w.x, w.x_p, (size_t)kDim}, {w.ctx, w.ctx_p, (size_t)kDim},
    {w.msg, w.msg_p, (size_t)kDim}, {w.h, w.h_p, (size_t)2 * kDim}, {w.md, w.md_p, (size_t)kDim}};
  for (auto& e : tab) {
    if (e.f && p >= e.f && p < e.f + c->Tmax * e.cols && (size_t)(p - e.f) % e.cols == 0) {
      *planes = e.q + 2 * (p - e.f);
      return true;
    }
  }
  return false;
}

// One recorded launch of the matcher schedule: stop_after bookkeeping, optional HIP events around it, and its row of the launch table (kernel
// class 0 = projection / FFN / similarity GEMM, 1 = attention; algorithmic flops and bytes; the kernel's own name unless `name` is given).
// Returns false when stop_after cut the launch.
template <typename F> bool timed_launch(gn_ctx* c, hipStream_t s, int kclass, double flops, double bytes, const char* name, F&& launch) {
  ++c->launch_count;
  if (c->stop_after && c->launch_count > c->stop_after) return false;
  const bool rec = c->ktiming && c->kused < c->kflops.size();
  if (rec) hipEventRecord(c->kev[2 * c->kused], s);
  launch();
  if (rec) {
    hipEventRecord(c->kev[2 * c->kused + 1], s);
    c->kflops[c->kused] = flops; c->kbytes[c->kused] = bytes; c->kclass[c->kused] = kclass; c->kname[c->kused] = name ? name : gn::g_last_kernel;
    ++c->kused;
  }
  return true;
}

void timed_gemm(gn_ctx* c, const View& w, int epi, const GemmArgs& g_in, int batch, hipStream_t s) {
  GemmArgs g = g_in;
  if (c->no_planes) g.Wp = nullptr;
  bool p2 = false;
  if (c->planes_mode) {
    uint16_t* q = nullptr;
    p2 = planes_of(c, w, g.A, &q);
    if (p2) {
      g.Ap = q;
      if (g.A2) { uint16_t* q2 = nullptr; p2 = planes_of(c, w, g.A2, &q2) && g.lda2 == g.lda; g.A2p = q2; }
    }
    if (p2 && !g.Wp) {   // similarity GEMM: the B operand is an activation too
      uint16_t* qw = nullptr;
      p2 = planes_of(c, w, g.W, &qw);
      g.Wp = qw; g.acc_scale = 1.f;
    }
    if (p2) g.ovf = c->guard ? w.ovf : nullptr;
    if (p2) {   // outputs that feed later GEMMs leave in hm16; f32 is kept only where something reads it
      uint16_t* qy = nullptr;
      if (g.Y == w.x) { planes_of(c, w, g.Y, &qy); g.Yp = qy; g.ldyp = g.ldy; if (g.drop_f32) g.Y = nullptr; }
      else if (g.Y == w.msg || g.Y == w.md) { planes_of(c, w, g.Y, &qy); g.Yp = qy; g.ldyp = g.ldy; g.Y = nullptr; }
      else if (epi == EPI_LN_GELU && g.Y == w.h) { planes_of(c, w, g.Y, &qy); g.Yp = qy; g.ldyp = g.ldy; g.Y = nullptr; }
    }
  }
  // compulsory bytes: A and W once (4 B per element as f32 or as an hm16 pair), every output array once, residual rows and rotary tables once
  const double mn = (double)g.M * g.N * batch;
  double by = 4.0 * ((double)g.M * g.K * batch + (double)g.N * g.K * (g.strideW ? batch : 1));
  if (epi == EPI_ROTARY_BF16 || epi == EPI_SCALE_BF16) by += 2.0 * mn;
  else if (epi == EPI_LN_GELU) by += 4.0 * mn;
  else if (epi != EPI_LN_GELU) by += (g.Y ? 4.0 * mn : 0.0) + (g.Yp ? 4.0 * mn : 0.0);
  if (epi == EPI_RESIDUAL) by += 4.0 * mn;
  if (epi == EPI_ROTARY || epi == EPI_ROTARY_BF16) by += 2.0 * 4.0 * (double)g.M * kFreq;
  timed_launch(c, s, 0, 2.0 * g.M * (double)g.N * g.K * batch, by, nullptr, [&] { if (p2) launch_gemm_p2(epi, g, batch, s, c->knobs); else launch_gemm_f32(epi, g, batch, s, c->knobs); });
}

void gemm(gn_ctx* c, const View& w, int epi, GemmArgs& g, hipStream_t s) {
  g.strideA = g.strideW = g.strideY = 0;
  timed_gemm(c, w, epi, g, 1, s);
}

// (re)build the three bf16 planes of a weight matrix (w = wh + wm + wl exactly) for the f32x3 GEMM
int build_planes(gn_ctx* ctx, Linear& L) {
  if (!L.w || L.out <= 0 || L.in <= 0) return GN_OK;
  const size_t n = (size_t)L.out * L.in;
  if (!L.wp) { int rc = dalloc(ctx, &L.wp, 3 * n); if (rc != GN_OK) return rc; }
  if (ctx->precision == GN_PREC_F16X2_BF16_ATTN) {
    // power-of-two scale that puts max |w| in [2^12, 2^13): both fp16 planes stay normal for every weight within
    // 2^-15 of the largest, and there is headroom to fp16's 65504
    std::vector<float> host(n);
    GN_HIP(hipMemcpy(host.data(), L.w, n * sizeof(float), hipMemcpyDeviceToHost));
    float mx = 0.f;
    for (float v : host) { const float av = fabsf(v); if (av > mx) mx = av; }
    int e = 0;
    if (mx > 0.f && std::isfinite(mx)) { frexpf(mx, &e); e = 13 - e; }   // mx = f * 2^(13 - e'), f in [0.5, 1)
    if (e > 60) e = 60;
    if (e < -60) e = -60;
    const float scale = ldexpf(1.0f, e);
    L.acc_scale = ldexpf(1.0f, -e);
    if (ctx->planes_mode) launch_split_hm16(L.w, L.wp, L.out, L.in, scale, 0);   // hm16 rows for k_gemm_p2
    else launch_split2_f16(L.w, L.wp, (long long)n, scale, 0);                   // [2][out][in] planes for k_gemm_f16x2
    if (ctx->planes_mode && L.frag_order >= 0 && L.out % 32 == 0 && L.in % 16 == 0) {   // fragment order for the fused block tail
      std::vector<uint16_t> frag(2 * n);
      build_weight_fragments(host.data(), L.out, L.in, scale, L.frag_order, frag.data());
      if (!L.wf) { int rc = dalloc(ctx, &L.wf, 2 * n); if (rc != GN_OK) return rc; }
      GN_HIP(hipMemcpy(L.wf, frag.data(), frag.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      if (L.frag_order == 1) {   // ffn.3: also in natural k order for the small-grid tail (gn_skinny.hip)
        build_weight_fragments(host.data(), L.out, L.in, scale, 0, frag.data());
        if (!L.wfn) { int rc = dalloc(ctx, &L.wfn, 2 * n); if (rc != GN_OK) return rc; }
        GN_HIP(hipMemcpy(L.wfn, frag.data(), frag.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      }
      if (L.out == 2 * kDim && L.in == 2 * kDim) {   // ffn.0: also the variant whose message half is fed from registers
        build_weight_fragments(host.data(), L.out, L.in, scale, 2, frag.data());
        if (!L.wf2) { int rc = dalloc(ctx, &L.wf2, 2 * n); if (rc != GN_OK) return rc; }
        GN_HIP(hipMemcpy(L.wf2, frag.data(), frag.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      }
    }
  } else {
    L.acc_scale = 1.f;
    launch_split3_bf16(L.w, L.wp, (long long)n, 0);
  }
  GN_HIP(hipStreamSynchronize(0));
  return GN_OK;
}

GemmArgs gemm_args(const float* A, int lda, const Linear& L, float* Y, int ldy, int M) {
  GemmArgs g;
  memset(&g, 0, sizeof g);
  g.Wp = L.wp; g.wp_plane = (long long)L.out * L.in; g.acc_scale = L.acc_scale;
  g.A = A; g.lda = lda; g.A2 = nullptr; g.lda2 = 0; g.K1 = L.in;
  g.W = L.w; g.ldw = L.in; g.bias = L.b; g.Y = Y; g.ldy = ldy; g.M = M; g.N = L.out; g.K = L.in;
  return g;
}

// k_attn_bf16_v5 on a grid that leaves CUs idle (one to three pairs): split the keys of every (slot, head, query block) over up to four workgroups
static void attn_split(gn_ctx* c, AttnArgs& a) {
  const int blocks = a.npad / 128 * kHeads * a.BS;
  int S = 1;
  while (S < 4 && S < c->attn_split && blocks * S * 2 <= (c->attn_split >= 8 ? 512 : 256) && a.npad / 64 >= 4 * S) S *= 2;   // (knob 23 >= 8: up to 256 partial results = the buffer; 4: at most 128)
  // (sub-batch streams would share the partial-result buffer)
  if (c->attn_part && c->attn_tickets && c->attn_split && c->n_sub <= 1 && S > 1) { a.nsplit = S; a.part = c->attn_part; a.tickets = c->attn_tickets; }
}

void attention(gn_ctx* c, const AttnArgs& a, hipStream_t s) {
  if (c->precision != GN_PREC_F32 && c->attn_f16 == 2) launch_attention_f16x2(a, s);
  else if (c->precision != GN_PREC_F32) launch_attention_bf16(a, s); else launch_attention_f32(a, s, c->knobs);
}

// one attention launch of the matcher schedule, optionally bracketed by HIP events (kernel class 1);
// flops = QK^T + PV over full npad x npad score panels (the bench fills every slot)
void timed_attention(gn_ctx* c, const AttnArgs& a, bool bf16v2, hipStream_t s) {
  timed_launch(c, s, 1, 4.0 * a.BS * kHeads * (double)a.npad * a.npad * kHeadDim,
               (double)a.BS * a.npad * kDim * (a.qb ? 2.0 + 2.0 + 2.0 : 12.0) + (double)a.BS * a.npad * kDim * 4.0,   // q, k, v in; context rows out
               nullptr, [&] { if (bf16v2) launch_attention_bf16_v2(a, s, c->knobs); else attention(c, a, s); });
}

// q | k | v (or qk | v) projection of one block straight into the attention kernel's bf16 layouts; false when the shape / mode
// needs the general GEMM
bool qkv_projection_applies(const gn_ctx* c, const View& w, const Block& blk, int T, int np, int vt_perm) {
  // (small batches keep the tiled GEMM: T / 128 workgroups would leave most of the chip idle)
  return c->planes_mode && c->qkv_fused && blk.proj_in.wf && w.x_p && w.qkb && w.vtb && w.rot4 && T % 128 == 0 && np % 128 == 0 && (vt_perm & 1) &&
         (T / 128 >= 128 || c->qkv_fused == 2);
}
// The choice depends on the number of pairs of the call only (at most two), never on the padded length: gn_set_active_kpts must not change a result
// bit (test_active_kpts_padding_does_not_change_results), and the small-grid tail rounds differently from the bulk kernels.
bool skinny_applies(const gn_ctx* c, int T, int np) {
  return (c->skinny & 3) && c->planes_mode && c->x_planes_only && T % 32 == 0 && np > 0 && ((c->skinny & 3) == 2 || T / np <= 4);
}
inline bool proj_one(const gn_ctx* c);                 // (below, with the block tail's levels)
inline bool tail_is_bulk(const gn_ctx* c, int T);
bool qkv_projection(gn_ctx* c, const View& w, const Block& blk, bool cross, int T, int np, int vt_perm, hipStream_t s) {
  // one product: beside the bulk one-product tail only, and by the bulk kernel whatever the number of pairs (the small-grid kernel keeps two products)
  const bool one = c->qkv_products != 3 && proj_one(c) && tail_is_bulk(c, T) && qkv_projection_applies(c, w, blk, T, np, vt_perm);
  const bool skinny = !one && skinny_applies(c, T, np) && !(c->skinny & 4) && c->qkv_fused && blk.proj_in.wf && w.x_p && w.qkb && w.vtb && w.rot4 && np % 32 == 0 && vt_perm == 1 && !c->qkv_stamps;
  if (!skinny && !qkv_projection_applies(c, w, blk, T, np, vt_perm)) return false;
  QkvArgs q;
  q.xp = w.x_p; q.wf = blk.proj_in.wf; q.acc_scale = blk.proj_in.acc_scale; q.bias = blk.proj_in.b;
  q.rot4 = w.rot4; q.rot_stride = (long long)c->Tmax; q.qkb = w.qkb; q.ldyb = cross ? kDim : 2 * kDim; q.vt = w.vtb; q.npad = np;
  q.qscale = 0.125f; q.scale = 0.35355339059327373f; q.vt_perm = vt_perm; q.T = T;
  q.half_fmt = c->attn_f16; q.ovf = (c->attn_f16 && c->guard) ? w.ovf : nullptr;
  q.tiles = (c->use_lists && w.lists && !c->qkv_stamps) ? w.lists : nullptr;
  q.products = c->qkv_products == 3 ? 3 : one ? 1 : 2; q.ncu = c->ncu;
  q.dbg_ts = (c->qkv_stamps && w.sim) ? reinterpret_cast<long long*>(w.sim) : nullptr;   // developer knob 20
  const double N = cross ? 2.0 * kDim : 3.0 * kDim;
  timed_launch(c, s, 0, 2.0 * T * N * kDim, 4.0 * T * kDim + 2.0 * T * N + 4.0 * N * kDim + (cross ? 0.0 : 2.0 * 4.0 * T * kFreq),   // x in (hm16), bf16 out, weights once, rotary tables
               nullptr, [&] { if (skinny) launch_skinny_qkv(q, cross, s); else launch_qkv(q, cross, s); });
  return true;
}

// [W1_x | W1_m Wo] and b1 + W1_m bo in double on the host, then the power-of-two scale and the fragment order of the other weights (natural k)
int build_composed(gn_ctx* ctx, Block& blk) {
  if (!blk.comp_dirty) return GN_OK;
  const Linear &F = blk.ffn0, &P = blk.proj_out;
  if (!ctx->planes_mode || !F.w || !F.b || !P.w || !P.b || F.out != 2 * kDim || F.in != 2 * kDim || P.out != kDim || P.in != kDim) return GN_OK;
  const int H = 2 * kDim, D = kDim;
  std::vector<float> w1((size_t)H * H), b1(H), wo((size_t)D * D), bo(D);
  GN_HIP(hipMemcpy(w1.data(), F.w, w1.size() * 4, hipMemcpyDeviceToHost));
  GN_HIP(hipMemcpy(b1.data(), F.b, b1.size() * 4, hipMemcpyDeviceToHost));
  GN_HIP(hipMemcpy(wo.data(), P.w, wo.size() * 4, hipMemcpyDeviceToHost));
  GN_HIP(hipMemcpy(bo.data(), P.b, bo.size() * 4, hipMemcpyDeviceToHost));
  std::vector<float> wc((size_t)H * H), bc(H);
  std::vector<double> row(D);
  float mx = 0.f;
  for (int h = 0; h < H; ++h) {
    const float* w1h = &w1[(size_t)h * H];
    for (int k = 0; k < D; ++k) { row[k] = 0.0; wc[(size_t)h * H + k] = w1h[k]; }
    double bb = b1[h];
    for (int f = 0; f < D; ++f) {
      const double wm = w1h[D + f];
      const float* wof = &wo[(size_t)f * D];
      for (int k = 0; k < D; ++k) row[k] += wm * wof[k];
      bb += wm * bo[f];
    }
    for (int k = 0; k < D; ++k) wc[(size_t)h * H + D + k] = (float)row[k];
    bc[h] = (float)bb;
    for (int k = 0; k < H; ++k) { const float av = fabsf(wc[(size_t)h * H + k]); if (av > mx) mx = av; }
  }
  int e = 0;
  if (mx > 0.f && std::isfinite(mx)) { frexpf(mx, &e); e = 13 - e; }
  if (e > 60) e = 60;
  if (e < -60) e = -60;
  std::vector<uint16_t> frag((size_t)2 * H * H);
  build_weight_fragments(wc.data(), H, H, ldexpf(1.0f, e), 0, frag.data());
  if (!blk.wfc) { int rc = dalloc(ctx, &blk.wfc, frag.size()); if (rc != GN_OK) return rc; }
  if (!blk.b1c) { int rc = dalloc(ctx, &blk.b1c, (size_t)H); if (rc != GN_OK) return rc; }
  GN_HIP(hipMemcpy(blk.wfc, frag.data(), frag.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  GN_HIP(hipMemcpy(blk.b1c, bc.data(), bc.size() * sizeof(float), hipMemcpyHostToDevice));
  blk.wfc_scale = ldexpf(1.0f, -e);
  blk.comp_dirty = false;
  return GN_OK;
}

int ensure_composed(gn_ctx* ctx) {
  if (!ctx->planes_mode || !ctx->ffn_compose) return GN_OK;
  for (int i = 0; i < ctx->n_layers; ++i) {
    int rc = build_composed(ctx, ctx->self_blk[i]); if (rc != GN_OK) return rc;
    rc = build_composed(ctx, ctx->cross_blk[i]); if (rc != GN_OK) return rc;
  }
  return GN_OK;
}

// true when the block-tail kernel also computes msg = out_proj(ctx): the schedule then skips the out_proj GEMM launch
bool tail_folds_out_proj(const gn_ctx* c, const Block& blk, int T) {
  return c->planes_mode && c->x_planes_only && c->ffn_fused == 3 && c->ffn_fold && blk.ffn0.wf && blk.ffn0.wf2 && blk.ffn3.wf && blk.proj_out.wf &&
         T % 64 == 0 && c->precision != GN_PREC_F32 && c->knobs.attn_variant >= 1;   // needs the attention kernel's hm16 output rows (ctx_p)
}

// The block tail's form on this call, predicted from the same sub-batch group's previous call (k_tile_lists leaves (all tiles, valid tiles) in pinned
// host memory; read without synchronisation, so the word is from some earlier call -- workloads are stationary, and both forms give the same bits).
bool tail_should_walk(const gn_ctx* c, int g) {
  if (!c->tile_feedback) return false;
  const unsigned long long word = __atomic_load_n(&c->tile_feedback[g], __ATOMIC_RELAXED);
  const unsigned all = (unsigned)(word >> 32), valid = (unsigned)word;
  return all > 0 && (unsigned long long)valid * 10u < (unsigned long long)all * 9u;
}

inline bool ffn_auto(const gn_ctx* c) { return c->ffn_products == 0 && c->cert_eps_lvl[0] >= 0.f && c->cert_eps_lvl[1] >= 0.f && c->certify >= 2; }
inline int ffn_level(const gn_ctx* c) { return c->attn_f16 == 2 ? 3 : c->ffn_products == 0 ? (ffn_auto(c) ? c->auto_level : 3) : c->ffn_products; }
inline float ffn_level_eps(const gn_ctx* c, int lvl) { return lvl == 1 ? c->cert_eps_one : c->cert_eps_lvl[lvl - 2]; }
// the rung below level 1: true when a call's attention input projections run on one product (on bulk grids, beside the one-product tail)
inline bool proj_one(const gn_ctx* c) {
  if (c->attn_f16 != 1 || c->qkv_products == 3 || ffn_level(c) != 1) return false;
  if (c->qkv_force != 0) return c->qkv_force > 0;
  return c->qkv_set == 1 || (c->qkv_set == 0 && ffn_auto(c) && c->auto_rung != 0 && c->cert_eps_proj1 >= 0.f);
}
// the arithmetic an automatic call runs on, as one number: its level, or kRung on the rung (ffn_level_update, deferred calls)
enum { kRung = 4 };
inline int ffn_auto_state(const gn_ctx* c) { return (c->auto_level == 1 && proj_one(c)) ? (int)kRung : c->auto_level; }
inline float cert_eps_now(const gn_ctx* c) { return ffn_auto(c) ? (ffn_auto_state(c) == kRung ? c->cert_eps_proj1 : ffn_level_eps(c, c->auto_level)) : c->cert_eps; }
// the bulk block tail (composed k_ffn128) is what a call of T token rows runs: the grids on which the one-product projections exist
inline bool tail_is_bulk(const gn_ctx* c, int T) {
  return c->planes_mode && c->x_planes_only && c->ffn_fused == 3 && c->ffn_fold && c->ffn_compose && ffn_bulk_shape(c->knobs.ffn_shape, T);
}
// the two levels whose certificates a call on level lvl evaluates beside its own (HeadArgs::uncert_alt, uncert_alt2): the other of {2, 3} and 1; on level 1: 2 and 3
inline int ffn_alt_level(int lvl, int k) { return lvl == 1 ? 2 + k : (k == 0 ? 5 - lvl : 1); }
inline void ffn_window_reset(gn_ctx* c, int level) { c->auto_level = level; c->auto_rung = 0; c->auto_pairs = c->auto_wide = c->auto_narrow = c->auto_one = c->auto_proj1 = 0; c->auto_ok1 = 0; }

// x += ffn3(gelu(ln(ffn0([x | msg]))))
// next / next_cross: the block whose attention input projection follows this tail (nullptr: none) -- when the tail runs as the composed k_ffn128 and that
// projection is a k_qkv<., true, 2> launch, it is computed inside the tail instead; returns true when it was (the caller then skips the projection)
bool ffn(gn_ctx* c, const View& w, const Block& blk, int T, hipStream_t s, bool keep_f32, const Block* next = nullptr, bool next_cross = false, int np = 0, int vt_perm = 0) {
  if (skinny_applies(c, T, np) && !(c->skinny & 8) && c->ffn_fused == 3 && c->ffn_compose && tail_folds_out_proj(c, blk, T) && blk.wfc && blk.b1c && !blk.comp_dirty && blk.ffn3.wfn &&
      w.h && w.ctx_p && c->knobs.ffn_stamps == 0 && c->knobs.ffn_shape == 0) {
    // small grid: the weight stream split across CUs -- two launches (gn_skinny.hip)
    SkinnyTailArgs a;
    a.xp = w.x_p; a.cp = w.ctx_p; a.w1 = blk.wfc; a.w1_scale = blk.wfc_scale; a.b1 = blk.b1c; a.h = w.h; a.ln_g = blk.ln_g; a.ln_b = blk.ln_b;
    a.w2 = blk.ffn3.wfn; a.w2_scale = blk.ffn3.acc_scale; a.b2 = blk.ffn3.b; a.xp_out = w.x_p; a.y = keep_f32 ? w.x : nullptr;
    a.ovf = c->guard ? w.ovf : nullptr; a.T = T;
    if (!timed_launch(c, s, 0, 2.0 * T * 512.0 * 512.0, 4.0 * T * (256.0 + 256.0 + 512.0) + 4.0 * 512.0 * 512.0, nullptr, [&] { launch_skinny_h(a, s, c->skinny >> 4); })) return false;
    timed_launch(c, s, 0, 2.0 * T * 256.0 * 512.0, 4.0 * T * (512.0 + 256.0 + 256.0) + 4.0 * 256.0 * 512.0, nullptr, [&] { launch_skinny_out(a, s, c->skinny >> 4); });
    return false;
  }
  if (c->planes_mode && c->x_planes_only && c->ffn_fused == 3 && blk.ffn0.wf && blk.ffn3.wf && T % 64 == 0) {   // the whole tail in one launch
    FfnArgs f;
    const bool fold = tail_folds_out_proj(c, blk, T);                     // out_proj computed inside the kernel from the attention output
    f.cp = fold ? w.ctx_p : nullptr; f.wos = blk.proj_out.wf; f.wo_scale = blk.proj_out.acc_scale; f.bo = blk.proj_out.b;
    f.xp = w.x_p; f.mp = w.msg_p; f.w1s = fold ? blk.ffn0.wf2 : blk.ffn0.wf; f.w1_scale = blk.ffn0.acc_scale; f.b1 = blk.ffn0.b; f.ln_g = blk.ln_g; f.ln_b = blk.ln_b;
    f.w2s = blk.ffn3.wf; f.w2_scale = blk.ffn3.acc_scale; f.b2 = blk.ffn3.b; f.yp = w.x_p; f.y = keep_f32 ? w.x : nullptr; f.T = T;
    const bool comp = fold && c->ffn_compose && blk.wfc && blk.b1c && !blk.comp_dirty;
    if (comp) { f.composed = 1; f.w1s = blk.wfc; f.w1_scale = blk.wfc_scale; f.b1 = blk.b1c; }
    f.ovf = c->guard ? w.ovf : nullptr;
    f.tiles = (c->use_lists && w.lists && c->knobs.ffn_stamps == 0) ? w.lists : nullptr;
    f.walk = c->use_lists == 2 || (c->use_lists == 1 && tail_should_walk(c, w.g));
    f.ncu = c->ncu;
    f.composed = comp ? 1 : 0;
    f.products = (comp && ffn_level(c) <= 2) ? ffn_level(c) : 3;
    const bool fuse_qkv = next != nullptr && c->qkv_in_tail && !c->fused_proj_off && comp && ffn_selects_128(f, c->knobs) && c->knobs.ffn_stamps == 0 && c->attn_f16 && c->qkv_products != 3 && !c->qkv_stamps &&
                          c->precision != GN_PREC_F32 && c->knobs.attn_variant >= 1 && qkv_projection_applies(c, w, *next, T, np, vt_perm) && !(vt_perm & 2);
    if (fuse_qkv) {
      f.qkv = next_cross ? 2 : 1;
      if (f.products == 1 && proj_one(c)) f.qkv += 2;      // 3 / 4: the projection on one product as well (what qkv_projection launches on this grid)
      f.q_wf = next->proj_in.wf; f.q_acc_scale = next->proj_in.acc_scale; f.q_bias = next->proj_in.b;
      f.q_rot4 = w.rot4; f.q_rot_stride = (long long)c->Tmax; f.q_qkb = w.qkb; f.q_vt = w.vtb;
      f.q_qscale = 0.125f; f.q_scale = 0.35355339059327373f;
      f.npad = np;
    }
    if (c->use_lists) { f.nvalid = w.nvalid; f.npad = c->npad_run; }
    f.dbg_ts = c->knobs.ffn_stamps ? reinterpret_cast<long long*>(w.sim) : nullptr;   // developer: phase stamps land in the (idle) sim buffer
    double flops = 2.0 * T * (512.0 * 512.0 + 256.0 * 512.0 + ((fold && !comp) ? 256.0 * 256.0 : 0.0));   // composed: the flops the kernel's own formulation needs (algorithmic: whatever the number of partial products)
    double bytes = 4.0 * T * (256.0 + 256.0 + 256.0 + 256.0) + 4.0 * (512.0 * 512.0 + 256.0 * 512.0);   // x, msg, residual rows in; x out; weights once
    if (fuse_qkv) {     // + the projection (k_qkv's figures without its read of the rows)
      const double N = next_cross ? 2.0 * kDim : 3.0 * kDim;
      flops += 2.0 * T * N * kDim;
      bytes += 2.0 * T * N + 4.0 * N * kDim + (next_cross ? 0.0 : 2.0 * 4.0 * T * kFreq);
    }
    return timed_launch(c, s, 0, flops, bytes, nullptr, [&] { launch_ffn_fused(f, s, c->knobs); }) && fuse_qkv;
  }
  GemmArgs g = gemm_args(w.x, kDim, blk.ffn0, w.h, 2 * kDim, T);
  g.A2 = w.msg; g.lda2 = kDim; g.K1 = kDim;
  // LayerNorm + GELU in the GEMM's epilogue (the hidden tensor leaves once, as hm16) when there are enough 128-row tiles to fill the chip:
  // measured 9.64 vs 9.86 ms at 512 tiles (32 pairs), 5.68 vs 5.90 at 256, but 3.95 vs 3.73 ms at 128 tiles and 3.00 vs 2.40 ms at 16 (knob 10: 2 = always)
  if (c->planes_mode && T % 128 == 0 && (c->ffn_fused == 2 || (c->ffn_fused == 1 && T / 128 >= 256))) {
    g.ln_g = blk.ln_g; g.ln_b = blk.ln_b;
    gemm(c, w, EPI_LN_GELU, g, s);
  } else {
    gemm(c, w, EPI_BIAS, g, s);
    launch_ln_gelu(w.h, blk.ln_g, blk.ln_b, T, s, c->planes_mode ? w.h_p : nullptr, c->planes_mode && c->guard ? w.ovf : nullptr);
  }
  GemmArgs g3 = gemm_args(w.h, 2 * kDim, blk.ffn3, w.x, kDim, T);
  g3.resid = w.x; g3.ldr = kDim;
  if (c->planes_mode && c->x_planes_only) {   // the residual stream between layers lives in hm16 only (f32 x is written by the last block, for the head)
    uint16_t* xp = nullptr;
    if (planes_of(c, w, w.x, &xp)) { g3.residp = xp; g3.ldrp = kDim; g3.resid = nullptr; g3.drop_f32 = keep_f32 ? 0 : 1; }
  }
  gemm(c, w, EPI_RESIDUAL, g3, s);
  return false;
}

// The match head of a call at the padded size c->npad_run, on projected descriptors (w.md, or w.md_p in the planes mode), matchabilities (w.ls) and
// counts (w.nvalid) that are already in the view: the fused two-sweep form, or (developer knob 16 = 0) the similarity GEMM + five passes.  Shared by
// run_matcher and gn_debug_match_head, so the stage-level entry launches what a call launches.
int run_head(gn_ctx* c, const View& w, int B, int64_t* idx, float* score, int32_t* n_match, bool pruning, hipStream_t s) {
  const int np = c->npad_run, T = B * 2 * np;
  HeadArgs hd;
  hd.n_in = pruning ? w.pr_nin : nullptr;
  hd.sim = w.sim; hd.ls = w.ls; hd.nvalid = w.nvalid; hd.B = B; hd.npad = np; hd.threshold = c->threshold;
  hd.rowmax = w.rowmax; hd.rowlog = w.rowlog; hd.colmax = w.colmax; hd.collog = w.collog;
  hd.m0 = w.m0; hd.max0 = w.max0; hd.m1 = w.m1;
  hd.ovf = (c->planes_mode && c->guard) ? w.ovf : nullptr;
  hd.max0b = w.max0b; hd.rpart_c = w.rpart_c; hd.uncert = c->certify ? w.uncert : nullptr;
  hd.cert_eps = (c->precision == GN_PREC_F32) ? c->cert_eps_f32 : cert_eps_now(c);
  if (hd.uncert && c->precision != GN_PREC_F32 && ffn_auto(c)) {
    hd.uncert_alt = w.uncert_alt; hd.cert_eps_alt = ffn_level_eps(c, ffn_alt_level(c->auto_level, 0));
    hd.uncert_alt2 = w.uncert_alt2; hd.cert_eps_alt2 = ffn_level_eps(c, ffn_alt_level(c->auto_level, 1));      // (< 0 -- level 1 not calibrated: flags stay 0, never read)
    // the fourth arithmetic: the rung's eps -- or, on the rung (whose own eps is cert_eps), level 1's
    hd.uncert_alt3 = w.uncert_alt3; hd.cert_eps_alt3 = ffn_auto_state(c) == kRung ? c->cert_eps_one : (c->qkv_set == 0 ? c->cert_eps_proj1 : -1.f);
  }
  hd.idx = idx; hd.score = score; hd.n_match = n_match; hd.kmax = c->npad;   // output stride: gn_kmax(), whatever the active size
  hd.md = c->planes_mode ? (const void*)w.md_p : (const void*)w.md; hd.md_f32 = c->planes_mode ? 0 : 1;
  hd.cpart_m = w.cpart_m; hd.cpart_s = w.cpart_s; hd.cpart_i = w.cpart_i; hd.rpart_a = w.rpart_a; hd.rpart_b = w.rpart_b; hd.tickets = w.tickets;
  hd.dbg_ts = (c->head_stamps && w.sim) ? reinterpret_cast<long long*>(w.sim) : nullptr;   // developer knob 17
  if (c->cal_cols) { hd.colbest = w.colbest; hd.col2 = w.col2; }
  if (c->head_fused || !w.sim) {   // both sweeps as one entry
    timed_launch(c, s, 0, 2.0 * 2.0 * B * (double)np * np * kDim,                         // the similarity tiles are computed twice
                 2.0 * (4.0 * T * kDim) + 4.0 * T * 4.0 + 8.0 * B * np * 3.0,            // descriptors once per sweep, per-row / per-column statistics, matches
                 "k_head_fused (2 sweeps)", [&] { launch_match_head_fused(hd, s); });
    if (pruning) launch_unprune_idx(idx, n_match, w.pr_ind, B, np, c->npad, s);
    return GN_OK;
  }
  GemmArgs gs;
  memset(&gs, 0, sizeof gs);
  gs.A = w.md; gs.lda = kDim; gs.K1 = kDim; gs.W = w.md + (size_t)np * kDim; gs.ldw = kDim;
  gs.Y = w.sim; gs.ldy = np; gs.M = np; gs.N = np; gs.K = kDim; gs.acc_scale = 1.f;
  gs.strideA = gs.strideW = 2LL * np * kDim; gs.strideY = (long long)np * np;
  timed_gemm(c, w, EPI_PLAIN, gs, B, s);
  launch_match_head(hd, s);
  if (pruning) launch_unprune_idx(idx, n_match, w.pr_ind, B, np, c->npad, s);
  return GN_OK;
}

int run_matcher(gn_ctx* c, const View& w, const Call& v, hipStream_t s) {
  const int B = v.B, np = c->npad_run, T = B * 2 * np, BS = B * 2;
  const bool bf16v2 = c->precision != GN_PREC_F32 && c->knobs.attn_variant >= 1 && c->attn_f16 != 2;   // (split attention: f32 projection rows, k_attn_f16x2)
  c->knobs.attn_stamps = (c->knobs.attn_variant == 73 && w.sim) ? reinterpret_cast<long long*>(w.sim) : nullptr;   // (the idle sim buffer of THIS view)
  const int vt_perm = (bf16v2 ? 1 : 0) | (c->dbg_vt_skip ? 2 : 0);   // k_attn_bf16_v5 reads V^T with keys permuted inside 16-groups   // k_attn_bf16_v4 reads permuted V^T
  const bool attn_planes = c->planes_mode && (bf16v2 || c->attn_f16 == 2);   // k_attn_bf16_v5 / k_attn_f16x2 write the hm16 rows themselves
  c->launch_count = 0;
  {
    StageTimer tm(c, s, ST_PREP);
    PrepArgs p;
    p.desc_q = v.desc_q; p.kpt_q = v.kpt_q; p.n_q = v.n_q; p.stride_q = v.stride_q;
    p.desc_r = v.desc_r; p.kpt_r = v.kpt_r; p.n_r = v.n_r; p.stride_r = v.stride_r;
    p.kpt_format = v.kpt_format; p.B = B; p.npad = np; p.wr = c->wr;
    p.desc = w.desc; p.kxy = nullptr; p.cos_t = w.cos_t; p.sin_t = w.sin_t; p.nvalid = w.nvalid; p.extent = w.extent;
    p.size_q[0] = c->size_q[0]; p.size_q[1] = c->size_q[1]; p.size_r[0] = c->size_r[0]; p.size_r[1] = c->size_r[1];
    p.feature = c->feature; p.x = nullptr; p.xp = nullptr;
    // the call's guard word starts clear -- or RAISED, developer knob 25 -- by k_extent, the call's first launch
    p.ovf_clear = (c->planes_mode && c->guard) ? w.ovf : nullptr;
    p.ovf_init = (c->dbg_trip_group && w.g == c->dbg_trip_group - 1) ? 1u : 0u;
    p.desc_p = nullptr; p.rot4 = nullptr; p.rot_stride = (long long)c->Tmax;
    const bool planes_only = c->planes_mode && c->x_planes_only && c->n_layers > 0;
    if (c->feature == 1) {   // 256-d descriptors ARE the initial residual stream (no input_proj)
      p.x = planes_only ? nullptr : w.x; p.xp = c->planes_mode ? w.x_p : nullptr;
      launch_prep(p, s);
      if (w.rot4 && c->qkv_fused) launch_rot_table(w.cos_t, w.sin_t, w.rot4, T, (long long)c->Tmax, s);
    } else {
      // k_prep also writes what k_rot_table and k_split_hm16 would make of its f32 outputs (which stay, for the modes that read them)
      const bool rot = w.rot4 && c->qkv_fused, split = c->planes_mode != 0;
      if (c->prep_fused) { p.rot4 = rot ? w.rot4 : nullptr; p.desc_p = split ? w.desc_p : nullptr; }
      launch_prep(p, s);
      if (rot && !p.rot4) launch_rot_table(w.cos_t, w.sin_t, w.rot4, T, (long long)c->Tmax, s);
      if (split && !p.desc_p) launch_split_hm16(w.desc, w.desc_p, T, kInDim, 1.0f, s);
      GemmArgs g = gemm_args(w.desc, kInDim, c->input_proj, w.x, kDim, T);
      g.drop_f32 = planes_only ? 1 : 0;
      gemm(c, w, EPI_BIAS, g, s);
    }
  }
  // the call's lists of tiles / query blocks that hold valid tokens (k_prep has written the per-slot counts)
  if (c->use_lists && w.lists) {
    launch_tile_lists(w.nvalid, BS, np, w.lists, c->tile_feedback ? c->tile_feedback + w.g : nullptr, s);
  }
  // point pruning: ind = arange, prune = ones behind k_prep's counts; then one k_prune + list rebuild behind every cross block but the last
  const bool pruning = c->width_conf > 0.f && w.pr_ind != nullptr;
  c->prune_last_on = pruning; c->prune_last_np = np; c->prune_last_layers = c->n_layers;
  if (!c->in_group) c->prune_last_B = B;      // (a sub-batch group sees its own share: estimate_call records the call's)
  if (pruning) launch_prune_init(w.pr_ind, w.pr_prune, w.pr_nin, w.nvalid, BS, np, s);
  bool qkv_done = false;      // the previous tail has already computed this block's attention input projection
  for (int i = 0; i < c->n_layers; ++i) {
    {  // SelfBlock on both sides at once
      const Block& blk = c->self_blk[i];
      if (!qkv_done) {
        StageTimer tm(c, s, ST_PROJ);
        GemmArgs g = gemm_args(w.x, kDim, blk.proj_in, w.qkv, 3 * kDim, T);
        g.cos_t = w.cos_t; g.sin_t = w.sin_t; g.rot_cols = 2 * kDim;
        if (bf16v2 && qkv_projection(c, w, blk, false, T, np, vt_perm, s)) {
        } else if (bf16v2) {
          g.Yb = w.qkb; g.ldyb = 2 * kDim; g.Vt = w.vtb; g.vt_start = 2 * kDim; g.q_cols = kDim; g.qscale = 0.125f; g.npad = np; g.vt_perm = vt_perm; g.half_fmt = c->attn_f16;
          gemm(c, w, EPI_ROTARY_BF16, g, s);
        } else {
          gemm(c, w, EPI_ROTARY, g, s);
        }
      }
      {
        StageTimer tm(c, s, ST_ATTN);
        AttnArgs a; a.ovf = nullptr;
        a.q = w.qkv; a.ldq = 3 * kDim; a.k = w.qkv + kDim; a.ldk = 3 * kDim; a.v = w.qkv + 2 * kDim; a.ldv = 3 * kDim;
        a.out = w.ctx; a.ldo = kDim; a.nvalid = w.nvalid; a.npad = np; a.cross = 0; a.qscale = 0.125f; a.BS = BS;
        a.outp = attn_planes ? w.ctx_p : nullptr; a.ovf = (attn_planes && c->guard) ? w.ovf : nullptr;
        a.qb = w.qkb; a.ldqb = 2 * kDim; a.kb = w.qkb + kDim; a.ldkb = 2 * kDim; a.vt = w.vtb; a.half_fmt = c->attn_f16; a.tiles = (c->use_lists && w.lists) ? w.lists : nullptr; a.ncu = c->ncu;
        if (bf16v2) attn_split(c, a);
        timed_attention(c, a, bf16v2, s);
        if (c->planes_mode && !attn_planes) launch_split_hm16(w.ctx, w.ctx_p, T, kDim, 1.0f, s);
      }
      if (!tail_folds_out_proj(c, blk, T)) {
        StageTimer tm(c, s, ST_PROJ);
        GemmArgs g = gemm_args(w.ctx, kDim, blk.proj_out, w.msg, kDim, T);
        gemm(c, w, EPI_BIAS, g, s);
      }
      { StageTimer tm(c, s, ST_FFN); qkv_done = ffn(c, w, blk, T, s, false, bf16v2 ? &c->cross_blk[i] : nullptr, true, np, vt_perm); }
    }
    {  // CrossBlock
      const Block& blk = c->cross_blk[i];
      if (!qkv_done) {
        StageTimer tm(c, s, ST_PROJ);
        GemmArgs g = gemm_args(w.x, kDim, blk.proj_in, w.qkv, 2 * kDim, T);
        g.scale = 0.35355339059327373f;  // (dim_head ** -0.5) ** 0.5 applied to both qk sides
        g.scale_cols = kDim;
        if (bf16v2 && qkv_projection(c, w, blk, true, T, np, vt_perm, s)) {
        } else if (bf16v2) {
          g.Yb = w.qkb; g.ldyb = kDim; g.Vt = w.vtb; g.vt_start = kDim; g.q_cols = 0; g.qscale = 1.0f; g.npad = np; g.vt_perm = vt_perm; g.half_fmt = c->attn_f16;
          gemm(c, w, EPI_SCALE_BF16, g, s);
        } else {
          gemm(c, w, EPI_SCALE_COLS, g, s);
        }
      }
      {
        StageTimer tm(c, s, ST_ATTN);
        AttnArgs a; a.ovf = nullptr;
        a.q = w.qkv; a.ldq = 2 * kDim; a.k = w.qkv; a.ldk = 2 * kDim; a.v = w.qkv + kDim; a.ldv = 2 * kDim;
        a.out = w.ctx; a.ldo = kDim; a.nvalid = w.nvalid; a.npad = np; a.cross = 1; a.qscale = 1.0f; a.BS = BS;
        a.outp = attn_planes ? w.ctx_p : nullptr; a.ovf = (attn_planes && c->guard) ? w.ovf : nullptr;
        a.qb = w.qkb; a.ldqb = kDim; a.kb = w.qkb; a.ldkb = kDim; a.vt = w.vtb; a.half_fmt = c->attn_f16; a.tiles = (c->use_lists && w.lists) ? w.lists : nullptr; a.ncu = c->ncu;
        if (bf16v2) attn_split(c, a);
        timed_attention(c, a, bf16v2, s);
        if (c->planes_mode && !attn_planes) launch_split_hm16(w.ctx, w.ctx_p, T, kDim, 1.0f, s);
      }
      if (!tail_folds_out_proj(c, blk, T)) {
        StageTimer tm(c, s, ST_PROJ);
        GemmArgs g = gemm_args(w.ctx, kDim, blk.proj_out, w.msg, kDim, T);
        gemm(c, w, EPI_BIAS, g, s);
      }
      // (pruning: the next self block's projection must see the pruned rows, so the cross tail does not fuse it)
      { StageTimer tm(c, s, ST_FFN); qkv_done = ffn(c, w, blk, T, s, i == c->n_layers - 1, (bf16v2 && i + 1 < c->n_layers && !pruning) ? &c->self_blk[i + 1] : nullptr, false, np, vt_perm); }   // the last block leaves f32 x for the match head
      if (pruning && i + 1 < c->n_layers && !(c->stop_after && c->launch_count >= c->stop_after)) {
        StageTimer tm(c, s, ST_PREP);
        const bool planes_only = c->planes_mode && c->x_planes_only;
        PruneArgs pa;
        pa.x = planes_only ? nullptr : w.x; pa.xp = c->planes_mode ? w.x_p : nullptr; pa.z_from_planes = planes_only ? 1 : 0;
        pa.cos_t = w.cos_t; pa.sin_t = w.sin_t; pa.rot4 = w.rot4; pa.rot_stride = (long long)c->Tmax;
        pa.ind = w.pr_ind; pa.prune = w.pr_prune; pa.dst = w.pr_dst; pa.nvalid = w.nvalid; pa.counts = w.pr_counts; pa.layer = i; pa.z = w.pr_z;
        pa.w = c->matchability[i].w; pa.b = c->matchability[i].b; pa.thresh = 1.0f - c->width_conf; pa.min_kpts = c->prune_min_kpts; pa.BS = BS; pa.npad = np;
        // (bytes: every row read once for z; the moved rows are counted as all of them, read and written)
        timed_launch(c, s, 0, 2.0 * T * kDim, (double)T * (pa.x ? 3.0 : 0.0) * 4.0 * kDim + (double)T * (pa.xp ? 3.0 : 0.0) * 4.0 * kDim, "k_prune", [&] { launch_prune(pa, s); });
        if (c->use_lists && w.lists) launch_tile_lists(w.nvalid, BS, np, w.lists, nullptr, s);
      }
    }
  }
  {
    StageTimer tm(c, s, ST_HEAD);
    const int li = c->n_layers - 1;
    GemmArgs g = gemm_args(w.x, kDim, c->final_proj[li], w.md, kDim, T);
    g.scale = 0.25f; g.scale_cols = kDim;  // / d ** 0.25
    gemm(c, w, EPI_SCALE_COLS, g, s);
    launch_matchability(w.x, c->matchability[li].w, c->matchability[li].b, w.ls, T, s);
    return run_head(c, w, B, v.idx, v.score, v.n_match, pruning, s);
  }
}

// The workspaces that exist `when` (a mask of kWs*), at the context's npad: max_batch x (elements per pair)
int alloc_workspaces(gn_ctx* ctx, int when) {
  int rc = GN_OK;
  for_each_workspace(ctx->ws, ctx->npad, ctx->npad, false, [&](auto*& p, long long per_pair, int exists, const char*) {
    if (rc == GN_OK && (exists & when)) rc = ws_alloc(ctx, &p, (size_t)ctx->max_batch * per_pair);
  });
  return rc;
}

// The [B][npad][npad] similarity buffer is no longer part of the matcher (fused match head): it exists only for TwistNode's
// brute-force matcher, the unfused developer path and the phase-stamp tools, and is allocated on their first use.
int ensure_sim(gn_ctx* ctx) { return ctx->ws.sim ? GN_OK : alloc_workspaces(ctx, kWsFirstUse); }

// The view of the pairs from b0 on, for sub-batch group g (the whole context: b0 = 0, g = 0).  Kernels capture pointer values at launch, so a
// group simply runs the ordinary path on its view.  (A null context gives an empty view: the entry points' argument checks refuse it.)
View view_of(const gn_ctx* c, long long b0 = 0, int g = 0) {
  View v;
  if (!c) return v;
  static_cast<Workspace&>(v) = c->ws;
  v.b0 = b0; v.g = g; v.ovf = c->ovf_base + g;
  if (b0 != 0) for_each_workspace(v, c->npad_run, c->npad, true, [&](auto*& p, long long per_pair, int, const char*) { if (p) p += b0 * per_pair; });
  return v;
}

int alloc_workspace(gn_ctx* ctx, int max_kpts) {
  ctx->npad = ((max_kpts + 127) / 128) * 128;
  ctx->npad_run = ctx->npad;
  const size_t np = ctx->npad, T = (size_t)ctx->max_batch * 2 * np, B = ctx->max_batch;
  ctx->ws = Workspace();
  ctx->Tmax = T;
  if (ctx->precision == GN_PREC_F16X2_BF16_ATTN) ctx->planes_mode = 1;
  int rc = alloc_workspaces(ctx, kWsAlways | (ctx->planes_mode ? kWsF16x2 : 0) | (ctx->precision != GN_PREC_F32 ? kWsNotF32 : 0) | (ctx->s_pnp ? kWsPnpStage : 0));
  // not per pair: the split-keys attention's partial results, TwistNode's matcher, the guard words
  if (rc == GN_OK && ctx->precision != GN_PREC_F32) rc = ws_alloc(ctx, &ctx->attn_part, (size_t)256 * 4 * 34 * 64);
  if (rc == GN_OK && ctx->precision != GN_PREC_F32) rc = ws_alloc(ctx, &ctx->attn_tickets, 256);
  if (rc == GN_OK) rc = ws_alloc(ctx, &ctx->vo_norm2, T);
  if (rc == GN_OK) rc = ws_alloc(ctx, &ctx->vo_nn_idx, B * np * 2);
  if (rc == GN_OK) rc = ws_alloc(ctx, &ctx->vo_nn_dist, B * np * 2);
  if (rc == GN_OK) rc = ws_alloc(ctx, &ctx->vo_good, B * np);
  if (rc == GN_OK) rc = ws_alloc(ctx, &ctx->ovf_base, 16);
  ctx->last_pnp_valid = false;
  ctx->prune_last_np = 0; ctx->prune_last_B = 0; ctx->prune_last_on = false;      // gn_get_prune: no matcher call yet on these workspaces
  return rc;
}

// words of two device arrays that differ (16-byte granules; one atomic per wave that saw a difference)
__global__ void k_count_diff(const uint4* a, const uint4* b, size_t n, unsigned int* cnt) {
  bool d = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 x = a[i], y = b[i];
    d |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
  }
  const unsigned long long bal = __ballot(d);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(cnt, (unsigned int)__popcll(bal));
}

// the NEXT block's attention input projection fused behind k_ffn128 (knob 32, on by default) once miscomputed in a way that moved
// with unrelated edits (DESIGN_HISTORY; the epilogue is pinned scalar arithmetic since) -- so every context PROVES the fused form against the separate
// k_qkv launches on ITS weights before it is used: the first forward call after a weight (re)load runs, on pseudo-random token rows in the context's own
// workspaces, the block tail with the projection fused (self and cross form, one-tile and walking form) and tail + k_qkv separately, and compares the
// q | k rows and V^T panels bit for bit.  Any difference switches the fusion off for this context (gn_fused_projection_status).  ~60 ms, once.
// Every block-tail level the context can select is proved: three products, two when gn_set_ffn_products is 2 or 0 (automatic), one when it is 1 or 0, and the
// one-product projection forms (k_ffn128<., ., ., 3 / 4, 1> against k_qkv<., true, 1>) when gn_set_qkv_products lets the context select them.  The check runs
// at the full padded size (the smallest bulk grid there) whatever gn_set_active_kpts has set: ffn() lays the rows out at npad_run.
int selfcheck_fused_projection(gn_ctx* c) {
  gn_ctx* ctx = c;
  const View w = view_of(c);             // the workspaces as allocated
  c->fused_proj_pending = false;
  c->fused_proj_status = -1;
  c->fused_proj_off = 0;
  const int np = c->npad;
  GN_HIP(hipDeviceSynchronize());        // (nothing of an earlier call may still be using the workspaces)
  if (!c->planes_mode || !c->qkv_in_tail || !c->attn_f16 || c->attn_f16 == 2 || c->qkv_products == 3 || !c->ffn_compose || c->ffn_fused != 3 || !c->x_planes_only || c->n_layers < 1 ||
      !c->qkv_fused || !w.rot4 || !w.lists || !w.msg_p || !w.h_p || c->feature < 0 || c->knobs.ffn_stamps != 0 || (c->knobs.ffn_shape != 0 && c->knobs.ffn_shape != 128)) return GN_OK;      // (shape 128 = k_ffn128 forced: the grid below selects it either way)
  int B = (256 * 128 + 2 * np - 1) / (2 * np);          // the smallest batch whose grid selects k_ffn128 (>= 256 tiles of 128 tokens)
  if (B > c->max_batch) return GN_OK;                   // this context never runs the bulk kernels
  const int T = B * 2 * np;
  std::vector<float> h((size_t)T * kDim);
  unsigned long long st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (float)((st >> 40) & 0xFFFF) * (1.0f / 32768.0f) - 1.0f; };   // U(-1, 1), 16 bits
  for (int pass = 0; pass < 2; ++pass) {
    for (auto& v : h) v = 1.5f * rnd();
    float* dst = pass == 0 ? w.x : w.ctx;
    GN_HIP(hipMemcpy(dst, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    launch_split_hm16(dst, pass == 0 ? w.x_p : w.ctx_p, T, kDim, 1.0f, 0);
  }
  {
    std::vector<float> cs((size_t)T * kFreq), sn((size_t)T * kFreq);
    for (size_t i = 0; i < cs.size(); ++i) { const float th = 3.14159265f * rnd(); cs[i] = cosf(th); sn[i] = sinf(th); }
    GN_HIP(hipMemcpy(w.cos_t, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    GN_HIP(hipMemcpy(w.sin_t, sn.data(), sn.size() * sizeof(float), hipMemcpyHostToDevice));
    launch_rot_table(w.cos_t, w.sin_t, w.rot4, T, (long long)c->Tmax, 0);
    std::vector<int32_t> nv(2 * (size_t)B, np);
    GN_HIP(hipMemcpy(w.nvalid, nv.data(), nv.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    launch_tile_lists(w.nvalid, 2 * B, np, w.lists, nullptr, 0);
  }
  const size_t xbytes = (size_t)T * kDim * 4, qbytes = (size_t)T * 2 * kDim * 2, vbytes = (size_t)T * kDim * 2;
  uint16_t* const keep_q = w.h_p;                                      // (k_ffn128 never writes the hidden tensor to memory: h_p is free scratch, 2 KB per token)
  uint16_t* const keep_v = w.h_p + (size_t)T * 2 * kDim;
  GN_HIP(hipMemcpy(w.msg_p, w.x_p, xbytes, hipMemcpyDeviceToDevice));  // the rows every run starts from (the tail updates x_p in place)
  unsigned int* cnt = c->ovf_base + 12;                                 // (words 9..15 of the guard block are unused)
  GN_HIP(hipMemset(cnt, 0, sizeof(unsigned int)));
  bool applicable = true;
  {
    const Restore keep(c->use_lists, c->qkv_in_tail, c->guard, c->ktiming, c->launch_count, c->stop_after, c->npad_run, c->ffn_products, c->qkv_force);
    const int prod0 = c->ffn_products;
    c->ktiming = false; c->stop_after = 0; c->guard = 0; c->npad_run = np;
    const int nblk = c->n_layers > 1 ? 1 : 0;
    int lvs[4] = {3, prod0 == 1 ? 1 : 2, 1, 1};
    const int n_lv = prod0 == 0 ? 3 : (prod0 == 2 || prod0 == 1) ? 2 : 1;     // levels: 3, then 2 and / or 1 when the context can select them
    // ... and the rung below level 1 (k_ffn128<., ., ., 3 / 4, 1> against k_qkv<., true, 1>) whenever the context can select it: pass n_lv
    const bool rung = c->attn_f16 == 1 && (c->qkv_set == 1 ? (prod0 == 0 || prod0 == 1) : (c->qkv_set == 0 && prod0 == 0));
    lvs[n_lv] = 1;
    for (int lv = 0; lv < n_lv + (rung ? 1 : 0) && applicable; ++lv)
    for (int cross = 0; cross < 2 && applicable; ++cross)
      for (int walk = 0; walk < 2 && applicable; ++walk) {
        c->ffn_products = lvs[lv]; c->qkv_force = lv == n_lv ? 1 : -1;
        const Block& tail = cross ? c->self_blk[0] : c->cross_blk[0];     // (any tail will do; the projection is the OTHER kind's)
        const Block* next = cross ? &c->cross_blk[0] : &c->self_blk[nblk];
        c->use_lists = walk ? 2 : 3;
        GN_HIP(hipMemcpyAsync(w.x_p, w.msg_p, xbytes, hipMemcpyDeviceToDevice, 0));
        GN_HIP(hipMemsetAsync(w.qkb, 0, qbytes, 0)); GN_HIP(hipMemsetAsync(w.vtb, 0, vbytes, 0));
        c->qkv_in_tail = 1;
        if (!ffn(c, w, tail, T, 0, false, next, cross != 0, np, 1)) { applicable = false; break; }
        GN_HIP(hipMemcpyAsync(keep_q, w.qkb, qbytes, hipMemcpyDeviceToDevice, 0));
        GN_HIP(hipMemcpyAsync(keep_v, w.vtb, vbytes, hipMemcpyDeviceToDevice, 0));
        GN_HIP(hipMemcpyAsync(w.x_p, w.msg_p, xbytes, hipMemcpyDeviceToDevice, 0));
        GN_HIP(hipMemsetAsync(w.qkb, 0, qbytes, 0)); GN_HIP(hipMemsetAsync(w.vtb, 0, vbytes, 0));
        c->qkv_in_tail = 0;
        ffn(c, w, tail, T, 0, false, next, cross != 0, np, 1);
        if (!qkv_projection(c, w, *next, cross != 0, T, np, 1, 0)) { applicable = false; break; }
        hipLaunchKernelGGL(k_count_diff, dim3(1024), dim3(256), 0, 0, reinterpret_cast<const uint4*>(keep_q), reinterpret_cast<const uint4*>(w.qkb), (cross ? qbytes / 2 : qbytes) / 16, cnt);
        hipLaunchKernelGGL(k_count_diff, dim3(1024), dim3(256), 0, 0, reinterpret_cast<const uint4*>(keep_v), reinterpret_cast<const uint4*>(w.vtb), vbytes / 16, cnt);
      }
  }
  unsigned int diffs = 0;
  GN_HIP(hipStreamSynchronize(0));
  GN_HIP(hipMemcpy(&diffs, cnt, sizeof diffs, hipMemcpyDeviceToHost));
  // leave the workspaces as a fresh context has them
  GN_HIP(hipMemset(w.x_p, 0, xbytes)); GN_HIP(hipMemset(w.ctx_p, 0, xbytes)); GN_HIP(hipMemset(w.msg_p, 0, xbytes)); GN_HIP(hipMemset(w.h_p, 0, qbytes + vbytes));
  GN_HIP(hipMemset(w.qkb, 0, qbytes)); GN_HIP(hipMemset(w.vtb, 0, vbytes)); GN_HIP(hipMemset(w.x, 0, xbytes)); GN_HIP(hipMemset(w.ctx, 0, xbytes));
  GN_HIP(hipMemset(cnt, 0, sizeof(unsigned int)));
  if (!applicable) return GN_OK;
  c->fused_proj_status = diffs == 0 ? 1 : 0;
  if (diffs != 0) {
    c->fused_proj_off = 1;
    fprintf(stderr, "[gisnav_amd] the projection fused behind the block tail differs from the separate k_qkv launches in %u 16-byte words on this context's weights: "
                    "fusion switched off for this context (results stay correct, ~4 %% slower)\n", diffs);
  }
  return GN_OK;
}

// gn_set_ffn_products(0): the window rule, on plain numbers.  level: the level in
// force; ok1_run: consecutive level-2 windows that passed level 1's test so far; n1 / n2 / n3: pairs of the window each level's certificate flags; have1: level
// 1 has an eps.  Between 3 and 2 the rule of round 6; down to 1 after two consecutive windows on 2 that pass level 1's test, back up after one that fails.
int ffn_level_next(int level, int* ok1_run, long long pairs, long long n1, long long n2, long long n3, bool have1) {
  const bool ok2 = (n2 - n3) * 64 <= pairs, ok1 = have1 && (n1 - n3) * 64 <= pairs;
  int next = level;
  if (level == 3) next = ok2 ? 2 : 3;
  else if (level == 2) {
    if (!ok2) next = 3;
    else { *ok1_run = ok1 ? *ok1_run + 1 : 0; next = *ok1_run >= 2 ? 1 : 2; }
  } else next = ok1 ? 1 : (ok2 ? 2 : 3);
  if (next != 2) *ok1_run = 0;
  return next;
}

// The same rule with the rung below level 1 (one-product attention input projections, gn_set_qkv_products): *rung says whether a context on level 1 stands
// on it; n0: pairs of the window the rung's certificate flags; have0: the rung has an eps.  Level 1 steps onto the rung after ONE window, evaluated on level
// 1, in which the rung would have flagged at most 1 pair in 64 more than three products; on the rung one window that fails that test goes back to level 1 --
// and further, by the rule above, when level 1 fails its own test too.  Everything else, and every answer when have0 is false, is ffn_level_next's.
int ffn_level_next_rung(int level, int* rung, int* ok1_run, long long pairs, long long n0, long long n1, long long n2, long long n3, bool have1, bool have0) {
  const bool ok0 = have0 && have1 && (n0 - n3) * 64 <= pairs;
  if (level == 1 && *rung && ok0) return 1;
  const bool was_rung = level == 1 && *rung;
  const int next = ffn_level_next(level, ok1_run, pairs, n1, n2, n3, have1);
  *rung = (level == 1 && !was_rung && next == 1 && ok0) ? 1 : 0;
  return next;
}

// one certified call's flags (those of the arithmetic it ran on, and the three others' from the same scores) into the window
void ffn_level_update(gn_ctx* c, int B, const int32_t* flags, const int32_t* alt, const int32_t* alt2, const int32_t* alt3, int lvl) {      // lvl: the level the call ran on, kRung = level 1 on the rung (a deferred call's: saved with it)
  if (!ffn_auto(c) || c->precision == GN_PREC_F32 || lvl < 1 || lvl > kRung) return;
  const int tail = lvl == kRung ? 1 : lvl;
  ++(tail == 1 ? c->auto_calls_one : c->auto_calls_lvl[tail - 2]);
  if (lvl == kRung) ++c->auto_calls_proj1;
  int n[5] = {0, 0, 0, 0, 0};
  const int la = ffn_alt_level(tail, 0), lb = ffn_alt_level(tail, 1), lc = lvl == kRung ? 1 : (int)kRung;
  for (int b = 0; b < B; ++b) { n[lvl] += flags[b] == 1; n[la] += alt[b] == 1; n[lb] += alt2[b] == 1; n[lc] += alt3 != nullptr && alt3[b] == 1; }
  c->auto_pairs += B; c->auto_one += n[1]; c->auto_wide += n[2]; c->auto_narrow += n[3]; c->auto_proj1 += n[kRung];
  if (c->auto_pairs < 64) return;
  const int rung0 = c->auto_rung;
  const int next = ffn_level_next_rung(c->auto_level, &c->auto_rung, &c->auto_ok1, c->auto_pairs, c->auto_proj1, c->auto_one, c->auto_wide, c->auto_narrow, c->cert_eps_one >= 0.f,
                                       c->qkv_set == 0 && c->cert_eps_proj1 >= 0.f && c->attn_f16 == 1 && c->qkv_products != 3);
  if (next != c->auto_level || c->auto_rung != rung0) ++c->auto_switches;
  c->auto_level = next;
  c->auto_pairs = c->auto_wide = c->auto_narrow = c->auto_one = c->auto_proj1 = 0;
}

// The arithmetics a call is run again in, each for the duration of a scope (counters and statistics are never part of one):
// ExactF32 -- the certificate's re-run: GN_PREC_F32's kernels inside a context of another precision.  They read the f32 weights (kept in every mode) and
//   the f32 workspaces (allocated in every mode); nothing of the hm16 / 16-bit state is touched.
// MidLevel -- the ladder's middle level: GN_PREC_F16X2_F16X2_ATTN's arithmetic (f32 projection rows, k_attn_f16x2, three-product block tail) on this
//   context's planes and split weights, certified against eps_mid.
// F32x3 -- gn_set_guard(2)'s fallback when an activation left the fp16 range: every operand split exactly into three bf16 terms (f32 range, f32
//   accuracy) on the f32 workspaces.  The weights stay as hm16 planes: f32x3 splits the f32 weights on the fly; the attention operands go back to
//   bf16 (f32's exponent range).
struct ExactF32 : Restore<int, int, int, int, int> {
  explicit ExactF32(gn_ctx* c) : Restore(c->precision, c->planes_mode, c->knobs.gemm_variant, c->no_planes, c->attn_f16) {
    c->precision = GN_PREC_F32; c->planes_mode = 0; c->knobs.gemm_variant = 3; c->no_planes = 1; c->attn_f16 = 0;
  }
};
struct MidLevel : Restore<int, int, int, float> {
  explicit MidLevel(gn_ctx* c) : Restore(c->attn_f16, c->ffn_products, c->dbg_trip_group, c->cert_eps) {
    c->attn_f16 = 2; c->ffn_products = 3; c->dbg_trip_group = 0; c->cert_eps = c->cert_eps_mid;
  }
};
struct F32x3 : Restore<int, int, int, int> {
  explicit F32x3(gn_ctx* c) : Restore(c->planes_mode, c->knobs.gemm_variant, c->no_planes, c->attn_f16) {
    c->planes_mode = 0; c->knobs.gemm_variant = 5; c->no_planes = 1; c->attn_f16 = 0;
  }
};
inline bool ladder_active(const gn_ctx* c) { return c->ladder && c->cert_eps_mid >= 0.f && c->precision != GN_PREC_F32 && c->planes_mode && c->attn_f16 != 2; }

// The flagged pairs `flagged` (ascending) of call v again, through `run(call)` = matcher (+ gather + PnP), in whatever arithmetic the caller has
// switched the context to; rflags[k] = the re-run's own certificate flag of flagged[k].  One contiguous run of flagged pairs is re-run IN PLACE
// (the call sliced at its first pair, on the view of the workspaces from that pair on).  Scattered flagged pairs are GATHERED into a staging block first (device-to-device
// copies of their inputs), run as ONE batch on workspace slots 0 .. nf - 1, and their outputs scattered back: a batched f32 call costs ~0.8 ms per
// pair where one- and two-pair calls cost 1.7 / 1.2 (round 6: mid-margin weights 1.26 k -> 1.9 k certified pairs/s).
template <typename F> int rerun_pairs(gn_ctx* ctx, hipStream_t s, const Call& v, F& run, const std::vector<int>& flagged, std::vector<int32_t>& rflags) {
  const int nf = (int)flagged.size();
  const bool contiguous = flagged.back() - flagged.front() + 1 == nf;
  int rc = GN_OK;
  Call st = slice(v, 0, nf);      // staged call (compact form)
  if (!contiguous) {
    // staging block: [inputs of nf pairs | outputs of nf pairs], 256-byte aligned pieces; grown on demand, owned by the context
    auto place = [&](char* base) {
      size_t off = 0;
      pair_arrays(st, [&](size_t bytes, bool, auto*& p) {
        if (!p) return;
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off = (off + nf * bytes + 255) & ~(size_t)255;
      }, st);
      return off;
    };
    const size_t need = place(nullptr);
    if (need > ctx->cert_stage_bytes) {
      if (ctx->cert_stage) { GN_HIP(hipStreamSynchronize(s)); GN_HIP(hipFree(ctx->cert_stage)); ctx->cert_stage = nullptr; ctx->cert_stage_bytes = 0; }
      GN_HIP(hipMalloc(&ctx->cert_stage, need));
      ctx->cert_stage_bytes = need;
    }
    place(static_cast<char*>(ctx->cert_stage));
  }
  // copies of one pair's inputs (gather) or outputs (scatter), in list order
  auto copy_pair = [&](const Call& dst, size_t bd, const Call& src, size_t bs, bool outputs) {
    hipError_t e = hipSuccess;
    pair_arrays(v, [&](size_t bytes, bool out, auto* d, auto* q) {
      if (d && out == outputs && e == hipSuccess)
        e = hipMemcpyAsync(const_cast<void*>(static_cast<const void*>(byte_offset(d, bd * bytes))), byte_offset(q, bs * bytes), bytes, hipMemcpyDeviceToDevice, s);
    }, dst, src);
    return e;
  };
  if (!contiguous)
    for (int k = 0; k < nf; ++k) GN_HIP(copy_pair(st, k, v, flagged[k], false));      // gather the inputs of flagged pair k into slot k
  {
    const Restore keep(ctx->cert_inner, ctx->in_group);
    ctx->cert_inner = true; ctx->in_group = true;
    // (guard word 0 either way)
    rc = contiguous ? run(view_of(ctx, flagged.front()), slice(v, flagged.front(), nf)) : run(view_of(ctx), st);
  }
  if (rc != GN_OK) return rc;
  if (!contiguous)
    for (int k = 0; k < nf; ++k) GN_HIP(copy_pair(v, flagged[k], st, k, true));       // scatter the outputs of slot k to flagged pair k
  GN_HIP(hipMemcpyAsync(ctx->uncert_host, ctx->ws.uncert, (size_t)v.B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  GN_HIP(hipStreamSynchronize(s));
  rflags.resize(nf);
  for (int k = 0; k < nf; ++k) rflags[k] = ctx->uncert_host[contiguous ? flagged[k] : k];
  return GN_OK;
}

// gn_set_certify(2 / 3): the per-pair flags of call v (read here from the device -- synchronises s -- or handed in), then the flagged pairs again in
// exact f32 (rerun_pairs).  With the ladder on (gn_set_certify_ladder, eps_mid calibrated) the pairs flagged for margin go through the middle level
// first (the same gather / run / scatter); those it certifies keep its results, the rest -- and every pair flagged for range -- go on to exact f32.
// Counts what it saw (gn_get_certify_stats, gn_get_certify_ladder_stats).
template <typename F> int certify_rerun(gn_ctx* ctx, hipStream_t s, const Call& v, F&& run, const int32_t* flags_ready = nullptr, int flags_level = 0) {
  const int B = v.B;
  if (!flags_ready) {
    GN_HIP(hipMemcpyAsync(ctx->uncert_host, ctx->ws.uncert, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (ffn_auto(ctx)) {
      GN_HIP(hipMemcpyAsync(ctx->uncert_host + ctx->max_batch, ctx->ws.uncert_alt, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      GN_HIP(hipMemcpyAsync(ctx->uncert_host + 2 * ctx->max_batch, ctx->ws.uncert_alt2, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      GN_HIP(hipMemcpyAsync(ctx->uncert_host + 3 * ctx->max_batch, ctx->ws.uncert_alt3, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    GN_HIP(hipStreamSynchronize(s));
    flags_ready = ctx->uncert_host;
  }
  ffn_level_update(ctx, B, flags_ready, flags_ready + ctx->max_batch, flags_ready + 2 * ctx->max_batch, flags_ready + 3 * ctx->max_batch,
                   flags_level ? flags_level : ffn_auto_state(ctx));     // (both callers lay the other arithmetics' flags max_batch, 2 and 3 max_batch entries behind)
  ++ctx->cert_calls; ctx->cert_pairs += B;
  std::vector<int> flagged, margin;
  for (int b = 0; b < B; ++b) {
    const int f = flags_ready[b];
    if (f == 1) ++ctx->cert_flag_margin; else if (f == 2) ++ctx->cert_flag_range;
    if (f != 0) flagged.push_back(b);
    if (f == 1) margin.push_back(b);
  }
  if (flagged.empty()) return GN_OK;
  if (ctx->precision == GN_PREC_F32) { ctx->cert_f32_marginal += (long long)flagged.size(); return GN_OK; }   // already the exact arithmetic: counted, nothing better to run
  std::vector<int32_t> rflags;
  if (ladder_active(ctx) && !margin.empty()) {
    std::vector<int> still(flagged.size() - margin.size());     // the pairs flagged for range first ...
    std::copy_if(flagged.begin(), flagged.end(), still.begin(), [&](int b) { return flags_ready[b] != 1; });
    int rc = GN_OK;
    { const MidLevel mid(ctx); rc = rerun_pairs(ctx, s, v, run, margin, rflags); }
    if (rc != GN_OK) return rc;
    ctx->mid_rerun += (long long)margin.size();
    for (size_t k = 0; k < margin.size(); ++k) {
      if (rflags[k] == 0) ++ctx->mid_certified;
      else { ++ctx->mid_passed; still.push_back(margin[k]); }   // ... then those the middle level leaves flagged (or whose middle pass left the fp16 range)
    }
    std::sort(still.begin(), still.end());
    flagged.swap(still);
    if (flagged.empty()) return GN_OK;
  }
  int rc = GN_OK;
  { const ExactF32 f32(ctx); rc = rerun_pairs(ctx, s, v, run, flagged, rflags); }
  ctx->cert_rerun += (long long)flagged.size();
  if (rc != GN_OK) return rc;
  // the re-run's own flags (stated for cert_eps_f32): how many of the pairs are marginal even in exact f32 -- counted, reported, not acted upon
  for (int32_t f : rflags) if (f != 0) ++ctx->cert_f32_marginal;
  return GN_OK;
}

// gn_calibrate_certify: one pass of the sample w (the whole sample, its first pair, or its first pair with the reference side cut) in arithmetic
// `arith` -- 1 / 2 / 3 = the context's own on that block-tail level, kCalProj1 = level 1 with one-product attention input projections (the rung),
// kCalExactF32, kCalMid = the ladder's middle level -- and the host copies of every row's
// best score and runner-up, of every column's when `cols`, of the per-slot counts when `nv`, and the guard word's trip bit (not read in exact f32)
enum { kCalExactF32 = 0, kCalMid = -1, kCalProj1 = 4 };
struct CalPass { std::vector<float> best, second, colbest, col2; unsigned int trip = 0u; };
int cal_pass(gn_ctx* ctx, const Call& w, int arith, bool cols, std::vector<int32_t>* nv, CalPass& out, hipStream_t s) {
  const View vw = view_of(ctx);
  int rc = GN_OK;
  {
    const Restore keep(ctx->in_group, ctx->cal_cols, ctx->ffn_products, ctx->qkv_force);
    // (under the automatic setting the levels 1 / 2 / 3 are measured with two-product projections and the rung separately; a fixed setting measures what it runs)
    ctx->qkv_force = arith == kCalProj1 ? 1 : (ctx->ffn_products == 0 ? -1 : 0);
    ctx->in_group = true;       // (no nested certification, ovf_groups_last untouched)
    ctx->cal_cols = cols;
    if (arith == kCalExactF32) { const ExactF32 f32(ctx); rc = run_matcher(ctx, vw, w, s); }
    else if (arith == kCalMid) { const MidLevel mid(ctx); rc = run_matcher(ctx, vw, w, s); }
    else { ctx->ffn_products = arith == kCalProj1 ? 1 : arith; rc = run_matcher(ctx, vw, w, s); }
  }
  if (rc != GN_OK) return rc;
  const size_t n = (size_t)w.B * ctx->npad_run;
  out.best.resize(n); out.second.resize(n);
  if (cols) { out.colbest.resize(n); out.col2.resize(n); }
  auto get = [&](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  const bool ok = hipStreamSynchronize(s) == hipSuccess && get(out.best.data(), vw.max0, n * 4) && get(out.second.data(), vw.max0b, n * 4) &&
                  (!nv || get(nv->data(), vw.nvalid, nv->size() * 4)) &&
                  (!cols || (get(out.colbest.data(), vw.colbest, n * 4) && get(out.col2.data(), vw.col2, n * 4))) &&
                  (arith == kCalExactF32 || !ctx->planes_mode || !ctx->guard || get(&out.trip, vw.ovf, 4));
  return ok ? GN_OK : GN_ERR_HIP;
}

// The largest difference between two passes (a: the arithmetic measured, e: exact f32) over the entries a decision looks at: the best score and
// runner-up of every valid row -- and column when `cols` -- of pairs [0, Bp) with at least two keypoints per side, restricted to the entries that come
// within 1 (in log units) of L in either arithmetic; over all of them when none does (a sample whose every decision is far away still calibrates,
// which only makes eps larger).  *entries: how many the maximum was taken over.
double max_diff(const CalPass& a, const CalPass& e, const std::vector<int32_t>& nv, int Bp, size_t np, bool cols, float L, long long* entries = nullptr) {
  double mx = 0.0, mx_all = 0.0; long long n_near = 0, n_all = 0;
  auto take = [&](float bm, float be, float sm, float se) {
    const double d1 = std::fabs((double)bm - be), d2 = std::fabs((double)sm - se);
    const double d = std::max(std::isfinite(d1) ? d1 : (double)INFINITY, std::isfinite(d2) ? d2 : 0.0);
    ++n_all; mx_all = std::max(mx_all, d);
    if (std::max(bm, be) >= L - 1.f) { ++n_near; mx = std::max(mx, d); }
  };
  for (int b = 0; b < Bp; ++b) {
    const int n0 = nv[2 * b], n1 = nv[2 * b + 1];
    if (n0 < 2 || n1 < 2) continue;
    for (int i = 0; i < n0; ++i) { const size_t o = (size_t)b * np + i; take(a.best[o], e.best[o], a.second[o], e.second[o]); }
    for (int j = 0; cols && j < n1; ++j) { const size_t o = (size_t)b * np + j; take(a.colbest[o], e.colbest[o], a.col2[o], e.col2[o]); }
  }
  if (entries) *entries = n_near ? n_near : n_all;
  return n_near ? mx : mx_all;
}

int check_fwd(gn_ctx* ctx, int B, int stride_q, int stride_r) {
  if (!ctx) return fail(nullptr, GN_ERR_ARG, "null context");
  if (ctx->npad <= 0) return fail(ctx, GN_ERR_ARG, "context has no workspaces (a gn_resize failed): call gn_resize again");
  if (B < 1 || B > ctx->max_batch) return fail(ctx, GN_ERR_ARG, "B out of range for this context");
  if (stride_q < 1 || stride_r < 1 || stride_q > ctx->npad || stride_r > ctx->npad)
    return fail(ctx, GN_ERR_ARG, "keypoint stride exceeds max_kpts of this context");
  if (gn_missing_tensors(ctx) != 0) return fail(ctx, GN_ERR_WEIGHTS, "weights not fully loaded");
  GN_HIP(hipSetDevice(ctx->device));          // (before anything below touches the GPU: the caller's current device need not be the context's)
  const int rc_c = ensure_composed(ctx);      // (host work on the first call after a (re)load only)
  if (rc_c != GN_OK) return rc_c;
  if (ctx->fused_proj_pending && !ctx->in_group && !ctx->cert_inner) return selfcheck_fused_projection(ctx);
  return GN_OK;
}

}  // namespace

extern "C" {

// gn_version / gn_source_digest: gn_build_id.hip (carries the digest of the sources this binary was built from)

const char* gn_last_error(const gn_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int gn_create(int device, int max_batch, int max_kpts, int precision, gn_ctx** out) {
  return gn_create_ex(device, max_batch, max_kpts, precision, GN_FEATURE_SIFT, out);
}

int gn_set_image_size(gn_ctx* ctx, float w_q, float h_q, float w_r, float h_r) {
  if (!ctx) return GN_ERR_ARG;
  ctx->size_q[0] = w_q; ctx->size_q[1] = h_q; ctx->size_r[0] = w_r; ctx->size_r[1] = h_r;
  return GN_OK;
}

int gn_set_distortion(gn_ctx* ctx, const double* d_host, int n) {
  if (!ctx) return GN_ERR_ARG;
  if (!d_host || n == 0) { ctx->dist_on = 0; return GN_OK; }
  if (n == 8 || n == 12 || n == 14)
    return fail(ctx, GN_ERR_ARG, "gn_set_distortion: the rational, thin-prism and tilted models (8, 12, 14 coefficients) are not built; plumb-bob (4 or 5) only");
  if (n != 4 && n != 5) return fail(ctx, GN_ERR_ARG, "gn_set_distortion: n must be 0, 4 or 5 (k1, k2, p1, p2[, k3])");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(d_host[i])) return fail(ctx, GN_ERR_ARG, "gn_set_distortion: non-finite coefficient");
    any = any || d_host[i] != 0.0;
  }
  for (int i = 0; i < 5; ++i) ctx->dist[i] = i < n ? d_host[i] : 0.0;
  ctx->dist_on = any ? 1 : 0;      // all zeros = off: the pinhole kernels run, bit for bit
  return GN_OK;
}

int gn_get_distortion(const gn_ctx* ctx, double* d5_host) {
  if (!ctx) return GN_ERR_ARG;
  if (d5_host) for (int i = 0; i < 5; ++i) d5_host[i] = ctx->dist_on ? ctx->dist[i] : 0.0;
  return ctx->dist_on;
}

int gn_set_pair_cameras(gn_ctx* ctx, const double* cams, int n, int model) {
  if (!ctx) return GN_ERR_ARG;
  if (n < 0 || n > ctx->max_batch) return fail(ctx, GN_ERR_ARG, "gn_set_pair_cameras: n must be in 0..max_batch of this context");
  if (model != 0 && model != 1) return fail(ctx, GN_ERR_ARG, "gn_set_pair_cameras: model must be 0 (pinhole) or 1 (plumb-bob)");
  if (!cams || n == 0) { ctx->pair_cams = nullptr; ctx->pair_cams_n = 0; ctx->pair_cams_model = 0; return GN_OK; }
  ctx->pair_cams = cams; ctx->pair_cams_n = n; ctx->pair_cams_model = model;
  return GN_OK;
}

int gn_get_pair_cameras(const gn_ctx* ctx, const double** cams, int* n, int* model) {
  if (!ctx) return GN_ERR_ARG;
  if (cams) *cams = ctx->pair_cams;
  if (n) *n = ctx->pair_cams_n;
  if (model) *model = ctx->pair_cams_model;
  return ctx->pair_cams ? 1 : 0;
}

int gn_set_ransac(gn_ctx* ctx, int iterations_count, float reproj_error_px, double confidence) {
  if (!ctx) return GN_ERR_ARG;
  if (iterations_count < 1 || iterations_count > GN_RANSAC_MAX_ITERATIONS)
    return fail(ctx, GN_ERR_ARG, "gn_set_ransac: iterations_count must be in 1..4096 (GN_RANSAC_MAX_ITERATIONS)");
  if (!(reproj_error_px > 0.0f) || !std::isfinite(reproj_error_px)) return fail(ctx, GN_ERR_ARG, "gn_set_ransac: reproj_error_px must be positive and finite");
  if (!(confidence > 0.0 && confidence < 1.0)) return fail(ctx, GN_ERR_ARG, "gn_set_ransac: confidence must lie strictly between 0 and 1");
  ctx->ransac_iters = iterations_count; ctx->ransac_reproj = reproj_error_px; ctx->ransac_conf = confidence;
  return GN_OK;
}

int gn_get_ransac(const gn_ctx* ctx, int* iterations_count, float* reproj_error_px, double* confidence) {
  if (!ctx) return GN_ERR_ARG;
  if (iterations_count) *iterations_count = ctx->ransac_iters;
  if (reproj_error_px) *reproj_error_px = ctx->ransac_reproj;
  if (confidence) *confidence = ctx->ransac_conf;
  return GN_OK;
}

int gn_undistort_points(gn_ctx* ctx, int B, const float* img, const int32_t* n_pts, int kstride, const double* K9, int to_pixels,
                        float* out, void* stream) {
  if (!ctx || !img || !n_pts || (!K9 && !ctx->pair_cams) || !out || B < 1 || kstride < 1) return fail(ctx, GN_ERR_ARG, "bad gn_undistort_points argument");
  if (ctx->pair_cams && B > ctx->pair_cams_n) return fail(ctx, GN_ERR_ARG, "gn_undistort_points: B exceeds the rows of the table (gn_set_pair_cameras)");
  GN_HIP(hipSetDevice(ctx->device));
  UndistortArgs a;
  a.img = img; a.n_pts = n_pts; a.kstride = kstride; a.B = B;
  if (ctx->pair_cams) {      // row b for pair b; K9 and the gn_set_distortion state are not read
    a.fx = a.fy = a.cx = a.cy = 0.0;
    a.cams = ctx->pair_cams; a.dist = ctx->pair_cams_model;
    for (int i = 0; i < 5; ++i) a.dk[i] = 0.0;
  } else {
    a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5];
    a.dist = ctx->dist_on;
    for (int i = 0; i < 5; ++i) a.dk[i] = ctx->dist[i];
  }
  a.to_pixels = to_pixels ? 1 : 0; a.out = out;
  launch_undistort(a, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_create_ex(int device, int max_batch, int max_kpts, int precision, int feature, gn_ctx** out) {
  gn_ctx* ctx = nullptr;
  if (!out || max_batch < 1 || max_kpts < 2) return fail(nullptr, GN_ERR_ARG, "bad gn_create argument");
  if (precision != GN_PREC_F32 && precision != GN_PREC_BF16_ATTN && precision != GN_PREC_F32X3_BF16_ATTN &&
      precision != GN_PREC_F16X2_BF16_ATTN && precision != GN_PREC_F16X2_F16_ATTN && precision != GN_PREC_F16X2_F16X2_ATTN)
    return fail(nullptr, GN_ERR_ARG, "bad precision");
  if (precision == GN_PREC_F16X2_F16X2_ATTN && feature != GN_FEATURE_SIFT)
    return fail(nullptr, GN_ERR_ARG, "GN_PREC_F16X2_F16X2_ATTN: SIFT-LightGlue contexts only (the SuperPoint extractor has no split-attention schedule)");
  const int precision_api = precision;
  if (precision == GN_PREC_F16X2_F16_ATTN || precision == GN_PREC_F16X2_F16X2_ATTN) precision = GN_PREC_F16X2_BF16_ATTN;   // the same projections / FFN / head; only the attention operand format differs (ctx->attn_f16)
  GN_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  GN_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, GN_ERR_ARCH, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  ctx = new gn_ctx();
  if (feature != GN_FEATURE_SIFT && feature != GN_FEATURE_SUPERPOINT) { delete ctx; return fail(nullptr, GN_ERR_ARG, "bad feature type"); }
  ctx->device = device; ctx->max_batch = max_batch; ctx->precision = precision; ctx->feature = feature;
  ctx->precision_api = precision_api; ctx->attn_f16 = precision_api == GN_PREC_F16X2_F16_ATTN ? 1 : precision_api == GN_PREC_F16X2_F16X2_ATTN ? 2 : 0;
  ctx->knobs.gemm_variant = precision == GN_PREC_F16X2_BF16_ATTN ? 6 : precision == GN_PREC_F32X3_BF16_ATTN ? 5 : 3;
  { const int rc_ws = alloc_workspace(ctx, max_kpts); if (rc_ws != GN_OK) { gn_destroy(ctx); return rc_ws; } }
  // pinned host words: [0, 16) guard words, [16, 16 + 4096) the per-image counters the SIFT / SuperPoint calls read back (up to 1024 images per call)
  if (hipHostMalloc((void**)&ctx->ovf_host, (16 + 4096 + 16) * sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) { gn_destroy(ctx); return fail(nullptr, GN_ERR_HIP, "hipHostMalloc failed"); }
  memset(ctx->ovf_host, 0, (16 + 4096 + 16) * sizeof(unsigned int));
  ctx->tile_feedback = reinterpret_cast<unsigned long long*>(ctx->ovf_host + 16 + 4096);   // [8] x 8 bytes behind the counters (8-byte aligned)
  if (hipHostMalloc((void**)&ctx->uncert_host, (size_t)4 * max_batch * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { gn_destroy(ctx); return fail(nullptr, GN_ERR_HIP, "hipHostMalloc failed"); }
  memset(ctx->uncert_host, 0, (size_t)4 * max_batch * sizeof(int32_t));
  for (auto& pd : ctx->cert_pend) {
    if (hipHostMalloc((void**)&pd.flags, (size_t)4 * max_batch * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&pd.ev, hipEventDisableTiming) != hipSuccess) { gn_destroy(ctx); return fail(nullptr, GN_ERR_HIP, "certificate slots: allocation failed"); }
  }
  ctx->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  for (int i = 0; i < 256; ++i) hipEventCreate(&ctx->ev[i]);
  ctx->ev_ready = true;
  // required tensor names
  auto req = [&](const std::string& n) { ctx->required.push_back(n + ".weight"); ctx->required.push_back(n + ".bias"); };
  if (feature == GN_FEATURE_SIFT) req("input_proj");
  ctx->required.push_back("posenc.Wr.weight");
  for (int i = 0; i < kMaxLayers; ++i) {
    const std::string ps = "transformers." + std::to_string(i) + ".self_attn.", pc = "transformers." + std::to_string(i) + ".cross_attn.";
    req(ps + "Wqkv"); req(ps + "out_proj"); req(ps + "ffn.0"); req(ps + "ffn.1"); req(ps + "ffn.3");
    req(pc + "to_qk"); req(pc + "to_v"); req(pc + "to_out"); req(pc + "ffn.0"); req(pc + "ffn.1"); req(pc + "ffn.3");
    req("log_assignment." + std::to_string(i) + ".final_proj");
    req("log_assignment." + std::to_string(i) + ".matchability");
  }
  *out = ctx;
  return GN_OK;
}

int gn_resize(gn_ctx* ctx, int max_kpts) {
  if (!ctx || max_kpts < 2) return fail(ctx, GN_ERR_ARG, "bad gn_resize argument");
  if (((max_kpts + 127) / 128) * 128 == ctx->npad) return GN_OK;
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipDeviceSynchronize());                      // nothing may still be reading the old workspaces
  for (void* p : ctx->ws_allocs) hipFree(p);
  ctx->ws_allocs.clear();
  for (bool& b : ctx->sub_pending) b = false;
  // A failure part-way (out of memory while growing) must not leave the context pointing at freed workspaces: every entry point goes
  // through check_fwd, which refuses a context whose npad is 0 until a later gn_resize succeeds.
  auto broken = [&](int rc) { for (void* p : ctx->ws_allocs) hipFree(p); ctx->ws_allocs.clear(); ctx->npad = 0; ctx->npad_run = 0; return rc; };
  // (sim: allocated on first use again, for the new size; the overlapped pose stage's double buffers follow the padded size too)
  { const int rc = alloc_workspace(ctx, max_kpts); if (rc != GN_OK) return broken(rc); }
  if (ctx->s_pnp) for (auto& slot : ctx->pnp_pending) for (bool& b : slot) b = false;
  return GN_OK;
}

void gn_destroy(gn_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  for (void* p : ctx->allocs) hipFree(p);
  for (void* p : ctx->ws_allocs) hipFree(p);
  if (ctx->ovf_host) hipHostFree(ctx->ovf_host);
  if (ctx->uncert_host) hipHostFree(ctx->uncert_host);
  if (ctx->cert_stage) hipFree(ctx->cert_stage);
  for (auto& pd : ctx->cert_pend) { if (pd.flags) hipHostFree(pd.flags); if (pd.ev) hipEventDestroy(pd.ev); }
  if (ctx->ev_ready) for (int i = 0; i < 256; ++i) hipEventDestroy(ctx->ev[i]);
  for (hipEvent_t e : ctx->kev) hipEventDestroy(e);
  for (void* p : ctx->sift_allocs) hipFree(p);
  for (void* p : ctx->sp_allocs) hipFree(p);
  if (ctx->sp_allocs_dbg) hipFree(ctx->sp_allocs_dbg);
  if (ctx->ev_fork) {
    for (int i = 0; i < 8; ++i) if (ctx->sub_s[i]) { hipStreamSynchronize(ctx->sub_s[i]); hipEventDestroy(ctx->ev_join[i]); hipStreamDestroy(ctx->sub_s[i]); }
    hipEventDestroy(ctx->ev_fork);
  }
  if (ctx->s_pnp) { hipStreamSynchronize(ctx->s_pnp); hipStreamDestroy(ctx->s_pnp); }
  for (int g = 0; g < 8; ++g)
    for (hipEvent_t e : {ctx->ev_gather[0][g], ctx->ev_gather[1][g], ctx->ev_pnp[0][g], ctx->ev_pnp[1][g], ctx->ev_head[g]}) if (e) hipEventDestroy(e);
  delete ctx;
}

int gn_missing_tensors(const gn_ctx* ctx) {
  if (!ctx) return -1;
  int missing = 0;
  for (const auto& n : ctx->required) {
    // log_assignment.{i} for i other than the last configured layer is optional
    if (n.compare(0, 15, "log_assignment.") == 0) {
      const int i = atoi(n.c_str() + 15);
      if (i != ctx->n_layers - 1) continue;
    }
    if (n.compare(0, 13, "transformers.") == 0) {
      const int i = atoi(n.c_str() + 13);
      if (i >= ctx->n_layers) continue;
    }
    if (!ctx->loaded.count(n)) ++missing;
  }
  return missing;
}

int gn_set_num_layers(gn_ctx* ctx, int n_layers) {
  if (!ctx || n_layers < 1 || n_layers > kMaxLayers) return fail(ctx, GN_ERR_ARG, "n_layers must be in 1..9");
  ctx->n_layers = n_layers;
  return GN_OK;
}

int gn_set_filter_threshold(gn_ctx* ctx, float th) {
  if (!ctx) return GN_ERR_ARG;
  ctx->threshold = th;
  return GN_OK;
}

int gn_set_width_pruning(gn_ctx* ctx, float width_confidence, int min_kpts) {
  if (!ctx) return GN_ERR_ARG;
  if (!std::isfinite(width_confidence) || width_confidence >= 1.f)
    return fail(ctx, GN_ERR_ARG, "gn_set_width_pruning: width_confidence must be finite and < 1 (<= 0 turns pruning off)");
  if (width_confidence > 0.f && ctx->certify > 0)
    return fail(ctx, GN_ERR_ARG, "gn_set_width_pruning: point pruning cannot run under the margin certificate (gn_set_certify mode > 0): the certificate's eps bounds "
                                 "|P - P_f32| on the same token set, and a fast mode may prune a different set -- gn_set_certify(ctx, 0, ...) first");
  ctx->width_conf = width_confidence > 0.f ? width_confidence : -1.f;
  ctx->prune_min_kpts = min_kpts < 0 ? 1536 : min_kpts;
  return GN_OK;
}

int gn_get_width_pruning(const gn_ctx* ctx, float* width_confidence, int* min_kpts) {
  if (!ctx) return GN_ERR_ARG;
  if (width_confidence) *width_confidence = ctx->width_conf;
  if (min_kpts) *min_kpts = ctx->prune_min_kpts;
  return GN_OK;
}

int gn_get_prune(gn_ctx* ctx, int B, int32_t* prune_q, int32_t* prune_r) {
  if (!ctx || !prune_q || !prune_r) return fail(ctx, GN_ERR_ARG, "gn_get_prune: null pointer");
  if (ctx->prune_last_np <= 0 || ctx->prune_last_np > ctx->npad || ctx->prune_last_B < 1 || !ctx->ws.nvalid) return fail(ctx, GN_ERR_ARG, "gn_get_prune: no matcher call yet on these workspaces");
  if (B < 1 || B > ctx->prune_last_B) return fail(ctx, GN_ERR_ARG, "gn_get_prune: B exceeds the pairs of the most recent matcher call");
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipDeviceSynchronize());
  const size_t np = (size_t)ctx->prune_last_np, km = (size_t)ctx->npad;
  int32_t* out[2] = {prune_q, prune_r};
  memset(prune_q, 0, (size_t)B * km * sizeof(int32_t)); memset(prune_r, 0, (size_t)B * km * sizeof(int32_t));
  if (ctx->prune_last_on) {
    std::vector<int32_t> host((size_t)B * 2 * np);
    GN_HIP(hipMemcpy(host.data(), ctx->ws.pr_prune, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int bs = 0; bs < 2 * B; ++bs) memcpy(out[bs & 1] + (size_t)(bs >> 1) * km, host.data() + (size_t)bs * np, np * sizeof(int32_t));
  } else {      // kornia without pruning: every keypoint took part in every layer
    std::vector<int32_t> nv((size_t)B * 2);
    GN_HIP(hipMemcpy(nv.data(), ctx->ws.nvalid, nv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int bs = 0; bs < 2 * B; ++bs)
      for (int i = 0; i < std::min(std::max(nv[bs], 0), (int)np); ++i) out[bs & 1][(size_t)(bs >> 1) * km + i] = ctx->prune_last_layers;
  }
  return GN_OK;
}

int gn_kmax(const gn_ctx* ctx) { return ctx ? ctx->npad : GN_ERR_ARG; }

int gn_load_tensor(gn_ctx* ctx, const char* name_c, const float* host, const int64_t* shape, int ndim) {
  if (!ctx || !name_c || !host || !shape || ndim < 1 || ndim > 2) return fail(ctx, GN_ERR_ARG, "bad gn_load_tensor argument");
  GN_HIP(hipSetDevice(ctx->device));
  const std::string name = canonical(name_c);
  if (name.compare(0, 17, "token_confidence.") == 0 || name == "confidence_thresholds") return GN_OK;  // dead in the live config
  const int64_t d0 = shape[0], d1 = ndim == 2 ? shape[1] : 1;
  auto upload = [&](float** dst, const float* src, size_t count) -> int {
    if (*dst == nullptr) { int rc = dalloc(ctx, dst, count); if (rc != GN_OK) return rc; }
    GN_HIP(hipMemcpy(*dst, src, count * sizeof(float), hipMemcpyHostToDevice));
    return GN_OK;
  };
  auto shape_err = [&]() { return fail(ctx, GN_ERR_SHAPE, "shape mismatch for " + name); };
  const bool is_w = name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0;
  const bool is_b = name.size() > 5 && name.compare(name.size() - 5, 5, ".bias") == 0;
  if (!is_w && !is_b) return fail(ctx, GN_ERR_NAME, "unknown tensor " + name);
  const std::string base = name.substr(0, name.size() - (is_w ? 7 : 5));

  auto load_linear = [&](Linear& L, int out, int in, int row_off, int rows_total) -> int {
    // loads rows [row_off, row_off + out) of a (rows_total x in) fused matrix
    if (is_w) {
      if (ndim != 2 || d0 != out || d1 != in) return shape_err();
      if (!L.w) { int rc = dalloc(ctx, &L.w, (size_t)rows_total * in); if (rc != GN_OK) return rc; }
      GN_HIP(hipMemcpy(L.w + (size_t)row_off * in, host, (size_t)out * in * sizeof(float), hipMemcpyHostToDevice));
      L.out = rows_total; L.in = in;
      { int rcp = build_planes(ctx, L); if (rcp != GN_OK) return rcp; }
    } else {
      if (d0 != out || d1 != 1) return shape_err();
      if (!L.b) { int rc = dalloc(ctx, &L.b, (size_t)rows_total); if (rc != GN_OK) return rc; }
      GN_HIP(hipMemcpy(L.b + row_off, host, (size_t)out * sizeof(float), hipMemcpyHostToDevice));
    }
    L.out = rows_total; L.in = in;
    return GN_OK;
  };

  int rc = GN_ERR_NAME;
  if (base == "input_proj") {
    if (ctx->feature != GN_FEATURE_SIFT) return fail(ctx, GN_ERR_NAME, "input_proj does not exist for 256-d features (input_dim == descriptor_dim)");
    rc = load_linear(ctx->input_proj, kDim, kInDim, 0, kDim);
  } else if (base == "posenc.Wr") {
    const int pin = ctx->feature == GN_FEATURE_SIFT ? 4 : 2;   // (x, y, scale, ori) or (x, y)
    if (!is_w || ndim != 2 || d0 != kFreq || d1 != pin) return shape_err();
    rc = upload(&ctx->wr, host, kFreq * pin);
  } else if (base.compare(0, 13, "transformers.") == 0) {
    const int i = atoi(base.c_str() + 13);
    if (i < 0 || i >= kMaxLayers) return fail(ctx, GN_ERR_NAME, "layer index out of range in " + name);
    const size_t p1 = base.find('.', 13);
    const std::string rest = base.substr(p1 + 1);  // e.g. self_attn.Wqkv
    const bool self = rest.compare(0, 10, "self_attn.") == 0;
    const bool cross = rest.compare(0, 11, "cross_attn.") == 0;
    if (!self && !cross) return fail(ctx, GN_ERR_NAME, "unknown tensor " + name);
    const std::string leaf = rest.substr(self ? 10 : 11);
    Block& blk = self ? ctx->self_blk[i] : ctx->cross_blk[i];
    if (self && leaf == "Wqkv") {
      // kornia splits the 768 outputs as unflatten(-1, (heads, 64, 3)): flat = h*192 + d*3 + s.
      // Re-order rows to [s][h][d] so q, k, v are contiguous 256-wide panels (numerically identical:
      // every output feature keeps its own weight row and bias).
      if (is_w) { if (ndim != 2 || d0 != 3 * kDim || d1 != kDim) return shape_err(); }
      else if (d0 != 3 * kDim || d1 != 1) return shape_err();
      const int in = is_w ? kDim : 1;
      std::vector<float> tmp((size_t)3 * kDim * in);
      for (int hh = 0; hh < kHeads; ++hh)
        for (int d = 0; d < kHeadDim; ++d)
          for (int s3 = 0; s3 < 3; ++s3) {
            const int src = hh * 192 + d * 3 + s3, dst = s3 * kDim + hh * kHeadDim + d;
            memcpy(&tmp[(size_t)dst * in], host + (size_t)src * in, in * sizeof(float));
          }
      Linear& L = blk.proj_in;
      L.frag_order = 0;
      if (is_w) { rc = upload(&L.w, tmp.data(), tmp.size()); } else { rc = upload(&L.b, tmp.data(), tmp.size()); }
      L.out = 3 * kDim; L.in = kDim;
      if (is_w && rc == GN_OK) rc = build_planes(ctx, L);
    } else if (self && leaf == "out_proj") { blk.comp_dirty = true; blk.proj_out.frag_order = 0; rc = load_linear(blk.proj_out, kDim, kDim, 0, kDim); }
    else if (cross && leaf == "to_qk") { blk.proj_in.frag_order = 0; rc = load_linear(blk.proj_in, kDim, kDim, 0, 2 * kDim); }
    else if (cross && leaf == "to_v") { blk.proj_in.frag_order = 0; rc = load_linear(blk.proj_in, kDim, kDim, kDim, 2 * kDim); }
    else if (cross && leaf == "to_out") { blk.comp_dirty = true; blk.proj_out.frag_order = 0; rc = load_linear(blk.proj_out, kDim, kDim, 0, kDim); }
    else if (leaf == "ffn.0") { blk.comp_dirty = true; blk.ffn0.frag_order = 0; rc = load_linear(blk.ffn0, 2 * kDim, 2 * kDim, 0, 2 * kDim); }
    else if (leaf == "ffn.3") { blk.ffn3.frag_order = 1; rc = load_linear(blk.ffn3, kDim, 2 * kDim, 0, kDim); }
    else if (leaf == "ffn.1") {
      if (d0 != 2 * kDim || d1 != 1) return shape_err();
      rc = upload(is_w ? &blk.ln_g : &blk.ln_b, host, 2 * kDim);
    } else return fail(ctx, GN_ERR_NAME, "unknown tensor " + name);
  } else if (base.compare(0, 15, "log_assignment.") == 0) {
    const int i = atoi(base.c_str() + 15);
    if (i < 0 || i >= kMaxLayers) return fail(ctx, GN_ERR_NAME, "layer index out of range in " + name);
    const std::string leaf = base.substr(base.find('.', 15) + 1);
    if (leaf == "final_proj") rc = load_linear(ctx->final_proj[i], kDim, kDim, 0, kDim);
    else if (leaf == "matchability") {
      if (is_w) { if (ndim != 2 || d0 != 1 || d1 != kDim) return shape_err(); rc = upload(&ctx->matchability[i].w, host, kDim); }
      else { if (d0 != 1) return shape_err(); rc = upload(&ctx->matchability[i].b, host, 1); }
    } else return fail(ctx, GN_ERR_NAME, "unknown tensor " + name);
  } else {
    return fail(ctx, GN_ERR_NAME, "unknown tensor " + name);
  }
  if (rc == GN_OK) {
    ctx->loaded[name] = true; ctx->fused_proj_pending = true;
    // a calibration belongs to the weights it was measured on: the automatic block-tail level goes back to "not calibrated" (three products, cert_eps)
    ctx->cert_eps_lvl[0] = ctx->cert_eps_lvl[1] = ctx->cert_eps_one = ctx->cert_eps_proj1 = -1.f; ffn_window_reset(ctx, 3);
    ctx->cert_eps_mid = -1.f;   // (the ladder sends flagged pairs straight to exact f32 until the next calibration)
    // and so does the single eps when it was measured (a stated one is the caller's to keep): every pair is flagged -- exact f32 -- until
    // gn_calibrate_certify runs again or gn_set_certify states an eps
    if (ctx->cert_eps_src >= 2) { ctx->cert_eps = INFINITY; ctx->cert_eps_src = 3; }
  }
  return rc;
}

namespace {
// gn_match on the view vw: the whole context, or a sub-batch group's / a re-run's share of it
int match_impl(gn_ctx* ctx, const View& vw, int B, int kpt_format,
               const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
               const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
               int64_t* idx, float* score, int32_t* n_match, void* stream) {
  int rc = check_fwd(ctx, B, stride_q, stride_r);
  if (rc != GN_OK) return rc;
  const int kfmt = kpt_format & 0xff;
  if (kfmt != GN_KPT_LAF && kfmt != GN_KPT_XYSA && kfmt != GN_KPT_RECORD) return fail(ctx, GN_ERR_ARG, "bad kpt_format");
  if (kfmt == GN_KPT_RECORD && ctx->feature != GN_FEATURE_SIFT) return fail(ctx, GN_ERR_ARG, "GN_KPT_RECORD (KEYPOINT_DTYPE wire records) needs a SIFT context");
  if (((!desc_q || !desc_r) && kfmt != GN_KPT_RECORD) || !kpt_q || !n_q || !kpt_r || !n_r || !idx || !score || !n_match)
    return fail(ctx, GN_ERR_ARG, "null pointer passed to gn_match");
  hipStream_t s = (hipStream_t)stream;
  ctx->n_ev = 0;
  if (!ctx->in_group) ctx->ovf_groups_last = 1;
  Call v(ctx->feature, ctx->npad, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r);
  v.idx = idx; v.score = score; v.n_match = n_match;
  rc = run_matcher(ctx, vw, v, s);
  if (rc != GN_OK) return rc;
  if (ctx->certify >= 2 && !ctx->in_group && !ctx->cert_inner) {
    // certified mode (3 = deferred exists for gn_estimate's sub-batch-stream path only; everywhere else it is 2): read this call's per-pair flags (one stream synchronisation -- the reference's call site synchronises right after the
    // matcher anyway, pose_node.py:296-297) and run the flagged pairs again on the exact-f32 kernels; covers the fp16-range fallback too
    rc = certify_rerun(ctx, s, v, [&](const View& rw, const Call& w) { return run_matcher(ctx, rw, w, s); });
    if (rc != GN_OK) return rc;
  } else if (ctx->planes_mode && ctx->guard == 2 && ctx->certify < 2) {
    // guarded mode: observe the domain word of THIS call (one stream synchronisation -- the reference's call site synchronises
    // right after the matcher anyway, pose_node.py:296-297) and, if an activation left the fp16 range, run the call again in f32x3
    GN_HIP(hipMemcpyAsync(ctx->ovf_host, vw.ovf, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (*ctx->ovf_host != 0u) {
      ++ctx->guard_trips;
      const F32x3 f32x3(ctx);
      rc = run_matcher(ctx, vw, v, s);
      if (rc != GN_OK) return rc;
    }
  }
  GN_HIP(hipGetLastError());
  return GN_OK;
}
}  // namespace

int gn_match(gn_ctx* ctx, int B, int kpt_format,
             const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
             const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
             int64_t* idx, float* score, int32_t* n_match, void* stream) {
  return match_impl(ctx, view_of(ctx), B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, idx, score, n_match, stream);
}

int gn_set_guard(gn_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return GN_ERR_ARG;
  if (mode != ctx->guard && ctx->ovf_base) {   // a mode change starts from clean words: a trip raised under the old mode must not be seen by the new one
    GN_HIP(hipSetDevice(ctx->device));
    GN_HIP(hipDeviceSynchronize());
    GN_HIP(hipMemset(ctx->ovf_base, 0, 8 * sizeof(unsigned int)));
  }
  ctx->guard = mode;
  return GN_OK;
}

int gn_get_guard_status(gn_ctx* ctx, void* stream, int32_t* last_call_tripped, int64_t* trips_total) {
  if (!ctx) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  // (with deferred joins the caller flushes first: the words of unjoined groups are still being written)
  GN_HIP(hipMemcpyAsync(ctx->ovf_host, ctx->ovf_base, 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GN_HIP(hipStreamSynchronize((hipStream_t)stream));
  unsigned int any = 0u;
  for (int g = 0; g < ctx->ovf_groups_last && g < 8; ++g) any |= ctx->ovf_host[g];
  const int tripped = (ctx->planes_mode && ctx->guard && any != 0u) ? 1 : 0;
  if (tripped && ctx->guard == 1) ++ctx->guard_trips;
  if (last_call_tripped) *last_call_tripped = tripped;
  if (trips_total) *trips_total = ctx->guard_trips;
  return GN_OK;
}

int gn_device_numa_node(int device) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) return -1;
  for (char* c = bus; *c; ++c) *c = (char)tolower((unsigned char)*c);
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}

int gn_fused_projection_status(const gn_ctx* ctx) { return ctx ? ctx->fused_proj_status : GN_ERR_ARG; }

int gn_set_ffn_products(gn_ctx* ctx, int products) {
  if (!ctx || products < 0 || products > 3) return GN_ERR_ARG;
  if (products != ctx->ffn_products) {
    ffn_window_reset(ctx, 3);
    ctx->fused_proj_pending = true;        // the fused projection is proved on every level the new setting can select
  }
  ctx->ffn_products = products;
  return GN_OK;
}

int gn_set_ffn_level_eps(gn_ctx* ctx, float eps2, float eps3, int level) {
  if (!ctx || !(eps2 >= 0.f) || !(eps3 >= 0.f) || level < 1 || level > 3) return GN_ERR_ARG;
  ctx->cert_eps_lvl[0] = std::max(eps2, eps3); ctx->cert_eps_lvl[1] = eps3;
  if (ctx->cert_eps_one >= 0.f) ctx->cert_eps_one = std::max(ctx->cert_eps_one, ctx->cert_eps_lvl[0]);
  ffn_window_reset(ctx, (level == 1 && !(ctx->cert_eps_one >= 0.f)) ? 2 : level);      // (level 1 without an eps of its own -- gn_set_ffn_level_eps1 -- starts on two products)
  return GN_OK;
}

int gn_set_ffn_level_eps1(gn_ctx* ctx, float eps1) {
  if (!ctx || !(eps1 >= 0.f)) return GN_ERR_ARG;
  ctx->cert_eps_one = std::max(eps1, std::max(ctx->cert_eps_lvl[0], ctx->cert_eps_lvl[1]));      // eps_one >= eps_two >= eps_three, as gn_calibrate_certify stores them
  if (ctx->cert_eps_proj1 >= 0.f) ctx->cert_eps_proj1 = std::max(ctx->cert_eps_proj1, ctx->cert_eps_one);
  return GN_OK;
}

int gn_set_qkv_products(gn_ctx* ctx, int products) {
  if (!ctx || products < 0 || products > 2) return GN_ERR_ARG;
  if (products != ctx->qkv_set) {
    ffn_window_reset(ctx, 3);
    ctx->fused_proj_pending = true;        // the one-product projection forms are proved whenever the new setting can select them
  }
  ctx->qkv_set = products;
  return GN_OK;
}

int gn_set_qkv_level_eps(gn_ctx* ctx, float eps_proj1) {
  if (!ctx || !(eps_proj1 >= 0.f)) return GN_ERR_ARG;
  ctx->cert_eps_proj1 = std::max(eps_proj1, std::max(ctx->cert_eps_one, std::max(ctx->cert_eps_lvl[0], ctx->cert_eps_lvl[1])));
  return GN_OK;
}

int gn_get_qkv_level(gn_ctx* ctx, int32_t* setting, int32_t* on_rung, float* eps_proj1, int64_t* calls_proj1) {
  if (!ctx) return GN_ERR_ARG;
  if (setting) *setting = ctx->qkv_set;
  if (on_rung) *on_rung = proj_one(ctx) ? 1 : 0;
  if (eps_proj1) *eps_proj1 = ctx->cert_eps_proj1;
  if (calls_proj1) *calls_proj1 = ctx->auto_calls_proj1;
  return GN_OK;
}

int gn_get_ffn_level1(gn_ctx* ctx, float* eps1, int64_t* calls1) {
  if (!ctx) return GN_ERR_ARG;
  if (eps1) *eps1 = ctx->cert_eps_one;
  if (calls1) *calls1 = ctx->auto_calls_one;
  return GN_OK;
}

int gn_debug_ffn_level_sim(int n_calls, int B, const int32_t* f1, const int32_t* f2, const int32_t* f3, int have1, int32_t* levels_out, int64_t* out4) {
  if (n_calls < 0 || B < 1 || !f1 || !f2 || !f3) return GN_ERR_ARG;
  // a context that owns nothing on the device: only the automatic level's state is touched (ffn_level_update reads no other field)
  std::unique_ptr<gn_ctx> c(new gn_ctx);
  c->ffn_products = 0; c->certify = 2; c->precision = GN_PREC_F16X2_BF16_ATTN;
  c->cert_eps_lvl[0] = 2.f; c->cert_eps_lvl[1] = 1.f; c->cert_eps_one = have1 ? 3.f : -1.f;
  const int32_t* f[4] = {nullptr, f1, f2, f3};
  for (int i = 0; i < n_calls; ++i) {
    const int lvl = c->auto_level;
    if (levels_out) levels_out[i] = lvl;
    const size_t o = (size_t)i * B;
    ffn_level_update(c.get(), B, f[lvl] + o, f[ffn_alt_level(lvl, 0)] + o, f[ffn_alt_level(lvl, 1)] + o, nullptr, lvl);      // (no rung eps: the rule of the three levels)
  }
  if (out4) { out4[0] = c->auto_level; out4[1] = c->auto_switches; out4[2] = c->auto_calls_lvl[0]; out4[3] = c->auto_calls_one; }
  return GN_OK;
}

int gn_debug_ffn_level_sim_rung(int n_calls, int B, const int32_t* f0, const int32_t* f1, const int32_t* f2, const int32_t* f3, int have1, int have0, int32_t* levels_out, int32_t* rung_out, int64_t* out5) {
  if (n_calls < 0 || B < 1 || !f0 || !f1 || !f2 || !f3) return GN_ERR_ARG;
  std::unique_ptr<gn_ctx> c(new gn_ctx);
  c->ffn_products = 0; c->certify = 2; c->precision = GN_PREC_F16X2_BF16_ATTN; c->attn_f16 = 1;
  c->cert_eps_lvl[0] = 2.f; c->cert_eps_lvl[1] = 1.f; c->cert_eps_one = have1 ? 3.f : -1.f; c->cert_eps_proj1 = have0 ? 4.f : -1.f;
  const int32_t* f[5] = {nullptr, f1, f2, f3, f0};
  for (int i = 0; i < n_calls; ++i) {
    const int st = ffn_auto_state(c.get()), tail = st == kRung ? 1 : st;
    if (levels_out) levels_out[i] = tail;
    if (rung_out) rung_out[i] = st == kRung ? 1 : 0;
    const size_t o = (size_t)i * B;
    ffn_level_update(c.get(), B, f[st] + o, f[ffn_alt_level(tail, 0)] + o, f[ffn_alt_level(tail, 1)] + o, f[st == kRung ? 1 : (int)kRung] + o, st);
  }
  if (out5) { out5[0] = c->auto_level; out5[1] = c->auto_switches; out5[2] = c->auto_calls_lvl[0]; out5[3] = c->auto_calls_one; out5[4] = ffn_auto_state(c.get()) == kRung ? 1 : 0; }
  return GN_OK;
}

int gn_get_ffn_level(gn_ctx* ctx, int32_t* level, float* eps2, float* eps3, int64_t* out4) {
  if (!ctx) return GN_ERR_ARG;
  if (level) *level = ffn_level(ctx);
  if (eps2) *eps2 = ctx->cert_eps_lvl[0];
  if (eps3) *eps3 = ctx->cert_eps_lvl[1];
  if (out4) { out4[0] = ctx->auto_calls_lvl[0]; out4[1] = ctx->auto_calls_lvl[1]; out4[2] = ctx->auto_switches; out4[3] = ffn_auto(ctx) ? 1 : 0; }
  return GN_OK;
}

int gn_set_certify(gn_ctx* ctx, int mode, float eps, float eps_f32) {
  if (!ctx || mode < 0 || mode > 3) return GN_ERR_ARG;
  if (ctx->certify == 3 && mode != 3 && (ctx->cert_pend[0].active || ctx->cert_pend[1].active))
    return fail(ctx, GN_ERR_ARG, "gn_set_certify: deferred certificates are still open -- gn_flush first");
  if (mode > 0 && ctx->width_conf > 0.f)
    return fail(ctx, GN_ERR_ARG, "gn_set_certify: the margin certificate cannot run with point pruning on (gn_set_width_pruning): its eps bounds |P - P_f32| on the same "
                                 "token set, and a fast mode may prune a different set -- gn_set_width_pruning(ctx, -1, -1) first");
  ctx->certify = mode;
  if (eps >= 0.f) { ctx->cert_eps = eps; ctx->cert_eps_src = 1; }
  if (eps_f32 >= 0.f) ctx->cert_eps_f32 = eps_f32;
  return GN_OK;
}

int gn_calibrate_certify(gn_ctx* ctx, int B, int kpt_format,
                         const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                         const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                         float safety, float floor_eps, float* measured_host, float* eps_host, void* stream) {
  int rc = check_fwd(ctx, B, stride_q, stride_r);
  if (rc != GN_OK) return rc;
  if (!(safety >= 1.f) || !(floor_eps >= 0.f)) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: safety must be >= 1, floor_eps >= 0");
  if (ctx->precision == GN_PREC_F32) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: this context already computes in exact f32");
  if (ctx->width_conf > 0.f)
    return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: point pruning is on (gn_set_width_pruning): the measured eps would compare scores of different token sets -- "
                                 "gn_set_width_pruning(ctx, -1, -1) first");
  if (ctx->n_sub > 1 || ctx->overlap) { const int rcf = gn_flush(ctx, stream); if (rcf != GN_OK) return rcf; }
  hipStream_t s = (hipStream_t)stream;
  const size_t np = (size_t)ctx->npad_run;
  int32_t* nm = nullptr;
  GN_HIP(hipMalloc((void**)&nm, (size_t)B * sizeof(int32_t)));
  Call v(ctx->feature, ctx->npad, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r);
  v.idx = ctx->ws.e_idx; v.score = ctx->ws.e_score; v.n_match = nm;
  // passes: the context's arithmetic -- on ALL THREE block-tail levels under gn_set_ffn_products(0), and on the rung below level 1 (one-product attention
  // input projections) unless gn_set_qkv_products(2) rules it out -- then the exact-f32 kernels
  const int setting = ctx->ffn_products;
  const bool rung = setting == 0 && ctx->qkv_set == 0 && ctx->attn_f16 == 1 && ctx->qkv_products != 3;
  const int n_lv = setting == 0 ? (rung ? 4 : 3) : 1;
  const int lv[4] = {setting == 0 ? 1 : setting, 2, 3, kCalProj1};
  const float L = ctx->threshold > 0.f ? logf(ctx->threshold) : -INFINITY;
  CalPass whole[5];
  std::vector<int32_t> nv(2 * (size_t)B);
  unsigned int tripped = 0u;
  const bool lad = ctx->ladder && ctx->planes_mode && ctx->attn_f16 != 2;   // (gn_set_certify_ladder refuses every other context)
  for (int pass = 0; pass <= n_lv && rc == GN_OK; ++pass) {      // (the exact pass keeps the column best / runner-up for the ladder)
    rc = cal_pass(ctx, v, pass == n_lv ? kCalExactF32 : lv[pass], pass == n_lv && lad, &nv, whole[pass], s);
    tripped |= whole[pass].trip;
  }
  // the ladder's middle level: mode-5 arithmetic on the whole sample and on its first pair alone (the ladder mostly runs small grids, whose kernels
  // differ), against the exact pass above, over every valid row's AND column's best score and runner-up
  double mid_mx = -1.0;
  for (int mp = 0; lad && mp < 2 && rc == GN_OK && !tripped; ++mp) {
    CalPass mid;
    rc = cal_pass(ctx, slice(v, 0, mp == 0 ? B : 1), kCalMid, true, nullptr, mid, s);
    if (rc != GN_OK) break;
    tripped |= mid.trip;
    mid_mx = std::max(mid_mx, max_diff(mid, whole[n_lv], nv, mp == 0 ? B : 1, np, true, L));
  }
  // the sample's first pair alone, and with its reference side cut to 128 and to 2 keypoints: the one-pair grid of bucket remainders, and the
  // few-keypoint sides of a ragged stream, where the fp16 attention's rounding averages over few keys (measured against fp64 on a ragged bulk
  // batch: 1.7x the eps of a 16 x 1024 sample alone, tests/test_gpu_fp64_parity.py).  Each level's eps is taken over these passes too.
  double var_mx[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t* nr1 = nullptr;
  if (rc == GN_OK && !tripped && nv[0] >= 2 && nv[1] >= 2 && hipMalloc((void**)&nr1, sizeof(int32_t)) != hipSuccess) rc = GN_ERR_HIP;
  Call v1 = slice(v, 0, 1);
  v1.n_r = nr1;
  for (int var = 0; nr1 && rc == GN_OK && var < 3; ++var) {
    const int32_t nr_cut = var == 0 ? nv[1] : std::min(nv[1], var == 1 ? 128 : 2);
    if (hipMemcpy(nr1, &nr_cut, sizeof nr_cut, hipMemcpyHostToDevice) != hipSuccess) { rc = GN_ERR_HIP; break; }
    CalPass p[5];
    unsigned int trip = 0u;
    for (int pass = 0; pass <= n_lv && rc == GN_OK; ++pass) {
      rc = cal_pass(ctx, v1, pass == n_lv ? kCalExactF32 : lv[pass], false, nullptr, p[pass], s);
      trip |= p[pass].trip;
    }
    if (rc != GN_OK || trip) continue;          // (a pass that left the fp16 range is re-run as a whole by the certificate: nothing to measure)
    for (int k = 0; k < n_lv; ++k) var_mx[k] = std::max(var_mx[k], max_diff(p[k], p[n_lv], nv, 1, np, false, L));
  }
  if (nr1) hipFree(nr1);
  // the whole sample once more with every descriptor cut to its three largest bins: the error of the 16-bit arithmetic follows the statistics of the
  // descriptors, not only the weights -- a sample of dense descriptors understated it for sparse ones (few strong bins: a larger input to every block;
  // measured against fp64, d / eps 1.15 on three-bin descriptors, tests/test_gpu_ood_inputs.py).  Every level's eps, and eps_mid, is taken over this
  // pass too.  (RootSIFT descriptors given as such -- GN_DESC_ROOTSIFT -- and 256-d features are used as they come: nothing normalises a cut row.)
  double cut_mx[4] = {0.0, 0.0, 0.0, 0.0}, cut_mid = -1.0;
  if (rc == GN_OK && !tripped && ctx->feature == GN_FEATURE_SIFT && !(kpt_format & GN_DESC_ROOTSIFT)) {
    const bool rec = (kpt_format & 0xff) == GN_KPT_RECORD;       // (the descriptor is the tail of the keypoint's own record)
    const int row_floats = rec ? gn::kRecordFloats : kInDim, off = rec ? 5 : 0;
    const float* src[2] = {rec ? kpt_q : desc_q, rec ? kpt_r : desc_r};
    const size_t rows[2] = {(size_t)B * stride_q, (size_t)B * stride_r};
    float* cut[2] = {nullptr, nullptr};
    for (int k = 0; k < 2 && rc == GN_OK; ++k) {
      const size_t bytes = rows[k] * row_floats * sizeof(float);
      if (hipMalloc((void**)&cut[k], bytes) != hipSuccess || hipMemcpyAsync(cut[k], src[k], bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) { rc = GN_ERR_HIP; break; }
      gn::launch_desc_top3(cut[k], (long long)rows[k], row_floats, off, s);
    }
    Call vc = v;
    (rec ? vc.kpt_q : vc.desc_q) = cut[0]; (rec ? vc.kpt_r : vc.desc_r) = cut[1];
    CalPass p[5];
    unsigned int trip = 0u;
    for (int pass = 0; pass <= n_lv && rc == GN_OK; ++pass) {
      rc = cal_pass(ctx, vc, pass == n_lv ? kCalExactF32 : lv[pass], pass == n_lv && lad, nullptr, p[pass], s);
      trip |= p[pass].trip;
    }
    for (int k = 0; k < n_lv && rc == GN_OK && !trip; ++k) cut_mx[k] = max_diff(p[k], p[n_lv], nv, B, np, false, L);
    if (lad && rc == GN_OK && !trip) {
      CalPass mid;
      rc = cal_pass(ctx, vc, kCalMid, true, nullptr, mid, s);
      if (rc == GN_OK && !mid.trip) cut_mid = max_diff(mid, p[n_lv], nv, B, np, true, L);
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == GN_OK) rc = GN_ERR_HIP;
    for (int k = 0; k < 2; ++k) if (cut[k]) hipFree(cut[k]);
  }
  hipFree(nm);
  if (rc != GN_OK) return rc == GN_ERR_HIP ? fail(ctx, rc, "gn_calibrate_certify: a HIP call failed") : rc;
  if (tripped) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: the sample left the fp16 range of this precision mode (nothing to calibrate: such calls are re-run as a whole)");
  // largest difference between the two arithmetics over every valid row's best score and runner-up (max_diff)
  float eps_of[4] = {0.f, 0.f, 0.f, 0.f}, mx_of[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < n_lv; ++k) {
    long long rows = 0;
    double mx = max_diff(whole[k], whole[n_lv], nv, B, np, false, L, &rows);
    if (!std::isfinite(mx)) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: non-finite scores in the sample");
    if (rows == 0) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: the sample holds no pair with at least two keypoints per side (nothing to measure)");
    if (!std::isfinite(var_mx[k])) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: non-finite scores in the one-pair passes");
    if (!std::isfinite(cut_mx[k])) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: non-finite scores in the cut-descriptor passes");
    mx = std::max(mx, std::max(var_mx[k], cut_mx[k]));
    mx_of[k] = (float)mx; eps_of[k] = std::max(floor_eps, safety * (float)mx);
  }
  if (setting == 0) {
    // the wider level's bound is never stated tighter than the narrower one's (a sample can happen to show the opposite)
    ctx->cert_eps_lvl[1] = eps_of[2]; ctx->cert_eps_lvl[0] = std::max(eps_of[1], eps_of[2]); ctx->cert_eps_one = std::max(eps_of[0], ctx->cert_eps_lvl[0]);
    ctx->cert_eps_proj1 = rung ? std::max(eps_of[3], ctx->cert_eps_one) : -1.f;      // eps_proj1 >= eps_one >= eps_two >= eps_three
    ffn_window_reset(ctx, 3);
  }
  if (lad && mid_mx >= 0.0) {
    mid_mx = std::max(mid_mx, cut_mid);
    if (!std::isfinite(mid_mx)) return fail(ctx, GN_ERR_ARG, "gn_calibrate_certify: non-finite scores in the middle level's pass");
    ctx->cert_eps_mid = std::max(floor_eps, safety * (float)mid_mx);
    ctx->cert_mid_measured = (float)mid_mx;
  }
  const int rep = setting == 0 ? 2 : 0;       // reported: the three-product level's values under the automatic setting (gn_get_ffn_level returns both eps)
  ctx->cert_eps = eps_of[rep]; ctx->cert_eps_src = 2;
  if (measured_host) *measured_host = mx_of[rep];
  if (eps_host) *eps_host = eps_of[rep];
  return GN_OK;
}

int gn_get_certify_stats(gn_ctx* ctx, int64_t* out8) {
  if (!ctx || !out8) return GN_ERR_ARG;
  out8[0] = ctx->cert_calls; out8[1] = ctx->cert_pairs; out8[2] = ctx->cert_flag_margin; out8[3] = ctx->cert_flag_range;
  out8[4] = ctx->cert_rerun; out8[5] = ctx->cert_f32_marginal; out8[6] = ctx->certify; out8[7] = ctx->cert_eps_src;
  return GN_OK;
}

int gn_set_certify_ladder(gn_ctx* ctx, int enable, float eps_mid) {
  if (!ctx) return GN_ERR_ARG;
  if (enable && (!ctx->planes_mode || ctx->attn_f16 == 2 || ctx->feature != GN_FEATURE_SIFT))
    return fail(ctx, GN_ERR_ARG, "gn_set_certify_ladder: the ladder needs a SIFT context of GN_PREC_F16X2_BF16_ATTN or GN_PREC_F16X2_F16_ATTN "
                                 "(its middle level is GN_PREC_F16X2_F16X2_ATTN's arithmetic on the same planes; exact f32 has nothing to ladder)");
  ctx->ladder = enable ? 1 : 0;
  if (eps_mid >= 0.f) ctx->cert_eps_mid = eps_mid;
  return GN_OK;
}

int gn_get_certify_ladder_stats(gn_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return GN_ERR_ARG;
  uint32_t bits = 0;
  memcpy(&bits, &ctx->cert_eps_mid, sizeof bits);
  out4[0] = ctx->mid_rerun; out4[1] = ctx->mid_certified; out4[2] = ctx->mid_passed; out4[3] = ctx->cert_eps_mid >= 0.f ? (int64_t)bits : -1;
  return GN_OK;
}

int gn_reset_certify_stats(gn_ctx* ctx) {
  if (!ctx) return GN_ERR_ARG;
  ctx->cert_calls = ctx->cert_pairs = ctx->cert_flag_margin = ctx->cert_flag_range = ctx->cert_rerun = ctx->cert_f32_marginal = 0;
  ctx->mid_rerun = ctx->mid_certified = ctx->mid_passed = 0;
  ctx->auto_calls_lvl[0] = ctx->auto_calls_lvl[1] = ctx->auto_calls_one = ctx->auto_calls_proj1 = ctx->auto_switches = 0;
  return GN_OK;
}

int gn_get_uncertain(gn_ctx* ctx, int B, int32_t* host_flags, void* stream) {
  if (!ctx || !host_flags || B < 1 || B > ctx->max_batch) return GN_ERR_ARG;
  if (!ctx->certify) return fail(ctx, GN_ERR_ARG, "gn_get_uncertain: the certificate is off (gn_set_certify)");
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipMemcpyAsync(ctx->uncert_host, ctx->ws.uncert, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GN_HIP(hipStreamSynchronize((hipStream_t)stream));
  memcpy(host_flags, ctx->uncert_host, (size_t)B * sizeof(int32_t));
  return GN_OK;
}

namespace {
// The gather stage under the DEM format `f` (the context's for gn_gather_points, the call's for gn_estimate*).  The default format, and a call
// without a DEM, launch k_gather as always; otherwise gn_dem.hip's typed lift, and with a void value its one-workgroup-per-pair compaction,
// which rewrites idx / score / n_match in place and counts into `dropped`.
int gather_impl(gn_ctx* ctx, const DemFormat& f, int32_t* dropped, int B, int kpt_format, const float* kpt_q, int stride_q, const float* kpt_r, int stride_r,
                int64_t* idx, float* score, int32_t* n_match, const uint8_t* dem, int H, int W, float* mkp_q, float* obj, void* stream) {
  if (!ctx || !kpt_q || !kpt_r || !idx || !n_match || !mkp_q || !obj || B < 1 || B > ctx->max_batch)
    return fail(ctx, GN_ERR_ARG, "bad gn_gather_points argument");
  if (dem && (H < 1 || W < 1)) return fail(ctx, GN_ERR_ARG, "bad DEM shape");
  GN_HIP(hipSetDevice(ctx->device));
  DemGatherArgs d;
  GatherArgs& g = d.g;
  g.kpt_q = kpt_q; g.stride_q = stride_q; g.kpt_r = kpt_r; g.stride_r = stride_r; g.kpt_format = kpt_format & 0xff;
  g.idx = idx; g.n_match = n_match; g.kmax = ctx->npad; g.B = B; g.dem = dem; g.H = H; g.W = W; g.mkp_q = mkp_q; g.obj = obj;
  StageTimer tm(ctx, (hipStream_t)stream, ST_GATHER);
  if (!dem || dem_format_is_default(f)) launch_gather(g, (hipStream_t)stream);
  else {
    d.f = f; d.idx = idx; d.score = score; d.n_match = n_match; d.dropped = dropped;
    launch_gather_dem(d, (hipStream_t)stream);
  }
  GN_HIP(hipGetLastError());
  return GN_OK;
}
}  // namespace

int gn_gather_points_scored(gn_ctx* ctx, int B, int kpt_format, const float* kpt_q, int stride_q, const float* kpt_r, int stride_r,
                            int64_t* idx, float* score, int32_t* n_match, const uint8_t* dem, int H, int W,
                            float* mkp_q, float* obj, void* stream) {
  return gather_impl(ctx, ctx ? ctx->demf : DemFormat(), ctx ? ctx->ws.dem_dropped : nullptr, B, kpt_format, kpt_q, stride_q, kpt_r, stride_r,
                     idx, score, n_match, dem, H, W, mkp_q, obj, stream);
}

int gn_gather_points(gn_ctx* ctx, int B, int kpt_format, const float* kpt_q, int stride_q, const float* kpt_r, int stride_r,
                     const int64_t* idx, const int32_t* n_match, const uint8_t* dem, int H, int W,
                     float* mkp_q, float* obj, void* stream) {
  // (the match list is written only while the context's DEM format states a void value: include/gisnav_amd.h)
  return gn_gather_points_scored(ctx, B, kpt_format, kpt_q, stride_q, kpt_r, stride_r, const_cast<int64_t*>(idx), nullptr, const_cast<int32_t*>(n_match),
                                 dem, H, W, mkp_q, obj, stream);
}

int gn_set_dem_format(gn_ctx* ctx, int type, double scale, double offset, int has_nodata, double nodata) {
  if (!ctx) return fail(nullptr, GN_ERR_ARG, "gn_set_dem_format: null context");
  if (type != GN_DEM_U8 && type != GN_DEM_U16 && type != GN_DEM_I16 && type != GN_DEM_F32)
    return fail(ctx, GN_ERR_ARG, "gn_set_dem_format: type must be GN_DEM_U8, GN_DEM_U16, GN_DEM_I16 or GN_DEM_F32");
  if (!std::isfinite(scale) || scale == 0.0) return fail(ctx, GN_ERR_ARG, "gn_set_dem_format: scale must be finite and not zero");
  if (!std::isfinite(offset)) return fail(ctx, GN_ERR_ARG, "gn_set_dem_format: offset must be finite");
  if (has_nodata && type != GN_DEM_F32) {
    const double lo = type == GN_DEM_I16 ? -32768.0 : 0.0, hi = type == GN_DEM_U8 ? 255.0 : type == GN_DEM_U16 ? 65535.0 : 32767.0;
    if (!(nodata >= lo && nodata <= hi) || nodata != std::floor(nodata))
      return fail(ctx, GN_ERR_ARG, "gn_set_dem_format: nodata is not representable in the element type (an integer within its range)");
  }
  ctx->demf.type = type; ctx->demf.scale = scale; ctx->demf.offset = offset;
  ctx->demf.has_nodata = has_nodata ? 1 : 0; ctx->demf.nodata = has_nodata ? nodata : 0.0;
  return GN_OK;
}

int gn_get_dem_format(const gn_ctx* ctx, int* type, double* scale, double* offset, int* has_nodata, double* nodata) {
  if (!ctx) return GN_ERR_ARG;
  if (type) *type = ctx->demf.type;
  if (scale) *scale = ctx->demf.scale;
  if (offset) *offset = ctx->demf.offset;
  if (has_nodata) *has_nodata = ctx->demf.has_nodata;
  if (nodata) *nodata = ctx->demf.nodata;
  return GN_OK;
}

int gn_dem_last_dropped(gn_ctx* ctx, int B, int32_t* dropped_host, void* stream) {
  if (!ctx || B < 1 || B > ctx->max_batch || !dropped_host) return fail(ctx, GN_ERR_ARG, "bad gn_dem_last_dropped argument");
  if (!ctx->ws.dem_dropped) return fail(ctx, GN_ERR_ARG, "gn_dem_last_dropped: context has no workspaces (a gn_resize failed)");
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipStreamSynchronize((hipStream_t)stream));
  GN_HIP(hipDeviceSynchronize());      // the gather may sit on the library's own streams (gn_set_substreams)
  GN_HIP(hipMemcpy(dropped_host, ctx->ws.dem_dropped, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  return GN_OK;
}

namespace {
// the context's coefficients (gn_set_distortion), null when off
const double* dist_of(const gn_ctx* c) { return c && c->dist_on ? c->dist : nullptr; }
// the per-pair table a PnP stage runs with (gn_set_pair_cameras): rows = null when off
struct PairCams { const double* rows = nullptr; int model = 0; };
extern "C++" {
PairCams pair_cams_of(const gn_ctx* c) { return c && c->pair_cams ? PairCams{c->pair_cams, c->pair_cams_model} : PairCams(); }
PairCams pair_cams_of(const Call& v) { return {v.cams, v.cam_model}; }
}
// a call of B pairs needs B rows
int pair_cams_fit(gn_ctx* ctx, int B) {
  return ctx && ctx->pair_cams && B > ctx->pair_cams_n ? fail(ctx, GN_ERR_ARG, "B exceeds the rows of the table (gn_set_pair_cameras)") : GN_OK;
}
// gn_pnp_ransac (cov, sigma_hat, cov_ok all null), gn_pnp_ransac_cov (all three given: k_pnp_cov runs behind k_pnp_refine) and
// gn_pnp_ransac_report (any of rep given: k_pnp_report runs last)
int pnp_impl(gn_ctx* ctx, const View& w, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
             const double* K9, const double* dk, int iterations_count, float reproj_error_px, double confidence, int min_pts,
             double* R, double* t, int32_t* n_inliers, uint8_t* ok, double sigma_px, double* cov, double* sigma_hat, uint8_t* cov_ok, void* stream,
             const Report& rep = Report(), const PairCams& pc = PairCams()) {
  if (!ctx || !obj || !img || !n_pts || (!K9 && !pc.rows) || !R || !t || !n_inliers || !ok || B < 1 || B > ctx->max_batch)
    return fail(ctx, GN_ERR_ARG, "bad gn_pnp_ransac argument");
  if ((cov || sigma_hat || cov_ok) && !(cov && sigma_hat && cov_ok)) return fail(ctx, GN_ERR_ARG, "cov_rt, sigma_hat and cov_ok go together");
  if (kstride < 1 || kstride > ctx->npad) return fail(ctx, GN_ERR_ARG, "kstride exceeds max_kpts of this context");
  if (iterations_count < 1 || iterations_count > GN_RANSAC_MAX_ITERATIONS)
    return fail(ctx, GN_ERR_ARG, "iterations_count must be in 1..4096 (GN_RANSAC_MAX_ITERATIONS; PoseNode uses 10)");
  GN_HIP(hipSetDevice(ctx->device));
  PnpArgs a;
  a.obj = obj; a.img = img; a.n_pts = n_pts; a.kstride = kstride; a.B = B;
  if (pc.rows) { a.fx = a.fy = a.cx = a.cy = 0.0; a.cams = pc.rows; a.dist = pc.model; dk = nullptr; }      // row b for pair b: K9 and dk are not read
  else { a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5]; }
  a.iterations = iterations_count; a.reproj = reproj_error_px; a.confidence = confidence; a.min_pts = min_pts;
  a.R = R; a.t = t; a.n_inliers = n_inliers; a.ok = ok; a.mask_ws = w.mask_ws; a.hyp = w.hyp_ws; a.pts_ws = w.pts_ws;
  a.dbg_ts = ctx->pnp_stamps ? reinterpret_cast<long long*>(w.sim) : nullptr;   // developer knob 15: phase stamps land in the (idle) sim buffer
  a.sigma_px = sigma_px; a.cov = cov; a.sigma_hat = sigma_hat; a.cov_ok = cov_ok;
  a.inlier_mask = rep.inlier_mask; a.inlier_idx = rep.inlier_idx; a.reproj_err = rep.reproj_err;
  if (dk) { a.dist = 1; for (int i = 0; i < 5; ++i) a.dk[i] = dk[i]; }     // (null = off; the arguments travel by value, like fx .. cy)
  a.rmask_ws = w.rmask_ws; a.rstate = w.rstate_ws; a.force_rounds = ctx->pnp_rounds;
  // gn_ransac_last_counts: a sub-batch group's stage is the pairs [b0, b0 + B) of its call
  if (w.b0 == 0 || !ctx->last_pnp_valid) { ctx->last_pnp = a; ctx->last_npts = n_pts - w.b0; ctx->last_pnp_valid = true; }
  StageTimer tm(ctx, (hipStream_t)stream, ST_PNP);
  launch_pnp(a, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}
}  // namespace

int gn_pnp_ransac(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                  const double* K9, int iterations_count, float reproj_error_px, double confidence, int min_pts,
                  double* R, double* t, int32_t* n_inliers, uint8_t* ok, void* stream) {
  if (const int rcf = pair_cams_fit(ctx, B)) return rcf;
  return pnp_impl(ctx, view_of(ctx), B, obj, img, n_pts, kstride, K9, dist_of(ctx), iterations_count, reproj_error_px, confidence, min_pts, R, t, n_inliers, ok,
                  0.0, nullptr, nullptr, nullptr, stream, Report(), pair_cams_of(ctx));
}

int gn_pnp_ransac_cov(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                      const double* K9, int iterations_count, float reproj_error_px, double confidence, int min_pts,
                      double* R, double* t, int32_t* n_inliers, uint8_t* ok,
                      double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream) {
  if (!cov_rt || !sigma_hat || !cov_ok) return fail(ctx, GN_ERR_ARG, "gn_pnp_ransac_cov: null covariance output");
  if (const int rcf = pair_cams_fit(ctx, B)) return rcf;
  return pnp_impl(ctx, view_of(ctx), B, obj, img, n_pts, kstride, K9, dist_of(ctx), iterations_count, reproj_error_px, confidence, min_pts, R, t, n_inliers, ok,
                  sigma_px, cov_rt, sigma_hat, cov_ok, stream, Report(), pair_cams_of(ctx));
}

int gn_pnp_ransac_report(gn_ctx* ctx, int B, const float* obj, const float* img, const int32_t* n_pts, int kstride,
                         const double* K9, int iterations_count, float reproj_error_px, double confidence, int min_pts,
                         double* R, double* t, int32_t* n_inliers, uint8_t* ok,
                         double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                         uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream) {
  if (const int rcf = pair_cams_fit(ctx, B)) return rcf;
  return pnp_impl(ctx, view_of(ctx), B, obj, img, n_pts, kstride, K9, dist_of(ctx), iterations_count, reproj_error_px, confidence, min_pts, R, t, n_inliers, ok,
                  sigma_px, cov_rt, sigma_hat, cov_ok, stream, Report{inlier_mask, inlier_idx, reproj_err}, pair_cams_of(ctx));
}

int gn_ransac_last_counts(gn_ctx* ctx, int B, int32_t* niters_host, int32_t* evaluated_host, void* stream) {
  if (!ctx || B < 1 || B > ctx->max_batch || !niters_host || !evaluated_host) return fail(ctx, GN_ERR_ARG, "bad gn_ransac_last_counts argument");
  if (!ctx->last_pnp_valid) return fail(ctx, GN_ERR_ARG, "gn_ransac_last_counts: no PnP stage has run on this context");
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipStreamSynchronize((hipStream_t)stream));
  GN_HIP(hipDeviceSynchronize());      // the stage may sit on the library's own streams (gn_set_overlap, gn_set_substreams)
  if (ctx->last_pnp.iterations <= 16 && !ctx->last_pnp.force_rounds) {
    // a classic stage keeps no RansacState: fold what k_pnp_hyp left, for all B pairs from the workspaces as allocated
    PnpArgs a = ctx->last_pnp;
    a.B = B; a.n_pts = ctx->last_npts; a.hyp = ctx->ws.hyp_ws; a.rstate = ctx->ws.rstate_ws;
    launch_pnp_counts(a, (hipStream_t)stream);
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  std::vector<RansacState> st((size_t)B);
  GN_HIP(hipMemcpy(st.data(), ctx->ws.rstate_ws, (size_t)B * sizeof(RansacState), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) { niters_host[b] = st[b].niters; evaluated_host[b] = st[b].evaluated; }
  return GN_OK;
}

namespace {
// The PnP stream, its events and the double-buffered PnP inputs (gn_set_overlap, gn_set_substreams).
int ensure_pnp_stage(gn_ctx* ctx) {
  if (ctx->s_pnp) return GN_OK;
  // s_pnp is what marks the stage as ready, so it is set last: a failure on the way leaves a context that tries again
  { const int rc = alloc_workspaces(ctx, kWsPnpStage); if (rc != GN_OK) return rc; }
  auto event = [](hipEvent_t& e) { return e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); };
  for (int g = 0; g < 8; ++g) {
    for (int i = 0; i < 2; ++i) { GN_HIP(event(ctx->ev_gather[i][g])); GN_HIP(event(ctx->ev_pnp[i][g])); }
    GN_HIP(event(ctx->ev_head[g]));
  }
  GN_HIP(hipStreamCreateWithFlags(&ctx->s_pnp, hipStreamNonBlocking));
  return GN_OK;
}

// `s` behind every PnP that the PnP stream still holds
int join_pnp(gn_ctx* ctx, hipStream_t s) {
  for (int i = 0; i < 2; ++i)
    for (int g = 0; g < 8; ++g)
      if (ctx->pnp_pending[i][g]) { GN_HIP(hipStreamWaitEvent(s, ctx->ev_pnp[i][g], 0)); ctx->pnp_pending[i][g] = false; }
  return GN_OK;
}

// `s` behind every unjoined sub-batch group (its matcher and gather; its PnP is join_pnp's)
int join_groups(gn_ctx* ctx, hipStream_t s) {
  for (int g = 0; g < 8; ++g)
    if (ctx->sub_pending[g]) { GN_HIP(hipStreamWaitEvent(s, ctx->ev_join[g], 0)); ctx->sub_pending[g] = false; }
  return GN_OK;
}

// `s` behind everything the library's internal streams still hold
int join_internal(gn_ctx* ctx, hipStream_t s) {
  const int rc = join_pnp(ctx, s);
  return rc != GN_OK ? rc : join_groups(ctx, s);
}

// Matcher, gather and PnP of call v on the view w -- the whole context, or sub-batch group w.g of a call on its share of the workspaces -- enqueued on `stream`.
// slot < 0: all three on `stream`.  slot 0 / 1: the latency-bound PnP kernels (a few hundred single-wave workgroups) run on the PnP stream from
// that slot of the double-buffered PnP inputs, and `stream` is free for the next call's matcher once the gather is enqueued; R / t / n_inliers / ok
// are complete behind ev_pnp[slot][g] (gn_flush, or the waits gn_estimate enqueues one call later).
int estimate_impl(gn_ctx* ctx, const View& w, const Call& v, void* stream, int slot = -1) {
  const int g = w.g;
  // the match list: the caller's arrays when the call has them (gn_estimate_report), else the workspaces
  int64_t* const m_idx = v.idx ? v.idx : w.e_idx;
  float* const m_score = v.score ? v.score : w.e_score;
  int rc = match_impl(ctx, w, v.B, v.kpt_format, v.desc_q, v.kpt_q, v.n_q, v.stride_q, v.desc_r, v.kpt_r, v.n_r, v.stride_r,
                    m_idx, m_score, v.n_match, stream);
  if (rc != GN_OK) return rc;
  if (slot < 0) {
    rc = gather_impl(ctx, v.demf, v.dropped, v.B, v.kpt_format, v.kpt_q, v.stride_q, v.kpt_r, v.stride_r, m_idx, m_score, v.n_match, v.dem, v.H, v.W,
                     w.e_mkp, w.e_obj, stream);
    if (rc != GN_OK) return rc;
    return pnp_impl(ctx, w, v.B, w.e_obj, w.e_mkp, v.n_match, ctx->npad, v.K9, v.dist ? v.dk : nullptr, v.ransac_iters, v.ransac_reproj, v.ransac_conf, v.min_matches,
                    v.R, v.t, v.n_inliers, v.ok, v.sigma_px, v.cov, v.sigma_hat, v.cov_ok, stream, report_of(v), pair_cams_of(v));
  }
  hipStream_t s = (hipStream_t)stream;
  float* const o_mkp = slot ? w.o_mkp1 : w.o_mkp0; float* const o_obj = slot ? w.o_obj1 : w.o_obj0; int32_t* const o_nmatch = slot ? w.o_nmatch1 : w.o_nmatch0;
  GN_HIP(hipSetDevice(ctx->device));
  GN_HIP(hipEventRecord(ctx->ev_head[g], s));
  if (ctx->pnp_recorded[slot][g]) GN_HIP(hipStreamWaitEvent(s, ctx->ev_pnp[slot][g], 0));   // the PnP that last read this slot (two calls ago)
  rc = gather_impl(ctx, v.demf, v.dropped, v.B, v.kpt_format, v.kpt_q, v.stride_q, v.kpt_r, v.stride_r, m_idx, m_score, v.n_match, v.dem, v.H, v.W,
                   o_mkp, o_obj, stream);
  if (rc != GN_OK) return rc;
  GN_HIP(hipMemcpyAsync(o_nmatch, v.n_match, (size_t)v.B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  // the call's camera rows travel with its match counts: the PnP stream reads the slot's copy, so the caller's table is read in the order of
  // `stream` like every other input (no table: neither the copy nor the line exists for this call)
  PairCams pc = pair_cams_of(v);
  if (pc.rows) {
    double* const o_cams = slot ? w.o_cams1 : w.o_cams0;
    GN_HIP(hipMemcpyAsync(o_cams, pc.rows, (size_t)v.B * GN_PAIR_CAMERA_DOUBLES * sizeof(double), hipMemcpyDeviceToDevice, s));
    pc.rows = o_cams;
  }
  GN_HIP(hipEventRecord(ctx->ev_gather[slot][g], s));
  GN_HIP(hipStreamWaitEvent(ctx->s_pnp, ctx->ev_gather[slot][g], 0));
  rc = pnp_impl(ctx, w, v.B, o_obj, o_mkp, o_nmatch, ctx->npad, v.K9, v.dist ? v.dk : nullptr, v.ransac_iters, v.ransac_reproj, v.ransac_conf, v.min_matches,
                v.R, v.t, v.n_inliers, v.ok, v.sigma_px, v.cov, v.sigma_hat, v.cov_ok, ctx->s_pnp, report_of(v), pc);
  if (rc != GN_OK) return rc;
  GN_HIP(hipEventRecord(ctx->ev_pnp[slot][g], ctx->s_pnp));
  ctx->pnp_pending[slot][g] = ctx->pnp_recorded[slot][g] = true;
  return GN_OK;
}

// deferred certificate: wait for the flags of the pending call in `slot` (its kernels are behind at most one later call on the GPU), re-run
// its flagged pairs from the saved call on `s`
int cert_resolve(gn_ctx* ctx, int slot, hipStream_t s) {
  gn_ctx::CertPending& p = ctx->cert_pend[slot];
  if (!p.active) return GN_OK;
  p.active = false;
  GN_HIP(hipEventSynchronize(p.ev));
  const Restore keep(ctx->npad_run);
  ctx->npad_run = p.npad_run;
  // a re-run writes outputs of this call and works in slices of the workspaces that the groups and the PnP stream may still be using: it
  // goes behind every pending PnP (this call's above all) and every group first (calls without a flagged pair never get here)
  return certify_rerun(ctx, s, p.call, [&](const View& rw, const Call& w) { const int rcj = join_internal(ctx, s); return rcj != GN_OK ? rcj : estimate_impl(ctx, rw, w, s); }, p.flags, p.level);
}
}  // namespace

namespace {
// gn_estimate (covariance pointers null), gn_estimate_cov and gn_estimate_report (idx / score / rep: each null = not asked for)
int estimate_call(gn_ctx* ctx, int B, int kpt_format,
                  const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                  const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                  const uint8_t* dem, int H, int W, const double* K9, int min_matches,
                  double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                  double sigma_px, double* cov, double* sigma_hat, uint8_t* cov_ok, void* stream,
                  int64_t* idx = nullptr, float* score = nullptr, const Report& rep = Report()) {
  if (!ctx) return fail(nullptr, GN_ERR_ARG, "null context");
  if ((cov || sigma_hat || cov_ok) && !(cov && sigma_hat && cov_ok)) return fail(ctx, GN_ERR_ARG, "cov_rt, sigma_hat and cov_ok go together");
  if (const int rcf = pair_cams_fit(ctx, B)) return rcf;
  if (ctx->pair_cams) K9 = nullptr;      // the table rules: the caller's matrix is neither read nor saved
  if (ctx->fused_proj_pending && ctx->npad > 0 && gn_missing_tensors(ctx) == 0) {      // (the sub-batch groups below skip it: it works on the workspaces as allocated)
    GN_HIP(hipSetDevice(ctx->device));
    int rcs = ensure_composed(ctx);
    if (rcs == GN_OK) rcs = selfcheck_fused_projection(ctx);
    if (rcs != GN_OK) return rcs;
  }
  Call v(ctx->feature, ctx->npad, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r);
  v.dem = dem; v.H = H; v.W = W; v.K9 = K9; v.min_matches = min_matches;
  v.R = R; v.t = t; v.n_match = n_match; v.n_inliers = n_inliers; v.ok = ok;
  v.sigma_px = sigma_px; v.cov = cov; v.sigma_hat = sigma_hat; v.cov_ok = cov_ok;
  v.idx = idx; v.score = score; v.inlier_mask = rep.inlier_mask; v.inlier_idx = rep.inlier_idx; v.reproj_err = rep.reproj_err;
  v.dist = ctx->dist_on; memcpy(v.dk, ctx->dist, sizeof v.dk);      // captured now: a deferred re-run of this call (cert_pend) keeps them
  v.cams = ctx->pair_cams; v.cam_model = ctx->pair_cams_model;      // (the pointer: the caller keeps the table alive as it keeps n_q)
  v.ransac_iters = ctx->ransac_iters; v.ransac_reproj = ctx->ransac_reproj; v.ransac_conf = ctx->ransac_conf;
  v.demf = ctx->demf; v.dropped = dem && v.demf.has_nodata ? ctx->ws.dem_dropped : nullptr;
  const int groups = std::min(ctx->n_sub, B);
  if (groups <= 1) {
    // An earlier grouped call may be unjoined (deferred join, deferred certificate) and this call works in the whole workspaces, on the
    // caller's stream: behind the groups first, and -- unless its own PnP goes to the PnP stream, which keeps the order -- behind their PnP.
    GN_HIP(hipSetDevice(ctx->device));
    const int rcj = ctx->overlap ? join_groups(ctx, (hipStream_t)stream) : join_internal(ctx, (hipStream_t)stream);
    if (rcj != GN_OK) return rcj;
    return estimate_impl(ctx, view_of(ctx), v, stream, ctx->overlap ? (int)(ctx->calls++ & 1) : -1);
  }
  if (ctx->npad <= 0) return fail(ctx, GN_ERR_ARG, "context has no workspaces (a gn_resize failed): call gn_resize again");
  if (B < 1 || B > ctx->max_batch) return fail(ctx, GN_ERR_ARG, "B out of range for this context");
  GN_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // deferred joins still pending from a call of another shape: group g of this call would overlap the workspace slice of a
  // different group of that call on another stream -> join them first (the fork event below is recorded behind the joins)
  if ((ctx->defer_join || ctx->certify == 3) && (ctx->sub_last_B != B || ctx->sub_last_np != ctx->npad_run)) {      // (deferred certificate: the caller's stream joins the heads only)
    const int rcj = gn_flush(ctx, stream);
    if (rcj != GN_OK) return rcj;
  }
  ctx->sub_last_B = B; ctx->sub_last_np = ctx->npad_run;
  ctx->prune_last_B = B;
  ctx->ovf_groups_last = groups;
  GN_HIP(hipEventRecord(ctx->ev_fork, s));
  // Every group runs matcher and gather on its own stream and hands its PnP to the PnP stream (slot = parity of the call), so the group's stream is
  // free for the next call while the PnP chains run.  Deferred certificate: the outputs of call n are final once call n + 1 has been enqueued --
  // the caller's stream takes the earlier calls' PnP here, BEHIND the fork, so that no group of this call waits for them.
  const int slot = (int)(ctx->calls++ & 1);
  if (ctx->certify == 3) { const int rcj = join_pnp(ctx, s); if (rcj != GN_OK) return rcj; }
  int rc_all = GN_OK, b0 = 0;
  for (int g = 0; g < groups; ++g) {
    const int Bg = B / groups + (g < B % groups ? 1 : 0);
    hipStream_t sg = ctx->sub_serial ? ctx->sub_s[0] : ctx->sub_s[g];
    GN_HIP(hipStreamWaitEvent(sg, ctx->ev_fork, 0));
    ctx->in_group = true;            // (the view carries this group's own guard word: cleared, raised and read on this group's stream only)
    const int rc = estimate_impl(ctx, view_of(ctx, b0, g), slice(v, b0, Bg), sg, slot);
    ctx->in_group = false;
    if (rc != GN_OK && rc_all == GN_OK) rc_all = rc;
    GN_HIP(hipEventRecord(ctx->ev_join[g], sg));
    ctx->sub_pending[g] = true;
    b0 += Bg;
  }
  // default: the caller's stream continues only after every group is done -- inputs may be released and outputs read in
  // stream order, like any other call.  gn_set_deferred_join(1) leaves the join to gn_flush (consecutive calls then pipeline
  // inside each group's stream; the caller keeps the INPUT buffers alive until it has flushed).
  if (ctx->certify == 3 && rc_all == GN_OK) {
    // deferred certificate: the caller's stream goes behind every group's match head (stream order only; gather and PnP of the call are still to
    // come -- gn_flush, a re-run of this call and the next call's waits above take them), leaves this call's flags in a pinned slot behind an
    // event, and resolves the PREVIOUS call now that this one is queued -- the host waits for call n while the GPU already works on call n + 1
    for (int g = 0; g < groups; ++g) GN_HIP(hipStreamWaitEvent(s, ctx->ev_head[g], 0));
    const int slot = ctx->cert_slot;
    gn_ctx::CertPending& p = ctx->cert_pend[slot];
    if (p.active) { const int rcr = cert_resolve(ctx, slot, s); if (rcr != GN_OK) return rcr; }     // (cannot happen in the alternating order; kept for safety)
    GN_HIP(hipMemcpyAsync(p.flags, ctx->ws.uncert, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (ffn_auto(ctx)) {
      GN_HIP(hipMemcpyAsync(p.flags + ctx->max_batch, ctx->ws.uncert_alt, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      GN_HIP(hipMemcpyAsync(p.flags + 2 * ctx->max_batch, ctx->ws.uncert_alt2, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      GN_HIP(hipMemcpyAsync(p.flags + 3 * ctx->max_batch, ctx->ws.uncert_alt3, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    } else memset(p.flags + ctx->max_batch, 0, (size_t)3 * ctx->max_batch * sizeof(int32_t));
    GN_HIP(hipEventRecord(p.ev, s));
    p.active = true; p.level = ffn_auto(ctx) ? ffn_auto_state(ctx) : -1; p.npad_run = ctx->npad_run;
    p.call = v;
    if (K9) { memcpy(p.K9, K9, sizeof p.K9); p.call.K9 = p.K9; }
    ctx->cert_slot ^= 1;
    return cert_resolve(ctx, slot ^ 1, s);
  }
  if (!ctx->defer_join || ctx->certify == 2) { const int rcj = gn_flush(ctx, stream); if (rcj != GN_OK && rc_all == GN_OK) rc_all = rcj; }
  if (ctx->certify == 2 && rc_all == GN_OK) {
    // the groups are joined: one read-back of the call's per-pair flags, then matcher + gather + PnP of the flagged pairs again in exact f32
    rc_all = certify_rerun(ctx, s, v, [&](const View& rw, const Call& w) { return estimate_impl(ctx, rw, w, s); });
  }
  return rc_all;
}
}  // namespace

int gn_estimate(gn_ctx* ctx, int B, int kpt_format,
                const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                const uint8_t* dem, int H, int W, const double* K9, int min_matches,
                double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok, void* stream) {
  return estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, dem, H, W, K9, min_matches,
                       R, t, n_match, n_inliers, ok, 0.0, nullptr, nullptr, nullptr, stream);
}

int gn_estimate_cov(gn_ctx* ctx, int B, int kpt_format,
                    const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                    const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                    const uint8_t* dem, int H, int W, const double* K9, int min_matches,
                    double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                    double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream) {
  if (!cov_rt || !sigma_hat || !cov_ok) return fail(ctx, GN_ERR_ARG, "gn_estimate_cov: null covariance output");
  return estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, dem, H, W, K9, min_matches,
                       R, t, n_match, n_inliers, ok, sigma_px, cov_rt, sigma_hat, cov_ok, stream);
}

int gn_estimate_report(gn_ctx* ctx, int B, int kpt_format,
                       const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                       const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                       const uint8_t* dem, int H, int W, const double* K9, int min_matches,
                       double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                       double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                       int64_t* idx, float* score, uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream) {
  return estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, dem, H, W, K9, min_matches,
                       R, t, n_match, n_inliers, ok, sigma_px, cov_rt, sigma_hat, cov_ok, stream, idx, score, Report{inlier_mask, inlier_idx, reproj_err});
}

int gn_set_deferred_join(gn_ctx* ctx, int enable) {
  if (!ctx) return GN_ERR_ARG;
  ctx->defer_join = enable ? 1 : 0;
  return GN_OK;
}

int gn_set_active_kpts(gn_ctx* ctx, int max_kpts_per_side) {
  if (!ctx || max_kpts_per_side < 1) return GN_ERR_ARG;
  ctx->npad_run = std::min(ctx->npad, ((max_kpts_per_side + 127) / 128) * 128);
  return ctx->npad_run;
}

int gn_set_substreams(gn_ctx* ctx, int n) {
  if (!ctx || n < 1 || n > 8) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  if (n > 1 && !ctx->ev_fork) GN_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  if (n > 1) { const int rc = ensure_pnp_stage(ctx); if (rc != GN_OK) return rc; }      // the groups' pose stage runs on the PnP stream
  for (int i = 0; i < n && n > 1; ++i)
    if (!ctx->sub_s[i]) {
      if (ctx->cu_mask_mode != 0) {
        // developer experiment (knob 29): every sub-batch stream on its own share of the CUs.  bit b of the mask = CU b of the device's enumeration:
        // 1 = contiguous shares, 2 = interleaved (b % n), 3 = by XCD assuming b % 8 is the XCD (share g gets XCDs g, g + n, ...)
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int b = 0; b < 256; ++b) {
          const int share = ctx->cu_mask_mode == 1 ? b * n / 256 : ctx->cu_mask_mode == 2 ? b % n : (b % 8) % n;
          if (share == i) mask[b >> 5] |= 1u << (b & 31);
        }
        GN_HIP(hipExtStreamCreateWithCUMask(&ctx->sub_s[i], 8, mask));
      } else {
        GN_HIP(hipStreamCreateWithFlags(&ctx->sub_s[i], hipStreamNonBlocking));
      }
      GN_HIP(hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming));
    }
  ctx->n_sub = n;
  return GN_OK;
}


int gn_set_overlap(gn_ctx* ctx, int enable) {
  if (!ctx) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  if (enable) { const int rc = ensure_pnp_stage(ctx); if (rc != GN_OK) return rc; }
  if (!enable && ctx->s_pnp) GN_HIP(hipStreamSynchronize(ctx->s_pnp));
  ctx->overlap = enable ? 1 : 0;
  return GN_OK;
}

int gn_flush(gn_ctx* ctx, void* stream) {
  if (!ctx) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  { const int rc = join_internal(ctx, (hipStream_t)stream); if (rc != GN_OK) return rc; }
  if (!ctx->cert_inner)
    for (int k = 0; k < 2; ++k) {       // deferred certificates still open: the older one first
      const int rc = cert_resolve(ctx, ctx->cert_slot ^ k, (hipStream_t)stream);
      if (rc != GN_OK) return rc;
    }
  return GN_OK;
}

// TwistNode's matcher for B frame pairs: BFMatcher(L2).knnMatch(k=2) + ratio test (twist_node.py:248-267)
int gn_vo_match(gn_ctx* ctx, int B, const float* desc_q, const int32_t* n_q, int stride_q,
                const float* desc_r, const int32_t* n_r, int stride_r, double ratio,
                int64_t* idx, float* dist, int32_t* n_good, int32_t* nn_idx, float* nn_dist, void* stream) {
  if (!ctx) return fail(nullptr, GN_ERR_ARG, "null context");
  if (ctx->npad <= 0) return fail(ctx, GN_ERR_ARG, "context has no workspaces (a gn_resize failed): call gn_resize again");
  if (B < 1 || B > ctx->max_batch) return fail(ctx, GN_ERR_ARG, "B out of range for this context");
  if (stride_q < 1 || stride_r < 1 || stride_q > ctx->npad || stride_r > ctx->npad)
    return fail(ctx, GN_ERR_ARG, "keypoint stride exceeds max_kpts of this context");
  if (!desc_q || !n_q || !desc_r || !n_r || !idx || !dist || !n_good) return fail(ctx, GN_ERR_ARG, "null argument");
  GN_HIP(hipSetDevice(ctx->device));
  { const int rc = ensure_sim(ctx); if (rc != GN_OK) return rc; }   // q . r panel of the brute-force matcher (first call allocates it)
  hipStream_t s = (hipStream_t)stream;
  const int np = ctx->npad;
  VoArgs v;
  v.desc_q = desc_q; v.n_q = n_q; v.stride_q = stride_q; v.desc_r = desc_r; v.n_r = n_r; v.stride_r = stride_r;
  v.B = B; v.npad = np; v.ratio = ratio;
  v.desc = ctx->ws.desc; v.norm2 = ctx->vo_norm2; v.nvalid = ctx->ws.nvalid; v.sim = ctx->ws.sim;
  v.nn_idx = ctx->vo_nn_idx; v.nn_dist = ctx->vo_nn_dist; v.good = ctx->vo_good;
  v.idx = idx; v.dist = dist; v.n_good = n_good; v.kmax = np;
  launch_vo_pack(v, s);
  // q.r for every (query, train) pair on the exact-f32 MFMA GEMM, whatever the context's precision mode
  GemmArgs gs;
  memset(&gs, 0, sizeof gs);
  gs.A = ctx->ws.desc; gs.lda = kInDim; gs.K1 = kInDim; gs.W = ctx->ws.desc + (size_t)np * kInDim; gs.ldw = kInDim;
  gs.Y = ctx->ws.sim; gs.ldy = np; gs.M = np; gs.N = np; gs.K = kInDim; gs.acc_scale = 1.f;
  gs.strideA = gs.strideW = 2LL * np * kInDim; gs.strideY = (long long)np * np;
  gn::LaunchKnobs exact = ctx->knobs;
  exact.gemm_variant = 3;
  launch_gemm_f32(EPI_PLAIN, gs, B, s, exact);
  launch_vo_knn2(v, s);
  if (nn_idx) GN_HIP(hipMemcpyAsync(nn_idx, ctx->vo_nn_idx, (size_t)B * np * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (nn_dist) GN_HIP(hipMemcpyAsync(nn_dist, ctx->vo_nn_dist, (size_t)B * np * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
  GN_HIP(hipGetLastError());
  return GN_OK;
}

// TwistNode._pose lines 227-289 for B frame pairs: 2-NN match -> ratio test -> MIN_MATCHES gate -> compute_pose with
// a zero elevation raster (planar PnP)
namespace {
int vo_estimate_call(gn_ctx* ctx, int B, int kpt_format,
                     const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                     const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                     const double* K9, double ratio, int min_matches,
                     double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                     double sigma_px, double* cov, double* sigma_hat, uint8_t* cov_ok, void* stream,
                     int64_t* idx = nullptr, float* score = nullptr, const Report& rep = Report()) {
  if (!ctx) return fail(nullptr, GN_ERR_ARG, "null context");
  if (const int rcf = pair_cams_fit(ctx, B)) return rcf;
  int64_t* const m_idx = idx ? idx : ctx->ws.e_idx;
  float* const m_score = score ? score : ctx->ws.e_score;
  int rc = gn_vo_match(ctx, B, desc_q, n_q, stride_q, desc_r, n_r, stride_r, ratio, m_idx, m_score, n_match,
                       nullptr, nullptr, stream);
  if (rc != GN_OK) return rc;
  rc = gn_gather_points(ctx, B, kpt_format, kpt_q, stride_q, kpt_r, stride_r, m_idx, n_match, nullptr, 0, 0,
                        ctx->ws.e_mkp, ctx->ws.e_obj, stream);
  if (rc != GN_OK) return rc;
  return pnp_impl(ctx, view_of(ctx), B, ctx->ws.e_obj, ctx->ws.e_mkp, n_match, ctx->npad, K9, dist_of(ctx), ctx->ransac_iters, ctx->ransac_reproj, ctx->ransac_conf, min_matches,
                  R, t, n_inliers, ok, sigma_px, cov, sigma_hat, cov_ok, stream, rep, pair_cams_of(ctx));
}
}  // namespace

int gn_vo_estimate(gn_ctx* ctx, int B, int kpt_format,
                   const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                   const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                   const double* K9, double ratio, int min_matches,
                   double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok, void* stream) {
  return vo_estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, K9, ratio, min_matches,
                          R, t, n_match, n_inliers, ok, 0.0, nullptr, nullptr, nullptr, stream);
}

int gn_vo_estimate_cov(gn_ctx* ctx, int B, int kpt_format,
                       const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                       const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                       const double* K9, double ratio, int min_matches,
                       double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                       double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok, void* stream) {
  if (!cov_rt || !sigma_hat || !cov_ok) return fail(ctx, GN_ERR_ARG, "gn_vo_estimate_cov: null covariance output");
  return vo_estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, K9, ratio, min_matches,
                          R, t, n_match, n_inliers, ok, sigma_px, cov_rt, sigma_hat, cov_ok, stream);
}

int gn_vo_estimate_report(gn_ctx* ctx, int B, int kpt_format,
                          const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q,
                          const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r,
                          const double* K9, double ratio, int min_matches,
                          double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok,
                          double sigma_px, double* cov_rt, double* sigma_hat, uint8_t* cov_ok,
                          int64_t* idx, float* score, uint8_t* inlier_mask, int32_t* inlier_idx, float* reproj_err, void* stream) {
  return vo_estimate_call(ctx, B, kpt_format, desc_q, kpt_q, n_q, stride_q, desc_r, kpt_r, n_r, stride_r, K9, ratio, min_matches,
                          R, t, n_match, n_inliers, ok, sigma_px, cov_rt, sigma_hat, cov_ok, stream, idx, score, Report{inlier_mask, inlier_idx, reproj_err});
}

namespace {
// cv::getRotationMatrix2D + the in-place inversion at the top of cv::warpAffine (f64, same operation order), and the
// matrix StereoNode._rotate_and_crop_center returns (inverse of the rotation, times the crop translation)
void rotate_crop_matrices(int H, int W, double angle_degrees, int crop_h, int crop_w, double Minv6[6], int* dx, int* dy, double back9[9]) {
  const int cxi = W / 2, cyi = H / 2;
  const double a = angle_degrees * (3.14159265358979323846 / 180.0);
  const double alpha = std::cos(a), beta = std::sin(a);
  const double cx = (double)(float)cxi, cy = (double)(float)cyi;
  const double m[6] = {alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy};
  double M[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  for (int i = 0; i < 6; ++i) Minv6[i] = M[i];
  *dx = cxi - crop_w / 2; *dy = cyi - crop_h / 2;
  if (back9) {   // inv([[m]; 0 0 1]) @ [[1 0 dx], [0 1 dy], [0 0 1]]  (adjugate form of the 3x3 inverse)
    const double det = m[0] * m[4] - m[1] * m[3];
    const double i00 = m[4] / det, i01 = -m[1] / det, i02 = (m[1] * m[5] - m[2] * m[4]) / det;
    const double i10 = -m[3] / det, i11 = m[0] / det, i12 = (m[2] * m[3] - m[0] * m[5]) / det;
    back9[0] = i00; back9[1] = i01; back9[2] = i00 * *dx + i01 * *dy + i02;
    back9[3] = i10; back9[4] = i11; back9[5] = i10 * *dx + i11 * *dy + i12;
    back9[6] = 0; back9[7] = 0; back9[8] = 1;
  }
}
}  // namespace

// StereoNode._rotate_and_crop_center on a 2-channel u8 stack (stereo_node.py:292-335)
int gn_rotate_crop_center(gn_ctx* ctx, const uint8_t* stack, int H, int W, double angle_degrees, int crop_h, int crop_w,
                          uint8_t* out_stack, double* back9_host, void* stream) {
  if (!ctx || !stack || !out_stack || H < 1 || W < 1 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W)
    return fail(ctx, GN_ERR_ARG, "bad gn_rotate_crop_center argument");
  GN_HIP(hipSetDevice(ctx->device));
  WarpArgs a;
  a.src0 = stack; a.src1 = nullptr; a.H = H; a.W = W; a.crop_h = crop_h; a.crop_w = crop_w; a.out0 = out_stack; a.out1 = nullptr;
  rotate_crop_matrices(H, W, angle_degrees, crop_h, crop_w, a.M, &a.dx, &a.dy, back9_host);
  launch_rotate_crop(a, false, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

// stereo_node.py:229-262 in one pass: BGR -> gray, stack with the DEM, rotate, crop -> reference raster + DEM raster
int gn_stereo_reference(gn_ctx* ctx, const uint8_t* bgr, const uint8_t* dem, int H, int W, double angle_degrees,
                        int crop_h, int crop_w, uint8_t* out_ref, uint8_t* out_dem, double* back9_host, void* stream) {
  if (!ctx || !bgr || !dem || !out_ref || !out_dem || H < 1 || W < 1 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W)
    return fail(ctx, GN_ERR_ARG, "bad gn_stereo_reference argument");
  GN_HIP(hipSetDevice(ctx->device));
  WarpArgs a;
  a.src0 = bgr; a.src1 = dem; a.H = H; a.W = W; a.crop_h = crop_h; a.crop_w = crop_w; a.out0 = out_ref; a.out1 = out_dem;
  rotate_crop_matrices(H, W, angle_degrees, crop_h, crop_w, a.M, &a.dx, &a.dy, back9_host);
  launch_rotate_crop(a, true, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_stereo_reference_dem(gn_ctx* ctx, const uint8_t* bgr, const void* dem, int dem_type, int has_nodata, double nodata, int H, int W,
                            double angle_degrees, int crop_h, int crop_w, uint8_t* out_ref, void* out_dem, double* back9_host, void* stream) {
  if (!ctx || !bgr || !dem || !out_ref || !out_dem || H < 1 || W < 1 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W)
    return fail(ctx, GN_ERR_ARG, "bad gn_stereo_reference_dem argument");
  if (dem_type != GN_DEM_U8 && dem_type != GN_DEM_U16 && dem_type != GN_DEM_I16 && dem_type != GN_DEM_F32)
    return fail(ctx, GN_ERR_ARG, "gn_stereo_reference_dem: dem_type must be GN_DEM_U8, GN_DEM_U16, GN_DEM_I16 or GN_DEM_F32");
  if (has_nodata && dem_type != GN_DEM_F32) {
    const double lo = dem_type == GN_DEM_I16 ? -32768.0 : 0.0, hi = dem_type == GN_DEM_U8 ? 255.0 : dem_type == GN_DEM_U16 ? 65535.0 : 32767.0;
    if (!(nodata >= lo && nodata <= hi) || nodata != std::floor(nodata))
      return fail(ctx, GN_ERR_ARG, "gn_stereo_reference_dem: nodata is not representable in the element type");
  }
  GN_HIP(hipSetDevice(ctx->device));
  DemWarpArgs d;
  WarpArgs& a = d.w;
  a.src0 = bgr; a.src1 = nullptr; a.H = H; a.W = W; a.crop_h = crop_h; a.crop_w = crop_w; a.out0 = out_ref; a.out1 = nullptr;
  d.dem = dem; d.out_dem = out_dem; d.dem_type = dem_type; d.has_nodata = has_nodata ? 1 : 0; d.nodata = has_nodata ? nodata : 0.0;
  rotate_crop_matrices(H, W, angle_degrees, crop_h, crop_w, a.M, &a.dx, &a.dy, back9_host);
  launch_rotate_crop_dem(d, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

namespace {
int sift_prepare(gn_ctx* ctx, int B, int H, int W, int max_kp) {
  const int nl = ctx->sift_layers, n_g = nl + 3, n_d = nl + 2;     // Gaussian / DoG planes per octave
  const bool same_params = ctx->sift_ws_layers == nl && ctx->sift_ws_sigma == ctx->sift_sigma;
  if (ctx->sift_h == H && ctx->sift_w == W && ctx->sift_max_kp >= max_kp && ctx->sift_batch >= B && same_params) return GN_OK;
  B = std::max(B, ctx->sift_h == H && ctx->sift_w == W ? ctx->sift_batch : 1);
  for (void* p : ctx->sift_allocs) hipFree(p);
  ctx->sift_allocs.clear();
  ctx->sift_h = ctx->sift_w = 0; ctx->sift_batch = 0;
  auto alloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) return nullptr; ctx->sift_allocs.push_back(p); return p; };
  const int bw = 2 * W, bh = 2 * H;
  int n_oct = (int)std::nearbyint(std::log((double)std::min(bw, bh)) / std::log(2.0) - 2) + 1;
  if (n_oct < 1) n_oct = 1;
  if (n_oct > kSiftMaxOctaves) n_oct = kSiftMaxOctaves;
  SiftPyramid& py = ctx->sift_py;
  py.n_oct = n_oct; py.n_layers = nl;
  int w = bw, h = bh;
  for (int o = 0; o < n_oct; ++o) {
    py.oct[o].w = w; py.oct[o].h = h;
    const size_t n = (size_t)w * h;
    py.oct[o].stride = (long long)((n_g + n_d) * n);   // per image: nOctaveLayers + 3 Gaussian + nOctaveLayers + 2 DoG levels (6 + 5 by default), images back to back
    float* block = (float*)alloc((size_t)B * (n_g + n_d) * n * sizeof(float));
    if (!block) return fail(ctx, GN_ERR_HIP, "SIFT pyramid allocation failed");
    for (int i = 0; i < kSiftMaxLayers + 3; ++i) py.oct[o].gauss[i] = i < n_g ? block + i * n : nullptr;
    for (int i = 0; i < kSiftMaxLayers + 2; ++i) py.oct[o].dog[i] = i < n_d ? block + (n_g + i) * n : nullptr;
    w /= 2; h /= 2;
    if (w < 1 || h < 1) { py.n_oct = o + 1; break; }
  }
  ctx->sift_tmp = (float*)alloc((size_t)bw * bh * sizeof(float));
  // blur kernels: sigma differences of createInitialImage / buildGaussianPyramid (f64 on the host, libm exp)
  const double sigma = ctx->sift_sigma;
  ctx->sift_kernels.assign(n_g, {});
  { const float sf = (float)sigma; sift_gaussian_kernel((double)sqrtf(std::max(sf * sf - 0.5f * 0.5f * 4, 0.01f)), ctx->sift_kernels[0]); }   // createInitialImage: float arithmetic
  const double k = std::pow(2.0, 1.0 / nl);
  for (int i = 1; i < n_g; ++i) {
    const double sp = std::pow(k, (double)(i - 1)) * sigma, st = sp * k;
    sift_gaussian_kernel(std::sqrt(st * st - sp * sp), ctx->sift_kernels[i]);
  }
  size_t tot = 0; ctx->sift_koff.assign(n_g, 0);
  for (int i = 0; i < n_g; ++i) { ctx->sift_koff[i] = (int)tot; tot += ctx->sift_kernels[i].size(); }
  ctx->sift_dk = (float*)alloc(tot * sizeof(float));
  for (int i = 0; i < n_g; ++i)
    if (hipMemcpy(ctx->sift_dk + ctx->sift_koff[i], ctx->sift_kernels[i].data(), ctx->sift_kernels[i].size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return fail(ctx, GN_ERR_HIP, "SIFT kernel upload failed");
  ctx->sift_max_cand = std::max(65536, 16 * max_kp);
  ctx->sift_max_kp = std::max(max_kp, 1024);
  ctx->sift_cand = (int4*)alloc((size_t)B * ctx->sift_max_cand * sizeof(int4));
  ctx->sift_counts = (int*)alloc((size_t)B * 4 * sizeof(int));
  ctx->sift_raw_cap = 16384;                                   // raw keypoints (several orientations per extremum, duplicates) before the sort
  while (ctx->sift_raw_cap < 8 * ctx->sift_max_kp) ctx->sift_raw_cap <<= 1;
  ctx->sift_kp_stride = (long long)2 * ctx->sift_raw_cap + ctx->sift_max_kp;                        // per image: raw | sorted | final
  ctx->sift_kp = (SiftKeypoint*)alloc((size_t)B * ctx->sift_kp_stride * sizeof(SiftKeypoint));
  if (!ctx->sift_tmp || !ctx->sift_dk || !ctx->sift_cand || !ctx->sift_counts || !ctx->sift_kp)
    return fail(ctx, GN_ERR_HIP, "SIFT workspace allocation failed");
  ctx->sift_h = H; ctx->sift_w = W; ctx->sift_batch = B;
  ctx->sift_ws_layers = nl; ctx->sift_ws_sigma = ctx->sift_sigma;
  return GN_OK;
}
}  // namespace

// cv2.SIFT_create().detectAndCompute(gray, None): pose_node.py:122,230-232, twist_node.py:93,227-245 -- for a batch of
// equally sized images in one pass (every launch covers all images; the reference extracts one image per message)
int gn_sift_detect_and_compute_batch(gn_ctx* ctx, const uint8_t* gray, int B, int H, int W, int max_kpts,
                                     float* kpt_xysa, float* response, int32_t* octave, float* desc, int32_t* n_out_host, void* stream) {
  if (!ctx || !gray || !kpt_xysa || !desc || !n_out_host || B < 1 || B > 4096 || H < 16 || W < 16 || max_kpts < 1)
    return fail(ctx, GN_ERR_ARG, "bad gn_sift_detect_and_compute argument");
  GN_HIP(hipSetDevice(ctx->device));
  int rc = sift_prepare(ctx, B, H, W, max_kpts);
  if (rc != GN_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  SiftPyramid& py = ctx->sift_py;
  auto blur = [&](int o_in, const float* in, int o_out, float* out, int ki, float* dog = nullptr, int in_step = 1, float* half_scratch = nullptr) {
    sift_blur(B, py.oct[o_in].stride, py.oct[o_out].stride, in, ctx->sift_tmp, out, py.oct[o_out].w, py.oct[o_out].h, ctx->sift_dk + ctx->sift_koff[ki],
              (int)ctx->sift_kernels[ki].size(), ctx->knobs.sift_general_blur, s, dog, in_step, py.oct[o_in].w, half_scratch);
  };
  // createInitialImage: 2x bilinear, blur to sigma; then the Gaussian and DoG pyramids
  const int nl = py.n_layers, n_g = nl + 3;
  sift_base_blur(gray, B, H, W, py.oct[0].gauss[n_g - 1], ctx->sift_tmp, py.oct[0].gauss[0], py.oct[0].stride, ctx->sift_dk + ctx->sift_koff[0],
                 (int)ctx->sift_kernels[0].size(), ctx->knobs.sift_general_blur, ctx->sift_counts, s);   // (scratch = the last level, overwritten later); also zeroes the counters
  int ksize[kSiftMaxLayers + 3] = {};
  for (int i = 0; i < n_g; ++i) ksize[i] = (int)ctx->sift_kernels[i].size();
  const int o_tail = sift_tail_first(py, ksize, ctx->knobs.sift_general_blur);                     // octaves from here on: one single-workgroup launch per image
  for (int o = 0; o < o_tail; ++o) {
    const SiftOctave& oc = py.oct[o];
    // level 1 of octave o > 0 samples level nOctaveLayers of the octave above directly (its level 0 is never stored)
    if (o > 0) blur(o - 1, py.oct[o - 1].gauss[nl], o, oc.gauss[1], 1, oc.dog[0], 2, oc.gauss[0]);
    for (int i = o > 0 ? 2 : 1; i < n_g; ++i) blur(o, oc.gauss[i - 1], o, oc.gauss[i], i, oc.dog[i - 1]);   // row + column pass + DoG level in one launch
  }
  sift_tail(py, B, o_tail, ctx->sift_dk, ctx->sift_koff.data(), ksize, s);
  const float threshold = (float)(int)std::floor(0.5 * ctx->sift_contrast / nl * 255);
  SiftParams prm;
  prm.n_layers = nl; prm.contrast_thr = (float)ctx->sift_contrast; prm.edge_thr = (float)ctx->sift_edge; prm.edge1 = (float)(ctx->sift_edge + 1.0); prm.sigma = (float)ctx->sift_sigma;
  sift_find(py, B, threshold, ctx->sift_cand, ctx->sift_counts, ctx->sift_max_cand, s);
  // raw keypoints, their sorted copy and the final list of an image live back to back in one allocation
  const int max_raw = ctx->sift_raw_cap;
  sift_refine(py, prm, B, ctx->sift_cand, ctx->sift_counts, ctx->sift_max_cand, ctx->sift_kp, ctx->sift_kp_stride, max_raw, s);
  // sort / de-duplicate / rescale on the device, then descriptors for the final keypoints; one sync at the very end
  const int max_out = std::min(max_kpts, ctx->sift_max_kp);
  sift_sort_dedup(B, ctx->sift_kp, ctx->sift_kp_stride, ctx->sift_counts, max_raw, max_out, kpt_xysa, response, octave, max_kpts, s);
  sift_descriptors(py, B, ctx->sift_kp + 2 * max_raw, ctx->sift_kp_stride, ctx->sift_counts, max_out, desc, max_kpts, s);
  std::vector<int> counts_v;
  int* counts = reinterpret_cast<int*>(ctx->ovf_host + 16);       // pinned (every per-message transfer of the library is: gisnav_amd/upload.py has the reason)
  if (B > 1024) { counts_v.assign((size_t)B * 4, 0); counts = counts_v.data(); }
  GN_HIP(hipMemcpyAsync(counts, ctx->sift_counts, (size_t)B * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GN_HIP(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b) {
    if (counts[4 * b] > ctx->sift_max_cand) return fail(ctx, GN_ERR_ARG, "SIFT candidate buffer overflow (raise max_kpts)");
    if (counts[4 * b + 1] > max_raw) return fail(ctx, GN_ERR_ARG, "SIFT keypoint buffer overflow (raise max_kpts)");
    n_out_host[b] = counts[4 * b + 2];     // <= max_out: beyond it the strongest max_out by response were kept (k_sift_dedup_emit)
  }
  ctx->sift_totals.assign((size_t)B, 0);
  for (int b = 0; b < B; ++b) ctx->sift_totals[b] = counts[4 * b + 3];
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_sift_detect_and_compute(gn_ctx* ctx, const uint8_t* gray, int H, int W, int max_kpts,
                               float* kpt_xysa, float* response, int32_t* octave, float* desc, int32_t* n_out_host, void* stream) {
  return gn_sift_detect_and_compute_batch(ctx, gray, 1, H, W, max_kpts, kpt_xysa, response, octave, desc, n_out_host, stream);
}

// cv2.SIFT_create(nOctaveLayers, contrastThreshold, edgeThreshold, sigma): sticky host-side state, like gn_set_ransac
int gn_sift_set_params(gn_ctx* ctx, int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma) {
  if (!ctx) return GN_ERR_ARG;
  if (n_octave_layers < 1 || n_octave_layers > kSiftMaxLayers) return fail(ctx, GN_ERR_ARG, "gn_sift_set_params: n_octave_layers must be in 1..5");
  if (!std::isfinite(contrast_threshold) || contrast_threshold < 0.0) return fail(ctx, GN_ERR_ARG, "gn_sift_set_params: contrast_threshold must be finite and >= 0");
  if (!std::isfinite(edge_threshold) || !(edge_threshold > 0.0)) return fail(ctx, GN_ERR_ARG, "gn_sift_set_params: edge_threshold must be finite and > 0");
  if (!(sigma >= 1.0 && sigma <= 2.4)) return fail(ctx, GN_ERR_ARG, "gn_sift_set_params: sigma must be in [1.0, 2.4]");
  ctx->sift_layers = n_octave_layers; ctx->sift_contrast = contrast_threshold; ctx->sift_edge = edge_threshold; ctx->sift_sigma = sigma;
  return GN_OK;   // the workspace follows n_octave_layers / sigma at the next gn_sift_detect_and_compute(_batch) (sift_prepare)
}

int gn_sift_get_params(const gn_ctx* ctx, int* n_octave_layers, double* contrast_threshold, double* edge_threshold, double* sigma) {
  if (!ctx) return GN_ERR_ARG;
  if (n_octave_layers) *n_octave_layers = ctx->sift_layers;
  if (contrast_threshold) *contrast_threshold = ctx->sift_contrast;
  if (edge_threshold) *edge_threshold = ctx->sift_edge;
  if (sigma) *sigma = ctx->sift_sigma;
  return GN_OK;
}

int gn_sift_last_totals(gn_ctx* ctx, int B, int32_t* totals_host) {
  if (!ctx || !totals_host || B < 1 || (size_t)B > ctx->sift_totals.size()) return fail(ctx, GN_ERR_ARG, "gn_sift_last_totals: no SIFT call of that batch size yet");
  for (int b = 0; b < B; ++b) totals_host[b] = ctx->sift_totals[b];
  return GN_OK;
}

// ---- SuperPoint extractor -----------------------------------------------------------------------------------------------
namespace {
const char* const kSpNames[12] = {
    "encoder.conv_blocks.0.conv_a", "encoder.conv_blocks.0.conv_b", "encoder.conv_blocks.1.conv_a", "encoder.conv_blocks.1.conv_b",
    "encoder.conv_blocks.2.conv_a", "encoder.conv_blocks.2.conv_b", "encoder.conv_blocks.3.conv_a", "encoder.conv_blocks.3.conv_b",
    "keypoint_decoder.conv_score_a", "keypoint_decoder.conv_score_b", "descriptor_decoder.conv_descriptor_a", "descriptor_decoder.conv_descriptor_b"};
const int kSpShape[12][3] = {{64, 1, 9}, {64, 64, 9}, {64, 64, 9}, {64, 64, 9}, {128, 64, 9}, {128, 128, 9}, {128, 128, 9}, {128, 128, 9},
                             {256, 128, 9}, {65, 256, 1}, {256, 128, 9}, {256, 256, 1}};   // Cout, Cin, taps
}  // namespace

int gn_sp_load_tensor(gn_ctx* ctx, const char* name_c, const float* host, const int64_t* shape, int ndim) {
  if (!ctx || !name_c || !host || !shape) return fail(ctx, GN_ERR_ARG, "bad gn_sp_load_tensor argument");
  GN_HIP(hipSetDevice(ctx->device));
  const std::string name(name_c);
  for (int i = 0; i < 12; ++i) {
    const std::string base(kSpNames[i]);
    const int cout = kSpShape[i][0], cin = kSpShape[i][1], taps = kSpShape[i][2];
    const int k = taps == 9 ? 3 : 1;
    gn_ctx::SpConv& c = ctx->sp[i];
    c.cout = cout; c.cin = cin; c.taps = taps; c.cout_pad = ((cout + 63) / 64) * 64;
    if (name == base + ".weight") {
      if (ndim != 4 || shape[0] != cout || shape[1] != cin || shape[2] != k || shape[3] != k) return fail(ctx, GN_ERR_SHAPE, "shape mismatch for " + name);
      std::vector<float> frag;
      const float* src = host;
      if (i > 0) { frag.resize((size_t)c.cout_pad * taps * cin); sp_weight_fragments(host, cout, cin, taps, c.cout_pad, frag.data()); src = frag.data(); }
      const size_t n = i > 0 ? frag.size() : (size_t)cout * 9;       // the first layer (1 input channel) keeps [64][9] for the FMA kernel
      if (!c.wf) { void* q = nullptr; GN_HIP(hipMalloc(&q, n * sizeof(float))); ctx->sp_allocs.push_back(q); c.wf = (float*)q; }
      GN_HIP(hipMemcpy(c.wf, src, n * sizeof(float), hipMemcpyHostToDevice));
      if (i > 0 && ctx->precision == GN_PREC_F16X2_BF16_ATTN && cin % 16 == 0) {   // the split-fp16 convolution of this precision mode
        float mx = 0.f;
        for (size_t q = 0; q < (size_t)cout * cin * taps; ++q) mx = std::max(mx, fabsf(host[q]));
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) { frexpf(mx, &e); e = 13 - e; }      // max |w| * 2^e in [2^12, 2^13), as for the matcher's weights (build_planes)
        e = std::max(-60, std::min(60, e));
        std::vector<uint16_t> fh((size_t)2 * c.cout_pad * taps * cin);
        sp_weight_fragments_hm16(host, cout, cin, taps, c.cout_pad, ldexpf(1.0f, e), fh.data());
        if (!c.wfh) { void* q = nullptr; GN_HIP(hipMalloc(&q, fh.size() * sizeof(uint16_t))); ctx->sp_allocs.push_back(q); c.wfh = (uint16_t*)q; }
        GN_HIP(hipMemcpy(c.wfh, fh.data(), fh.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        c.acc_scale = ldexpf(1.0f, -e);
      }
      c.have_w = true;
      return GN_OK;
    }
    if (name == base + ".bias") {
      if (shape[0] != cout) return fail(ctx, GN_ERR_SHAPE, "shape mismatch for " + name);
      std::vector<float> pad((size_t)c.cout_pad, 0.f);
      memcpy(pad.data(), host, (size_t)cout * sizeof(float));
      if (!c.b) { void* q = nullptr; GN_HIP(hipMalloc(&q, pad.size() * sizeof(float))); ctx->sp_allocs.push_back(q); c.b = (float*)q; }
      GN_HIP(hipMemcpy(c.b, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
      c.have_b = true;
      return GN_OK;
    }
  }
  return fail(ctx, GN_ERR_NAME, "unknown SuperPoint tensor " + name);
}

int gn_sp_detect_and_describe(gn_ctx* ctx, const float* gray01, int B, int H, int W, int max_kpts,
                              float* kpt_xysa, float* score, float* desc, int32_t* n_out_host, void* stream) {
  if (!ctx || !gray01 || !kpt_xysa || !desc || !n_out_host || B < 1 || H < 16 || W < 16 || H % 8 || W % 8 || max_kpts < 1 || max_kpts > 2048)
    return fail(ctx, GN_ERR_ARG, "bad gn_sp_detect_and_describe argument (H, W multiples of 8; max_kpts <= 2048)");
  for (int i = 0; i < 12; ++i) if (!ctx->sp[i].have_w || !ctx->sp[i].have_b) return fail(ctx, GN_ERR_WEIGHTS, "SuperPoint weights not fully loaded");
  GN_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int chunk = std::min(B, 4);                       // images per pass: the full-resolution 64-channel maps are 0.5 GB per 1080p image
  const int h = H / 8, w = W / 8;
  const int cap = std::max(16384, H * W / 16);            // candidates after NMS (radius 4): at most one per ~5 x 5 neighbourhood in practice
  if (ctx->sp_h != H || ctx->sp_w != W || ctx->sp_chunk < chunk || ctx->sp_max < max_kpts) {
    for (void* p : ctx->sp_allocs) { bool is_weight = false; for (int i = 0; i < 12; ++i) is_weight |= (p == ctx->sp[i].wf || p == ctx->sp[i].b || p == ctx->sp[i].wfh); if (!is_weight) hipFree(p); }
    std::vector<void*> keep;
    for (void* p : ctx->sp_allocs) { for (int i = 0; i < 12; ++i) if (p == ctx->sp[i].wf || p == ctx->sp[i].b || p == ctx->sp[i].wfh) { keep.push_back(p); break; } }
    ctx->sp_allocs = keep;
    auto alloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) return nullptr; ctx->sp_allocs.push_back(p); return p; };
    const size_t full = (size_t)chunk * H * W;
    ctx->sp_x = (float*)alloc(full * 64 * sizeof(float));
    ctx->sp_y = (float*)alloc(full * 64 * sizeof(float));
    ctx->sp_z = (float*)alloc((size_t)chunk * h * w * 256 * sizeof(float));
    bool ok = ctx->sp_x && ctx->sp_y && ctx->sp_z;
    for (int k = 0; k < 3; ++k) { ctx->sp_maps[k] = (float*)alloc(full * sizeof(float)); ok = ok && ctx->sp_maps[k]; }
    ctx->sp_cand = (int*)alloc((size_t)chunk * cap * 2 * sizeof(int));      // (raster index, score bits) pairs
    ctx->sp_counts = (int*)alloc((size_t)chunk * 4 * sizeof(int));
    ctx->sp_index = (int*)alloc((size_t)chunk * 2048 * sizeof(int));
    if (!ok || !ctx->sp_cand || !ctx->sp_counts || !ctx->sp_index) return fail(ctx, GN_ERR_HIP, "SuperPoint workspace allocation failed");
    ctx->sp_h = H; ctx->sp_w = W; ctx->sp_chunk = chunk; ctx->sp_cap = cap; ctx->sp_max = max_kpts;
  }
  float *X = ctx->sp_x, *Y = ctx->sp_y, *Z = ctx->sp_z;
  // contexts of the f16x2 mode run the convolutions on split-fp16 operands (5 x the matrix-pipe rate of the exact f32 instruction,
  // the same accuracy class); an activation that does not fit fp16 raises ovf[1] and the pass is repeated on the exact path
  bool split = ctx->sp_split && ctx->sp[1].wfh != nullptr;
  // GN_SP_FP16: the activations of the layers above 1 / 8 resolution (layers 0 .. 6: 95 % of the extractor's bytes) travel as fp16;
  // layer 6 writes f32 again, the 1 / 8-resolution layers and the heads read and write f32 as in the other modes
  bool hm16_io = false;
  auto conv = [&](int i, const float* in, float* out, int n, int hh, int ww, int relu, int pool = 0) {
    if (ctx->sp_stop > 0 && i > ctx->sp_stop) return;      // developer knob 39: the layers behind layer sp_stop are skipped (their outputs are garbage)
    const bool hm = split && ctx->sp[i].wfh != nullptr;
    const bool half_io = hm && ctx->sp_split == 2;
    // split mode (round 5): every activation between the layers travels as hm16 records (k_sp_conv_s); the two head outputs stay f32
    // GN_SP_FP16 (k_sp_conv_h16): fp16 activations all the way to the two head outputs (the single-product staging rounds the same values to fp16 anyway)
    const int in_fmt = hm16_io ? 2 : (half_io && i >= 1 ? 1 : 0);
    const int out_fmt = hm16_io ? (i == 9 || i == 11 ? 0 : 2) : (half_io && i >= 1 && i != 9 && i != 11 ? 1 : 0);
    sp_conv(in, n, hh, ww, ctx->sp[i].cin, ctx->sp[i].wf, ctx->sp[i].b, out, ctx->sp[i].cout_pad, ctx->sp[i].taps, relu, s,
            hm ? ctx->sp[i].wfh : nullptr, ctx->sp[i].acc_scale, ctx->ovf_base + 8, pool, ctx->sp_split == 2, in_fmt, out_fmt,
            (ctx->sp_ts_layer == i && ctx->sp_ts != nullptr) ? ctx->sp_ts : nullptr);
  };
  std::vector<int> counts((size_t)chunk * 4);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int n = std::min(chunk, B - b0);
    if (split) GN_HIP(hipMemsetAsync(ctx->ovf_base + 8, 0, sizeof(unsigned int), s));
    // (k_sp_conv_s addresses a frame's activations with 32-bit buffer offsets, 0x80000000 marking a pixel outside the image: frames whose
    // full-resolution 64-channel map reaches 2 GB -- beyond 8 Mpixel -- stay on the round-2 kernels)
    hm16_io = split && ctx->sp_split == 1 && ctx->knobs.sp_conv_s != 0 && (size_t)H * W * 256 < 0x7fffffffull;
    for (int i = 1; i < 12; ++i) hm16_io = hm16_io && ctx->sp[i].wfh != nullptr;
    ctx->sp_enc_hm16 = hm16_io;
    ctx->sp_enc_fp16 = !hm16_io && split && ctx->sp_split == 2 && ctx->sp[7].wfh != nullptr;
    // round 6: in the split-fp16 mode the first convolution is evaluated inside the second one's halo staging (k_sp_conv_s16<., ., true>): its
    // full-resolution 64-channel map -- 0.53 GB of records per 1080p frame -- is neither written nor read; same bits (knob 46 = 0: two launches)
    const bool fuse1 = hm16_io && ctx->knobs.sp_fuse1 && ctx->knobs.sp_conv_s == 2 && ctx->sp[1].cin == 64 && ctx->sp[1].cout_pad == 64 && ctx->sp[1].taps == 9 && ctx->sp_stop != 1 &&
                       !(ctx->sp_ts_layer == 1 && ctx->sp_ts != nullptr);
    if (fuse1) {
      sp_conv_fused1(gray01 + (size_t)b0 * H * W, ctx->sp[0].wf, ctx->sp[0].b, n, H, W, ctx->sp[1].b, Y, ctx->sp[1].cout_pad, s, ctx->sp[1].wfh, ctx->sp[1].acc_scale, ctx->ovf_base + 8);
    } else {
    sp_conv1(gray01 + (size_t)b0 * H * W, ctx->sp[0].wf, ctx->sp[0].b, X, n, H, W, s,
             hm16_io ? 2 : (split && ctx->sp_split == 2 && ctx->sp[1].wfh != nullptr ? 1 : 0), ctx->ovf_base + 8);
    // the three 2 x 2 max-pools are fused into the epilogues of the convolutions in front of them (the full-resolution 64-channel map of
    // block 0 alone is 0.5 GB per 1080p image: writing it and reading it back was a quarter of the extractor's HBM traffic)
    conv(1, X, Y, n, H, W, 1, 1);                                                                   // block 0 -> Y [H/2][W/2][64]
    }
    conv(2, Y, X, n, H / 2, W / 2, 1);     conv(3, X, Y, n, H / 2, W / 2, 1, 1);                    // block 1 -> Y [H/4][W/4][64]
    conv(4, Y, X, n, H / 4, W / 4, 1);     conv(5, X, Y, n, H / 4, W / 4, 1, 1);                    // block 2 -> Y [H/8][W/8][128]
    conv(6, Y, X, n, h, w, 1);             conv(7, X, Y, n, h, w, 1);                               // block 3 -> Y = encoder output
    conv(8, Y, X, n, h, w, 1);             conv(9, X, Z, n, h, w, 0);                               // detector head: Z = logits [h][w][128 (65 used)]
    // developer knob 39 stopped the pass in front of the logits / the raw descriptor map: the stages that read them are skipped as well (they would
    // run on another pass's buffers), the keypoint count is 0 / the descriptor rows stay the caller's
    const bool tail_det = ctx->sp_stop <= 0 || ctx->sp_stop >= 9, tail_desc = ctx->sp_stop <= 0 || ctx->sp_stop >= 11;
    if (tail_det) {
    sp_scores(Z, ctx->sp[9].cout_pad, ctx->sp_maps[0], n, h, w, s);
    sp_nms(ctx->sp_maps[0], n, H, W, ctx->sp_maps[1], s);
    sp_select(ctx->sp_maps[1], n, H, W, 0.005f, 4, ctx->sp_cand, ctx->sp_counts, ctx->sp_cap, max_kpts,
              kpt_xysa + (size_t)b0 * max_kpts * 4, score ? score + (size_t)b0 * max_kpts : ctx->sp_maps[2], ctx->sp_index, max_kpts, ctx->knobs.sp_select_stream, s);
    }
    conv(10, Y, X, n, h, w, 1);            conv(11, X, Z, n, h, w, 0);                          // descriptor head: Z = raw descriptor map [h][w][256]
    if (tail_desc) sp_describe(Z, n, h, w, kpt_xysa + (size_t)b0 * max_kpts * 4, ctx->sp_counts, max_kpts, max_kpts, desc + (size_t)b0 * max_kpts * 256, s);
    std::fill(counts.begin(), counts.end(), 0);
    if (tail_det) GN_HIP(hipMemcpyAsync(counts.data(), ctx->sp_counts, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    unsigned int tripped = 0;
    if (split) GN_HIP(hipMemcpyAsync(&tripped, ctx->ovf_base + 8, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (split && tripped) { split = false; ++ctx->sp_split_trips; b0 -= chunk; continue; }   // repeat this pass with exact f32 convolutions
    for (int b = 0; b < n; ++b) {
      if (counts[4 * b] > ctx->sp_cap) return fail(ctx, GN_ERR_ARG, "SuperPoint candidate buffer overflow");
      n_out_host[b0 + b] = counts[4 * b + 1];
    }
  }
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int64_t gn_debug_read(gn_ctx* ctx, const char* name, void* host_out, int64_t max_bytes, void* stream) {
  if (!ctx || !name || !host_out) return GN_ERR_ARG;
  hipSetDevice(ctx->device);
  const size_t np = ctx->npad, B = ctx->max_batch;
  struct Ent { const char* n; const void* p; size_t count; };
  // the matcher's workspaces by their table names: the whole buffer in 4-byte words (nothing when it does not exist)
  Ent ws_ent = {nullptr, nullptr, 0};      // (no name: matches nothing)
  for_each_workspace(ctx->ws, (long long)np, (long long)np, false, [&](auto* p, long long per_pair, int, const char* n) {
    if (n && strcmp(n, name) == 0) ws_ent = {n, p, p ? B * (size_t)per_pair * sizeof(*p) / 4 : 0};
  });
  const Ent tab[] = {
      ws_ent,
      {"sp_enc", ctx->sp_y, ctx->sp_y ? (size_t)ctx->sp_chunk * (ctx->sp_h / 8) * (ctx->sp_w / 8) * 128 : 0},          // SuperPoint: encoder output of the last pass, NHWC
      {"sp_scores", ctx->sp_maps[0], ctx->sp_maps[0] ? (size_t)ctx->sp_chunk * ctx->sp_h * ctx->sp_w : 0},             // softmax + depth-to-space scores
      {"sp_nms", ctx->sp_maps[1], ctx->sp_maps[1] ? (size_t)ctx->sp_chunk * ctx->sp_h * ctx->sp_w : 0},                // after simple_nms
      {"sp_counts", ctx->sp_counts, ctx->sp_counts ? (size_t)ctx->sp_chunk * 4 : 0},                                    // per image: candidates, keypoints, candidates seen by the select
      {"sp_cand", ctx->sp_cand, ctx->sp_cand ? (size_t)ctx->sp_chunk * ctx->sp_cap * 2 : 0},                            // (raster index, score bits) pairs, [image][cap]
      {"sp_x", ctx->sp_x, ctx->sp_x ? (size_t)ctx->sp_chunk * ctx->sp_h * ctx->sp_w * 64 : 0},                         // raw words of the two activation buffers
      {"sp_y", ctx->sp_y, ctx->sp_y ? (size_t)ctx->sp_chunk * ctx->sp_h * ctx->sp_w * 64 : 0},
      {"sp_z", ctx->sp_z, ctx->sp_z ? (size_t)ctx->sp_chunk * (ctx->sp_h / 8) * (ctx->sp_w / 8) * 256 : 0},          // f32: the raw descriptor map [h][w][256] after a full pass, the logits [h][w][128] after a pass stopped at layer 9 (knob 39)
      {"sp_ts", ctx->sp_ts, ctx->sp_ts ? (size_t)8192 * 32 * 2 : 0}};                                                     // phase stamps (knob 35), int64 pairs of 4-byte words
  for (const Ent& e : tab)
    if (e.n && strcmp(e.n, name) == 0) {
      size_t count = e.count;
      if ((int64_t)(count * 4) > max_bytes) count = (size_t)max_bytes / 4;
      if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GN_ERR_HIP;
      if (hipMemcpy(host_out, e.p, count * 4, hipMemcpyDeviceToHost) != hipSuccess) return GN_ERR_HIP;
      if (strcmp(name, "sp_enc") == 0 && ctx->sp_enc_fp16) {
        // fp16 NHWC values (the first half of the bytes read) -> f32, back to front in place
        const uint16_t* hsrc = (const uint16_t*)host_out;
        float* dst = (float*)host_out;
        for (size_t g = count; g-- > 0;) dst[g] = (float)__builtin_bit_cast(_Float16, hsrc[g]);
      }
      if (strcmp(name, "sp_enc") == 0 && ctx->sp_enc_hm16) {
        // hm16 records (per 16 channels: 16 high halfs, 16 residual halfs) -> f32 values in channel order, in place
        uint16_t rec[32];
        for (size_t g = 0; g + 16 <= count; g += 16) {
          memcpy(rec, (const char*)host_out + g * 4, 64);
          float* dst = (float*)host_out + g;
          for (int c = 0; c < 16; ++c) dst[c] = (float)__builtin_bit_cast(_Float16, rec[c]) + (float)__builtin_bit_cast(_Float16, rec[16 + c]);
        }
      }
      return (int64_t)count;
    }
  if (strcmp(name, "sp_split_trips") == 0) {      // one int64: passes of this context that the split-fp16 guard repeated on the exact f32 convolutions
    if (max_bytes < 8) return GN_ERR_ARG;
    const long long trips = ctx->sp_split_trips;
    memcpy(host_out, &trips, 8);
    return 1;
  }
  if (strcmp(name, "e_idx") == 0) {
    size_t count = B * np * 2;
    if ((int64_t)(count * 8) > max_bytes) count = (size_t)max_bytes / 8;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GN_ERR_HIP;
    if (hipMemcpy(host_out, ctx->ws.e_idx, count * 8, hipMemcpyDeviceToHost) != hipSuccess) return GN_ERR_HIP;
    return (int64_t)count;
  }
  return fail(ctx, GN_ERR_NAME, std::string("unknown debug tensor ") + name);
}

int gn_debug_gemm(gn_ctx* ctx, int M, int N, int K, const float* A, const float* W, const float* bias, float* Y, void* stream) {
  if (!ctx || !A || !W || !Y || M % 128 || N % 128 || K % 32 || M < 128 || N < 128 || K < 32)
    return fail(ctx, GN_ERR_ARG, "gn_debug_gemm needs M,N multiples of 128 and K a multiple of 32");
  GN_HIP(hipSetDevice(ctx->device));
  GemmArgs g;
  memset(&g, 0, sizeof g);
  g.A = A; g.lda = K; g.K1 = K; g.W = W; g.ldw = K; g.bias = bias; g.Y = Y; g.ldy = N; g.M = M; g.N = N; g.K = K;
  g.acc_scale = 1.f;
  if (ctx->knobs.gemm_variant == 7) {   // k_gemm_p2: both operands as fp16 planes (W scaled by 2^(dbg_planes - 1) if dbg_planes > 0)
    
    const size_t na = (size_t)M * K, nw = (size_t)N * K;
    if (ctx->dbg_ap_n < na) { ctx->dbg_ap = nullptr; int rc = dalloc(ctx, &ctx->dbg_ap, 2 * na); if (rc != GN_OK) return rc; ctx->dbg_ap_n = na; }
    if (ctx->dbg_wp_n < nw) { ctx->dbg_wp = nullptr; int rc = dalloc(ctx, &ctx->dbg_wp, 3 * nw); if (rc != GN_OK) return rc; ctx->dbg_wp_n = nw; }
    const int e = ctx->dbg_planes > 0 ? ctx->dbg_planes - 1 : 0;
    if (!ctx->dbg_reuse) {
      launch_split_hm16(A, ctx->dbg_ap, M, K, 1.0f, (hipStream_t)stream);
      launch_split_hm16(W, ctx->dbg_wp, N, K, ldexpf(1.0f, e), (hipStream_t)stream);
    }
    g.Ap = ctx->dbg_ap; g.Wp = ctx->dbg_wp; g.acc_scale = ldexpf(1.0f, -e);
    if (ctx->dbg_out) {
      const size_t ny = (size_t)M * N;
      if (ctx->dbg_yp_n < ny) { ctx->dbg_yp = nullptr; int rc = dalloc(ctx, &ctx->dbg_yp, 2 * ny); if (rc != GN_OK) return rc; ctx->dbg_yp_n = ny; }
      g.Yp = ctx->dbg_yp; g.ldyp = N;
      if (ctx->dbg_out == 1) g.Y = nullptr;
    }
    launch_gemm_p2(bias ? EPI_BIAS : EPI_PLAIN, g, 1, (hipStream_t)stream, ctx->knobs);
    GN_HIP(hipGetLastError());
    return GN_OK;
  }
  if (ctx->dbg_planes) {
    const size_t n = (size_t)N * K;
    if (ctx->dbg_wp_n < n) { ctx->dbg_wp = nullptr; int rc = dalloc(ctx, &ctx->dbg_wp, 3 * n); if (rc != GN_OK) return rc; ctx->dbg_wp_n = n; }
    if (ctx->knobs.gemm_variant == 6 || ctx->knobs.gemm_variant >= 60) {   // fp16 planes of W * 2^(dbg_planes - 1)
      launch_split2_f16(W, ctx->dbg_wp, (long long)n, ldexpf(1.0f, ctx->dbg_planes - 1), (hipStream_t)stream);
      g.acc_scale = ldexpf(1.0f, 1 - ctx->dbg_planes);
    } else {
      launch_split3_bf16(W, ctx->dbg_wp, (long long)n, (hipStream_t)stream);
    }
    g.Wp = ctx->dbg_wp; g.wp_plane = (long long)n;
  }
  launch_gemm_f32(bias ? EPI_BIAS : EPI_PLAIN, g, 1, (hipStream_t)stream, ctx->knobs);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_debug_attention(gn_ctx* ctx, int BS, int npad, int cross, float qscale, const float* q, int ldq, const float* k, int ldk,
                       const float* v, int ldv, const int32_t* nkv, float* out, int ldo, void* stream) {
  if (!ctx || !q || !k || !v || !nkv || !out || npad % 128 || BS < 1 || (cross && (BS & 1)))
    return fail(ctx, GN_ERR_ARG, "bad gn_debug_attention argument");
  GN_HIP(hipSetDevice(ctx->device));
  AttnArgs a; a.ovf = nullptr;
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out = out; a.ldo = ldo;
  a.nvalid = nkv; a.npad = npad; a.cross = cross; a.qscale = qscale; a.BS = BS;
  a.qb = a.kb = a.vt = nullptr; a.ldqb = a.ldkb = 0; a.outp = nullptr; a.half_fmt = ctx->attn_f16; a.ncu = ctx->ncu;
  const long long cap = (long long)ctx->max_batch * 2 * ctx->npad;
  if (ctx->precision != GN_PREC_F32 && ctx->attn_f16 != 2 && ctx->knobs.attn_variant >= 1 && ctx->ws.qkb && ctx->ws.vtb && (long long)BS * npad <= cap) {
    // the production kernel (k_attn_bf16_v5) on the layouts the projection epilogues would have written
    launch_pack_attn_bf16(a, ctx->ws.qkb, ctx->ws.vtb, (hipStream_t)stream);
    a.qb = ctx->ws.qkb; a.kb = ctx->ws.qkb + kDim; a.ldqb = a.ldkb = 2 * kDim; a.vt = ctx->ws.vtb;
    ctx->knobs.attn_stamps = (ctx->knobs.attn_variant == 73 && ctx->ws.sim) ? reinterpret_cast<long long*>(ctx->ws.sim) : nullptr;
    attn_split(ctx, a);
    launch_attention_bf16_v2(a, (hipStream_t)stream, ctx->knobs);
  } else {
    attention(ctx, a, (hipStream_t)stream);
  }
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_debug_match_head(gn_ctx* ctx, int B, int np, const float* md, const float* ls, const int32_t* nvalid, int64_t* idx, float* score,
                        int32_t* n_match, void* stream) {
  if (!ctx || !md || !ls || !nvalid || !idx || !score || !n_match || B < 1 || B > ctx->max_batch || np < 128 || np % 128 || np > ctx->npad)
    return fail(ctx, GN_ERR_ARG, "gn_debug_match_head needs 1 <= B <= max_batch and np a multiple of 128, at most gn_kmax()");
  GN_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // the call's workspaces are laid out at np, and the fused head also writes the column values (gn_debug_read "colbest" / "col2")
  const Restore keep(ctx->npad_run, ctx->cal_cols);
  ctx->npad_run = np; ctx->cal_cols = true;
  const View w = view_of(ctx);
  const size_t T = (size_t)B * 2 * np;
  GN_HIP(hipMemcpyAsync(w.md, md, T * kDim * sizeof(float), hipMemcpyDeviceToDevice, s));
  GN_HIP(hipMemcpyAsync(w.ls, ls, T * sizeof(float), hipMemcpyDeviceToDevice, s));
  GN_HIP(hipMemcpyAsync(w.nvalid, nvalid, (size_t)B * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (ctx->planes_mode) {   // the hm16 rows the projection's epilogue writes; the guard word starts clear as k_extent leaves it
    launch_split_hm16(w.md, w.md_p, (long long)T, kDim, 1.0f, s);
    if (ctx->guard) GN_HIP(hipMemsetAsync(w.ovf, 0, sizeof(unsigned int), s));
  }
  ctx->n_ev = 0; ctx->launch_count = 0;
  const int rc = run_head(ctx, w, B, idx, score, n_match, false, s);
  if (rc != GN_OK) return rc;
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_sp_set_arithmetic(gn_ctx* ctx, int mode) {
  if (!ctx || mode < GN_SP_EXACT_F32 || mode > GN_SP_FP16) return GN_ERR_ARG;
  if (mode != GN_SP_EXACT_F32 && ctx->precision != GN_PREC_F16X2_BF16_ATTN) return fail(ctx, GN_ERR_ARG, "the fp16 SuperPoint arithmetic needs a context of the f16x2 precision");
  ctx->sp_split = mode;
  return GN_OK;
}

// knob values of timing-only ablations and rejected experiments that have been retired: refused, so that a stale script fails
// instead of timing the default kernel under their label
static bool retired_variant(int which, int value) {
  switch (which) {
    case 0: return (value >= 51 && value <= 57) || (value >= 61 && value <= 67);
    case 1: return (value >= 41 && value <= 46) || value == 48 || (value >= 51 && value <= 55) || value == 57 || value == 58 ||
                   value == 71 || value == 72 || value >= 1000;
    case 8: return value != 0 && value != 1;
    case 12: return value != 0 && value != 8 && value != 136;
    case 24: case 36: return true;            // SuperPoint's older single-product kernels and the 16-launch simple_nms
    case 34: return value != 0 && value != 2; // ... and its 3 x 3 k_sp_conv_s (1): the round-2 kernels (0) and the shipped form (2) live on
    case 42: return true;                     // lf_conv's cost model: it reaches nothing on a matcher context (gn_loftr_debug_set_variant)
    default: return false;
  }
}

int gn_debug_set_variant(gn_ctx* ctx, int which, int value) {
  if (!ctx || retired_variant(which, value)) return GN_ERR_ARG;
  if ((which == 1 && value == 73) || (which == 12 && (value & 8)) || (which == 15 && value) || (which == 16 && !value) || (which == 17 && value) || (which == 20 && value)) {   // these developer paths use the similarity buffer
    GN_HIP(hipSetDevice(ctx->device));
    const int rc = ensure_sim(ctx); if (rc != GN_OK) return rc;
  }
  if (which == 0) ctx->knobs.gemm_variant = value;
  else if (which == 1) ctx->knobs.attn_variant = value;
  else if (which == 2) ctx->dbg_planes = value;
  else if (which == 3) ctx->no_planes = value;
  else if (which == 4) ctx->stop_after = value;
  else if (which == 5) ctx->planes_mode = (value && ctx->ws.x_p) ? 1 : 0;
  else if (which == 6) ctx->dbg_reuse = value;
  else if (which == 7) ctx->dbg_out = value;
  else if (which == 10) ctx->ffn_fused = value;
  else if (which == 11) ctx->x_planes_only = value;
  else if (which == 8) ctx->knobs.p2_wide = value;
  else if (which == 9) ctx->dbg_vt_skip = value;
  else if (which == 12) ctx->knobs.ffn_stamps = value;
  else if (which == 13) ctx->ffn_fold = value;
  else if (which == 14) ctx->knobs.ffn_shape = value;
  else if (which == 15) ctx->pnp_stamps = value;
  else if (which == 16) ctx->head_fused = value;
  else if (which == 17) ctx->head_stamps = value;
  else if (which == 19) ctx->qkv_fused = value;
  else if (which == 20) ctx->qkv_stamps = value;
  else if (which == 21) ctx->sp_split = value;
  else if (which == 34) ctx->knobs.sp_conv_s = value;
  else if (which == 40) ctx->knobs.sp_select_stream = value;
  else if (which == 41) ctx->knobs.gemm_m64 = value;
  else if (which == 43) ctx->knobs.attn_f32_ks = value;
  else if (which == 44) ctx->knobs.gemm_r64 = value;
  else if (which == 46) ctx->knobs.sp_fuse1 = value;
  else if (which == 47) { ctx->fused_proj_pending = value == 0; }   // 1: skip the fused-projection self-check of the next forward call (profiling passes: its launches are set-up, not steps)
  else if (which == 39) ctx->sp_stop = value;
  else if (which == 35) {
    ctx->sp_ts_layer = value;
    if (value > 0 && ctx->sp_ts == nullptr) { void* q = nullptr; if (hipMalloc(&q, (size_t)8192 * 32 * sizeof(long long)) == hipSuccess) { ctx->sp_ts = (long long*)q; ctx->sp_allocs_dbg = q; } }
    if (ctx->sp_ts != nullptr) hipMemset(ctx->sp_ts, 0, (size_t)8192 * 32 * sizeof(long long));
  }
  else if (which == 23) ctx->attn_split = value;
  else if (which == 25) ctx->dbg_trip_group = value;
  else if (which == 26) ctx->sub_serial = value;
  else if (which == 27) { ctx->qkv_products = value == 3 ? 3 : 2; if (value == 1) ctx->qkv_set = 1; ctx->fused_proj_pending = true; }      // (1: as gn_set_qkv_products(1))
  else if (which == 28) ctx->ffn_compose = value;
  else if (which == 31) ctx->use_lists = value;
  else if (which == 32) ctx->qkv_in_tail = value ? 1 : 0;
  else if (which == 33) ctx->skinny = value;
  else if (which == 48) ctx->prep_fused = value ? 1 : 0;
  else if (which == 49) ctx->pnp_rounds = value ? 1 : 0;
  else if (which == 50) ctx->knobs.sift_general_blur = value ? 1 : 0;   // SIFT scale space through k_blur_row + k_blur_col only (the cost table of DESIGN.md 18)
  else if (which == 29) {   // CU shares for the sub-batch streams: takes effect for streams created afterwards
    GN_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 8; ++i) if (ctx->sub_s[i]) { hipStreamSynchronize(ctx->sub_s[i]); hipEventDestroy(ctx->ev_join[i]); hipStreamDestroy(ctx->sub_s[i]); ctx->sub_s[i] = nullptr; ctx->ev_join[i] = nullptr; }
    ctx->cu_mask_mode = value;
    if (ctx->n_sub > 1) { const int n = ctx->n_sub; ctx->n_sub = 1; return gn_set_substreams(ctx, n); }
  }
  else return GN_ERR_ARG;
  return GN_OK;
}

int gn_debug_epnp(gn_ctx* ctx, int n, const double* pws, const double* us, double* out, void* stream) {
  if (!ctx || n < 1 || !pws || !us || !out) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  launch_epnp_debug(pws, us, out, n, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_debug_lds_dma_probe(gn_ctx* ctx, const float* pattern, unsigned int* out, int blocks, int spin, void* stream) {
  if (!ctx || !pattern || !out || blocks < 1) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  launch_lds_dma_probe(pattern, out, blocks, spin, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_debug_mfma_probe(gn_ctx* ctx, int blocks, int iters, void* stream) {
  if (!ctx || blocks < 1 || iters == 0) return GN_ERR_ARG;
  GN_HIP(hipSetDevice(ctx->device));
  launch_mfma_probe(ctx->ws.ls, blocks, iters, (hipStream_t)stream);
  GN_HIP(hipGetLastError());
  return GN_OK;
}

int gn_set_kernel_timing(gn_ctx* ctx, int max_launches) {
  if (!ctx || max_launches < 0) return GN_ERR_ARG;
  hipSetDevice(ctx->device);
  while ((int)ctx->kflops.size() < max_launches) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return GN_ERR_HIP;
    ctx->kev.push_back(a); ctx->kev.push_back(b); ctx->kflops.push_back(0.0); ctx->kbytes.push_back(0.0); ctx->kclass.push_back(0); ctx->kname.push_back("");
  }
  ctx->ktiming = max_launches > 0;
  ctx->kused = 0;
  return GN_OK;
}

int gn_get_kernel_stats(gn_ctx* ctx, int kernel_class, double* out3) {
  if (!ctx || !out3 || kernel_class < 0 || kernel_class > 1) return GN_ERR_ARG;
  hipSetDevice(ctx->device);
  double ms = 0.0, fl = 0.0, n = 0.0;
  for (size_t i = 0; i < ctx->kused; ++i) {
    if (hipEventSynchronize(ctx->kev[2 * i + 1]) != hipSuccess) return GN_ERR_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, ctx->kev[2 * i], ctx->kev[2 * i + 1]) != hipSuccess) return GN_ERR_HIP;
    if (ctx->kclass[i] != kernel_class) continue;
    ms += t; fl += ctx->kflops[i]; n += 1.0;
  }
  out3[0] = n; out3[1] = ms; out3[2] = fl;
  return GN_OK;
}

// Per-kernel table of the recorded launches as a JSON array (HIP-event time on the launch stream, algorithmic flops and bytes):
// [{"name": "k_ffn_fused<0, true>", "launches": n, "ms": total, "flops": total, "bytes": total}, ...].  Names are the ones
// rocprofv3's kernel_stats rows carry (namespace prefix and argument list stripped).  Returns the length written, or a negative status.
int gn_get_kernel_table(gn_ctx* ctx, char* json, int capacity) {
  if (!ctx || !json || capacity < 64) return GN_ERR_ARG;
  hipSetDevice(ctx->device);
  std::map<std::string, std::vector<double>> tab;   // name -> {launches, ms, flops, bytes}
  for (size_t i = 0; i < ctx->kused; ++i) {
    if (hipEventSynchronize(ctx->kev[2 * i + 1]) != hipSuccess) return GN_ERR_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, ctx->kev[2 * i], ctx->kev[2 * i + 1]) != hipSuccess) return GN_ERR_HIP;
    std::vector<double>& v = tab[ctx->kname[i] ? ctx->kname[i] : "?"];
    if (v.empty()) v.assign(4, 0.0);
    v[0] += 1.0; v[1] += t; v[2] += ctx->kflops[i]; v[3] += ctx->kbytes[i];
  }
  std::string out = "[";
  bool first = true;
  for (const auto& kv : tab) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s{\"name\": \"%s\", \"launches\": %.0f, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}", first ? "" : ", ",
             kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2], kv.second[3]);
    out += buf; first = false;
  }
  out += "]";
  if ((int)out.size() + 1 > capacity) return GN_ERR_ARG;
  memcpy(json, out.c_str(), out.size() + 1);
  return (int)out.size();
}

int gn_get_kernel_bytes(gn_ctx* ctx, int kernel_class, double* out1) {
  if (!ctx || !out1 || kernel_class < 0 || kernel_class > 1) return GN_ERR_ARG;
  double by = 0.0;
  for (size_t i = 0; i < ctx->kused; ++i)
    if (ctx->kclass[i] == kernel_class) by += ctx->kbytes[i];
  *out1 = by;
  return GN_OK;
}

int gn_set_stage_timing(gn_ctx* ctx, int enable) {
  if (!ctx) return GN_ERR_ARG;
  ctx->timing = enable != 0;
  ctx->n_ev = 0;
  return GN_OK;
}

int gn_get_stage_ms(gn_ctx* ctx, float* host_ms, int max_stages) {
  if (!ctx || !host_ms) return GN_ERR_ARG;
  hipSetDevice(ctx->device);
  for (int i = 0; i < ST_COUNT; ++i) ctx->stage_ms[i] = 0.f;
  if (ctx->n_ev > 0) {
    if (hipEventSynchronize(ctx->ev[2 * (ctx->n_ev - 1) + 1]) != hipSuccess) return GN_ERR_HIP;
    for (int i = 0; i < ctx->n_ev; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]) == hipSuccess) ctx->stage_ms[ctx->ev_stage[i]] += ms;
    }
  }
  const int n = max_stages < ST_COUNT ? max_stages : (int)ST_COUNT;
  for (int i = 0; i < n; ++i) host_ms[i] = ctx->stage_ms[i];
  return n;
}

}  // extern "C"
