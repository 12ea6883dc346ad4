// LightGlue point pruning (width_confidence > 0, early exit off): gn_set_width_pruning.
//
//   k_prune_init    ind = arange(n), prune = ones(n) (zeros past a slot's count) at the start of a call
//   k_prune_z       after the cross block of layer i < n_layers - 1, for every slot whose CURRENT count is > min_kpts: z = matchability_i(x) per row -- one
//                   wave per row over the whole grid, the lane / butterfly summation order of k_matchability (gn_prep.hip); in the modes whose residual
//                   stream lives in hm16 rows only, from h + m -- and the keep flag sigmoid(z) > 1 - width_confidence in f32
//   k_prune         one workgroup per (pair, side) slot (a slot at or under min_kpts returns at once):
//                     - block-wide exclusive scan of the keep flags, 1024 rows at a time with a running base: the stable destination row of every
//                       kept row; a layer that keeps every row only counts (prune += 1) and leaves
//                     - the rows move IN PLACE: destination <= source, so this one workgroup walks its slot in ascending chunks of 64 rows (four
//                       per wave) with a barrier between a chunk's loads and its stores -- a store of chunk k lands at or before chunk k's own
//                       rows, which every wave has read by then, and no later chunk is ever a destination of an earlier one.  Moved per row: the
//                       residual row in every form the mode keeps (f32 x, hm16 x_p: 1 KB each), cos_t / sin_t, the row's 16 float4 of the
//                       rot4 table ([fg][t], rot_stride apart) and ind; prune[ind] += 1 for the kept rows
//                     - the vacated rows [n_new, n_old) are reset to what k_prep leaves in padding (zeros, cos 1, sin 0), nvalid[slot] = n_new
//   k_unprune_idx   maps the match head's (query, reference) rows back through ind to original keypoint indices, before anything reads the list
//
// Semantics restated from the public kornia 0.7.2 / cvg LightGlue source (`_forward`: pruning after every layer but the last, per side, only while the
// side holds more than the pruning threshold; with early exit off there is no token-confidence term).  kornia is not part of this tree's oracle
// environment, so parity with it is UNPINNED.  The threshold (min_kpts, default 1536 = kornia's `pruning_keypoint_thresholds` entry for CUDA with
// flash attention; 1024 without) is recalled from that source, not verified.  This build's own: a side left with no keypoint makes the pair report
// zero matches (kornia would raise in a max over an empty dimension).  A side left with one keypoint runs on, as in kornia: the match head applies
// kornia's fewer-than-two rule (_no_match) to the call's INPUT counts (HeadArgs::n_in).
#include "gn_common.h"

namespace gn {

namespace {
constexpr int kPruneThreads = 1024, kPruneWaves = kPruneThreads / 64, kPruneRows = 4;

__device__ inline float prune_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void k_prune_init(int32_t* ind, int32_t* prune, int32_t* n_in, const int32_t* nvalid, int npad) {
  const int bs = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= npad) return;
  if (t == 0) n_in[bs] = nvalid[bs];           // the input count, for the match head's no-match rule
  ind[(size_t)bs * npad + t] = t;
  prune[(size_t)bs * npad + t] = t < nvalid[bs] ? 1 : 0;
}

// keep flags of every row of every slot that is up for pruning: one wave per row, the whole grid in parallel
__global__ __launch_bounds__(256) void k_prune_z(PruneArgs a) {
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  const int slot = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = min(max(a.nvalid[slot], 0), a.npad);
  if (n <= a.min_kpts || i >= n) return;
  const size_t t = (size_t)slot * a.npad + i;
  const float4 ww = *reinterpret_cast<const float4*>(a.w + lane * 4);
  float4 v;
  if (a.z_from_planes) {
    const uint16_t* q = a.xp + hm16_off(t, kDim, lane * 4);
    const f16x4 h = *reinterpret_cast<const f16x4*>(q), m = *reinterpret_cast<const f16x4*>(q + 16);
    v.x = (float)h.x + (float)m.x; v.y = (float)h.y + (float)m.y; v.z = (float)h.z + (float)m.z; v.w = (float)h.w + (float)m.w;
  } else {
    v = *reinterpret_cast<const float4*>(a.x + t * kDim + lane * 4);
  }
  const float z = prune_wave_sum(v.x * ww.x + v.y * ww.y + v.z * ww.z + v.w * ww.w) + a.b[0];
  const float sg = 1.0f / (1.0f + expf(-z));
  if (lane == 0) { a.dst[t] = sg > a.thresh ? 1 : 0; if (a.z != nullptr) a.z[t] = z; }
}

__global__ __launch_bounds__(kPruneThreads) void k_prune(PruneArgs a) {
  __shared__ int sc[kPruneThreads];
  __shared__ int base_s;
  const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(a.nvalid[slot], 0), a.npad);
  if (n <= a.min_kpts) {                      // (uniform over the workgroup)
    if (tid == 0 && a.counts != nullptr) a.counts[slot * kMaxLayers + a.layer] = n;
    return;
  }
  const size_t t0 = (size_t)slot * a.npad;
  int32_t* const dst = a.dst + t0;            // k_prune_z has left the keep flags here
  int32_t* const ind = a.ind + t0;
  if (tid == 0) base_s = 0;
  __syncthreads();

  // 2. destination rows
  for (int c0 = 0; c0 < n; c0 += kPruneThreads) {
    const int i = c0 + tid;
    const int k = i < n ? dst[i] : 0;
    sc[tid] = k;
    __syncthreads();
    for (int d = 1; d < kPruneThreads; d <<= 1) {
      const int v = tid >= d ? sc[tid - d] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    if (i < n) dst[i] = k ? base_s + sc[tid] - k : -1;
    __syncthreads();
    if (tid == kPruneThreads - 1) base_s += sc[kPruneThreads - 1];
    __syncthreads();
  }
  const int n_new = base_s;
  if (n_new == n) {                           // the layer fired and kept every row: nothing moves
    for (int i = tid; i < n; i += kPruneThreads) a.prune[t0 + ind[i]] += 1;
    if (tid == 0 && a.counts != nullptr) a.counts[slot * kMaxLayers + a.layer] = n;
    return;
  }

  // 3. in-place compaction, ascending chunks of kPruneRows rows per wave
  for (int c0 = 0; c0 < n; c0 += kPruneWaves * kPruneRows) {
    int d[kPruneRows], id[kPruneRows];
    float4 vx[kPruneRows]; uint4 vp[kPruneRows]; float cs[kPruneRows]; f32x4 r4[kPruneRows];
#pragma unroll
    for (int j = 0; j < kPruneRows; ++j) {
      const int i = c0 + wave * kPruneRows + j;
      d[j] = i < n ? dst[i] : -1;
      id[j] = d[j] >= 0 ? ind[i] : 0;
      vx[j] = float4{0.f, 0.f, 0.f, 0.f}; vp[j] = uint4{0u, 0u, 0u, 0u}; cs[j] = 0.f; r4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (d[j] >= 0 && d[j] != i) {
        const size_t t = t0 + i;
        if (a.x != nullptr) vx[j] = *reinterpret_cast<const float4*>(a.x + t * kDim + lane * 4);
        if (a.xp != nullptr) vp[j] = *reinterpret_cast<const uint4*>(a.xp + t * (2 * kDim) + lane * 8);
        cs[j] = lane < kFreq ? a.cos_t[t * kFreq + lane] : a.sin_t[t * kFreq + lane - kFreq];
        if (a.rot4 != nullptr && lane < kFreq / 2) r4[j] = reinterpret_cast<const f32x4*>(a.rot4)[(size_t)lane * a.rot_stride + t];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPruneRows; ++j) {
      const int i = c0 + wave * kPruneRows + j;
      if (d[j] < 0) continue;
      if (lane == 0) { a.prune[t0 + id[j]] += 1; ind[d[j]] = id[j]; }
      if (d[j] != i) {
        const size_t t = t0 + d[j];
        if (a.x != nullptr) *reinterpret_cast<float4*>(a.x + t * kDim + lane * 4) = vx[j];
        if (a.xp != nullptr) *reinterpret_cast<uint4*>(a.xp + t * (2 * kDim) + lane * 8) = vp[j];
        if (lane < kFreq) a.cos_t[t * kFreq + lane] = cs[j]; else a.sin_t[t * kFreq + lane - kFreq] = cs[j];
        if (a.rot4 != nullptr && lane < kFreq / 2) reinterpret_cast<f32x4*>(a.rot4)[(size_t)lane * a.rot_stride + t] = r4[j];
      }
    }
  }
  __syncthreads();

  // the vacated rows: what k_prep leaves in padding
  for (int i = n_new + wave; i < n; i += kPruneWaves) {
    const size_t t = t0 + i;
    if (a.x != nullptr) *reinterpret_cast<float4*>(a.x + t * kDim + lane * 4) = float4{0.f, 0.f, 0.f, 0.f};
    if (a.xp != nullptr) *reinterpret_cast<uint4*>(a.xp + t * (2 * kDim) + lane * 8) = uint4{0u, 0u, 0u, 0u};
    if (lane < kFreq) a.cos_t[t * kFreq + lane] = 1.f; else a.sin_t[t * kFreq + lane - kFreq] = 0.f;
    if (a.rot4 != nullptr && lane < kFreq / 2) reinterpret_cast<f32x4*>(a.rot4)[(size_t)lane * a.rot_stride + t] = f32x4{1.f, 1.f, 0.f, 0.f};
    if (lane == 0) ind[i] = i;
  }
  if (tid == 0) {
    a.nvalid[slot] = n_new;
    if (a.counts != nullptr) a.counts[slot * kMaxLayers + a.layer] = n_new;
  }
}

__global__ __launch_bounds__(256) void k_unprune_idx(int64_t* idx, const int32_t* n_match, const int32_t* ind, int npad, int kmax) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= min(n_match[b], kmax)) return;
  int64_t* p = idx + ((size_t)b * kmax + k) * 2;
  const int64_t q = p[0], r = p[1];
  if (q >= 0 && q < npad) p[0] = ind[(size_t)(2 * b) * npad + q];
  if (r >= 0 && r < npad) p[1] = ind[(size_t)(2 * b + 1) * npad + r];
}
}  // namespace

void launch_prune_init(int32_t* ind, int32_t* prune, int32_t* n_in, const int32_t* nvalid, int BS, int npad, hipStream_t s) {
  hipLaunchKernelGGL(k_prune_init, dim3((npad + 255) / 256, BS), dim3(256), 0, s, ind, prune, n_in, nvalid, npad);
  g_last_kernel = "k_prune_init";
}
void launch_prune(const PruneArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_prune_z, dim3(a.npad / 4, a.BS), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_prune, dim3(a.BS), dim3(kPruneThreads), 0, s, a);
  g_last_kernel = "k_prune";
}
void launch_unprune_idx(int64_t* idx, const int32_t* n_match, const int32_t* ind, int B, int npad, int kmax, hipStream_t s) {
  hipLaunchKernelGGL(k_unprune_idx, dim3((kmax + 255) / 256, B), dim3(256), 0, s, idx, n_match, ind, npad, kmax);
  g_last_kernel = "k_unprune_idx";
}

}  // namespace gn
