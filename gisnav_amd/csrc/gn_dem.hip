// Elevation rasters beyond 8 bits (DESIGN.md "Elevation rasters: element types, scale, offset, voids"): the lift of gn_gather_points for a
// DEM of uint8 / uint16 / int16 / float32 elements under an affine map, and the removal of matches whose reference keypoint lands on a void cell.
//
//   k_gather_dem<T>         k_gather (gn_match_head.hip) with a typed load and z = (float)(raw * scale + offset): same grid, one thread per match
//   k_gather_dem_voids<T>   one workgroup per pair: classify every row, compact idx / score in place and write mkp_q / obj of the rows kept
//
// The cell is chosen as k_gather chooses it (floorf, clamped to the raster).  The product and the sum of the lift are f64, rounded once each
// (__dmul_rn / __dadd_rn: the file is compiled with contraction on), then rounded to f32 -- exact for every integer type at scale 1, offset 0.
#include "gn_common.h"

namespace gn {

namespace {
constexpr int kVoidThreads = 1024, kVoidWaves = kVoidThreads / 64;

struct MatchRow { float qx, qy, rx, ry; size_t cell; };

__device__ __forceinline__ MatchRow match_row(const GatherArgs& a, int b, int iq, int ir) {
  const int w = a.kpt_format == GN_KPT_LAF ? 6 : a.kpt_format == GN_KPT_RECORD ? kRecordFloats : 4;
  const int xo = a.kpt_format == GN_KPT_LAF ? 2 : 0, yo = a.kpt_format == GN_KPT_LAF ? 5 : 1;
  const float* kq = a.kpt_q + ((size_t)b * a.stride_q + iq) * w;
  const float* kr = a.kpt_r + ((size_t)b * a.stride_r + ir) * w;
  MatchRow r;
  r.qx = kq[xo]; r.qy = kq[yo]; r.rx = kr[xo]; r.ry = kr[yo];
  int xi = (int)floorf(r.rx), yi = (int)floorf(r.ry);      // x, y = floor(mkp_ref).astype(int); z = elevation[y, x]
  xi = min(max(xi, 0), a.W - 1); yi = min(max(yi, 0), a.H - 1);
  r.cell = ((size_t)b * a.H + yi) * a.W + xi;              // in ELEMENTS of the raster's type
  return r;
}

template <typename T> __device__ __forceinline__ float lift(T raw, const DemFormat& f) {
  return (float)__dadd_rn(__dmul_rn((double)raw, f.scale), f.offset);
}

template <typename T> __device__ __forceinline__ bool is_void(T raw, const DemFormat& f) {
  if (sizeof(T) == 4 && !isfinite((float)raw)) return true;      // float32 only: NaN and +-Inf cells (nodata = NaN never compares equal: those alone)
  return (double)raw == f.nodata;
}

// grid (kmax/256, B)
template <typename T>
__global__ __launch_bounds__(256) void k_gather_dem(DemGatherArgs a) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.g.n_match[b]) return;
  const size_t o = (size_t)b * a.g.kmax + k;
  const MatchRow r = match_row(a.g, b, (int)a.g.idx[2 * o], (int)a.g.idx[2 * o + 1]);
  const float z = lift(reinterpret_cast<const T*>(a.g.dem)[r.cell], a.f);
  a.g.mkp_q[2 * o] = r.qx; a.g.mkp_q[2 * o + 1] = r.qy;
  a.g.obj[3 * o] = r.rx; a.g.obj[3 * o + 1] = r.ry; a.g.obj[3 * o + 2] = z;
}

// grid (B): the rows of pair b in ascending chunks of kVoidThreads.  A row's destination is never behind its source, and a chunk's stores land
// in rows that this chunk or an earlier one has already loaded (the barrier between a chunk's loads and its stores), so idx and score are
// compacted in place -- the argument of k_prune (gn_prune.hip).  Stable: ballot + popcount prefix over the waves + the running base.
template <typename T>
__global__ __launch_bounds__(kVoidThreads) void k_gather_dem_voids(DemGatherArgs a) {
  __shared__ int wcount[kVoidWaves];
  __shared__ int base_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(a.n_match[b], 0), a.g.kmax);
  const size_t o0 = (size_t)b * a.g.kmax;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += kVoidThreads) {
    const int k = c0 + tid;
    const bool active = k < n;
    int64_t iq = 0, ir = 0; float sc = 0.f, z = 0.f; bool keep = false;
    MatchRow r = {0.f, 0.f, 0.f, 0.f, 0};
    if (active) {
      iq = a.idx[2 * (o0 + k)]; ir = a.idx[2 * (o0 + k) + 1];
      if (a.score != nullptr) sc = a.score[o0 + k];
      r = match_row(a.g, b, (int)iq, (int)ir);
      const T raw = reinterpret_cast<const T*>(a.g.dem)[r.cell];
      keep = !is_void(raw, a.f);
      z = lift(raw, a.f);
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();                        // every load of the chunk is behind this barrier, every store in front of it
    int off = base_s, tot = 0;
    for (int w = 0; w < kVoidWaves; ++w) { const int c = wcount[w]; if (w < wave) off += c; tot += c; }
    if (keep) {
      const size_t d = o0 + off + before;
      a.idx[2 * d] = iq; a.idx[2 * d + 1] = ir;
      if (a.score != nullptr) a.score[d] = sc;
      a.g.mkp_q[2 * d] = r.qx; a.g.mkp_q[2 * d + 1] = r.qy;
      a.g.obj[3 * d] = r.rx; a.g.obj[3 * d + 1] = r.ry; a.g.obj[3 * d + 2] = z;
    }
    __syncthreads();
    if (tid == 0) base_s = off + tot;       // (thread 0: wave 0, so off is the base the chunk started from)
    __syncthreads();
  }
  if (tid == kVoidThreads - 1) {
    const int kept = base_s;
    a.n_match[b] = kept;
    if (a.dropped != nullptr) a.dropped[b] = n - kept;
  }
}

template <typename T> void launch_typed(const DemGatherArgs& a, hipStream_t s) {
  if (a.f.has_nodata) {
    hipLaunchKernelGGL(k_gather_dem_voids<T>, dim3(a.g.B), dim3(kVoidThreads), 0, s, a);
    g_last_kernel = "k_gather_dem_voids";
  } else {
    hipLaunchKernelGGL(k_gather_dem<T>, dim3((a.g.kmax + 255) / 256, a.g.B), dim3(256), 0, s, a);
    g_last_kernel = "k_gather_dem";
  }
}
}  // namespace

void launch_gather_dem(const DemGatherArgs& a, hipStream_t s) {
  switch (a.f.type) {
    case GN_DEM_U8: launch_typed<uint8_t>(a, s); break;
    case GN_DEM_U16: launch_typed<uint16_t>(a, s); break;
    case GN_DEM_I16: launch_typed<int16_t>(a, s); break;
    default: launch_typed<float>(a, s); break;
  }
}

}  // namespace gn
