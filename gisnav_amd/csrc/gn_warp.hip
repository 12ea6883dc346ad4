// Reference-raster preparation of GISNav's StereoNode: BGR -> gray, stack with the DEM, rotate
// about the centre and centre-crop to the camera frame -- ros/gisnav/gisnav/core/stereo_node.py:229-262, 292-335
// (`cv2.cvtColor(BGR2GRAY)`, `cv2.getRotationMatrix2D`, `cv2.warpAffine`, numpy crop).
//
// One thread per OUTPUT (cropped) pixel; only the cropped window of the rotated image is ever computed.  The
// arithmetic is OpenCV's fixed-point path restated exactly (oracle/stereo_warp.py): source coordinates in 1/32 pixel
// from `cvRound` of f64 products (no FMA contraction: __dmul_rn / __dadd_rn), 15-bit bilinear weights, taps outside the
// source read 0, (sum + 2^14) >> 15.  HBM-bound byte work: 2 B written and <= 16 B gathered per pixel.
#include "gn_common.h"

namespace gn {

namespace {
__device__ __forceinline__ int gray_of(const uint8_t* p) {   // RGB2Gray<uchar>: B, G, R interleaved
  return (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14;
}

template <bool FUSED_GRAY>
__global__ __launch_bounds__(256) void k_rotate_crop(WarpArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.crop_w || y >= a.crop_h) return;
  const double xf = (double)(x + a.dx), yf = (double)(y + a.dy);
  // WarpAffineInvoker: adelta / bdelta / X0 / Y0, AB_BITS = 10, round_delta = 16
  const long long ad = (long long)rint(__dmul_rn(__dmul_rn(a.M[0], xf), 1024.0));
  const long long bd = (long long)rint(__dmul_rn(__dmul_rn(a.M[3], xf), 1024.0));
  const long long X0 = (long long)rint(__dmul_rn(__dadd_rn(__dmul_rn(a.M[1], yf), a.M[2]), 1024.0)) + 16;
  const long long Y0 = (long long)rint(__dmul_rn(__dadd_rn(__dmul_rn(a.M[4], yf), a.M[5]), 1024.0)) + 16;
  const long long X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
  long long sxl = X >> 5, syl = Y >> 5;
  sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);     // saturate_cast<short>
  syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
  const int sx = (int)sxl, sy = (int)syl, fx = (int)(X & 31), fy = (int)(Y & 31);
  int w[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
  if (fx == 0 && fy == 0) { w[0] = 32767; w[3] = 1; }            // BilinearTab_i[0]: 32768 saturates to short, compensated on tap 3
  int acc0 = 0, acc1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = sx + (k & 1), yy = sy + (k >> 1);
    if (xx >= 0 && xx < a.W && yy >= 0 && yy < a.H) {            // BORDER_CONSTANT, value 0
      const size_t p = (size_t)yy * a.W + xx;
      if (FUSED_GRAY) { acc0 += gray_of(a.src0 + 3 * p) * w[k]; acc1 += a.src1[p] * w[k]; }
      else { acc0 += a.src0[2 * p] * w[k]; acc1 += a.src0[2 * p + 1] * w[k]; }
    }
  }
  const int v0 = min(max((acc0 + (1 << 14)) >> 15, 0), 255), v1 = min(max((acc1 + (1 << 14)) >> 15, 0), 255);
  const size_t o = (size_t)y * a.crop_w + x;
  if (a.out1 != nullptr) { a.out0[o] = (uint8_t)v0; a.out1[o] = (uint8_t)v1; }
  else { a.out0[2 * o] = (uint8_t)v0; a.out0[2 * o + 1] = (uint8_t)v1; }
}
// The DEM channel of k_rotate_crop_dem.  uint8_t: the fixed-point form above, bit for bit.  Every other element type: the float form
// (DESIGN.md "Elevation rasters"): f32 weights (32 - fx)(32 - fy) / 1024 ... (exact, no special case at (0, 0)),
// v = ((t0 w0 + t1 w1) + t2 w2) + t3 w3 with every product and sum rounded to f32, taps outside the source read 0; integer outputs are
// rint (half to even) saturated to the type.  VOIDS: the output cell is the void value when a tap of non-zero weight is void or outside.
template <typename T> struct Blend {
  float v = 0.f, t[4] = {0.f, 0.f, 0.f, 0.f};
  __device__ __forceinline__ void tap(int k, T raw, int, bool live) { t[k] = live ? (float)raw : 0.f; }      // a tap of zero weight reads 0: a non-finite cell under it does not spread
  __device__ __forceinline__ T result(int fx, int fy) {
    const float w0 = (float)((32 - fx) * (32 - fy)) * (1.f / 1024.f), w1 = (float)(fx * (32 - fy)) * (1.f / 1024.f);
    const float w2 = (float)((32 - fx) * fy) * (1.f / 1024.f), w3 = (float)(fx * fy) * (1.f / 1024.f);
    v = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(t[0], w0), __fmul_rn(t[1], w1)), __fmul_rn(t[2], w2)), __fmul_rn(t[3], w3));
    if (sizeof(T) == 4) return (T)v;
    const float lo = sizeof(T) == 2 && (T)(-1) < (T)0 ? -32768.f : 0.f, hi = (T)(-1) < (T)0 ? 32767.f : 65535.f;
    const float r = rintf(v);
    return (T)(int)(r < lo ? lo : (r > hi ? hi : r));      // (a NaN tap of an integer raster cannot occur)
  }
};
template <> struct Blend<uint8_t> {
  int acc = 0;
  __device__ __forceinline__ void tap(int, uint8_t raw, int w, bool) { acc += raw * w; }
  __device__ __forceinline__ uint8_t result(int, int) { return (uint8_t)min(max((acc + (1 << 14)) >> 15, 0), 255); }
};

template <typename T> __device__ __forceinline__ bool warp_void(T raw, double nodata) {
  if (sizeof(T) == 4 && !isfinite((float)raw)) return true;
  return (double)raw == nodata;
}

template <typename T, bool VOIDS>
__global__ __launch_bounds__(256) void k_rotate_crop_dem(DemWarpArgs d) {
  const WarpArgs& a = d.w;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.crop_w || y >= a.crop_h) return;
  const double xf = (double)(x + a.dx), yf = (double)(y + a.dy);
  const long long ad = (long long)rint(__dmul_rn(__dmul_rn(a.M[0], xf), 1024.0));
  const long long bd = (long long)rint(__dmul_rn(__dmul_rn(a.M[3], xf), 1024.0));
  const long long X0 = (long long)rint(__dmul_rn(__dadd_rn(__dmul_rn(a.M[1], yf), a.M[2]), 1024.0)) + 16;
  const long long Y0 = (long long)rint(__dmul_rn(__dadd_rn(__dmul_rn(a.M[4], yf), a.M[5]), 1024.0)) + 16;
  const long long X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
  long long sxl = X >> 5, syl = Y >> 5;
  sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);
  syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
  const int sx = (int)sxl, sy = (int)syl, fx = (int)(X & 31), fy = (int)(Y & 31);
  int w[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
  const bool live[4] = {w[0] != 0, w[1] != 0, w[2] != 0, w[3] != 0};      // taps of non-zero weight, before the (0, 0) entry's compensation
  if (fx == 0 && fy == 0) { w[0] = 32767; w[3] = 1; }
  const T* const dem = static_cast<const T*>(d.dem);
  int acc0 = 0; bool hole = false;
  Blend<T> bl;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = sx + (k & 1), yy = sy + (k >> 1);
    if (xx >= 0 && xx < a.W && yy >= 0 && yy < a.H) {
      const size_t p = (size_t)yy * a.W + xx;
      acc0 += gray_of(a.src0 + 3 * p) * w[k];
      const T raw = dem[p];
      bl.tap(k, raw, w[k], live[k]);
      if (VOIDS && live[k] && warp_void(raw, d.nodata)) hole = true;
    } else if (VOIDS && live[k]) hole = true;
  }
  const size_t o = (size_t)y * a.crop_w + x;
  a.out0[o] = (uint8_t)min(max((acc0 + (1 << 14)) >> 15, 0), 255);
  T out = bl.result(fx, fy);
  if (VOIDS && hole) out = (T)d.nodata;      // (representable in T: gn_stereo_reference_dem checked)
  static_cast<T*>(d.out_dem)[o] = out;
}
}  // namespace

template <typename T> static void launch_rotate_crop_dem_t(const DemWarpArgs& a, hipStream_t s) {
  dim3 grid((a.w.crop_w + 63) / 64, (a.w.crop_h + 3) / 4), block(256);
  if (a.has_nodata) hipLaunchKernelGGL((k_rotate_crop_dem<T, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_rotate_crop_dem<T, false>), grid, block, 0, s, a);
}
void launch_rotate_crop_dem(const DemWarpArgs& a, hipStream_t s) {
  switch (a.dem_type) {
    case GN_DEM_U8: launch_rotate_crop_dem_t<uint8_t>(a, s); break;
    case GN_DEM_U16: launch_rotate_crop_dem_t<uint16_t>(a, s); break;
    case GN_DEM_I16: launch_rotate_crop_dem_t<int16_t>(a, s); break;
    default: launch_rotate_crop_dem_t<float>(a, s); break;
  }
}

void launch_rotate_crop(const WarpArgs& a, bool fused_gray, hipStream_t s) {
  dim3 grid((a.crop_w + 63) / 64, (a.crop_h + 3) / 4), block(256);
  if (fused_gray) hipLaunchKernelGGL(k_rotate_crop<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_rotate_crop<false>, grid, block, 0, s, a);
}

}  // namespace gn
