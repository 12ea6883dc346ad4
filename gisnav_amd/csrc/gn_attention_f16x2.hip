// k_attn_f16x2: softmax(q k^T * qscale) v with f32-accurate operands on the 16-bit matrix pipe (GN_PREC_F16X2_F16X2_ATTN, and the middle
// level of the certificate's re-run ladder).  The contract is k_attn_f32's: f32 rows q | k | v in, f32 rows out (and optionally hm16 rows for
// the block tail), keys of slot bs ^ 1 for cross attention, keys >= nvalid masked.
//
// Arithmetic:
//   * q, k and v are split on load into two fp16 terms, x * 2^s = xh + xl (xh = fp16(x * 2^s), xl = fp16(x * 2^s - xh)), with a power-of-two
//     scale 2^s that puts the largest magnitude of the piece in [2^12, 2^13): one scale per query row for q, one per 32-key tile for k and for v.
//     Without it rows of small magnitude would lose their low term to fp16 subnormals.  Scaling by a power of two is exact, and so is its
//     removal: the score is ldexp(acc, -(s_q + s_k)), the output ldexp(acc, -(14 + s_v)).
//   * S = qh kh + qh kl + ql kh on v_mfma_f32_32x32x16_f16, f32 accumulation (the dropped ql kl is below 2^-22 of |q||k|).
//   * Softmax in f32 with the EXACT running maximum at every key tile (no deferred rescale: this is an accuracy level); the denominator sums the
//     f32 probabilities.
//   * p in [0, 1] is scaled by 2^14 and split the same way; O = ph vh + ph vl + pl vh.  The v scale of the output accumulator is the smallest
//     tile scale seen so far (it only ever decreases, so the accumulator is rescaled by a power of two <= 1 together with the softmax factor and
//     every v tile fits fp16 under it).
//   * Range guard: a high term that would leave the fp16 range (only a non-finite input can do that under the scaling) and hm16 output rows that
//     do not fit fp16 raise a.ovf, as the f16x2 kernels do.
//
// Layout: a wave owns 32 queries and walks its key tiles (32 keys) through its OWN LDS region -- no workgroup barrier inside the loop -- and requests
// the next tile into registers before it computes on the current one (k_attn_f32_ks' scheme).  S^T = K Q^T with the operands swapped, so every lane
// holds the scores of one query (see gn_attention.hip); O^T = V^T P^T takes the probabilities straight from those registers.
//   NKS = 1 (bulk grids): four waves = 128 queries, each wave all keys.
//   NKS = 4 (one to eight pairs): four waves share 32 queries and split the keys (tiles w, w + 4, ..); the partial results meet through LDS by the
//   log-sum-exp identity in a fixed order.
#include "gn_common.h"

namespace gn {

namespace {
constexpr int KT = 32;                 // keys per tile
constexpr int KH = 72;                 // K tile row stride (halves): [key][d], 16-byte aligned rows
constexpr int VH = 40;                 // V^T tile row stride (halves): [d][key]
constexpr int WREG = 2 * KT * KH + 2 * 64 * VH;   // halves of one wave's region: Kh | Kl | Vh | Vl
constexpr int PSHIFT = 14;             // p * 2^14 <= 16384: both fp16 terms of a probability stay in range
constexpr float kF16Max = 65504.0f;

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
// power-of-two exponent s with max * 2^s in [2^12, 2^13) (s = 0 for max = 0 or a non-finite max; clamped so that 2^s and 2^-s stay normal)
__device__ __forceinline__ int scale_exp(float mx) {
  if (!(mx > 0.f) || !(mx <= 3.0e38f)) return 0;
  int e;
  frexpf(mx, &e);
  return min(max(13 - e, -120), 120);
}
__device__ __forceinline__ void split4(const float4 x, int s, f16x4_t& h, f16x4_t& l) {
  const f32x4_t v = {ldexpf(x.x, s), ldexpf(x.y, s), ldexpf(x.z, s), ldexpf(x.w, s)};
  h = __builtin_convertvector(v, f16x4_t);
  l = __builtin_convertvector(v - __builtin_convertvector(h, f32x4_t), f16x4_t);
}
__device__ __forceinline__ f32x16 mfma_f16(const f16x8_t& x, const f16x8_t& y, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0);
}
__device__ __forceinline__ f16x8_t ld8(const _Float16* p) { return *reinterpret_cast<const f16x8_t*>(p); }
__device__ __forceinline__ f16x8_t ld4x2(const _Float16* p) {   // halves p[0..3] and p[8..11]
  const f16x4_t a = *reinterpret_cast<const f16x4_t*>(p), b = *reinterpret_cast<const f16x4_t*>(p + 8);
  return (f16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <int NKS>
__global__ __launch_bounds__(256) void k_attn_f16x2(AttnArgs a) {
  constexpr int MERGE = NKS > 1 ? 4 * 32 * 64 + 2 * 4 * 64 : 0;        // floats of the merge buffers (reuse the tile regions)
  constexpr int SMEM_B = 4 * WREG * 2 > MERGE * 4 ? 4 * WREG * 2 : MERGE * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, ql = lane & 31;
  const int h = blockIdx.y, bs = blockIdx.z;
  const int kvs = a.cross ? (bs ^ 1) : bs;
  const int nkv = min(a.nvalid[kvs], a.npad);
  const int share = NKS > 1 ? wave : 0;                                  // key share of this wave
  const int q0 = NKS > 1 ? blockIdx.x * 32 : blockIdx.x * 128 + wave * 32;
  _Float16* const Kh = reinterpret_cast<_Float16*>(smem) + wave * WREG;
  _Float16* const Kl = Kh + KT * KH;
  _Float16* const Vh = Kl + KT * KH;
  _Float16* const Vl = Vh + 64 * VH;
  bool bad = false;                                                      // a high term left the fp16 range

  // Q as the B operand: lane (query ql, half hh) holds q[16c + 8hh + 0..7], c = 0..3; one scale per query row
  f16x8_t qh[4], ql8[4];
  int sq;
  {
    const float* qp = a.q + ((size_t)bs * a.npad + q0 + ql) * a.ldq + h * 64 + 8 * hh;
    float4 t[8];
    float mx = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      t[2 * c] = *reinterpret_cast<const float4*>(qp + 16 * c);
      t[2 * c + 1] = *reinterpret_cast<const float4*>(qp + 16 * c + 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      t[i].x *= a.qscale; t[i].y *= a.qscale; t[i].z *= a.qscale; t[i].w *= a.qscale;
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(t[i].x), fabsf(t[i].y)), fmaxf(fabsf(t[i].z), fabsf(t[i].w))));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    sq = scale_exp(mx);
    bad |= !(ldexpf(mx, sq) < kF16Max);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f16x4_t h0, l0, h1, l1;
      split4(t[2 * c], sq, h0, l0);
      split4(t[2 * c + 1], sq, h1, l1);
      qh[c] = (f16x8_t){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      ql8[c] = (f16x8_t){l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    }
  }

  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  int sv_run = 127;                      // v scale of the accumulator (above any tile's: the first tile sets it; o is zero until then)

  const float* kbase = a.k + (size_t)kvs * a.npad * a.ldk + h * 64;
  const float* vbase = a.v + (size_t)kvs * a.npad * a.ldv + h * 64;
  const int ntiles = (nkv + KT - 1) / KT;
  // the wave's loads of a tile: lane -> rows 8g + p (p = 0 .. 7), columns 4c .. 4c + 3 -- eight consecutive keys per lane, so that the
  // transposed V tile is written as whole 16-byte rows
  const int lg = lane >> 4, lc = (lane & 15) * 4;
  float4 pk[8], pv[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) { pk[p] = make_float4(0.f, 0.f, 0.f, 0.f); pv[p] = pk[p]; }   // (defined on every path: no scratch)
  auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int row = t * KT + 8 * lg + p;    // (< npad; rows of padding enter neither the tile scales nor the sums)
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      pk[p] = row < nkv ? *reinterpret_cast<const float4*>(kbase + (size_t)row * a.ldk + lc) : z;
      pv[p] = row < nkv ? *reinterpret_cast<const float4*>(vbase + (size_t)row * a.ldv + lc) : z;
    }
  };
  if (share < ntiles) fetch(share);
  for (int t = share; t < ntiles; t += NKS) {
    // tile scales (one per 32 x 64 piece of k and of v)
    float kmx = 0.f, vmx = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      kmx = fmaxf(kmx, fmaxf(fmaxf(fabsf(pk[p].x), fabsf(pk[p].y)), fmaxf(fabsf(pk[p].z), fabsf(pk[p].w))));
      vmx = fmaxf(vmx, fmaxf(fmaxf(fabsf(pv[p].x), fabsf(pv[p].y)), fmaxf(fabsf(pv[p].z), fabsf(pv[p].w))));
    }
    kmx = wave_max(kmx); vmx = wave_max(vmx);
    const int sk = scale_exp(kmx);
    const int sv = min(sv_run, scale_exp(vmx));
    bad |= !(ldexpf(kmx, sk) < kF16Max) || !(ldexpf(vmx, sv) < kF16Max);
    {
      f16x4_t vh4[8], vl4[8];
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        f16x4_t kh4, kl4;
        split4(pk[p], sk, kh4, kl4);
        *reinterpret_cast<f16x4_t*>(&Kh[(8 * lg + p) * KH + lc]) = kh4;
        *reinterpret_cast<f16x4_t*>(&Kl[(8 * lg + p) * KH + lc]) = kl4;
        split4(pv[p], sv, vh4[p], vl4[p]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // V^T: row d = lc + e, keys 8g .. 8g + 7
        *reinterpret_cast<f16x8_t*>(&Vh[(lc + e) * VH + 8 * lg]) =
            (f16x8_t){vh4[0][e], vh4[1][e], vh4[2][e], vh4[3][e], vh4[4][e], vh4[5][e], vh4[6][e], vh4[7][e]};
        *reinterpret_cast<f16x8_t*>(&Vl[(lc + e) * VH + 8 * lg]) =
            (f16x8_t){vl4[0][e], vl4[1][e], vl4[2][e], vl4[3][e], vl4[4][e], vl4[5][e], vl4[6][e], vl4[7][e]};
      }
    }
    if (t + NKS < ntiles) fetch(t + NKS);
    __builtin_amdgcn_wave_barrier();     // (a wave's LDS operations complete in order: its stores above are what its reads below see)

    // S^T[key][query], keys (r & 3) + 8 (r >> 2) + 4 hh of the tile
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f16x8_t kh = ld8(&Kh[ql * KH + 16 * c + 8 * hh]), kl = ld8(&Kl[ql * KH + 16 * c + 8 * hh]);
      st = mfma_f16(kl, qh[c], st);
      st = mfma_f16(kh, ql8[c], st);
      st = mfma_f16(kh, qh[c], st);
    }
    const int unscale = -(sq + sk);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = t * KT + (r & 3) + 8 * (r >> 2) + 4 * hh;
      st[r] = key < nkv ? ldexpf(st[r], unscale) : -INFINITY;
    }
    float mloc = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, st[r]);
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
    const float m_new = fmaxf(m_run, mloc);                  // exact running maximum, every tile
    const float alpha = expf(m_run - m_new);
    l_run *= alpha;
    const float oscale = ldexpf(alpha, sv - sv_run);          // (the first tile: alpha = 0)
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] *= oscale;
    sv_run = sv;
    f16x8_t ph[2], pl[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p = expf(st[8 * u + e] - m_new);
        l_run += p;
        const float ps = ldexpf(p, PSHIFT);
        const _Float16 hi = (_Float16)ps;
        ph[u][e] = hi;
        pl[u][e] = (_Float16)(ps - (float)hi);
      }
    m_run = m_new;
    // O^T[d][query] += V^T[d][keys 16u + 4hh + {0..3, 8..11}] P^T
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int off = (d * 32 + ql) * VH + 16 * u + 4 * hh;
        const f16x8_t vh = ld4x2(&Vh[off]), vl = ld4x2(&Vl[off]);
        o[d] = mfma_f16(vl, ph[u], o[d]);
        o[d] = mfma_f16(vh, pl[u], o[d]);
        o[d] = mfma_f16(vh, ph[u], o[d]);
      }
    __builtin_amdgcn_wave_barrier();     // (the next iteration overwrites the region only after these reads: same wave, in order)
  }
  // the accumulator back in output units (still unnormalised)
  const int ounscale = -(PSHIFT + sv_run);
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = ldexpf(o[d][r], ounscale);
  const float l_wave = l_run + __shfl_xor(l_run, 32);
  float amax = 0.f;

  if constexpr (NKS == 1) {
    const float inv = l_wave > 0.f ? 1.0f / l_wave : 0.f;
    const size_t row = (size_t)bs * a.npad + q0 + ql;
    float* op = a.out + row * a.ldo + h * 64 + 4 * hh;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w = make_float4(o[d][4 * g] * inv, o[d][4 * g + 1] * inv, o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
        *reinterpret_cast<float4*>(op + d * 32 + 8 * g) = w;
        if (a.outp != nullptr) {
          f16x4_t hi, lo;
          split4(w, 0, hi, lo);
          _Float16* pp = reinterpret_cast<_Float16*>(a.outp) + hm16_off(row, a.ldo, h * 64 + d * 32 + 8 * g + 4 * hh);
          *reinterpret_cast<f16x4_t*>(pp) = hi;
          *reinterpret_cast<f16x4_t*>(pp + 16) = lo;
          ovf_track(amax, fmaxf(fabsf(w.x), fabsf(w.y)), fmaxf(fabsf(w.z), fabsf(w.w)));
        }
      }
  } else {
    // merge: every wave publishes (m, l, O) of its key share; wave w then finishes two of the eight groups of four output registers
    __syncthreads();                                      // every wave is done with its tile region
    float* Om = reinterpret_cast<float*>(smem);          // [4 waves][32 registers][64 lanes]
    float* Mm = Om + 4 * 32 * 64;                         // [4][64]
    float* Lm = Mm + 4 * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) Om[(wave * 32 + d * 16 + r) * 64 + lane] = o[d][r];
    Mm[wave * 64 + lane] = m_run;
    Lm[wave * 64 + lane] = l_wave;
    __syncthreads();
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, Mm[w * 64 + lane]);
    float sc[4], L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = Mm[w * 64 + lane];
      sc[w] = mw == -INFINITY ? 0.f : expf(mw - M);
      L += Lm[w * 64 + lane] * sc[w];
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const int d2 = wave >> 1, g0 = (wave & 1) * 2;
    const size_t row = (size_t)bs * a.npad + q0 + ql;
    float* op = a.out + row * a.ldo + h * 64 + 4 * hh + d2 * 32;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) v += Om[(w * 32 + d2 * 16 + 4 * (g0 + g) + e) * 64 + lane] * sc[w];
        acc[e] = v * inv;
      }
      const float4 w4 = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(op + 8 * (g0 + g)) = w4;
      if (a.outp != nullptr) {
        f16x4_t hi, lo;
        split4(w4, 0, hi, lo);
        _Float16* pp = reinterpret_cast<_Float16*>(a.outp) + hm16_off(row, a.ldo, h * 64 + d2 * 32 + 8 * (g0 + g) + 4 * hh);
        *reinterpret_cast<f16x4_t*>(pp) = hi;
        *reinterpret_cast<f16x4_t*>(pp + 16) = lo;
        ovf_track(amax, fmaxf(fabsf(w4.x), fabsf(w4.y)), fmaxf(fabsf(w4.z), fabsf(w4.w)));
      }
    }
  }
  if (a.ovf != nullptr) {
    if (bad) amax = INFINITY;
    ovf_commit(a.ovf, amax);
  }
}
}  // namespace

// one to eight pairs (BS <= 16): the key-split form fills the chip (npad / 32 x 4 heads x BS workgroups); bulk grids: 128 queries per workgroup.
// The choice depends on the number of pairs only -- never on the padded length (gn_set_active_kpts changes no result bit).
void launch_attention_f16x2(const AttnArgs& a, hipStream_t s) {
  if (a.BS <= 16) {
    hipLaunchKernelGGL(k_attn_f16x2<4>, dim3(a.npad / 32, kHeads, a.BS), dim3(256), 0, s, a);
    g_last_kernel = "k_attn_f16x2<4>(";
  } else {
    hipLaunchKernelGGL(k_attn_f16x2<1>, dim3(a.npad / 128, kHeads, a.BS), dim3(256), 0, s, a);
    g_last_kernel = "k_attn_f16x2<1>(";
  }
}

}  // namespace gn
