// ofdm_dev.hpp — device functions the OFDM kernels share (k_ofdm.hip, k_acquire.hip, k_dvbt.hip):
// the constellation mapper, hard decider and max-log LLRs, the equalizer's complex arithmetic and
// the LDS transform fft_lds, each the host's (ofdm.cpp) operation for operation.
#pragma once
#include "hip_common.hpp"
#include "ofdm.hpp"

namespace orion {

// ---- constellations (ofdm.cpp map_bits / decide / soft_llr) ---------------------------
__device__ __forceinline__ f2 map_point(int order, const uint8_t* __restrict__ b, const float* __restrict__ axis) {
  const float r = 0.70710678118654752440f;
  if (order == ofdm::kBpsk) return f2{(b[0] & 1u) == 0 ? 1.0f : -1.0f, 0.0f};
  if (order == ofdm::kQpsk) return f2{(b[0] & 1u) == 0 ? r : -r, (b[1] & 1u) == 0 ? r : -r};
  const int k = order;  // kQam16 = 2, kQam64 = 3, kQam256 = 4: the bits per axis
  int ii = 0, iq = 0;
  for (int i = 0; i < k; ++i) {
    ii = (ii << 1) | (b[i] & 1);
    iq = (iq << 1) | (b[k + i] & 1);
  }
  return f2{axis[ii], axis[iq]};
}
__device__ __forceinline__ int decide_axis(float v, int k, const float* __restrict__ thr) {
  int nat = 0;
  for (int t = 0; t < (1 << k) - 1; ++t) nat += v > thr[t] ? 1 : 0;
  return nat ^ (nat >> 1);
}
__device__ __forceinline__ void decide_sym(int order, f2 v, const float* __restrict__ thr, uint8_t* __restrict__ out) {
  if (order == ofdm::kBpsk) {
    out[0] = v.x < 0.0f ? 1 : 0;
  } else if (order == ofdm::kQpsk) {
    out[0] = v.x < 0.0f ? 1 : 0;
    out[1] = v.y < 0.0f ? 1 : 0;
  } else {
    const int k = order;
    const int gi = decide_axis(v.x, k, thr), gq = decide_axis(v.y, k, thr);
    for (int b = 0; b < k; ++b) {
      out[b] = static_cast<uint8_t>((gi >> (k - 1 - b)) & 1);
      out[k + b] = static_cast<uint8_t>((gq >> (k - 1 - b)) & 1);
    }
  }
}
__device__ __forceinline__ void axis_llr(float v, int k, const float* __restrict__ axis, float* __restrict__ out) {
  for (int b = 0; b < k; ++b) {
    const int shift = k - 1 - b;
    float d0 = __builtin_inff(), d1 = __builtin_inff();
    for (int g = 0; g < (1 << k); ++g) {
      const float d = (v - axis[g]) * (v - axis[g]);
      if (((g >> shift) & 1) == 0)
        d0 = fminf(d0, d);
      else
        d1 = fminf(d1, d);
    }
    out[b] = d1 - d0;
  }
}
__device__ __forceinline__ void llr_sym(int order, f2 v, const float* __restrict__ axis, float* __restrict__ out) {
  if (order == ofdm::kBpsk) {
    out[0] = 4.0f * v.x;
  } else if (order == ofdm::kQpsk) {
    const float scale = 4.0f * 1.41421356237309504880f;
    out[0] = scale * v.x;
    out[1] = scale * v.y;
  } else {
    const int k = order;
    axis_llr(v.x, k, axis, out);
    axis_llr(v.y, k, axis, out + k);
  }
}

// ---- the equalizer (ofdm.cpp cdiv / equalizer_weight / interpolate_at) ----------------
__device__ __forceinline__ f2 cdiv_nc(f2 a, f2 b) {
  const float ns = b.x * b.x + b.y * b.y;
  return f2{(a.x * b.x + a.y * b.y) / ns, (a.y * b.x - a.x * b.y) / ns};
}
__device__ __forceinline__ f2 cmul_nc(f2 a, f2 b) { return f2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ f2 eq_weight(f2 h) {
  const float m = h.x * h.x + h.y * h.y;
  return m >= ofdm::kEqualizerFloor ? f2{h.x / m, -h.y / m} : f2{0.0f, 0.0f};
}


// ---- the LDS transform (k_ofdm.hip's header comment; ofdm.cpp fft_inplace's arithmetic) --------
__device__ __forceinline__ int pad(int p) { return p + (p >> 5); }
__device__ __forceinline__ int brev(int k, int log2n) { return static_cast<int>(__brev(static_cast<unsigned>(k)) >> (32 - log2n)); }
// b w, the host's butterfly product.
__device__ __forceinline__ f2 twmul(f2 d, f2 w) { return f2{d.x * w.x - d.y * w.y, d.x * w.y + d.y * w.x}; }
__device__ __forceinline__ f2 twid(const f2* __restrict__ tw, int k, bool inv) {
  f2 w = tw[k];
  if (inv) w.y = -w.y;
  return w;
}

// In place over x (one symbol, bit-reversed order in, natural order out). Every lane of the
// workgroup calls it (the barriers are the workgroup's); t < T indexes the symbol's lanes.
__device__ __forceinline__ void fft_lds(f2* x, int n, int log2n, const f2* __restrict__ tw, bool inv, int t, int T) {
  int cur = 1;  // the size of the transforms already done
  if (log2n & 1) {
    __syncthreads();
    const f2 w = twid(tw, 0, inv);
    for (int q = t; q < (n >> 1); q += T) {
      const f2 a = x[pad(2 * q)], tt = twmul(x[pad(2 * q + 1)], w);
      x[pad(2 * q)] = a + tt;
      x[pad(2 * q + 1)] = a - tt;
    }
    cur = 2;
  }
  while (cur < n) {  // the stages of size len = 2 cur and 2 len in one pass
    __syncthreads();
    const int len = 2 * cur, half = cur, step = n / len;
    for (int q = t; q < (n >> 2); q += T) {
      const int j = q & (half - 1);
      const int base = ((q - j) << 2) + j;
      const f2 x0 = x[pad(base)], x1 = x[pad(base + half)], x2 = x[pad(base + len)], x3 = x[pad(base + len + half)];
      // the stage of size len: pairs (x0, x1) and (x2, x3), both at offset j
      const f2 w1 = twid(tw, j * step, inv);
      const f2 t1 = twmul(x1, w1), t3 = twmul(x3, w1);
      const f2 y0 = x0 + t1, y1 = x0 - t1, y2 = x2 + t3, y3 = x2 - t3;
      // the stage of size 2 len: pairs (y0, y2) at offset j and (y1, y3) at offset j + half
      const f2 t2 = twmul(y2, twid(tw, j * (step >> 1), inv));
      const f2 t4 = twmul(y3, twid(tw, (j + half) * (step >> 1), inv));
      x[pad(base)] = y0 + t2;
      x[pad(base + len)] = y0 - t2;
      x[pad(base + half)] = y1 + t4;
      x[pad(base + len + half)] = y1 - t4;
    }
    cur <<= 2;
  }
  __syncthreads();
}

}  // namespace orion
