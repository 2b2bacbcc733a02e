// k_dvbt.hip — the DVB-T 2K frame on the device (dvbt_blocks.hpp), each kernel stateless across
// launches and held to dvbt.cpp's bits:
//
//   k_dvbt_mod    one 256-lane workgroup per (frame, symbol): every bin's value from the phase's
//                 role table (a data carrier mapped per Figure 9a straight from the coded-bit
//                 row, a boosted pilot, a TPS cell, a null), the inverse transform (fft_lds, the
//                 host's arithmetic), 1 / n, the cyclic prefix and the symbol window, stored at
//                 the symbol's place in the frame's row. A TPS cell has no serial state: its
//                 sign is ref_sign[j] (-1)^popcount(s_1 .. s_l), l = symbol mod 68.
//   k_gi_metric   the van de Beek sums of every candidate offset of every capture, one lane per
//                 offset. A lane runs the host's sequential sums in the host's order (over k,
//                 then over the symbols that fit; no contraction), so gamma, phi and the metric
//                 carry the host's bits; a sliding sum would round differently. A workgroup's
//                 256 offsets read 511 consecutive samples per 256-sample step of k, twice
//                 (the prefix and its copy n_fft later): staged in LDS, consecutive lanes
//                 reading consecutive cf32 values (ds_read_b64, conflict-free; 8-byte coalesced
//                 global loads).
//   k_gi_select   one wave per capture: the argmax in total_cmp order, the last of equal maxima
//                 (Iterator::max_by), by a wave reduction over (key, offset); the two
//                 single-symbol scores of the origin unwrap; start, score, cfo_hz, gamma, phi.
//   k_dvbt_demod  the modulator's geometry: the window at start[c] + s sps + cp - back-off, the
//                 forward transform, the 17 raw TPS cells, the phase's pilot ratios rx / known
//                 once into LDS, the estimate of each data bin from a precomputed bracket table,
//                 the equalizer weight (its erasure rule included) and the Figure-9a LLRs.
//   k_tps_decode  one wave per frame: the 67 differential bits (17 products summed in carrier
//                 order), then BCH(67,53): syndromes, the t = 2 locator, Chien, the re-encode
//                 check, the fields.
#include "dvbt_blocks.hpp"
#include "hip_common.hpp"
#include "ofdm_dev.hpp"

namespace orion {

namespace {

constexpr int kN = static_cast<int>(dvbt::kNFft), kLog2N = 11, kNd = static_cast<int>(dvbt::kData);
constexpr int kNTps = static_cast<int>(dvbt::kTps), kTpsSyms = static_cast<int>(dvbt::kTpsSymbols);
constexpr float kTauF = 6.28318530717958647692f;

// Figure 9a's per-axis levels (index: the axis' bits, the lowest y index first).
__device__ __forceinline__ int axis_level(int v, int idx) {
  constexpr int q2[2] = {1, -1}, q4[4] = {3, 1, -3, -1}, q6[8] = {7, 5, 1, 3, -7, -5, -1, -3};
  return v == 2 ? q2[idx] : v == 4 ? q4[idx] : q6[idx];
}
// dvb_t_map_symbol: even bits on I, odd on Q.
__device__ __forceinline__ f2 map_9a(const uint8_t* __restrict__ b, int v, float scale) {
  int ii = 0, qi = 0;
  for (int j = 0; j < v; j += 2) {
    ii = (ii << 1) | (b[j] & 1);
    qi = (qi << 1) | (b[j + 1] & 1);
  }
  return f2{static_cast<float>(axis_level(v, ii)) * scale, static_cast<float>(axis_level(v, qi)) * scale};
}
// dvb_t_soft_llr's axis_llrs: out[b * 2].
__device__ __forceinline__ void axis_llr_9a(float coord, int v, float scale, float* __restrict__ out) {
  const int k = v >> 1;
  for (int b = 0; b < k; ++b) {
    const int shift = k - 1 - b;
    float d0 = __builtin_inff(), d1 = __builtin_inff();
    for (int idx = 0; idx < (1 << k); ++idx) {
      const float d = coord - static_cast<float>(axis_level(v, idx)) * scale;
      const float dsq = d * d;
      if (((idx >> shift) & 1) == 0)
        d0 = fminf(d0, dsq);
      else
        d1 = fminf(d1, dsq);
    }
    out[2 * b] = d1 - d0;
  }
}
// |z| as dvbt::norm32 defines it.
__device__ __forceinline__ float norm32_dev(float re, float im) {
  const double r = static_cast<double>(re), i = static_cast<double>(im);
  return static_cast<float>(__dsqrt_rn(r * r + i * i));
}
__device__ __forceinline__ int total_key(float v) {
  const int b = __float_as_int(v);
  return b ^ static_cast<int>(static_cast<unsigned>(b >> 31) >> 1);
}

}  // namespace

// ---- k_dvbt_mod -------------------------------------------------------------------------------
__global__ __launch_bounds__(kDvbtThreads) void k_dvbt_mod(const uint8_t* __restrict__ bits, long long row_bits,
                                                           const int32_t* __restrict__ nbits,
                                                           const uint32_t* __restrict__ tps, int v, float scale, int cp,
                                                           int roll, const float* __restrict__ ramp, int n_symbols,
                                                           f2* __restrict__ iq, DvbtDev c) {
  __shared__ f2 x[kN + (kN >> 5)];
  const int t = threadIdx.x, s = blockIdx.x;
  const long long f = blockIdx.y;
  const int phase = s & 3, l = s % kTpsSyms;
  const int32_t* __restrict__ role = c.role + phase * kN;
  const uint8_t* __restrict__ row = bits + f * row_bits;
  const long long have = nbits ? min(static_cast<long long>(nbits[f]), row_bits) : row_bits;  // never past the row
  const long long sym_base = static_cast<long long>(s) * kNd * v;
  // the parity of s_1 .. s_l: the TPS encoder's running sign
  float tps_sign = 1.0f;
  if (l > 0) {
    const uint32_t* __restrict__ w = tps + f * 3;
    const unsigned long long lo = static_cast<unsigned long long>(w[0]) | (static_cast<unsigned long long>(w[1]) << 32);
    const unsigned long long mlo = l >= 63 ? ~1ULL : (((1ULL << (l + 1)) - 1ULL) & ~1ULL);  // bits 1 .. min(l, 63)
    const uint32_t mhi = l >= 64 ? ((1u << (l - 63)) - 1u) : 0u;                               // bits 64 .. l
    const int par = (__popcll(lo & mlo) + __popc(w[2] & mhi)) & 1;
    tps_sign = par ? -1.0f : 1.0f;
  }
  for (int bin = t; bin < kN; bin += kDvbtThreads) {
    const int m = role[bin];
    f2 val{0.0f, 0.0f};
    if (m >= 0) {
      const long long base = sym_base + static_cast<long long>(m) * v;
      if (base + v <= have) val = map_9a(row + base, v, scale);
    } else if (m == dvbt::kRolePilotPos) {
      val.x = (4.0f / 3.0f) * 2.0f * (0.5f - 0.0f);
    } else if (m == dvbt::kRolePilotNeg) {
      val.x = (4.0f / 3.0f) * 2.0f * (0.5f - 1.0f);
    } else if (m <= dvbt::kRoleTps0) {
      val.x = tps_sign * c.tps_sign[dvbt::kRoleTps0 - m];
    }
    x[pad(brev(bin, kLog2N))] = val;
  }
  fft_lds(x, kN, kLog2N, c.tw, true, t, kDvbtThreads);
  const float g = 1.0f / static_cast<float>(kN);
  const int len = kN + cp;
  f2* __restrict__ out = iq + (f * n_symbols + s) * len;
  for (int i = t; i < len; i += kDvbtThreads) {
    const int m = i < cp ? kN - cp + i : i - cp;  // CyclicPrefixInsert
    f2 val = x[pad(m)];
    val = f2{val.x * g, val.y * g};
    if (i < roll) {  // SymbolWindow: both edges, the host's multiply order
      const float w = ramp[i];
      val = f2{val.x * w, val.y * w};
    }
    if (len - 1 - i < roll) {
      const float w = ramp[len - 1 - i];
      val = f2{val.x * w, val.y * w};
    }
    out[i] = val;
  }
}

// ---- k_gi_metric ------------------------------------------------------------------------------
__global__ __launch_bounds__(kGiThreads) void k_gi_metric(const f2* __restrict__ iq, long long n, int n_fft, int cp,
                                                          int search_len, int max_syms, float rho,
                                                          float* __restrict__ metric, f2* __restrict__ gamma_all,
                                                          float* __restrict__ phi_all) {
  __shared__ f2 A[2 * kGiThreads], B[2 * kGiThreads];
  const int t = threadIdx.x;
  const long long c = blockIdx.y;
  const f2* __restrict__ x = iq + c * n;
  const long long d0 = static_cast<long long>(blockIdx.x) * kGiThreads, d = d0 + t;
  const long long period = static_cast<long long>(n_fft) + cp;
  float gr = 0.0f, gi = 0.0f, phi = 0.0f;
  for (int u = 0; u < max_syms; ++u) {
    const long long base0 = d0 + u * period;  // the workgroup's first offset: wave-uniform
    if (base0 + period > n) break;            // no lane's symbol u fits (a lane's base is >= base0)
    const bool mine = d < search_len && d + u * period + period <= n;
    for (int kc = 0; kc < cp; kc += kGiThreads) {
      const int kn = min(kGiThreads, cp - kc);
      __syncthreads();  // the previous step's reads
      for (int i = t; i < kGiThreads + kn - 1; i += kGiThreads) {
        const long long g = base0 + kc + i, g2 = g + n_fft;
        A[i] = g < n ? x[g] : f2{0.0f, 0.0f};
        B[i] = g2 < n ? x[g2] : f2{0.0f, 0.0f};
      }
      __syncthreads();
      if (mine) {
        for (int k = 0; k < kn; ++k) {
          const f2 a = A[t + k], b = B[t + k];
          const float nbi = -b.y;  // a conj(b), the plain product
          gr += a.x * b.x - a.y * nbi;
          gi += a.x * nbi + a.y * b.x;
          phi += (a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y);
        }
      }
    }
  }
  if (d >= search_len) return;
  phi *= 0.5f;
  const long long o = c * search_len + d;
  metric[o] = norm32_dev(gr, gi) - rho * phi;
  gamma_all[o] = f2{gr, gi};
  phi_all[o] = phi;
}

// ---- k_gi_select ------------------------------------------------------------------------------
// ratio < 0: no unwrap (origin_score_ratio <= 0). ok == 0: the capture is too short, found = 0.
__global__ __launch_bounds__(64) void k_gi_select(const f2* __restrict__ iq, long long n, int n_fft, int cp, float fs,
                                                  int search_len, float ratio, int ok, GiOut o) {
  const int t = threadIdx.x;
  const long long c = blockIdx.x;
  if (!ok) {
    if (t == 0) {
      o.start[c] = 0;
      o.found[c] = 0;
      o.score[c] = 0.0f;
      o.cfo_hz[c] = 0.0f;
      o.gamma[c] = f2{0.0f, 0.0f};
      o.phi[c] = 0.0f;
    }
    return;
  }
  const float* __restrict__ metric = o.metric + c * search_len;
  int key = 0, idx = -1;
  for (int d = t; d < search_len; d += 64) {  // ascending d: >= keeps the last of equal maxima
    const int k = total_key(metric[d]);
    if (idx < 0 || k >= key) {
      key = k;
      idx = d;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int k2 = __shfl_xor(key, off, 64), i2 = __shfl_xor(idx, off, 64);
    if (i2 >= 0 && (idx < 0 || k2 > key || (k2 == key && i2 > idx))) {
      key = k2;
      idx = i2;
    }
  }
  const int argmax = idx;
  const int period = n_fft + cp;
  const int phase = argmax % period, origin = argmax - phase;
  const bool unwrap = ratio >= 0.0f && phase != 0 && period - phase <= (cp + 1) / 2;
  // lane 0: the origin's single-symbol score, lane 1: the peak's
  float sc = 0.0f;
  if (unwrap && t < 2) {
    const long long d = t == 0 ? origin : argmax;
    if (d + period <= n) {
      const f2* __restrict__ x = iq + c * n + d;
      float gr = 0.0f, gi = 0.0f, phi = 0.0f;
      for (int k = 0; k < cp; ++k) {
        const f2 a = x[k], b = x[n_fft + k];
        const float nbi = -b.y;
        gr += a.x * b.x - a.y * nbi;
        gi += a.x * nbi + a.y * b.x;
        phi += (a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y);
      }
      phi *= 0.5f;
      sc = phi > 0.0f ? fminf(norm32_dev(gr, gi) / phi, 1.0f) : 0.0f;
    }
  }
  const float sc_origin = __shfl(sc, 0, 64), sc_peak = __shfl(sc, 1, 64);
  if (t != 0) return;
  const int best = (unwrap && sc_origin >= ratio * sc_peak) ? origin : argmax;
  const f2 g = o.gamma_all[c * search_len + best];
  const float phi = o.phi_all[c * search_len + best];
  o.start[c] = best;
  o.found[c] = 1;
  o.score[c] = phi > 0.0f ? fminf(norm32_dev(g.x, g.y) / phi, 1.0f) : 0.0f;
  o.cfo_hz[c] = -atan2f(g.y, g.x) * fs / (kTauF * static_cast<float>(n_fft));
  o.gamma[c] = g;
  o.phi[c] = phi;
}

// ---- k_dvbt_demod -----------------------------------------------------------------------------
__global__ __launch_bounds__(kDvbtThreads) void k_dvbt_demod(const f2* __restrict__ iq, long long n,
                                                             const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ found, int n_symbols, int cp,
                                                             int win, int v, float scale, float* __restrict__ llr,
                                                             f2* __restrict__ cells, f2* __restrict__ syms, DvbtDev c) {
  __shared__ f2 x[kN + (kN >> 5)];
  __shared__ f2 ratio[kDvbtRefMax];
  const int t = threadIdx.x, s = blockIdx.x;
  const long long f = blockIdx.y;
  const int sps = kN + cp;
  const long long st = start[f];
  // the reference's Acquisition / Incomplete: nothing is written (workgroup-uniform)
  if (found[f] == 0 || st < 0 || st + static_cast<long long>(n_symbols) * sps > n) return;
  const int phase = s & 3;
  const f2* __restrict__ src = iq + f * n + st + static_cast<long long>(s) * sps + win;
  for (int i = t; i < kN; i += kDvbtThreads) x[pad(brev(i, kLog2N))] = src[i];
  fft_lds(x, kN, kLog2N, c.tw, false, t, kDvbtThreads);
  const long long sym = f * n_symbols + s;
  if (t < kNTps) cells[sym * kNTps + t] = x[pad(static_cast<int>(c.tps_bins[t]))];
  const int np = c.n_ref[phase];
  const uint32_t* __restrict__ pb = c.ref_bins + phase * kDvbtRefMax;
  const float* __restrict__ pv = c.ref_val + phase * kDvbtRefMax;
  // rx / known per reference pilot: interp_est's cdiv_nc, once per pilot instead of per bin
  if (t < np) ratio[t] = cdiv_nc(x[pad(static_cast<int>(pb[t]))], f2{pv[t], 0.0f});
  __syncthreads();
  const uint32_t* __restrict__ dbin = c.data_bins + phase * kNd;
  const uint16_t* __restrict__ br = c.bracket + phase * kNd * 2;
  for (int d = t; d < kNd; d += kDvbtThreads) {
    const uint32_t bin = dbin[d];
    const int lo = br[2 * d], hi = br[2 * d + 1];
    // The bracket table holds what interp_est's binary search finds for this bin, and each
    // ratio and the interpolation below are interp_est's expressions: the bits do not change.
    f2 h = ratio[lo];
    if (lo != hi) {
      const f2 ur = ratio[hi];
      const float w = static_cast<float>(bin - pb[lo]) / static_cast<float>(pb[hi] - pb[lo]);
      h = f2{h.x + (ur.x - h.x) * w, h.y + (ur.y - h.y) * w};
    }
    const f2 e = cmul_nc(x[pad(static_cast<int>(bin))], eq_weight(h));
    const long long o = sym * kNd + d;
    if (syms) syms[o] = e;
    float* __restrict__ out = llr + o * v;
    axis_llr_9a(e.x, v, scale, out);
    axis_llr_9a(e.y, v, scale, out + 1);
  }
}

// ---- k_tps_decode -----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tps_decode(const f2* __restrict__ cells, int n_symbols,
                                                   int32_t* __restrict__ fields, int32_t* __restrict__ status,
                                                   DvbtDev c) {
  __shared__ uint8_t cw[128];  // cw[l] = s_l, l = 1 .. 67
  const int t = threadIdx.x;
  const long long f = blockIdx.x;
  if (n_symbols < kTpsSyms) {  // TpsDecoder::word() is None before 68 symbols
    if (t == 0) status[f] = 1;
    if (t < 5) fields[f * 5 + t] = 0;
    return;
  }
  const f2* __restrict__ row = cells + f * static_cast<long long>(n_symbols) * kNTps;
  for (int l = 1 + t; l < kTpsSyms; l += 64) {
    const f2* __restrict__ cur = row + l * kNTps;
    const f2* __restrict__ prev = cur - kNTps;
    float acc = 0.0f;
    for (int j = 0; j < kNTps; ++j) acc += cur[j].x * prev[j].x - cur[j].y * (-prev[j].y);  // (cell conj(prev)).re
    cw[l] = acc < 0.0f ? 1 : 0;
  }
  __syncthreads();
  if (t != 0) return;
  const uint8_t* __restrict__ ex = c.gf_exp;
  const uint8_t* __restrict__ lg = c.gf_log;
  auto mul = [&](int a, int b) { return (a == 0 || b == 0) ? 0 : static_cast<int>(ex[lg[a] + lg[b]]); };
  int synd[4] = {0, 0, 0, 0};
  for (int pos = 0; pos < 67; ++pos)
    if (cw[1 + pos]) {
      const int deg = 66 - pos + 60;
      for (int i = 1; i <= 4; ++i) synd[i - 1] ^= ex[(i * deg) % 127];
    }
  bool good = true;
  if (synd[0] | synd[1] | synd[2] | synd[3]) {
    const int s1 = synd[0], s3 = synd[2];
    if (s1 == 0) {
      good = false;
    } else {
      const int num = s3 ^ mul(mul(s1, s1), s1);
      const int sig2 = num == 0 ? 0 : static_cast<int>(ex[(lg[num] + 127 - lg[s1]) % 127]);
      int nroots = 0;
      for (int pos = 0; pos < 67; ++pos) {
        const int deg = 66 - pos + 60;
        const int xv = ex[(127 - (deg % 127)) % 127];
        const int val = 1 ^ mul(s1, xv) ^ mul(sig2, mul(xv, xv));
        if (val == 0) {
          cw[1 + pos] ^= 1;
          ++nroots;
        }
      }
      good = nroots == (sig2 == 0 ? 1 : 2);
      if (good) {  // the re-encode check: the parity of the corrected information bits
        uint32_t reg = 0;
        for (int i = 0; i < 67; ++i) {
          reg = (reg << 1) | (i < 53 ? cw[1 + i] : 0u);
          if (reg & (1u << 14)) reg ^= 0x4377u;
        }
        for (int i = 0; i < 14; ++i) good = good && cw[54 + i] == ((reg >> (13 - i)) & 1u);
      }
    }
  }
  auto get = [&](int a, int b) {  // info indices a .. b - 1, s_(a+1) first
    int val = 0;
    for (int i = a; i < b; ++i) val = (val << 1) | cw[1 + i];
    return val;
  };
  const int con = get(24, 26), rate = get(29, 32);
  if (con > 2 || rate > 4) good = false;
  status[f] = good ? 0 : 1;
  fields[f * 5 + 0] = good ? get(22, 24) : 0;
  fields[f * 5 + 1] = good ? con + 1 : 0;  // ofdm::kQpsk = 1, kQam16 = 2, kQam64 = 3
  fields[f * 5 + 2] = good ? rate : 0;
  fields[f * 5 + 3] = good ? get(35, 37) : 0;
  fields[f * 5 + 4] = good ? get(39, 47) : 0;
}

// ---- launchers --------------------------------------------------------------------------------
void launch_dvbt_mod(const uint8_t* bits, long long row_bits, const int32_t* nbits, const uint32_t* tps, int frames,
                     int n_symbols, int v, float scale, int cp, int roll, const float* ramp, f2* iq, const DvbtDev& d,
                     hipStream_t s) {
  k_dvbt_mod<<<dim3(n_symbols, frames), kDvbtThreads, 0, s>>>(bits, row_bits, nbits, tps, v, scale, cp, roll, ramp,
                                                             n_symbols, iq, d);
  ORION_LAUNCH_CHECK();
}

void launch_gi_sync(const f2* iq, int ncap, long long n, int n_fft, int cp, float fs, int search_len, int max_syms,
                    float rho, float ratio, const GiOut& out, hipStream_t s) {
  const bool ok = cp > 0 && n_fft > 0 && search_len > 0 && n >= static_cast<long long>(search_len) - 1 + n_fft + cp;
  if (ok) {
    k_gi_metric<<<dim3(div_up(search_len, kGiThreads), ncap), kGiThreads, 0, s>>>(iq, n, n_fft, cp, search_len, max_syms, rho,
                                                                                out.metric, out.gamma_all, out.phi_all);
    ORION_LAUNCH_CHECK();
  }
  k_gi_select<<<ncap, 64, 0, s>>>(iq, n, n_fft, cp, fs, search_len, ratio, ok ? 1 : 0, out);
  ORION_LAUNCH_CHECK();
}

void launch_dvbt_demod(const f2* iq, int ncap, long long n, const int32_t* start, const int32_t* found, int n_symbols,
                       int cp, int win, int v, float scale, float* llr, f2* cells, f2* syms, const DvbtDev& d,
                       hipStream_t s) {
  k_dvbt_demod<<<dim3(n_symbols, ncap), kDvbtThreads, 0, s>>>(iq, n, start, found, n_symbols, cp, win, v, scale, llr, cells,
                                                             syms, d);
  ORION_LAUNCH_CHECK();
}

void launch_tps_decode(const f2* cells, int frames, int n_symbols, int32_t* fields, int32_t* status, const DvbtDev& d,
                       hipStream_t s) {
  k_tps_decode<<<frames, 64, 0, s>>>(cells, n_symbols, fields, status, d);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
