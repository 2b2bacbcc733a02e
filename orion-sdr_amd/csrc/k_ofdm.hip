// k_ofdm.hip — the OFDM symbol layer on the device: the batched transform (k_fft), the fused
// modulator (k_ofdm_mod: mapper, grid scatter, inverse transform, cyclic prefix, window,
// gain) and demodulator (k_ofdm_demod: window select, forward transform, equalizer, grid
// gather, gain, hard bits / LLRs), the RF stage (k_ofdm_rf) and the elementwise blocks a
// caller composes by hand (k_ofdm_decide, k_ofdm_llr, k_ofdm_equalize).
//
// The transform. One symbol lives in LDS; kOfdmThreads / T symbols share a workgroup, T =
// min(n / 4, kOfdmThreads) lanes each, so that a workgroup's four waves are full at every
// size. fft_lds (ofdm_dev.hpp) is radix-2 decimation in time, two stages fused per pass: a lane holds the
// four values of a radix-4 butterfly in registers, so a pass costs one LDS read and one LDS
// write per value where two radix-2 passes cost two; a first radix-2 pass when log2 n is
// odd. The arithmetic of each fused stage is the host's (ofdm.cpp fft_inplace): the same
// twiddle table, t = b w with four multiplies, one subtraction and one addition, each
// rounded (-ffp-contract=off), W^0 multiplied like any other, then a + t and a - t. The
// input is written to LDS in bit-reversed order (__brev) and the output read in natural
// order. The stand-alone block and both fused kernels call this one function, so they give
// identical bits for identical input, and those bits are the host transform's.
// LDS index p is stored at p + (p >> 5): the bit-reversed placement of consecutive samples
// strides by n / 64 values, which without the skew lands every lane of a group in one bank.
//
// Global accesses are 8-byte (one cf32 per lane, consecutive lanes consecutive values):
// always aligned for cf32 data at any 8-byte offset, so an odd symbol stride needs no
// fallback path.
#include "hip_common.hpp"
#include "ofdm_blocks.hpp"
#include "ofdm_dev.hpp"

namespace orion {

namespace {
// The estimate at bin from np > 0 bin-sorted pilots; rx(bin) is the received value of a bin.
// The two bracketing pilots' ratios are computed here, per bin, by binary search as the
// reference does; no ratio table is kept between bins.
template <class Rx>
__device__ __forceinline__ f2 interp_est(const uint32_t* __restrict__ pb, const f2* __restrict__ pv, int np,
                                         uint32_t bin, Rx rx) {
  int pick;
  if (np == 1) {
    pick = 0;
  } else {
    int lo = 0, hi = np;  // the first pilot with pbin >= bin
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (pb[mid] < bin)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == 0) {
      pick = 0;
    } else if (lo == np) {
      pick = np - 1;
    } else if (pb[lo] == bin) {
      pick = lo;
    } else {
      const f2 lr = cdiv_nc(rx(pb[lo - 1]), pv[lo - 1]), ur = cdiv_nc(rx(pb[lo]), pv[lo]);
      const float t = static_cast<float>(bin - pb[lo - 1]) / static_cast<float>(pb[lo] - pb[lo - 1]);
      return f2{lr.x + (ur.x - lr.x) * t, lr.y + (ur.y - lr.y) * t};
    }
  }
  return cdiv_nc(rx(pb[pick]), pv[pick]);
}
}  // namespace

// ---- k_fft ------------------------------------------------------------------------------
__global__ __launch_bounds__(kOfdmThreads) void k_fft(const f2* __restrict__ in, long long in_stride,
                                                      f2* __restrict__ out, long long out_stride, long long batch,
                                                      int n, int log2n, int T, const f2* __restrict__ tw, int inverse) {
  extern __shared__ f2 lds[];
  const int tid = threadIdx.x, sl = tid / T, t = tid - sl * T;
  const long long sym = static_cast<long long>(blockIdx.x) * (kOfdmThreads / T) + sl;
  const bool valid = sym < batch;
  f2* x = lds + sl * (n + (n >> 5));
  for (int i = t; i < n; i += T) x[pad(brev(i, log2n))] = valid ? in[sym * in_stride + i] : f2{0.0f, 0.0f};
  fft_lds(x, n, log2n, tw, inverse != 0, t, T);
  if (!valid) return;
  const float g = 1.0f / static_cast<float>(n);
  for (int k = t; k < n; k += T) {
    f2 v = x[pad(k)];
    if (inverse) v = f2{v.x * g, v.y * g};
    out[sym * out_stride + k] = v;
  }
}

// ---- k_ofdm_mod -------------------------------------------------------------------------
// bits [batch][nd * bps] u8 -> out [batch][n + cp] cf32; batch = channels x symbols.
__global__ __launch_bounds__(kOfdmThreads) void k_ofdm_mod(const uint8_t* __restrict__ bits, f2* __restrict__ out,
                                                           long long batch, OfdmDev c, float gain, int apply_gain) {
  extern __shared__ f2 lds[];
  const int n = c.n, T = c.T;
  const int tid = threadIdx.x, sl = tid / T, t = tid - sl * T;
  const long long sym = static_cast<long long>(blockIdx.x) * (kOfdmThreads / T) + sl;
  const bool valid = sym < batch;
  f2* x = lds + sl * (n + (n >> 5));
  const uint8_t* b = bits + sym * (static_cast<long long>(c.nd) * c.bps);
  for (int bin = t; bin < n; bin += T) {  // GridMap as a gather: data, pilot or null per bin
    f2 v{0.0f, 0.0f};
    if (valid) {
      const int m = c.map[bin];
      if (m >= 0)
        v = map_point(c.order, b + static_cast<long long>(m) * c.bps, c.axis);
      else if (m <= -2)
        v = c.pilot_val[-2 - m];
    }
    x[pad(brev(bin, c.log2n))] = v;
  }
  fft_lds(x, n, c.log2n, c.tw, true, t, T);
  if (!valid) return;
  const float s = 1.0f / static_cast<float>(n);
  const int len = n + c.cp;
  for (int i = t; i < len; i += T) {
    const int m = i < c.cp ? n - c.cp + i : i - c.cp;  // CyclicPrefixInsert
    f2 v = x[pad(m)];
    v = f2{v.x * s, v.y * s};
    if (i < c.roll) {  // SymbolWindow: both edges
      const float w = c.ramp[i];
      v = f2{v.x * w, v.y * w};
    }
    if (len - 1 - i < c.roll) {
      const float w = c.ramp[len - 1 - i];
      v = f2{v.x * w, v.y * w};
    }
    if (apply_gain) v = f2{gain * v.x, gain * v.y};
    out[sym * len + i] = v;
  }
}

// The RF stage (modulate/ofdm.rs:525-532) in place: iq [nch][per_ch], channel sample j takes
// oscillator output k0 + j: g fma(s.re, r.re, -(s.im r.im)), g fma(s.im, r.re, s.re r.im).
__global__ __launch_bounds__(256) void k_ofdm_rf(f2* __restrict__ iq, long long per_ch, long long total, uint64_t k0,
                                                 OscDev o, float gain) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= total) return;
  const f2 r = osc_at(o, k0 + static_cast<uint64_t>(i % per_ch));
  const f2 v = cmul_rot(iq[i], r);
  iq[i] = f2{gain * v.x, gain * v.y};
}

// ---- k_ofdm_demod -----------------------------------------------------------------------
// iq [batch][n + cp] -> soft [batch][nd] cf32, and from the same values bits [batch][nd * bps]
// u8 and llr [batch][nd * bps] f32 where asked for. eq: ofdm::kEqNone, kEqTrainingSymbolHold
// (c.weight) or kEqPerSymbolPilotInterp (the bin-sorted pilots; c.hold with no pilot).
__global__ __launch_bounds__(kOfdmThreads) void k_ofdm_demod(const f2* __restrict__ iq, f2* __restrict__ soft,
                                                             uint8_t* __restrict__ bits, float* __restrict__ llr,
                                                             long long batch, OfdmDev c, int start, float gain,
                                                             int apply_gain, int eq) {
  extern __shared__ f2 lds[];
  const int n = c.n, T = c.T;
  const int tid = threadIdx.x, sl = tid / T, t = tid - sl * T;
  const long long sym = static_cast<long long>(blockIdx.x) * (kOfdmThreads / T) + sl;
  const bool valid = sym < batch;
  f2* x = lds + sl * (n + (n >> 5));
  const f2* src = iq + sym * (n + c.cp) + start;
  for (int i = t; i < n; i += T) x[pad(brev(i, c.log2n))] = valid ? src[i] : f2{0.0f, 0.0f};
  fft_lds(x, n, c.log2n, c.tw, false, t, T);
  if (!valid) return;
  auto rx = [x](uint32_t bin) { return x[pad(static_cast<int>(bin))]; };
  for (int d = t; d < c.nd; d += T) {
    const uint32_t bin = c.data_bins[d];
    f2 v = rx(bin);
    if (eq == ofdm::kEqTrainingSymbolHold) {
      v = cmul_nc(v, c.weight[bin]);
    } else if (eq == ofdm::kEqPerSymbolPilotInterp) {
      const f2 h = c.np > 0 ? interp_est(c.spbin, c.spval, c.np, bin, rx) : c.hold[bin];
      v = cmul_nc(v, eq_weight(h));
    }
    if (apply_gain) v = f2{gain * v.x, gain * v.y};
    const long long o = sym * c.nd + d;
    soft[o] = v;
    if (bits) decide_sym(c.order, v, c.thr, bits + o * c.bps);
    if (llr) llr_sym(c.order, v, c.axis, llr + o * c.bps);
  }
}

// ---- the elementwise blocks -------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ofdm_decide(const f2* __restrict__ soft, long long n, int order, int bps,
                                                     const float* __restrict__ thr, uint8_t* __restrict__ bits) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) decide_sym(order, soft[i], thr, bits + i * bps);
}
__global__ __launch_bounds__(256) void k_ofdm_llr(const f2* __restrict__ soft, long long n, int order, int bps,
                                                  const float* __restrict__ axis, float* __restrict__ llr) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) llr_sym(order, soft[i], axis, llr + i * bps);
}
// OfdmEqualizer::process over nsym n-bin vectors. emap (kEqPerSymbolPilotInterp with pilots):
// 0 the held estimate, 1 a data bin (interpolated), 2 + p the bin of sorted pilot p (its own ratio).
__global__ __launch_bounds__(256) void k_ofdm_equalize(const f2* __restrict__ in, f2* __restrict__ out, long long nsym,
                                                       OfdmDev c, int eq) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nsym * c.n) return;
  const long long sym = i / c.n;
  const uint32_t bin = static_cast<uint32_t>(i - sym * c.n);
  const f2* row = in + sym * c.n;
  auto rx = [row](uint32_t b) { return row[b]; };
  f2 w;
  if (eq == ofdm::kEqTrainingSymbolHold) {
    w = c.weight[bin];
  } else {
    f2 h = c.hold[bin];
    if (c.np > 0) {
      const int role = c.emap[bin];
      if (role == 1)
        h = interp_est(c.spbin, c.spval, c.np, bin, rx);
      else if (role >= 2)
        h = cdiv_nc(row[bin], c.spval[role - 2]);
    }
    w = eq_weight(h);
  }
  out[i] = cmul_nc(row[bin], w);
}

// ---- launchers --------------------------------------------------------------------------
namespace {
unsigned sym_grid(long long batch, int T) {
  const long long per = kOfdmThreads / T, g = (batch + per - 1) / per;
  if (g > 0x7fffffffLL) throw std::invalid_argument("ofdm: too many symbols for one launch");
  return static_cast<unsigned>(g);
}
size_t sym_lds(int n, int T) { return static_cast<size_t>(kOfdmThreads / T) * (n + (n >> 5)) * sizeof(f2); }
unsigned flat_grid(long long total) {
  const long long g = (total + 255) / 256;
  if (g > 0x7fffffffLL) throw std::invalid_argument("ofdm: too many values for one launch");
  return static_cast<unsigned>(g);
}
}  // namespace

int ofdm_threads_per_symbol(size_t n) { return static_cast<int>(std::min<size_t>(n / 4, kOfdmThreads)); }

void launch_fft(const f2* in, long long in_stride, f2* out, long long out_stride, long long batch, int n, int log2n,
                const f2* tw, bool inverse, hipStream_t s) {
  if (batch < 1) return;
  const int T = ofdm_threads_per_symbol(n);
  k_fft<<<sym_grid(batch, T), kOfdmThreads, sym_lds(n, T), s>>>(in, in_stride, out, out_stride, batch, n, log2n, T, tw,
                                                               inverse ? 1 : 0);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_mod(const uint8_t* bits, f2* out, long long batch, const OfdmDev& c, float gain, bool apply_gain,
                     hipStream_t s) {
  if (batch < 1) return;
  k_ofdm_mod<<<sym_grid(batch, c.T), kOfdmThreads, sym_lds(c.n, c.T), s>>>(bits, out, batch, c, gain, apply_gain ? 1 : 0);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_rf(f2* iq, long long per_ch, long long nch, uint64_t k0, const OscDev& o, float gain, hipStream_t s) {
  const long long total = per_ch * nch;
  if (total < 1) return;
  k_ofdm_rf<<<flat_grid(total), 256, 0, s>>>(iq, per_ch, total, k0, o, gain);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_demod(const f2* iq, f2* soft, uint8_t* bits, float* llr, long long batch, const OfdmDev& c, int start,
                       float gain, bool apply_gain, int eq, hipStream_t s) {
  if (batch < 1) return;
  k_ofdm_demod<<<sym_grid(batch, c.T), kOfdmThreads, sym_lds(c.n, c.T), s>>>(iq, soft, bits, llr, batch, c, start, gain,
                                                                          apply_gain ? 1 : 0, eq);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_decide(const f2* soft, long long n, int order, const float* thr, uint8_t* bits, hipStream_t s) {
  if (n < 1) return;
  k_ofdm_decide<<<flat_grid(n), 256, 0, s>>>(soft, n, order, static_cast<int>(ofdm::bits_per_symbol(order)), thr, bits);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_llr(const f2* soft, long long n, int order, const float* axis, float* llr, hipStream_t s) {
  if (n < 1) return;
  k_ofdm_llr<<<flat_grid(n), 256, 0, s>>>(soft, n, order, static_cast<int>(ofdm::bits_per_symbol(order)), axis, llr);
  ORION_LAUNCH_CHECK();
}
void launch_ofdm_equalize(const f2* in, f2* out, long long nsym, const OfdmDev& c, int eq, hipStream_t s) {
  if (nsym < 1) return;
  k_ofdm_equalize<<<flat_grid(nsym * c.n), 256, 0, s>>>(in, out, nsym, c, eq);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
