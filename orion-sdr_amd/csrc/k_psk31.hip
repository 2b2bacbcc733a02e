// k_psk31.hip — PSK31 on the device: the batched soft Viterbi decode of QPSK31's rate 1/2,
// K = 5 convolutional code (codec/psk31.rs:95-160, viterbi_decode), and the demodulator bank
// (demodulate/psk31.rs, further down).
//
// The Viterbi decode is trellis_wave.hpp's engine (sixteen lanes per stream, four streams per
// wave64 workgroup; the exactness argument is there), minimising. What is this kernel's: every
// lane fetches the stream's soft values eight symbols ahead of the metric chain (their
// addresses do not depend on it); the branch metric is (s0 - e0) * (s0 - e0) + (s1 - e1) *
// (s1 - e1) against the branch's expected phasor, every * and + its own rounding
// (-ffp-contract=off); the first minimum wins the final-state search; all n_syms bits are written.
#include "hip_common.hpp"
#include "kernels.hpp"
#include "psk31.hpp"
#include "trellis_wave.hpp"

namespace orion {

namespace {
constexpr int kVitAhead = 8;  // symbols fetched ahead of the dependent chain
constexpr int kDemodAhead = 8;  // samples (and window values) the bank fetches ahead of its chains
}  // namespace

__global__ __launch_bounds__(64) void k_psk31_viterbi(const float* __restrict__ soft, long long nstreams,
                                                      long long n_syms, uint8_t* __restrict__ bits,
                                                      uint32_t* __restrict__ work) {
  const trellis::Wave<4> tw(nstreams);
  const float* S = soft + tw.row * 2 * n_syms;

  // the expected phasors of the branches from this state's two predecessors (psk31.rs:63-85)
  float e[2][2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t window = tw.inbit << 4 | static_cast<uint32_t>(tw.p0 + k);
    const uint32_t dibit = trellis::parity(window & 0x15) * 2 + trellis::parity(window & 0x13);
    e[k][0] = dibit == 0 ? 1.0f : (dibit == 3 ? -1.0f : 0.0f);
    e[k][1] = dibit == 2 ? 1.0f : (dibit == 1 ? -1.0f : 0.0f);
  }

  float pm = tw.st == 0 ? 0.0f : trellis::Minimise::start();
  float cur[2 * kVitAhead], nxt[2 * kVitAhead];
#pragma unroll
  for (int k = 0; k < 2 * kVitAhead; ++k) cur[k] = k < 2 * n_syms ? S[k] : 0.0f;

  for (long long t0 = 0; t0 < n_syms; t0 += kVitAhead) {
#pragma unroll
    for (int k = 0; k < 2 * kVitAhead; ++k) {
      const long long i = 2 * (t0 + kVitAhead) + k;
      nxt[k] = i < 2 * n_syms ? S[i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kVitAhead; ++k) {
      if (t0 + k < n_syms) {  // uniform over the wave
        const float s0 = cur[2 * k], s1 = cur[2 * k + 1];
        const float bm0 = (s0 - e[0][0]) * (s0 - e[0][0]) + (s1 - e[0][1]) * (s1 - e[0][1]);
        const float bm1 = (s0 - e[1][0]) * (s0 - e[1][0]) + (s1 - e[1][1]) * (s1 - e[1][1]);
        tw.store(work, t0 + k, tw.acs<trellis::Minimise>(pm, bm0, bm1));
      }
    }
#pragma unroll
    for (int k = 0; k < 2 * kVitAhead; ++k) cur[k] = nxt[k];
  }

  // psk31.rs:139-144: min_by keeps the first of equal minima (and the earlier of an unordered pair)
  uint32_t best = 0;
  float best_pm = __shfl(pm, 0, 16);
#pragma unroll
  for (int i = 1; i < 16; ++i) {
    const float v = __shfl(pm, i, 16);
    if (best_pm > v) {
      best_pm = v;
      best = i;
    }
  }
  tw.traceback(work, n_syms, best, bits + tw.stream * n_syms, n_syms);  // psk31.rs:147-157
}

// ---- the demodulator bank ------------------------------------------------------------------
// Bpsk31Demod / Qpsk31Demod::process (demodulate/psk31.rs:151-219, :329-396) for nstreams
// independent streams: one lane per stream, each running the reference's loop sample by
// sample over its channel of x [nch][n]. The chain is serial in time by construction (every
// sample's correction uses prev_sym, which the previous symbol's sum decides), so the
// parallelism is over streams alone. The records are sorted by channel and start sample, so
// the lanes of a wave read the same cache lines. A lane works a symbol at a time: within a
// symbol the loop tests nothing but its own bound and the rotator's renormalisation, samples
// and window values are fetched eight to sixteen ahead of the dependent chains (a chunk is
// loaded while the one before it runs), and the rotator recurrence and the accumulation are
// two independent chains the scheduler overlaps.
//
// The arithmetic is the host demodulator's (psk31.cpp) operation for operation: the fused
// form of Rotator::next with its renormalisation every 1024 steps (IEEE sqrt and divide), no
// rotator when the record has none, the unfused down-mix, acc += h * (s - prev * (1 - h)),
// and at each symbol the scale, the phase correction, the differential product, the
// decision, the phase error behind its mag_sq > 1e-6 guard and the wrap at +-pi. The one
// difference is phase_acc's sine and cosine: sincos_cr here, glibc on the host; they agree
// but for rare near-ties, and the loop is contractive, so the soft values
// follow the host's to a few ulp rather than bit for bit.
// State (count, acc, prev_sym, phase_acc, the rotator's z and renorm_ctr) lives in st and is
// carried across calls: chunked calls equal one call byte for byte.
__global__ __launch_bounds__(64) void k_psk31_demod(const f2* __restrict__ x, long long n, unsigned long long base,
                                                    const psk31::BankRecord* __restrict__ rec,
                                                    psk31::DemodState* __restrict__ st, int nstreams,
                                                    const float* __restrict__ hann, uint32_t sps,
                                                    float* __restrict__ soft, long long out_stride,
                                                    uint8_t* __restrict__ bits, unsigned long long* __restrict__ report) {
  const int tid = blockIdx.x * 64 + threadIdx.x;
  if (tid >= nstreams) return;
  const psk31::BankRecord R = rec[tid];
  psk31::DemodState S = st[tid];
  const f2* X = x + static_cast<long long>(R.channel) * n;
  float* O = soft + static_cast<long long>(R.slot) * out_stride;
  uint8_t* B = bits ? bits + static_cast<long long>(R.slot) * out_stride : nullptr;
  const uint32_t need = R.mode == psk31::kQpsk ? 2u : 1u, cap = R.out_cap;
  const float kPi = 3.14159265358979323846f, kTau = 6.28318530717958647692f;

  // the stream's first sample in this call: start counts from the bank's first call
  long long i = 0;
  if (R.start > base) i = R.start - base < static_cast<unsigned long long>(n) ? static_cast<long long>(R.start - base) : n;
  const long long i_first = i;
  uint32_t out_pos = 0;
  // A symbol at a time: the samples up to the next symbol dump (or the end of the input) run
  // in an inner loop whose only tests are its own bound and the rotator's renormalisation;
  // the input's end, the capacity and the dump are looked at once per run. Inside a run the
  // next kDemodAhead samples and window values are loaded while the chunk before them is
  // worked on, so the chains do not wait for memory.
  while (i < n && out_pos + need <= cap) {
    const long long left = n - i;
    const int to_dump = static_cast<int>(sps - S.count);
    const int run = left < to_dump ? static_cast<int>(left) : to_dump;
    const f2* Xp = X + i;
    const float* Hp = hann + S.count;
    f2 v[kDemodAhead], vn[kDemodAhead];
    float hw[kDemodAhead], hn[kDemodAhead];
#pragma unroll
    for (int u = 0; u < kDemodAhead; ++u) {
      v[u] = u < run ? Xp[u] : f2{0.0f, 0.0f};
      hw[u] = u < run ? Hp[u] : 0.0f;
    }
    for (int j = 0; j < run; j += kDemodAhead) {
#pragma unroll
      for (int u = 0; u < kDemodAhead; ++u) {
        const int k = j + kDemodAhead + u;
        vn[u] = k < run ? Xp[k] : f2{0.0f, 0.0f};
        hn[u] = k < run ? Hp[k] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kDemodAhead; ++u) {
        if (j + u < run) {
          float xr = v[u].x, xi = v[u].y;
          if (R.rot) {
            // Rotator::next, dsp/rotator.rs:44-61
            const float zr = __builtin_fmaf(S.z_re, R.w_re, -S.z_im * R.w_im);
            const float zi = __builtin_fmaf(S.z_im, R.w_re, S.z_re * R.w_im);
            S.z_re = zr;
            S.z_im = zi;
            S.renorm_ctr += 1u;
            if ((S.renorm_ctr & 0x3FFu) == 0u) {
              const float r2 = S.z_re * S.z_re + S.z_im * S.z_im;
              const float inv = 1.0f / sqrtf(r2);
              S.z_re *= inv;
              S.z_im *= inv;
            }
            const float re = xr * S.z_re - xi * S.z_im;
            const float im = xi * S.z_re + xr * S.z_im;
            xr = re;
            xi = im;
          }
          const float h = hw[u];
          const float one_minus_h = 1.0f - h;
          const float corr_re = xr - S.prev_re * one_minus_h;
          const float corr_im = xi - S.prev_im * one_minus_h;
          S.acc_re += h * corr_re;
          S.acc_im += h * corr_im;
        }
      }
#pragma unroll
      for (int u = 0; u < kDemodAhead; ++u) {
        v[u] = vn[u];
        hw[u] = hn[u];
      }
    }
    S.count += static_cast<uint32_t>(run);
    i += run;
    if (S.count == sps) {
      const float sr = S.acc_re * R.scale, si = S.acc_im * R.scale;
      S.acc_re = 0.0f;
      S.acc_im = 0.0f;
      S.count = 0u;
      float sin_pa, cos_pa;
      sincos_cr(S.phase_acc, &sin_pa, &cos_pa);
      const float sym_re = sr * cos_pa + si * sin_pa;
      const float sym_im = si * cos_pa - sr * sin_pa;
      const float d_re = sym_re * S.prev_re + sym_im * S.prev_im;
      const float d_im = sym_im * S.prev_re - sym_re * S.prev_im;
      float cross_im;
      if (need == 1u) {
        O[out_pos] = d_re;
        if (B) B[out_pos] = d_re >= 0.0f ? 1 : 0;
        out_pos += 1u;
        const float dec_re = d_re >= 0.0f ? 1.0f : -1.0f;
        cross_im = d_im * dec_re;
      } else {
        O[out_pos] = d_re;
        O[out_pos + 1u] = d_im;
        // no hard bits for a QPSK31 pair: one of its components is noise about zero that nobody
        // slices; QPSK31's decisions are the Viterbi decoder's
        out_pos += 2u;
        float dec_re, dec_im;
        if (fabsf(d_re) >= fabsf(d_im)) {
          dec_re = d_re >= 0.0f ? 1.0f : -1.0f;
          dec_im = 0.0f;
        } else {
          dec_re = 0.0f;
          dec_im = d_im >= 0.0f ? 1.0f : -1.0f;
        }
        cross_im = d_im * dec_re - d_re * dec_im;
      }
      const float mag_sq = d_re * d_re + d_im * d_im;
      const float phase_err = mag_sq > 1e-6f ? cross_im / sqrtf(mag_sq) : 0.0f;
      S.phase_acc += 0.05f * phase_err;
      if (S.phase_acc > kPi) S.phase_acc -= kTau;
      if (S.phase_acc < -kPi) S.phase_acc += kTau;
      S.prev_re = sym_re;
      S.prev_im = sym_im;
    }
  }
  st[tid] = S;
  report[2 * static_cast<long long>(R.slot)] = static_cast<unsigned long long>(i - i_first);
  report[2 * static_cast<long long>(R.slot) + 1] = out_pos;
}

void launch_psk31_demod(const f2* x_dev, long long n, unsigned long long base, const psk31::BankRecord* rec_dev,
                        psk31::DemodState* st_dev, int nstreams, const float* hann_dev, uint32_t sps, float* soft_dev,
                        long long out_stride, uint8_t* bits_dev, unsigned long long* report_dev, hipStream_t s) {
  if (nstreams < 1) return;
  k_psk31_demod<<<div_up(nstreams, 64), 64, 0, s>>>(x_dev, n, base, rec_dev, st_dev, nstreams, hann_dev, sps, soft_dev,
                                                    out_stride, bits_dev, report_dev);
  ORION_LAUNCH_CHECK();
}

// ---- the modulator -----------------------------------------------------------------------------
// Bpsk31Mod / Qpsk31Mod::modulate_bits (modulate/psk31.rs:164-192, :302-338) for a batch of bit
// streams, one lane per output sample: write_symbol's gain * (p0 + h * (p1 - p0)) per
// component with every operation its own rounding (:79-101), then, with an RF stage,
// rotate_block's fused form (dsp/rotator.rs:74-84) on the phasors of a fresh Rotator, which
// the host tabulates from the reference's own recurrence (rot [>= n_syms * sps]). ph
// [nstreams][n_syms + 1] are each stream's symbol phasors as the host's arithmetic gives
// them, signed zeros included, so the output is the host modulator's byte for byte.
__global__ __launch_bounds__(256) void k_psk31_mod(const f2* __restrict__ ph, const float* __restrict__ hann,
                                                   const f2* __restrict__ rot, int nstreams, long long n_syms,
                                                   uint32_t sps, float gain, f2* __restrict__ out) {
  const long long per = n_syms * sps;
  const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= per * nstreams) return;
  const long long st = t / per, i = t % per;
  const long long k = i / sps;
  const f2 p0 = ph[st * (n_syms + 1) + k], p1 = ph[st * (n_syms + 1) + k + 1];
  const float h = hann[i % sps];
  const float dr = p1.x - p0.x, di = p1.y - p0.y;
  const float a = gain * (p0.x + h * dr), b = gain * (p0.y + h * di);
  f2 v = {a, b};
  if (rot) {
    const f2 z = rot[i];
    v.x = __builtin_fmaf(a, z.x, -b * z.y);
    v.y = __builtin_fmaf(b, z.x, a * z.y);
  }
  out[t] = v;
}

void launch_psk31_mod(const f2* ph_dev, const float* hann_dev, const f2* rot_dev, int nstreams, long long n_syms,
                      uint32_t sps, float gain, f2* out_dev, hipStream_t s) {
  const long long total = n_syms * sps * nstreams;
  if (total < 1) return;
  if (total > 0x7fffffffLL * 256) throw std::invalid_argument("psk31 mod: too many samples for one launch");
  k_psk31_mod<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(ph_dev, hann_dev, rot_dev, nstreams, n_syms, sps,
                                                                          gain, out_dev);
  ORION_LAUNCH_CHECK();
}

// ---- band synthesis ----------------------------------------------------------------------------
// out [nch][n] cf32 = (accumulate ? out : 0) + every signal of the channel, one lane per output
// sample, the signals added in table order with plain f32 adds (bit-reproducible). A signal
// is what k_psk31_mod gives for its bits from a fresh modulator, placed at its offset and
// clipped to the channel, except for the RF stage: a lane cannot run the Rotator's recurrence
// from the signal's start, so the phasor of output j is the closed form of the f32 step,
// phasor_at((j + 1) step_q64), as k_ft_synth does; it follows the recurrence to its rounding
// drift (2 d0 + 2e-6 per unit gain, d0 taken per case).
__global__ __launch_bounds__(256) void k_psk31_synth(const psk31::SynthRecord* __restrict__ rec,
                                                     const uint32_t* __restrict__ rows, const f2* __restrict__ ph,
                                                     const float* __restrict__ hann, uint32_t sps, int nch,
                                                     long long n, int accumulate, f2* __restrict__ out) {
  const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n * nch) return;
  const long long ch = t / n, i = t % n;
  f2 v = accumulate ? out[t] : f2{0.0f, 0.0f};
  for (uint32_t r = rows[ch]; r < rows[ch + 1]; ++r) {
    const psk31::SynthRecord R = rec[r];
    if (i < R.offset || i - R.offset >= R.len) continue;
    const long long j = i - R.offset;
    const long long k = j / sps;
    const f2 p0 = ph[R.ph0 + k], p1 = ph[R.ph0 + k + 1];
    const float h = hann[j % sps];
    const float dr = p1.x - p0.x, di = p1.y - p0.y;
    float a = R.gain * (p0.x + h * dr), b = R.gain * (p0.y + h * di);
    if (R.rot) {
      const f2 z = phasor_at(static_cast<uint64_t>(j + 1) * R.step_q64);
      const float re = __builtin_fmaf(a, z.x, -b * z.y);
      const float im = __builtin_fmaf(b, z.x, a * z.y);
      a = re;
      b = im;
    }
    v.x += a;
    v.y += b;
  }
  out[t] = v;
}

void launch_psk31_synth(const psk31::SynthRecord* rec_dev, const uint32_t* rows_dev, const f2* ph_dev,
                        const float* hann_dev, uint32_t sps, int nch, long long n, bool accumulate, f2* out_dev,
                        hipStream_t s) {
  const long long total = n * nch;
  if (total < 1) return;
  if (total > 0x7fffffffLL * 256) throw std::invalid_argument("psk31 synth: too many samples for one launch");
  k_psk31_synth<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(rec_dev, rows_dev, ph_dev, hann_dev, sps, nch, n,
                                                                            accumulate ? 1 : 0, out_dev);
  ORION_LAUNCH_CHECK();
}

// ---- the carrier search -----------------------------------------------------------------------
// psk31_sync's search (sync/psk31_sync.rs:82-203) on a device log waterfall [nch][num_syms]
// [num_bins], in four small kernels whose results do not depend on scheduling:
//  k_psk31_medians   one lane per (channel, bin): the median over time by exact selection
//                    (a 32-pass radix selection on the ordered-integer image of the floats:
//                    the median is one of the values, or the f32 mean of the two middle ones,
//                    whatever the method);
//  k_psk31_floor     one lane per channel: the median of its bins' medians, the same way;
//  k_psk31_runs      one lane per (channel, bin): the reference's serial scan over the symbols,
//                    the f32 run sum in symbol order, and the bin's own max_cand best runs kept
//                    sorted (score descending, the earlier run first among equals);
//  k_psk31_merge     one lane per channel: the bins' lists merged, ties to the lower bin, so
//                    the order is score, then freq_bin, then time_sym, as the host search
//                    (psk31.cpp find_carriers) defines it. No list is appended to in arrival order.
namespace {
__device__ __forceinline__ uint32_t f_key(float v) {  // order-preserving; NaN last
  if (v != v) return 0xFFFFFFFFu;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// the k-th smallest (k < n) of p[0], p[stride], ..., p[(n - 1) stride]
__device__ float select_kth(const float* __restrict__ p, long long stride, int n, int k) {
  uint32_t prefix = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t high = bit == 31 ? 0u : ~((2u << bit) - 1u);  // the bits above this one
    int zeros = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t key = f_key(p[i * stride]);
      zeros += ((key & high) == prefix && ((key >> bit) & 1u) == 0u) ? 1 : 0;
    }
    if (k >= zeros) {
      k -= zeros;
      prefix |= 1u << bit;
    }
  }
  return f_unkey(prefix);
}
// median_f32, psk31_sync.rs:242-253
__device__ float median_of(const float* __restrict__ p, long long stride, int n) {
  if (n == 0) return 0.0f;
  const int mid = n / 2;
  if (n % 2) return select_kth(p, stride, n, mid);
  return (select_kth(p, stride, n, mid - 1) + select_kth(p, stride, n, mid)) * 0.5f;
}
}  // namespace

__global__ __launch_bounds__(64) void k_psk31_medians(const float* __restrict__ wf, int nch, int num_syms, int num_bins,
                                                      float* __restrict__ med) {
  const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
  if (t >= static_cast<long long>(nch) * num_bins) return;
  const long long ch = t / num_bins, bin = t % num_bins;
  med[t] = median_of(wf + ch * num_syms * num_bins + bin, num_bins, num_syms);
}

__global__ __launch_bounds__(64) void k_psk31_floor(const float* __restrict__ med, int nch, int num_bins,
                                                    float* __restrict__ floor_out) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= nch) return;
  floor_out[ch] = median_of(med + static_cast<long long>(ch) * num_bins, 1, num_bins);
}

__global__ __launch_bounds__(64) void k_psk31_runs(const float* __restrict__ wf, const float* __restrict__ med,
                                                   const float* __restrict__ floor_in, int nch, int num_syms,
                                                   int num_bins, int min_run, float ln_margin, int max_cand,
                                                   SyncCandidate* __restrict__ runs, uint32_t* __restrict__ nruns) {
  const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
  if (t >= static_cast<long long>(nch) * num_bins) return;
  const long long ch = t / num_bins;
  const int bin = static_cast<int>(t % num_bins);
  const float* W = wf + ch * num_syms * num_bins;
  SyncCandidate* L = runs + t * max_cand;
  const float bin_median = med[t];
  const float per_bin_threshold = bin_median + ln_margin;
  const bool loud = bin_median > floor_in[ch] + ln_margin;
  const float neg_inf = -__builtin_huge_valf();
  uint32_t kept = 0;
  bool in_run = false;
  int run_start = 0, run_len = 0;
  float run_sum = 0.0f;
  for (int sym = 0; sym <= num_syms; ++sym) {
    bool is_peak = false;
    float e = 0.0f;
    if (sym < num_syms) {
      const float* row = W + static_cast<long long>(sym) * num_bins;
      e = row[bin];
      const float e_left = bin > 0 ? row[bin - 1] : neg_inf;
      const float e_right = bin + 1 < num_bins ? row[bin + 1] : neg_inf;
      is_peak = (e > per_bin_threshold || loud) && e >= e_left && e >= e_right;
    }
    if (is_peak) {
      if (!in_run) {
        in_run = true;
        run_start = sym;
        run_sum = 0.0f;
        run_len = 0;
      }
      run_sum += e;
      run_len += 1;
    } else if (in_run) {  // a run ends here, or at the end of the buffer (sym == num_syms)
      in_run = false;
      if (run_len >= min_run) {
        const float score = run_sum / static_cast<float>(run_len);
        // after every kept run that scores at least as much (they are earlier in time)
        uint32_t pos = kept;
        while (pos > 0 && score > L[pos - 1].score) --pos;
        if (pos < static_cast<uint32_t>(max_cand)) {
          const uint32_t last = kept < static_cast<uint32_t>(max_cand) ? kept : static_cast<uint32_t>(max_cand) - 1u;
          for (uint32_t j = last; j > pos; --j) L[j] = L[j - 1];
          L[pos] = SyncCandidate{run_start, static_cast<uint32_t>(bin), score};
          if (kept < static_cast<uint32_t>(max_cand)) ++kept;
        }
      }
      run_len = 0;
    }
  }
  nruns[t] = kept;
}

__global__ __launch_bounds__(64) void k_psk31_merge(const SyncCandidate* __restrict__ runs,
                                                    const uint32_t* __restrict__ nruns, int nch, int num_bins,
                                                    int max_cand, uint32_t* __restrict__ head,
                                                    SyncCandidate* __restrict__ cand, uint32_t* __restrict__ count) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= nch) return;
  const long long b0 = static_cast<long long>(ch) * num_bins;
  for (int b = 0; b < num_bins; ++b) head[b0 + b] = 0u;
  SyncCandidate* C = cand + static_cast<long long>(ch) * max_cand;
  uint32_t n = 0;
  for (; n < static_cast<uint32_t>(max_cand); ++n) {
    int best = -1;
    float best_score = 0.0f;
    for (int b = 0; b < num_bins; ++b) {
      const uint32_t h = head[b0 + b];
      if (h >= nruns[b0 + b]) continue;
      const float sc = runs[(b0 + b) * max_cand + h].score;
      if (best < 0 || sc > best_score) {  // strict: ties stay with the lower bin
        best = b;
        best_score = sc;
      }
    }
    if (best < 0) break;
    C[n] = runs[(b0 + best) * max_cand + head[b0 + best]];
    head[b0 + best] += 1u;
  }
  count[ch] = n;
  for (uint32_t k = n; k < static_cast<uint32_t>(max_cand); ++k) C[k] = SyncCandidate{0, 0u, 0.0f};
}

// One lane per candidate slot: the bank record and the initial state of a BPSK31 stream started
// as record_candidate starts it (psk31_sync.rs:209-239): Bpsk31Demod::new(fs, base_hz + bin *
// 31.25, 1.0) from sample time_sym * sps, out_cap soft values. steps [num_bins][3]: the bin's
// Rotator step (host cosf / sinf, so the stream is the host's) and whether it has a rotator.
// A slot past its channel's count gets a stream of capacity 0, which reads nothing.
__global__ __launch_bounds__(64) void k_psk31_cand_records(const SyncCandidate* __restrict__ cand,
                                                           const uint32_t* __restrict__ count, int nch, int max_cand,
                                                           const float* __restrict__ steps, uint32_t sps,
                                                           uint32_t out_cap, float scale,
                                                           psk31::BankRecord* __restrict__ rec,
                                                           psk31::DemodState* __restrict__ st) {
  const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
  if (t >= static_cast<long long>(nch) * max_cand) return;
  const uint32_t ch = static_cast<uint32_t>(t / max_cand), k = static_cast<uint32_t>(t % max_cand);
  const bool live = k < count[ch];
  const SyncCandidate c = cand[t];
  psk31::BankRecord r;
  r.start = live ? static_cast<uint64_t>(c.time_sym) * sps : 0ull;
  r.mode = psk31::kBpsk;
  r.channel = ch;
  r.slot = static_cast<uint32_t>(t);
  r.out_cap = live ? out_cap : 0u;
  r.rot = live && steps[3 * c.freq_bin + 2] != 0.0f ? 1u : 0u;
  r.w_re = live ? steps[3 * c.freq_bin] : 1.0f;
  r.w_im = live ? steps[3 * c.freq_bin + 1] : 0.0f;
  r.scale = scale;
  rec[t] = r;
  st[t] = psk31::DemodState{0u, 0u, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.0f};
}

void launch_psk31_carriers(const float* wf_dev, int nch, int num_syms, int num_bins, int min_run, float ln_margin,
                           int max_cand, float* med_dev, float* floor_dev, SyncCandidate* runs_dev, uint32_t* nruns_dev,
                           uint32_t* head_dev, SyncCandidate* cand_dev, uint32_t* count_dev, hipStream_t s) {
  if (nch < 1 || max_cand < 1) return;
  const long long cells = static_cast<long long>(nch) * num_bins;
  if (cells > 0) {
    k_psk31_medians<<<div_up(cells, 64), 64, 0, s>>>(wf_dev, nch, num_syms, num_bins, med_dev);
    ORION_LAUNCH_CHECK();
  }
  k_psk31_floor<<<div_up(nch, 64), 64, 0, s>>>(med_dev, nch, num_bins, floor_dev);
  ORION_LAUNCH_CHECK();
  if (cells > 0) {
    k_psk31_runs<<<div_up(cells, 64), 64, 0, s>>>(wf_dev, med_dev, floor_dev, nch, num_syms, num_bins, min_run, ln_margin,
                                                  max_cand, runs_dev, nruns_dev);
    ORION_LAUNCH_CHECK();
  }
  k_psk31_merge<<<div_up(nch, 64), 64, 0, s>>>(runs_dev, nruns_dev, nch, num_bins, max_cand, head_dev, cand_dev, count_dev);
  ORION_LAUNCH_CHECK();
}

void launch_psk31_cand_records(const SyncCandidate* cand_dev, const uint32_t* count_dev, int nch, int max_cand,
                               const float* steps_dev, uint32_t sps, uint32_t out_cap, float scale,
                               psk31::BankRecord* rec_dev, psk31::DemodState* st_dev, hipStream_t s) {
  if (nch < 1 || max_cand < 1) return;
  k_psk31_cand_records<<<div_up(static_cast<long long>(nch) * max_cand, 64), 64, 0, s>>>(
      cand_dev, count_dev, nch, max_cand, steps_dev, sps, out_cap, scale, rec_dev, st_dev);
  ORION_LAUNCH_CHECK();
}

void launch_psk31_viterbi(const float* soft_dev, long long nstreams, long long n_syms, uint8_t* bits_dev,
                          uint32_t* work_dev, hipStream_t s) {
  if (nstreams < 1 || n_syms < 1) return;
  if (nstreams > 0x7fffffffLL - 3 || n_syms > 0x7fffffffLL)
    throw std::invalid_argument("psk31 viterbi: nstreams <= 2^31 - 4 and n_syms <= 2^31 - 1");
  k_psk31_viterbi<<<static_cast<unsigned>((nstreams + 3) / 4), 64, 0, s>>>(soft_dev, nstreams, n_syms, bits_dev, work_dev);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
