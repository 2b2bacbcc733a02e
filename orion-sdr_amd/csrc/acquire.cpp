// acquire.cpp — the host side of acquire.hpp: ofdm_sync, earliest_accepted and the integer
// carrier-offset search in the reference's f32 operation order, and AcquireEngine, which
// queues the batched search of k_acquire.hip.
#include "acquire.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace orion {
namespace acquire {

namespace {
constexpr float kTau = 6.28318530717958647692f;
}

size_t search_end(size_t n, const Preamble& pre, size_t end) {
  const size_t total = pre.total_len();
  return std::min(end, n > total ? n - total : size_t{0});
}

bool search_ok(size_t n, float fs, const Preamble& pre, size_t start, size_t end) {
  if (pre.repeat_len == 0 || pre.num_repeats < 2 || !(fs > 0.0f)) return false;
  return start < search_end(n, pre, end);
}

void sc_metric(const float* iq, const Preamble& pre, size_t start, size_t end, float* p, float* r) {
  const size_t len = pre.repeat_len;
  for (size_t d = start; d < end; ++d) {
    float pr = 0.0f, pi = 0.0f, rr = 0.0f;
    for (size_t seg = 0; seg + 1 < pre.num_repeats; ++seg) {
      const float* a = iq + 2 * (d + seg * len);
      const float* b = a + 2 * len;
      float sr = 0.0f, si = 0.0f, se = 0.0f;  // correlate_segment: from zero, in sample order
      for (size_t i = 0; i < len; ++i) {
        const float ar = a[2 * i], ai = -a[2 * i + 1], br = b[2 * i], bi = b[2 * i + 1];
        sr += ar * br - ai * bi;
        si += ar * bi + ai * br;
        se += br * br + bi * bi;
      }
      pr += sr;
      pi += si;
      rr += se;
    }
    p[2 * (d - start)] = pr;
    p[2 * (d - start) + 1] = pi;
    r[d - start] = rr;
  }
}

float sc_score(float pr, float pi, float r) {
  float s = (pr * pr + pi * pi) / (r * r);
  if (s < 0.0f) s = 0.0f;
  if (s > 1.0f) s = 1.0f;
  return s;
}

float sc_cfo_den(size_t repeat_len, float fs) { return kTau * static_cast<float>(repeat_len) / fs; }

std::vector<SyncResult> ofdm_sync(const float* iq, size_t n, float fs, const Preamble& pre, size_t start, size_t end_arg,
                                  float* r_peak_out) {
  if (r_peak_out) *r_peak_out = 0.0f;
  if (!search_ok(n, fs, pre, start, end_arg)) return {};
  const size_t end = search_end(n, pre, end_arg), nd = end - start;
  std::vector<float> p(2 * nd), r(nd);
  sc_metric(iq, pre, start, end, p.data(), r.data());
  const float den = sc_cfo_den(pre.repeat_len, fs);
  std::vector<std::pair<float, SyncResult>> all;
  all.reserve(nd);
  float r_peak = 0.0f;
  for (size_t k = 0; k < nd; ++k) {
    if (r[k] <= 0.0f) continue;
    r_peak = std::fmax(r_peak, r[k]);
    SyncResult s{};
    s.start_sample = static_cast<int64_t>(start + k);
    s.score = sc_score(p[2 * k], p[2 * k + 1], r[k]);
    s.cfo_hz = std::atan2(p[2 * k + 1], p[2 * k]) / den;
    all.emplace_back(r[k], s);
  }
  if (r_peak_out) *r_peak_out = r_peak;
  if (all.empty() || r_peak <= 0.0f) return {};
  for (auto& e : all) e.first = e.second.score * (e.first / r_peak);
  // descending by the key, equal (and unordered) keys in offset order
  std::stable_sort(all.begin(), all.end(),
                   [](const std::pair<float, SyncResult>& a, const std::pair<float, SyncResult>& b) { return a.first > b.first; });
  std::vector<SyncResult> out;
  out.reserve(all.size());
  for (const auto& e : all) out.push_back(e.second);
  if (pre.training) {
    const size_t top = std::min(out.size(), kTopN);
    for (size_t k = 0; k < top; ++k)
      out[k].integer_cfo_bins = estimate_integer_cfo_bins(iq, n, fs, pre.tn_fft, pre.tcp,
                                                          static_cast<size_t>(out[k].start_sample) + pre.lead(), out[k].cfo_hz);
  }
  return out;
}

long long earliest_accepted(const SyncResult* results, size_t n, float thr, size_t cluster_len) {
  int64_t earliest = -1;
  for (size_t k = 0; k < n; ++k)
    if (results[k].score >= thr && (earliest < 0 || results[k].start_sample < earliest)) earliest = results[k].start_sample;
  if (earliest < 0) return -1;
  const int64_t span = static_cast<int64_t>(std::max<size_t>(cluster_len, 1));
  for (size_t k = 0; k < n; ++k)
    if (results[k].score >= thr && results[k].start_sample - earliest < span) return static_cast<long long>(k);
  return -1;
}

int32_t estimate_integer_cfo_bins(const float* iq, size_t n, float fs, size_t tn_fft, size_t tcp, size_t training_start,
                                  float frac, float* corr2) {
  const size_t total = tn_fft + tcp;
  if (corr2) std::fill(corr2, corr2 + tn_fft + 1, 0.0f);
  if (training_start + total > n) return 0;
  const ofdm::Fft fft(tn_fft, false);  // throws unless the size is one the transform takes
  std::vector<float> cor(2 * total), known(2 * tn_fft);
  ofdm::Rotator rot(-frac, fs);
  for (size_t i = 0; i < total; ++i) {  // Rotator::rotate_block (dsp/rotator.rs:74-84)
    float pr, pi;
    rot.next(&pr, &pi);
    const float a = iq[2 * (training_start + i)], b = iq[2 * (training_start + i) + 1];
    cor[2 * i] = std::fma(a, pr, -b * pi);
    cor[2 * i + 1] = std::fma(b, pr, a * pi);
  }
  float* freq = cor.data() + 2 * tcp;  // the CP-boundary window, no back-off
  ofdm::fft_inplace(freq, tn_fft, fft.twiddles().data(), false);
  ofdm::training_pattern(tn_fft, known.data());
  const long long nf = static_cast<long long>(tn_fft), max_shift = nf / 2;
  int32_t best_shift = 0;
  float best = -1.0f;
  for (long long shift = -max_shift; shift <= max_shift; ++shift) {
    float cr = 0.0f, ci = 0.0f;
    for (long long bin = 0; bin < nf; ++bin) {
      const long long src = ((bin + shift) % nf + nf) % nf;
      const float kr = known[2 * bin], ki = -known[2 * bin + 1], fr = freq[2 * src], fi = freq[2 * src + 1];
      cr += kr * fr - ki * fi;
      ci += kr * fi + ki * fr;
    }
    const float mag = cr * cr + ci * ci;
    if (corr2) corr2[shift + max_shift] = mag;
    if (mag > best) {
      best = mag;
      best_shift = static_cast<int32_t>(shift);
    }
  }
  return best_shift;
}

void rotate_block(float freq_hz, float fs, const float* in, size_t n, float* out) {
  ofdm::Rotator rot(freq_hz, fs);
  for (size_t i = 0; i < n; ++i) {
    float pr, pi;
    rot.next(&pr, &pi);
    const float a = in[2 * i], b = in[2 * i + 1];
    out[2 * i] = std::fma(a, pr, -b * pi);
    out[2 * i + 1] = std::fma(b, pr, a * pi);
  }
}

namespace {
// c *= (cos, sin) as num-complex multiplies: (a c - b d, a d + b c)
void turn(const float* in, float* out, size_t n, float angle) {
  const float s = std::sin(angle), c = std::cos(angle);
  for (size_t i = 0; i < n; ++i) {
    const float a = in[2 * i], b = in[2 * i + 1];
    out[2 * i] = a * c - b * s;
    out[2 * i + 1] = a * s + b * c;
  }
}
}  // namespace

void remove_common_phase_error(int order, float* syms, size_t n_sym, size_t n_data) {
  if (n_sym < 4 || n_data == 0) return;
  const size_t bps = ofdm::bits_per_symbol(order) * n_data;
  constexpr float kAlpha = 0.5f, kBeta = 0.05f;
  std::vector<float> llr(bps), ideal(2 * n_data), rotated(2 * n_data), measured(n_sym);
  std::vector<uint8_t> bits(bps);
  float phase = 0.0f, freq = 0.0f;
  for (size_t k = 0; k < n_sym; ++k) {
    turn(syms + 2 * k * n_data, rotated.data(), n_data, -phase);
    ofdm::soft_llr(order, rotated.data(), n_data, llr.data());
    for (size_t i = 0; i < bps; ++i) bits[i] = llr[i] <= 0.0f ? 1 : 0;
    ofdm::map_bits(order, bits.data(), n_data, ideal.data());
    float ar = 0.0f, ai = 0.0f;
    for (size_t i = 0; i < n_data; ++i) {  // acc += y * conj(ideal)
      const float yr = rotated[2 * i], yi = rotated[2 * i + 1], ir = ideal[2 * i], ii = -ideal[2 * i + 1];
      ar += yr * ir - yi * ii;
      ai += yr * ii + yi * ir;
    }
    const float err = (ar == 0.0f && ai == 0.0f) ? 0.0f : std::atan2(ai, ar);
    measured[k] = phase + err;
    phase += freq + kAlpha * err;
    freq += kBeta * err;
  }
  const float n = static_cast<float>(n_sym);
  const float sum_k = n * (n - 1.0f) / 2.0f;
  const float sum_k2 = (n - 1.0f) * n * (2.0f * n - 1.0f) / 6.0f;
  float sum_y = 0.0f, sum_ky = 0.0f;
  for (size_t k = 0; k < n_sym; ++k) {
    sum_y += measured[k];
    sum_ky += static_cast<float>(k) * measured[k];
  }
  const float denom = n * sum_k2 - sum_k * sum_k;
  if (std::fabs(denom) <= 1.1920929e-7f) return;
  const float slope = (n * sum_ky - sum_k * sum_y) / denom;
  const float intercept = (sum_y - slope * sum_k) / n;
  for (size_t k = 0; k < n_sym; ++k)
    turn(syms + 2 * k * n_data, syms + 2 * k * n_data, n_data, -(intercept + slope * static_cast<float>(k)));
}

void soft_demap_equalized(const ofdm::Config& c, const float* iq, size_t n_sym, const float* training_freq, float* syms,
                          float* llr) {
  ofdm::Demod demod(c);  // its gain stays 1
  ofdm::Equalizer eq(c, ofdm::kEqTrainingSymbolHold);
  eq.estimate_from_training_symbol(training_freq, c.plan.n_fft);
  const size_t nd = demod.grid().data_bins.size();
  size_t r = 0, w = 0;
  demod.process(iq, n_sym * c.samples_per_ofdm_symbol(), syms, n_sym * nd, &eq, &r, &w);
  if (w != n_sym * nd) throw std::invalid_argument("acquire: fewer symbols demodulated than asked for");
  remove_common_phase_error(c.constellation, syms, n_sym, nd);
  if (llr) ofdm::soft_llr(c.constellation, syms, n_sym * nd, llr);
}

}  // namespace acquire

// ---- AcquireEngine ------------------------------------------------------------------------
AcquireEngine::AcquireEngine(const acquire::Preamble& pre) : pre_(pre) {
  if (pre.training) {
    if (pre.tcp > pre.tn_fft) throw std::invalid_argument("acquire: a training prefix longer than its transform");
    fft_.reset(new FftDev(pre.tn_fft, false));  // throws unless the size is one the transform takes
  }
}

const f2* AcquireEngine::known(hipStream_t s) {
  if (known_.empty()) {
    std::vector<float> k(2 * pre_.tn_fft);
    ofdm::training_pattern(pre_.tn_fft, k.data());
    known_.set(k, s);
  }
  return known_.as<f2>();
}

void AcquireEngine::sync_batch(const void* iq, size_t ncap, size_t n, float fs, size_t start, size_t end_arg, float thr,
                               const SyncOut& o, hipStream_t s) {
  if (ncap == 0) return;
  if (!acquire::search_ok(n, fs, pre_, start, end_arg)) throw std::invalid_argument("acquire: an empty search range");
  if (n >= (size_t{1} << 31) || ncap >= (size_t{1} << 24)) throw std::invalid_argument("acquire: n < 2^31 and ncap < 2^24");
  if (pre_.lead() >= (size_t{1} << 24)) throw std::invalid_argument("acquire: the repeats span 2^24 samples or more");
  if (reinterpret_cast<uintptr_t>(iq) % 8) throw std::invalid_argument("acquire: cf32 buffer not 8-byte aligned");
  const size_t end = acquire::search_end(n, pre_, end_arg), nd = end - start;
  const long long nc = static_cast<long long>(ncap), nn = static_cast<long long>(n);
  const f2* x = static_cast<const f2*>(iq);
  launch_sc_metric(x, nc, nn, static_cast<int>(pre_.num_repeats), static_cast<int>(pre_.repeat_len),
                   static_cast<long long>(start), static_cast<long long>(nd), acquire::sc_cfo_den(pre_.repeat_len, fs), o, s);
  launch_sc_select(nc, static_cast<long long>(nd), static_cast<long long>(start), thr,
                   static_cast<long long>(pre_.total_len()), o, s);
  if (!pre_.training) return;
  const size_t nf = pre_.tn_fft, cand = ncap * acquire::kTopN;
  sym_.resize(cand * nf * 8);
  freq_.resize(cand * nf * 8);
  launch_icfo_gather(x, nc, nn, static_cast<long long>(nd), static_cast<long long>(start), static_cast<int>(pre_.lead()),
                     static_cast<int>(nf), static_cast<int>(pre_.tcp), fs, o, sym_.as<f2>(), s);
  fft_->batch(sym_.as<void>(), nf, freq_.as<void>(), nf, cand, s);
  launch_icfo_corr(freq_.as<f2>(), known(s), nc, nn, static_cast<int>(pre_.lead()), static_cast<int>(nf),
                   static_cast<int>(pre_.tcp), o, s);
}

void AcquireEngine::correct(const void* iq, size_t ncap, size_t n, float fs, size_t n_fft, const SyncOut& o, void* rows,
                            int32_t* avail, float* total_cfo, hipStream_t s) {
  if (ncap == 0 || n == 0) return;
  if (n >= (size_t{1} << 31) || ncap >= (size_t{1} << 24) || n_fft == 0)
    throw std::invalid_argument("acquire: n < 2^31, ncap < 2^24 and n_fft > 0");
  if (reinterpret_cast<uintptr_t>(iq) % 8 || reinterpret_cast<uintptr_t>(rows) % 8)
    throw std::invalid_argument("acquire: cf32 buffer not 8-byte aligned");
  launch_acq_correct(static_cast<const f2*>(iq), static_cast<long long>(ncap), static_cast<long long>(n),
                     fs / static_cast<float>(n_fft), fs, o, static_cast<f2*>(rows), avail, total_cfo, s);
}

void AcquireEngine::weights(const void* rows, size_t ncap, size_t n, size_t window, void* w, hipStream_t s) {
  if (ncap == 0) return;
  if (!pre_.training) throw std::invalid_argument("acquire: the preamble has no training symbol to estimate from");
  const size_t nf = pre_.tn_fft, at = pre_.lead() + window;
  if (window > pre_.tcp || at + nf > n) throw std::invalid_argument("acquire: the rows are shorter than the training symbol");
  freq_.resize(std::max(ncap * nf * 8, freq_.size()));
  fft_->batch(static_cast<const f2*>(rows) + at, n, freq_.as<void>(), nf, ncap, s);
  launch_acq_weights(freq_.as<f2>(), known(s), static_cast<long long>(ncap * nf), static_cast<int>(nf),
                     static_cast<f2*>(w), s);
}

}  // namespace orion
