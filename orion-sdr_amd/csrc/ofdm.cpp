// ofdm.cpp — the OFDM symbol layer in scalar f32 on the host (ofdm.hpp). No HIP: the file
// also builds with the host compiler alone (tests/ofdm_host).
#include "ofdm.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <unordered_set>

namespace orion {
namespace ofdm {

namespace {
constexpr float kFrac1Sqrt2 = 0.70710678118654752440f;  // std::f32::consts::FRAC_1_SQRT_2
constexpr float kSqrt2 = 1.41421356237309504880f;       // std::f32::consts::SQRT_2
constexpr float kPi = 3.14159265358979323846f;
constexpr float kTau = 6.28318530717958647692f;

int32_t rem_euclid(int32_t a, int32_t n) {
  const int32_t r = a % n;
  return r < 0 ? r + n : r;
}
void index_bounds(size_t n_fft, int32_t* lo, int32_t* hi) {  // config.rs:211-214
  const int32_t n = static_cast<int32_t>(n_fft);
  *lo = -(n / 2);
  *hi = (n - 1) / 2;
}
size_t qam_bits(int order) { return order == kQam16 ? 4 : order == kQam64 ? 6 : order == kQam256 ? 8 : 0; }

// QamMapper::axis_amp, modulate/qam.rs:92-101
float axis_amp(const float* table, const uint8_t* in, size_t k) {
  size_t idx = 0;
  for (size_t b = 0; b < k; ++b) idx = (idx << 1) | (in[b] & 1u);
  return table[idx];
}
// QamDecider::decide_axis, demodulate/qam.rs:120-140
void decide_axis(const float* thr, size_t k, float v, uint8_t* out) {
  const size_t m = size_t{1} << k;
  size_t nat = 0;
  for (size_t t = 0; t + 1 < m; ++t)
    if (v > thr[t]) nat += 1;
  const size_t gray = nat ^ (nat >> 1);
  for (size_t b = 0; b < k; ++b) out[b] = static_cast<uint8_t>((gray >> (k - 1 - b)) & 1u);
}
// qam_axis_soft_llr, demodulate/ofdm.rs:606-627
void axis_llr(const float* table, size_t k, float v, float* out) {
  const size_t m = size_t{1} << k;
  for (size_t b = 0; b < k; ++b) {
    const size_t shift = k - 1 - b;
    float d0 = std::numeric_limits<float>::infinity(), d1 = d0;
    for (size_t gray = 0; gray < m; ++gray) {
      const float d = (v - table[gray]) * (v - table[gray]);
      if (((gray >> shift) & 1u) == 0)
        d0 = std::fmin(d0, d);
      else
        d1 = std::fmin(d1, d);
    }
    out[b] = d1 - d0;
  }
}
}  // namespace

size_t bits_per_symbol(int order) {
  switch (order) {
    case kBpsk: return 1;
    case kQpsk: return 2;
    case kQam16: return 4;
    case kQam64: return 6;
    case kQam256: return 8;
    default: return 0;
  }
}

float axis_scale(size_t bits) {
  const size_t m = size_t{1} << (bits / 2);
  const double avg = 2.0 * static_cast<double>(m * m - 1) / 3.0;
  return static_cast<float>(1.0 / std::sqrt(avg));
}

void axis_table(size_t bits, float* t) {
  const size_t m = size_t{1} << (bits / 2);
  const float scale = axis_scale(bits);
  for (size_t i = 0; i < 16; ++i) t[i] = 0.0f;
  for (size_t g = 0; g < m; ++g) t[g ^ (g >> 1)] = (static_cast<float>(2 * g + 1) - static_cast<float>(m)) * scale;
}

void threshold_table(size_t bits, float* t) {
  const size_t m = size_t{1} << (bits / 2);
  const float scale = axis_scale(bits);
  for (size_t i = 0; i < 15; ++i) t[i] = 0.0f;
  for (size_t j = 0; j + 1 < m; ++j) t[j] = (static_cast<float>(2 * j) - static_cast<float>(m - 2)) * scale;
}

void map_bits(int order, const uint8_t* bits, size_t n, float* s) {
  if (order == kBpsk) {
    for (size_t i = 0; i < n; ++i) {
      s[2 * i] = (bits[i] & 1u) == 0 ? 1.0f : -1.0f;
      s[2 * i + 1] = 0.0f;
    }
  } else if (order == kQpsk) {
    for (size_t i = 0; i < n; ++i) {
      s[2 * i] = (bits[2 * i] & 1u) == 0 ? kFrac1Sqrt2 : -kFrac1Sqrt2;
      s[2 * i + 1] = (bits[2 * i + 1] & 1u) == 0 ? kFrac1Sqrt2 : -kFrac1Sqrt2;
    }
  } else {
    const size_t nb = qam_bits(order), k = nb / 2;
    if (nb == 0) throw std::invalid_argument("ofdm: unknown constellation");
    float table[16];
    axis_table(nb, table);
    for (size_t i = 0; i < n; ++i) {
      s[2 * i] = axis_amp(table, bits + i * nb, k);
      s[2 * i + 1] = axis_amp(table, bits + i * nb + k, k);
    }
  }
}

void decide(int order, const float* s, size_t n, uint8_t* bits) {
  if (order == kBpsk) {
    for (size_t i = 0; i < n; ++i) bits[i] = s[2 * i] < 0.0f ? 1 : 0;
  } else if (order == kQpsk) {
    for (size_t i = 0; i < n; ++i) {
      bits[2 * i] = s[2 * i] < 0.0f ? 1 : 0;
      bits[2 * i + 1] = s[2 * i + 1] < 0.0f ? 1 : 0;
    }
  } else {
    const size_t nb = qam_bits(order), k = nb / 2;
    if (nb == 0) throw std::invalid_argument("ofdm: unknown constellation");
    float thr[15];
    threshold_table(nb, thr);
    for (size_t i = 0; i < n; ++i) {
      decide_axis(thr, k, s[2 * i], bits + i * nb);
      decide_axis(thr, k, s[2 * i + 1], bits + i * nb + k);
    }
  }
}

void soft_llr(int order, const float* s, size_t n, float* llr) {
  if (order == kBpsk) {
    for (size_t i = 0; i < n; ++i) llr[i] = 4.0f * s[2 * i];
  } else if (order == kQpsk) {
    const float scale = 4.0f * kSqrt2;
    for (size_t i = 0; i < n; ++i) {
      llr[2 * i] = scale * s[2 * i];
      llr[2 * i + 1] = scale * s[2 * i + 1];
    }
  } else {
    const size_t nb = qam_bits(order), k = nb / 2;
    if (nb == 0) throw std::invalid_argument("ofdm: unknown constellation");
    float table[16];
    axis_table(nb, table);
    for (size_t i = 0; i < n; ++i) {
      axis_llr(table, k, s[2 * i], llr + i * nb);
      axis_llr(table, k, s[2 * i + 1], llr + i * nb + k);
    }
  }
}

// ---- CarrierPlan ------------------------------------------------------------------------
int plan_validate(const Plan& p, int32_t* bad) {
  int32_t lo, hi, dummy;
  if (!bad) bad = &dummy;
  *bad = 0;
  if (p.data.empty()) return kPlanEmptyData;
  index_bounds(p.n_fft, &lo, &hi);
  for (int32_t idx : p.data)
    if (idx < lo || idx > hi) return *bad = idx, kPlanOutOfRange;
  for (int32_t idx : p.pilot_idx)
    if (idx < lo || idx > hi) return *bad = idx, kPlanOutOfRange;
  std::unordered_set<int32_t> seen;
  for (int32_t idx : p.data)
    if (!seen.insert(idx).second) return *bad = idx, kPlanOverlap;
  for (int32_t idx : p.pilot_idx)
    if (!seen.insert(idx).second) return *bad = idx, kPlanOverlap;
  return kPlanOk;
}

int plan_validate_edge_guard(const Plan& p, size_t edge_guard, int32_t* bad) {
  int32_t lo, hi, dummy;
  if (!bad) bad = &dummy;
  const int rc = plan_validate(p, bad);
  if (rc != kPlanOk) return rc;
  index_bounds(p.n_fft, &lo, &hi);
  const int64_t g = static_cast<int64_t>(std::min<size_t>(edge_guard, size_t{1} << 30));
  const int64_t glo = lo + g, ghi = hi - g;
  for (int32_t idx : p.data)
    if (idx < glo || idx > ghi) return *bad = idx, kPlanInGuardBand;
  for (int32_t idx : p.pilot_idx)
    if (idx < glo || idx > ghi) return *bad = idx, kPlanInGuardBand;
  return kPlanOk;
}

void plan_contiguous_data(Plan& p, size_t edge_guard, bool include_dc) {
  int32_t lo, hi;
  index_bounds(p.n_fft, &lo, &hi);
  const int64_t g = static_cast<int64_t>(std::min<size_t>(edge_guard, size_t{1} << 30));
  const std::unordered_set<int32_t> pilots(p.pilot_idx.begin(), p.pilot_idx.end());
  for (int64_t idx = lo + 1 + g; idx <= hi - g; ++idx) {
    if (idx == 0 && !include_dc) continue;
    if (pilots.count(static_cast<int32_t>(idx))) continue;
    p.data.push_back(static_cast<int32_t>(idx));
  }
}

size_t plan_occupied_half_carriers(const Plan& p) {
  size_t m = 0;
  for (int32_t idx : p.data) m = std::max<size_t>(m, static_cast<size_t>(std::abs(static_cast<int64_t>(idx))));
  for (int32_t idx : p.pilot_idx) m = std::max<size_t>(m, static_cast<size_t>(std::abs(static_cast<int64_t>(idx))));
  return m;
}

std::vector<size_t> plan_occupied_bins(const Plan& p) {
  std::vector<size_t> bins;
  if (p.n_fft == 0) return bins;
  const int32_t n = static_cast<int32_t>(p.n_fft);
  for (int32_t idx : p.data) bins.push_back(static_cast<size_t>(rem_euclid(idx, n)));
  for (int32_t idx : p.pilot_idx) bins.push_back(static_cast<size_t>(rem_euclid(idx, n)));
  std::sort(bins.begin(), bins.end());
  bins.erase(std::unique(bins.begin(), bins.end()), bins.end());
  return bins;
}

Grid grid_from_plan(const Plan& p) {
  int32_t bad = 0;
  const int rc = plan_validate(p, &bad);
  if (rc != kPlanOk)
    throw std::invalid_argument(rc == kPlanEmptyData ? std::string("ofdm: no data carriers specified")
                                : rc == kPlanOverlap
                                    ? "ofdm: carrier index " + std::to_string(bad) + " is assigned more than one role"
                                    : "ofdm: carrier index " + std::to_string(bad) + " is out of range for n_fft");
  if (p.pilot_val.size() != 2 * p.pilot_idx.size()) throw std::invalid_argument("ofdm: one value per pilot carrier");
  Grid g;
  g.n_fft = p.n_fft;
  const int32_t n = static_cast<int32_t>(p.n_fft);
  for (int32_t idx : p.data) g.data_bins.push_back(static_cast<uint32_t>(rem_euclid(idx, n)));
  for (int32_t idx : p.pilot_idx) g.pilot_bins.push_back(static_cast<uint32_t>(rem_euclid(idx, n)));
  g.pilot_val = p.pilot_val;
  return g;
}

// ---- the transform ----------------------------------------------------------------------
bool fft_size_ok(size_t n) { return n >= 8 && n <= 4096 && (n & (n - 1)) == 0; }

std::vector<float> fft_twiddles(size_t n) {
  std::vector<float> tw(n);  // n / 2 pairs
  for (size_t k = 0; k < n / 2; ++k) {
    const double a = 2.0 * 3.14159265358979323846 * static_cast<double>(k) / static_cast<double>(n);
    tw[2 * k] = static_cast<float>(std::cos(a));
    tw[2 * k + 1] = static_cast<float>(-std::sin(a));
  }
  return tw;
}

void fft_inplace(float* x, size_t n, const float* tw, bool inverse) {
  size_t bits = 0;
  while ((size_t{1} << bits) < n) ++bits;
  for (size_t i = 0; i < n; ++i) {
    size_t r = 0;
    for (size_t b = 0; b < bits; ++b) r |= ((i >> b) & 1u) << (bits - 1 - b);
    if (r > i) {
      std::swap(x[2 * i], x[2 * r]);
      std::swap(x[2 * i + 1], x[2 * r + 1]);
    }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const size_t half = len / 2, step = n / len;
    for (size_t base = 0; base < n; base += len) {
      for (size_t j = 0; j < half; ++j) {
        float* a = x + 2 * (base + j);
        float* b = x + 2 * (base + j + half);
        const float wr = tw[2 * j * step], wi = inverse ? -tw[2 * j * step + 1] : tw[2 * j * step + 1];
        const float tr = b[0] * wr - b[1] * wi, ti = b[0] * wi + b[1] * wr;
        b[0] = a[0] - tr;
        b[1] = a[1] - ti;
        a[0] = a[0] + tr;
        a[1] = a[1] + ti;
      }
    }
  }
  if (inverse) {
    const float g = 1.0f / static_cast<float>(n);
    for (size_t i = 0; i < 2 * n; ++i) x[i] = x[i] * g;
  }
}

Fft::Fft(size_t n, bool inverse) : n_(n), inv_(inverse) {
  if (!fft_size_ok(n)) throw std::invalid_argument("ofdm: n_fft must be a power of two from 8 to 4096");
  tw_ = fft_twiddles(n);
}

void Fft::process(const float* in, size_t n_in, float* out, size_t out_cap, size_t* in_read,
                  size_t* out_written) const {
  *in_read = *out_written = 0;
  if (n_in < n_ || out_cap < n_) return;
  if (out != in) std::memmove(out, in, 2 * n_ * sizeof(float));
  fft_inplace(out, n_, tw_.data(), inv_);
  *in_read = *out_written = n_;
}

std::vector<float> window_ramp(size_t symbol_len, size_t roll_off) {
  const size_t l = std::min(roll_off, symbol_len / 2);
  std::vector<float> r(l);
  for (size_t i = 0; i < l; ++i) {
    const float x = kPi * (static_cast<float>(i) + 0.5f) / static_cast<float>(l);
    r[i] = 0.5f * (1.0f - std::cos(x));
  }
  return r;
}

void window_apply(float* s, size_t n, const std::vector<float>& ramp) {
  for (size_t i = 0; i < ramp.size(); ++i) {
    const float w = ramp[i];
    s[2 * i] *= w;
    s[2 * i + 1] *= w;
    s[2 * (n - 1 - i)] *= w;
    s[2 * (n - 1 - i) + 1] *= w;
  }
}

size_t max_pilot_safe_backoff(size_t n_fft, size_t pilot_spacing) {
  return n_fft / (2 * std::max<size_t>(pilot_spacing, 1));
}

void cp_insert(const float* t, size_t n, size_t cp, float* out) {
  if (cp > n) throw std::invalid_argument("ofdm: cp_len > n_fft");
  if (cp) std::memcpy(out, t + 2 * (n - cp), 2 * cp * sizeof(float));
  std::memcpy(out + 2 * cp, t, 2 * n * sizeof(float));
}

void cp_remove(const float* s, size_t n, size_t cp, float* out) {
  if (cp > n) throw std::invalid_argument("ofdm: cp_len > n_fft");
  std::memcpy(out, s + 2 * cp, 2 * n * sizeof(float));
}

void config_check(const Config& c) {
  if (!fft_size_ok(c.plan.n_fft)) throw std::invalid_argument("ofdm: n_fft must be a power of two from 8 to 4096");
  if (c.plan.cp_len > c.plan.n_fft) throw std::invalid_argument("ofdm: cp_len > n_fft");
  if (bits_per_symbol(c.constellation) == 0) throw std::invalid_argument("ofdm: unknown constellation");
  (void)grid_from_plan(c.plan);
}

Rotator::Rotator(float freq_hz, float fs) {
  const float phi = kTau * freq_hz / fs;
  wr = std::cos(phi);
  wi = std::sin(phi);
}

void Rotator::next(float* re, float* im) {
  const float r = std::fma(zr, wr, -zi * wi);
  const float i = std::fma(zi, wr, zr * wi);
  zr = r;
  zi = i;
  ctr += 1;
  if ((ctr & 0x3FFu) == 0) {
    const float r2 = zr * zr + zi * zi;
    const float inv = 1.0f / std::sqrt(r2);
    zr *= inv;
    zi *= inv;
  }
  *re = zr;
  *im = zi;
}

// ---- OfdmMod ----------------------------------------------------------------------------
namespace {
const Config& checked(const Config& c) {
  config_check(c);
  return c;
}
}  // namespace

Mod::Mod(const Config& c)
    : cfg_(checked(c)),
      grid_(grid_from_plan(c.plan)),
      ifft_(c.plan.n_fft, true),
      ramp_(window_ramp(c.plan.n_fft + c.plan.cp_len, c.plan.roll_off)),
      syms_(2 * c.plan.data.size()),
      freq_(2 * c.plan.n_fft),
      rot_(c.rf_hz, c.fs) {}

void Mod::symbol(const uint8_t* bits, float* out) {
  const size_t n = cfg_.plan.n_fft, cp = cfg_.plan.cp_len, len = n + cp;
  map_bits(cfg_.constellation, bits, grid_.data_bins.size(), syms_.data());
  std::fill(freq_.begin(), freq_.end(), 0.0f);  // GridMap, grid.rs:129-137
  for (size_t k = 0; k < grid_.data_bins.size(); ++k) {
    freq_[2 * grid_.data_bins[k]] = syms_[2 * k];
    freq_[2 * grid_.data_bins[k] + 1] = syms_[2 * k + 1];
  }
  for (size_t p = 0; p < grid_.pilot_bins.size(); ++p) {
    freq_[2 * grid_.pilot_bins[p]] = grid_.pilot_val[2 * p];
    freq_[2 * grid_.pilot_bins[p] + 1] = grid_.pilot_val[2 * p + 1];
  }
  fft_inplace(freq_.data(), n, ifft_.twiddles().data(), true);
  cp_insert(freq_.data(), n, cp, out);
  window_apply(out, len, ramp_);
  const float g = cfg_.gain;
  if (cfg_.rf_hz != 0.0f) {
    for (size_t i = 0; i < len; ++i) {
      float rr, ri;
      rot_.next(&rr, &ri);
      const float sr = out[2 * i], si = out[2 * i + 1];
      out[2 * i] = g * std::fma(sr, rr, -si * ri);
      out[2 * i + 1] = g * std::fma(si, rr, sr * ri);
    }
  } else {
    for (size_t i = 0; i < 2 * len; ++i) out[i] = g * out[i];
  }
}

void Mod::process(const uint8_t* bits, size_t n_bits, float* out, size_t out_cap, size_t* in_read,
                  size_t* out_written) {
  const size_t bps = cfg_.bits_per_ofdm_symbol(), len = cfg_.samples_per_ofdm_symbol();
  const size_t k = std::min(n_bits / bps, out_cap / len);
  for (size_t s = 0; s < k; ++s) symbol(bits + s * bps, out + 2 * s * len);
  *in_read = k * bps;
  *out_written = k * len;
}

std::vector<float> Mod::modulate(const uint8_t* bits, size_t n_bits) {
  const size_t bps = cfg_.bits_per_ofdm_symbol(), len = cfg_.samples_per_ofdm_symbol();
  const size_t nsym = (n_bits + bps - 1) / bps;
  std::vector<uint8_t> padded(nsym * bps, 0);
  if (n_bits) std::memcpy(padded.data(), bits, n_bits);
  std::vector<float> out(2 * nsym * len);
  for (size_t s = 0; s < nsym; ++s) symbol(padded.data() + s * bps, out.data() + 2 * s * len);
  return out;
}

// ---- OfdmEqualizer ----------------------------------------------------------------------
void training_pattern(size_t n_fft, float* out) {
  uint64_t state = 0x4F46444D54524E31ull;
  auto next = [&state]() -> float {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return static_cast<float>(state) / 18446744073709551616.0f - 0.5f;  // u64::MAX as f32 = 2^64
  };
  for (size_t i = 0; i < n_fft; ++i) {
    out[2 * i] = next() >= 0.0f ? kFrac1Sqrt2 : -kFrac1Sqrt2;
    out[2 * i + 1] = next() >= 0.0f ? kFrac1Sqrt2 : -kFrac1Sqrt2;
  }
}

void cdiv(float ar, float ai, float br, float bi, float* re, float* im) {
  const float ns = br * br + bi * bi;
  *re = (ar * br + ai * bi) / ns;
  *im = (ai * br - ar * bi) / ns;
}

void equalizer_weight(float hr, float hi, float* wr, float* wi) {
  const float m = hr * hr + hi * hi;
  if (m >= kEqualizerFloor) {
    *wr = hr / m;
    *wi = -hi / m;
  } else {
    *wr = 0.0f;
    *wi = 0.0f;
  }
}

void interpolate_at(const uint32_t* bins, const float* r, size_t n, uint32_t bin, float* re, float* im) {
  size_t pick;
  if (n == 1) {
    pick = 0;
  } else {
    const size_t hi = static_cast<size_t>(std::lower_bound(bins, bins + n, bin) - bins);  // partition_point(pbin < bin)
    if (hi == 0) {
      pick = 0;
    } else if (hi == n) {
      pick = n - 1;
    } else if (bins[hi] == bin) {
      pick = hi;
    } else {
      const float t = static_cast<float>(bin - bins[hi - 1]) / static_cast<float>(bins[hi] - bins[hi - 1]);
      const float lr = r[2 * (hi - 1)], li = r[2 * (hi - 1) + 1];
      *re = lr + (r[2 * hi] - lr) * t;
      *im = li + (r[2 * hi + 1] - li) * t;
      return;
    }
  }
  *re = r[2 * pick];
  *im = r[2 * pick + 1];
}

namespace {
void sort_pilots(std::vector<uint32_t>& bins, std::vector<float>& vals) {  // sort_by_key: stable
  std::vector<size_t> order(bins.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return bins[a] < bins[b]; });
  std::vector<uint32_t> b2(bins.size());
  std::vector<float> v2(vals.size());
  for (size_t i = 0; i < order.size(); ++i) {
    b2[i] = bins[order[i]];
    v2[2 * i] = vals[2 * order[i]];
    v2[2 * i + 1] = vals[2 * order[i] + 1];
  }
  bins.swap(b2);
  vals.swap(v2);
}
}  // namespace

Equalizer::Equalizer(const Config& c, int method) : method_(method), n_fft_(c.plan.n_fft) {
  if (method != kEqTrainingSymbolHold && method != kEqPerSymbolPilotInterp)
    throw std::invalid_argument("ofdm: unknown equalizer method");
  config_check(c);
  const Grid g = grid_from_plan(c.plan);
  pbin_ = g.pilot_bins;
  pval_ = g.pilot_val;
  sort_pilots(pbin_, pval_);
  dbin_ = g.data_bins;
  est_.assign(2 * n_fft_, 0.0f);
  for (size_t i = 0; i < n_fft_; ++i) est_[2 * i] = 1.0f;
  weight_ = est_;
}

void Equalizer::set_pilot_bins(const uint32_t* bins, const float* vals, size_t n, const uint32_t* data_bins,
                               size_t n_data) {
  for (size_t i = 0; i < n; ++i)
    if (bins[i] >= n_fft_) throw std::invalid_argument("ofdm: pilot bin >= n_fft");
  for (size_t i = 0; i < n_data; ++i)
    if (data_bins[i] >= n_fft_) throw std::invalid_argument("ofdm: data bin >= n_fft");
  pbin_.assign(bins, bins + n);
  pval_.assign(vals, vals + 2 * n);
  sort_pilots(pbin_, pval_);
  dbin_.assign(data_bins, data_bins + n_data);
}

void Equalizer::estimate_from_training_symbol(const float* rx, size_t n) {
  if (method_ != kEqTrainingSymbolHold || n < n_fft_) return;
  std::vector<float> known(2 * n_fft_);
  training_pattern(n_fft_, known.data());
  for (size_t b = 0; b < n_fft_; ++b) {
    float hr, hi;
    cdiv(rx[2 * b], rx[2 * b + 1], known[2 * b], known[2 * b + 1], &hr, &hi);
    equalizer_weight(hr, hi, &weight_[2 * b], &weight_[2 * b + 1]);
  }
}

void Equalizer::process(const float* in, size_t n_in, float* out, size_t out_cap, size_t* in_read,
                        size_t* out_written) {
  *in_read = *out_written = 0;
  if (n_in < n_fft_ || out_cap < n_fft_) return;
  if (method_ == kEqPerSymbolPilotInterp && !pbin_.empty()) {  // interpolate_from_pilots, :467-486
    ratios_.resize(2 * pbin_.size());
    for (size_t p = 0; p < pbin_.size(); ++p)
      cdiv(in[2 * pbin_[p]], in[2 * pbin_[p] + 1], pval_[2 * p], pval_[2 * p + 1], &ratios_[2 * p], &ratios_[2 * p + 1]);
    for (uint32_t b : dbin_) interpolate_at(pbin_.data(), ratios_.data(), pbin_.size(), b, &est_[2 * b], &est_[2 * b + 1]);
    for (size_t p = 0; p < pbin_.size(); ++p) {
      est_[2 * pbin_[p]] = ratios_[2 * p];
      est_[2 * pbin_[p] + 1] = ratios_[2 * p + 1];
    }
  }
  for (size_t b = 0; b < n_fft_; ++b) {
    float wr = weight_[2 * b], wi = weight_[2 * b + 1];
    if (method_ == kEqPerSymbolPilotInterp) equalizer_weight(est_[2 * b], est_[2 * b + 1], &wr, &wi);
    const float xr = in[2 * b], xi = in[2 * b + 1];  // num-complex Mul: (a c - b d, a d + b c)
    out[2 * b] = xr * wr - xi * wi;
    out[2 * b + 1] = xr * wi + xi * wr;
  }
  *in_read = *out_written = n_fft_;
}

// ---- OfdmDemod --------------------------------------------------------------------------
Demod::Demod(const Config& c)
    : cfg_(checked(c)),
      grid_(grid_from_plan(c.plan)),
      fft_(c.plan.n_fft, false),
      start_(c.plan.cp_len - std::min(c.rx_window_backoff, c.plan.cp_len)),
      freq_(2 * c.plan.n_fft),
      eqd_(2 * c.plan.n_fft) {}

void Demod::symbol_freq(const float* sym, float* freq) const {
  std::memcpy(freq, sym + 2 * start_, 2 * cfg_.plan.n_fft * sizeof(float));
  fft_inplace(freq, cfg_.plan.n_fft, fft_.twiddles().data(), false);
}

void Demod::process(const float* iq, size_t n, float* soft, size_t out_cap, Equalizer* eq, size_t* in_read,
                    size_t* out_written) {
  const size_t len = cfg_.samples_per_ofdm_symbol(), nd = grid_.data_bins.size(), nf = cfg_.plan.n_fft;
  const size_t k = std::min(n / len, out_cap / nd);
  const float g = gain_;
  const bool scale = std::fabs(g - 1.0f) > std::numeric_limits<float>::epsilon();
  for (size_t s = 0; s < k; ++s) {
    symbol_freq(iq + 2 * s * len, freq_.data());
    const float* f = freq_.data();
    if (eq) {
      size_t r, w;
      eq->process(freq_.data(), nf, eqd_.data(), nf, &r, &w);
      f = eqd_.data();
    }
    float* o = soft + 2 * s * nd;
    for (size_t d = 0; d < nd; ++d) {
      o[2 * d] = f[2 * grid_.data_bins[d]];
      o[2 * d + 1] = f[2 * grid_.data_bins[d] + 1];
    }
    if (scale)
      for (size_t i = 0; i < 2 * nd; ++i) o[i] = g * o[i];
  }
  *in_read = k * len;
  *out_written = k * nd;
}

bool evm_db(int order, const float* soft, size_t n_soft, const uint8_t* bits, size_t n_bits, size_t num_symbols,
            float* out) {
  const size_t bps = bits_per_symbol(order);
  if (num_symbols == 0 || n_soft == 0 || bps == 0) return false;
  const size_t mapped = std::min(n_bits / bps, n_soft);  // the mapper's out_written
  if (mapped != n_soft) return false;
  std::vector<float> ideal(2 * n_soft);
  map_bits(order, bits, n_soft, ideal.data());
  double err = 0.0, ref = 0.0;
  for (size_t i = 0; i < n_soft; ++i) {
    const float er = soft[2 * i] - ideal[2 * i], ei = soft[2 * i + 1] - ideal[2 * i + 1];
    err += static_cast<double>(er * er + ei * ei);
    ref += static_cast<double>(ideal[2 * i] * ideal[2 * i] + ideal[2 * i + 1] * ideal[2 * i + 1]);
  }
  if (ref <= 0.0) return false;
  *out = static_cast<float>(10.0 * std::log10(err / ref));
  return true;
}

}  // namespace ofdm
}  // namespace orion
