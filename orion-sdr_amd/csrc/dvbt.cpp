// dvbt.cpp — the DVB-T 2K frame on the host (dvbt.hpp). Scalar f32 in the reference's operation
// order; the constants are restated from ETSI EN 300 744 (Tables 7 and 8, Figure 9a, 4.6.2).
#include "dvbt.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <set>
#include <stdexcept>

#include "ofdm.hpp"

namespace orion {
namespace dvbt {

const uint16_t kContinualPilots2k[kContinual] = {
    0,   48,  54,  87,  141, 156, 192, 201, 255, 279, 282, 333,  432,  450,  483,  525,  531,  618,  636,  714,  759,  765, 780,
    804, 873, 888, 918, 939, 942, 969, 984, 1050, 1101, 1107, 1110, 1137, 1140, 1146, 1206, 1269, 1323, 1377, 1491, 1683, 1704};
const uint16_t kTpsCarriers2k[kTps] = {34, 50, 209, 346, 413, 569, 595, 688, 790, 901, 1073, 1219, 1262, 1286, 1469, 1594, 1687};

std::vector<uint8_t> wk_prbs(size_t len) {
  std::vector<uint8_t> out(len);
  uint32_t reg = 0x7FF;
  for (size_t i = 0; i < len; ++i) {
    out[i] = static_cast<uint8_t>((reg >> 10) & 1u);
    const uint32_t fb = ((reg >> 10) ^ (reg >> 1)) & 1u;
    reg = ((reg << 1) | fb) & 0x7FF;
  }
  return out;
}

float boosted_pilot_value(uint8_t wk) { return (4.0f / 3.0f) * 2.0f * (0.5f - static_cast<float>(wk)); }

std::vector<uint32_t> scattered_pilot_indices(size_t phase) {
  std::vector<uint32_t> v;
  for (size_t k = 3 * (phase % kPhases); k <= kKmax; k += kPilotSpacing) v.push_back(static_cast<uint32_t>(k));
  return v;
}

uint32_t active_to_bin(size_t a) {
  const int32_t s = static_cast<int32_t>(a) - static_cast<int32_t>(kKmax / 2);
  return static_cast<uint32_t>(s < 0 ? s + static_cast<int32_t>(kNFft) : s);
}

namespace {
Tables build_tables() {
  Tables t;
  const std::vector<uint8_t> wk = wk_prbs(kActive);
  for (size_t j = 0; j < kTps; ++j) {
    t.tps_bins[j] = active_to_bin(kTpsCarriers2k[j]);
    t.tps_sign[j] = 2.0f * (0.5f - static_cast<float>(wk[kTpsCarriers2k[j]]));
  }
  for (size_t j = 0; j < kContinual; ++j) t.continual_bins[j] = active_to_bin(kContinualPilots2k[j]);
  for (size_t p = 0; p < kPhases; ++p) {
    Phase& ph = t.phase[p];
    std::set<uint32_t> reserved(kContinualPilots2k, kContinualPilots2k + kContinual);
    for (uint32_t k : scattered_pilot_indices(p)) reserved.insert(k);
    const std::set<uint32_t> tps(kTpsCarriers2k, kTpsCarriers2k + kTps);
    reserved.insert(tps.begin(), tps.end());
    ph.role.assign(kNFft, kRoleNull);
    std::vector<std::pair<uint32_t, float>> ref;
    for (uint32_t a : reserved) {
      const uint32_t bin = active_to_bin(a);
      const float val = boosted_pilot_value(wk[a]);
      ph.pilot_bins.push_back(bin);
      ph.pilot_val.push_back(val);
      ph.role[bin] = val > 0.0f ? kRolePilotPos : kRolePilotNeg;
      if (!tps.count(a)) ref.emplace_back(bin, val);
    }
    for (size_t j = 0; j < kTps; ++j) ph.role[t.tps_bins[j]] = kRoleTps0 - static_cast<int32_t>(j);
    for (size_t a = 0; a <= kKmax; ++a)
      if (!reserved.count(static_cast<uint32_t>(a))) {
        ph.role[active_to_bin(a)] = static_cast<int32_t>(ph.data_bins.size());
        ph.data_bins.push_back(active_to_bin(a));
      }
    if (ph.data_bins.size() != kData) throw std::logic_error("dvbt: a scattered plan phase must carry exactly 1512 data carriers");
    std::sort(ref.begin(), ref.end());
    if (ref.size() > kMaxRefPilots) throw std::logic_error("dvbt: more reference pilots than the tables hold");
    for (const auto& r : ref) {
      ph.ref_bins.push_back(r.first);
      ph.ref_val.push_back(r.second);
    }
    // interpolate_at's choice per data bin (ofdm.cpp): no data bin is itself a pilot
    const size_t n = ph.ref_bins.size();
    for (uint32_t bin : ph.data_bins) {
      const size_t hi = static_cast<size_t>(std::lower_bound(ph.ref_bins.begin(), ph.ref_bins.end(), bin) - ph.ref_bins.begin());
      size_t lo = hi == 0 ? 0 : hi - 1, up = hi;
      if (hi == 0) up = 0;
      if (hi == n) lo = up = n - 1;
      ph.br_lo.push_back(static_cast<uint16_t>(lo));
      ph.br_hi.push_back(static_cast<uint16_t>(up));
    }
  }
  return t;
}
}  // namespace

const Tables& tables() {
  static const Tables t = build_tables();
  return t;
}

// ---- Figure 9a ------------------------------------------------------------------------------
namespace {
const int kAxisQpsk[2] = {1, -1};
const int kAxis16[4] = {3, 1, -3, -1};
const int kAxis64[8] = {7, 5, 1, 3, -7, -5, -1, -3};
const int* axis_of(size_t v) { return v == 2 ? kAxisQpsk : v == 4 ? kAxis16 : v == 6 ? kAxis64 : nullptr; }

void axis_llrs(const int* table, size_t k, float scale, float coord, float* out, size_t stride) {
  for (size_t b = 0; b < k; ++b) {
    const size_t shift = k - 1 - b;
    float d0 = std::numeric_limits<float>::infinity(), d1 = d0;
    for (size_t idx = 0; idx < (size_t{1} << k); ++idx) {
      const float d = coord - static_cast<float>(table[idx]) * scale;
      const float dsq = d * d;
      if (((idx >> shift) & 1u) == 0)
        d0 = std::fmin(d0, dsq);
      else
        d1 = std::fmin(d1, dsq);
    }
    out[b * stride] = d1 - d0;
  }
}
}  // namespace

bool map_symbol(const uint8_t* bits, size_t v, float* re, float* im) {
  const int* table = axis_of(v);
  if (!table) return false;
  const float scale = ofdm::axis_scale(v);
  size_t ii = 0, qi = 0;
  for (size_t j = 0; j < v; ++j) {
    size_t& axis = (j % 2 == 0) ? ii : qi;
    axis = (axis << 1) | (bits[j] & 1u);
  }
  *re = static_cast<float>(table[ii]) * scale;
  *im = static_cast<float>(table[qi]) * scale;
  return true;
}

bool demap_symbol(float re, float im, size_t v, uint8_t* bits) {
  const int* table = axis_of(v);
  if (!table) return false;
  const float scale = ofdm::axis_scale(v);
  const size_t k = v / 2;
  auto nearest = [&](float coord) {
    size_t best = 0;
    float best_d = std::numeric_limits<float>::infinity();
    for (size_t idx = 0; idx < (size_t{1} << k); ++idx) {
      const float d = std::fabs(coord - static_cast<float>(table[idx]) * scale);
      if (d < best_d) {
        best_d = d;
        best = idx;
      }
    }
    return best;
  };
  const size_t ii = nearest(re), qi = nearest(im);
  for (size_t j = 0; j < k; ++j) {
    bits[2 * j] = static_cast<uint8_t>((ii >> (k - 1 - j)) & 1u);
    bits[2 * j + 1] = static_cast<uint8_t>((qi >> (k - 1 - j)) & 1u);
  }
  return true;
}

bool soft_llr(float re, float im, size_t v, float* llr) {
  const int* table = axis_of(v);
  if (!table) return false;
  const float scale = ofdm::axis_scale(v);
  axis_llrs(table, v / 2, scale, re, llr, 2);
  axis_llrs(table, v / 2, scale, im, llr + 1, 2);
  return true;
}

// ---- TPS ------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kGfPrim = 0x89, kBchGen = 0x4377;
constexpr size_t kGfOrder = 127;
struct Gf128 {
  uint8_t exp[2 * kGfOrder], log[kGfOrder + 1];
  Gf128() {
    std::memset(log, 0, sizeof(log));
    uint32_t x = 1;
    for (size_t i = 0; i < kGfOrder; ++i) {
      exp[i] = static_cast<uint8_t>(x);
      log[x] = static_cast<uint8_t>(i);
      x <<= 1;
      if (x & 0x80) x ^= kGfPrim;
    }
    for (size_t i = kGfOrder; i < 2 * kGfOrder; ++i) exp[i] = exp[i - kGfOrder];
  }
  uint8_t mul(uint8_t a, uint8_t b) const { return a == 0 || b == 0 ? 0 : exp[log[a] + log[b]]; }
  uint8_t pow_alpha(size_t i) const { return exp[i % kGfOrder]; }
};
const Gf128& gf() {
  static const Gf128 g;
  return g;
}
}  // namespace

uint32_t tps_bch_parity(const uint8_t* info) {
  uint32_t reg = 0;
  const uint32_t top = 1u << kTpsParity;
  for (size_t i = 0; i < kTpsInfo + kTpsParity; ++i) {
    const uint32_t b = i < kTpsInfo ? (info[i] & 1u) : 0u;
    reg = (reg << 1) | b;
    if (reg & top) reg ^= kBchGen;
  }
  return reg & (top - 1);
}

void tps_bch_encode(const uint8_t* info, uint8_t* cw) {
  const uint32_t parity = tps_bch_parity(info);
  std::memcpy(cw, info, kTpsInfo);
  for (size_t i = 0; i < kTpsParity; ++i) cw[kTpsInfo + i] = static_cast<uint8_t>((parity >> (kTpsParity - 1 - i)) & 1u);
}

bool tps_bch_decode(const uint8_t* cw, uint8_t* info) {
  const Gf128& g = gf();
  const size_t shift = kGfOrder - kTpsCodeword;  // the 60 implicit zeros
  uint8_t synd[4];
  for (size_t s = 0; s < 4; ++s) {
    uint8_t acc = 0;
    for (size_t pos = 0; pos < kTpsCodeword; ++pos)
      if (cw[pos] & 1u) acc ^= g.pow_alpha((s + 1) * (kTpsCodeword - 1 - pos + shift));
    synd[s] = acc;
  }
  if (!(synd[0] | synd[1] | synd[2] | synd[3])) {
    std::memcpy(info, cw, kTpsInfo);
    return true;
  }
  const uint8_t s1 = synd[0], s3 = synd[2];
  if (s1 == 0) return false;
  const uint8_t num = static_cast<uint8_t>(s3 ^ g.mul(g.mul(s1, s1), s1));
  const uint8_t sig1 = s1, sig2 = num == 0 ? 0 : g.exp[(g.log[num] + kGfOrder - g.log[s1]) % kGfOrder];
  uint8_t fixed[kTpsCodeword];
  size_t found = 0;
  for (size_t pos = 0; pos < kTpsCodeword; ++pos) {
    const size_t deg = kTpsCodeword - 1 - pos + shift;
    const uint8_t x = g.pow_alpha((kGfOrder - (deg % kGfOrder)) % kGfOrder);
    const uint8_t val = static_cast<uint8_t>(1u ^ g.mul(sig1, x) ^ g.mul(sig2, g.mul(x, x)));
    fixed[pos] = static_cast<uint8_t>((cw[pos] ^ (val == 0 ? 1u : 0u)));
    found += val == 0;
  }
  if (found != (sig2 == 0 ? 1u : 2u)) return false;
  uint8_t re[kTpsCodeword];
  tps_bch_encode(fixed, re);
  if (std::memcmp(re, fixed, kTpsCodeword) != 0) return false;  // fixed holds 0 / 1 only where cw does
  std::memcpy(info, fixed, kTpsInfo);
  return true;
}

void tps_pack(const TpsWord& w, uint8_t* bits68) {
  uint8_t info[kTpsInfo] = {0};
  auto set = [&](size_t a, size_t b, uint32_t value) {
    for (size_t j = 0; a + j < b; ++j) info[a + j] = static_cast<uint8_t>((value >> (b - a - 1 - j)) & 1u);
  };
  set(0, 16, (w.frame_number % 2 == 0) ? 0x35EEu : 0xCA11u);
  set(16, 22, 0x1Fu);
  set(22, 24, static_cast<uint32_t>(w.frame_number) & 3u);
  set(24, 26, w.constellation == ofdm::kQam16 ? 1u : w.constellation == ofdm::kQam64 ? 2u : 0u);
  set(29, 32, static_cast<uint32_t>(w.code_rate));
  set(32, 35, static_cast<uint32_t>(w.code_rate));
  set(35, 37, static_cast<uint32_t>(w.guard));
  set(39, 47, static_cast<uint32_t>(w.cell_id) & 0xFFu);
  bits68[0] = 0;
  tps_bch_encode(info, bits68 + 1);
}

bool tps_unpack(const uint8_t* bits68, TpsWord* w) {
  uint8_t info[kTpsInfo];
  if (!tps_bch_decode(bits68 + 1, info)) return false;
  auto get = [&](size_t a, size_t b) {
    uint32_t v = 0;
    for (size_t i = a; i < b; ++i) v = (v << 1) | (info[i] & 1u);
    return v;
  };
  const uint32_t c = get(24, 26), r = get(29, 32);
  if (c > 2 || r > 4) return false;
  w->frame_number = static_cast<int>(get(22, 24));
  w->constellation = c == 0 ? ofdm::kQpsk : c == 1 ? ofdm::kQam16 : ofdm::kQam64;
  w->code_rate = static_cast<int>(r);
  w->guard = static_cast<int>(get(35, 37));
  w->cell_id = static_cast<int>(get(39, 47));
  return true;
}

void tps_symbol_signs(const uint8_t* bits68, size_t n_symbols, float* signs) {
  float s = 1.0f;
  for (size_t l = 0; l < n_symbols; ++l) {
    const size_t sym = l % kTpsSymbols;
    if (sym == 0) s = 1.0f;
    if (sym > 0 && (bits68[sym] & 1u)) s = -s;
    signs[l] = s;
  }
}

size_t tps_decide(const float* cells, size_t n_symbols, uint8_t* bits68) {
  const size_t n = std::min(n_symbols, kTpsSymbols);
  for (size_t l = 0; l < n; ++l) {
    if (l == 0) {
      bits68[0] = 0;
      continue;
    }
    const float* c = cells + 2 * kTps * l;
    const float* p = c - 2 * kTps;
    float acc = 0.0f;
    for (size_t j = 0; j < kTps; ++j) acc += c[2 * j] * p[2 * j] - c[2 * j + 1] * (-p[2 * j + 1]);  // (cell * conj(prev)).re
    bits68[l] = acc < 0.0f ? 1 : 0;
  }
  return n;
}

// ---- guard-interval acquisition -------------------------------------------------------------
float norm32(float re, float im) {
  const double r = static_cast<double>(re), i = static_cast<double>(im);
  return static_cast<float>(std::sqrt(r * r + i * i));
}

void gi_sums(const float* iq, size_t n, size_t n_fft, size_t cp, size_t d, size_t max_symbols, float* gre, float* gim,
             float* phi_out) {
  const size_t period = n_fft + cp;
  float gr = 0.0f, gi = 0.0f, phi = 0.0f;
  size_t base = d;
  for (size_t used = 0; used < max_symbols && base + n_fft + cp <= n; ++used, base += period) {
    for (size_t k = 0; k < cp; ++k) {
      const float ar = iq[2 * (base + k)], ai = iq[2 * (base + k) + 1];
      const float br = iq[2 * (base + n_fft + k)], bi = iq[2 * (base + n_fft + k) + 1];
      gr += ar * br - ai * (-bi);  // a * conj(b)
      gi += ar * (-bi) + ai * br;
      phi += (ar * ar + ai * ai) + (br * br + bi * bi);
    }
  }
  *gre = gr;
  *gim = gi;
  *phi_out = phi * 0.5f;
}

namespace {
int32_t total_key(float v) {  // f32::total_cmp's order as a signed integer
  int32_t b;
  std::memcpy(&b, &v, 4);
  return b ^ static_cast<int32_t>(static_cast<uint32_t>(b >> 31) >> 1);
}
float single_score(const float* iq, size_t n, size_t n_fft, size_t cp, size_t d) {
  if (d + n_fft + cp > n) return 0.0f;
  float gr, gi, phi;
  gi_sums(iq, n, n_fft, cp, d, 1, &gr, &gi, &phi);
  return phi > 0.0f ? std::fmin(norm32(gr, gi) / phi, 1.0f) : 0.0f;
}
}  // namespace

bool gi_sync(const float* iq, size_t n, size_t n_fft, size_t cp, float fs, size_t search_len, const GiConfig& cfg,
             GiResult* out, float* metric_out) {
  if (cp == 0 || n_fft == 0 || search_len == 0) return false;
  if (n < search_len - 1 + n_fft + cp) return false;
  const size_t period = n_fft + cp, max_syms = std::max<size_t>(cfg.max_symbols, 1);
  std::vector<float> g(3 * search_len);
  size_t argmax = 0;
  int32_t best = 0;
  for (size_t d = 0; d < search_len; ++d) {
    gi_sums(iq, n, n_fft, cp, d, max_syms, &g[3 * d], &g[3 * d + 1], &g[3 * d + 2]);
    const float metric = norm32(g[3 * d], g[3 * d + 1]) - cfg.rho * g[3 * d + 2];
    if (metric_out) metric_out[d] = metric;
    const int32_t key = total_key(metric);
    if (d == 0 || key >= best) {  // Iterator::max_by keeps the last of equal maxima
      best = key;
      argmax = d;
    }
  }
  const size_t phase = argmax % period, origin = argmax - phase;
  size_t best_d = argmax;
  if (cfg.origin_score_ratio > 0.0f && phase != 0 && period - phase <= (cp + 1) / 2) {
    const float ratio = std::fmin(std::fmax(cfg.origin_score_ratio, 0.0f), 1.0f);
    if (single_score(iq, n, n_fft, cp, origin) >= ratio * single_score(iq, n, n_fft, cp, argmax)) best_d = origin;
  }
  const float gr = g[3 * best_d], gi = g[3 * best_d + 1], phi = g[3 * best_d + 2];
  out->start = best_d;
  out->gamma_re = gr;
  out->gamma_im = gi;
  out->phi = phi;
  out->score = phi > 0.0f ? std::fmin(norm32(gr, gi) / phi, 1.0f) : 0.0f;
  out->cfo_hz = -std::atan2(gi, gr) * fs / (6.28318530717958647692f * static_cast<float>(n_fft));
  return true;
}

bool integer_cfo(const float* freq, size_t n_freq, size_t n_fft, int max_bins, int32_t* bins, float* confidence) {
  if (n_freq < n_fft || n_fft == 0 || max_bins <= 0) return false;
  const Tables& t = tables();
  int32_t best_k = 0;
  float best_e = -std::numeric_limits<float>::infinity(), sum = 0.0f;
  uint32_t count = 0;
  for (int k = -max_bins; k <= max_bins; ++k) {
    float e = 0.0f;
    for (uint32_t b : t.continual_bins) {
      int64_t idx = (static_cast<int64_t>(b) + k) % static_cast<int64_t>(n_fft);
      if (idx < 0) idx += static_cast<int64_t>(n_fft);
      e += freq[2 * idx] * freq[2 * idx] + freq[2 * idx + 1] * freq[2 * idx + 1];
    }
    sum += e;
    ++count;
    if (e > best_e) {
      best_e = e;
      best_k = k;
    }
  }
  const float mean = sum / static_cast<float>(count);
  *bins = best_k;
  if (confidence) *confidence = mean > 0.0f ? best_e / mean : 0.0f;
  return true;
}

// ---- the per-symbol modulator and demodulator ----------------------------------------------
void mod_symbols(const uint8_t* bits, size_t n_bits, size_t v, size_t cp, const uint8_t* tps68, size_t n_symbols,
                 size_t roll_off, float* iq) {
  if (!axis_of(v)) throw std::invalid_argument("dvbt: v is 2, 4 or 6");
  if (cp == 0 || cp > kNFft) throw std::invalid_argument("dvbt: cp_len");
  const Tables& t = tables();
  const size_t sps = kNFft + cp;
  const std::vector<float> tw = ofdm::fft_twiddles(kNFft);
  const std::vector<float> ramp = roll_off ? ofdm::window_ramp(sps, roll_off) : std::vector<float>();
  std::vector<float> signs(n_symbols), freq(2 * kNFft);
  tps_symbol_signs(tps68, n_symbols, signs.data());
  for (size_t s = 0; s < n_symbols; ++s) {
    const Phase& ph = t.phase[s % kPhases];
    std::fill(freq.begin(), freq.end(), 0.0f);
    for (size_t c = 0; c < kData; ++c) {
      const size_t base = s * kData * v + c * v;
      if (base + v <= n_bits) map_symbol(bits + base, v, &freq[2 * ph.data_bins[c]], &freq[2 * ph.data_bins[c] + 1]);
    }
    for (size_t p = 0; p < ph.pilot_bins.size(); ++p) {
      freq[2 * ph.pilot_bins[p]] = ph.pilot_val[p];
      freq[2 * ph.pilot_bins[p] + 1] = 0.0f;
    }
    for (size_t j = 0; j < kTps; ++j) {
      freq[2 * t.tps_bins[j]] = signs[s] * t.tps_sign[j];  // the encoder's running sign: exact, +-1
      freq[2 * t.tps_bins[j] + 1] = 0.0f;
    }
    ofdm::fft_inplace(freq.data(), kNFft, tw.data(), true);
    float* out = iq + 2 * s * sps;
    ofdm::cp_insert(freq.data(), kNFft, cp, out);
    if (!ramp.empty()) ofdm::window_apply(out, sps, ramp);
  }
}

void demod_symbols(const float* iq, size_t n_symbols, size_t cp, size_t backoff, size_t v, float* llr, float* cells,
                   float* syms) {
  if (!axis_of(v)) throw std::invalid_argument("dvbt: v is 2, 4 or 6");
  if (cp == 0 || cp > kNFft) throw std::invalid_argument("dvbt: cp_len");
  const Tables& t = tables();
  const size_t sps = kNFft + cp, start = cp - std::min(backoff, cp);
  const std::vector<float> tw = ofdm::fft_twiddles(kNFft);
  std::vector<float> freq(2 * kNFft), ratios(2 * kMaxRefPilots);
  for (size_t s = 0; s < n_symbols; ++s) {
    const Phase& ph = t.phase[s % kPhases];
    std::memcpy(freq.data(), iq + 2 * (s * sps + start), 2 * kNFft * sizeof(float));
    ofdm::fft_inplace(freq.data(), kNFft, tw.data(), false);
    for (size_t j = 0; j < kTps; ++j) {
      cells[2 * (s * kTps + j)] = freq[2 * t.tps_bins[j]];
      cells[2 * (s * kTps + j) + 1] = freq[2 * t.tps_bins[j] + 1];
    }
    const size_t np = ph.ref_bins.size();
    for (size_t p = 0; p < np; ++p)
      ofdm::cdiv(freq[2 * ph.ref_bins[p]], freq[2 * ph.ref_bins[p] + 1], ph.ref_val[p], 0.0f, &ratios[2 * p], &ratios[2 * p + 1]);
    for (size_t c = 0; c < kData; ++c) {
      const uint32_t bin = ph.data_bins[c];
      float hr, hi, wr, wi;
      ofdm::interpolate_at(ph.ref_bins.data(), ratios.data(), np, bin, &hr, &hi);
      ofdm::equalizer_weight(hr, hi, &wr, &wi);
      const float xr = freq[2 * bin], xi = freq[2 * bin + 1];
      const float er = xr * wr - xi * wi, ei = xr * wi + xi * wr;
      if (syms) {
        syms[2 * (s * kData + c)] = er;
        syms[2 * (s * kData + c) + 1] = ei;
      }
      soft_llr(er, ei, v, llr + (s * kData + c) * v);
    }
  }
}

}  // namespace dvbt
}  // namespace orion
