// psk31.cpp — PSK31 channel code and scalar modems on the host (psk31.hpp). No HIP in this file.
#include "psk31.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

namespace orion {
namespace psk31 {

// ---- Varicode --------------------------------------------------------------------------
namespace {
// The G3PLX Varicode alphabet, ASCII 0 .. 127, each codeword as transmitted (first bit
// first). No codeword holds "00"; all begin and end with 1.
const char* const kAlphabet[128] = {
    "1010101011", "1011011011", "1011101101", "1101110111", "1011101011", "1101011111", "1011101111", "1011111101",
    "1011111111", "11101111",   "11101",      "1101101111", "1011011101", "11111",      "1101110101", "1110101011",
    "1011110111", "1011110101", "1110101101", "1110101111", "1101011011", "1101101011", "1101101101", "1101010111",
    "1101111011", "1101111101", "1110110111", "1101010101", "1101011101", "1110111011", "1011111011", "1101111111",
    "1",          "111111111",  "101011111",  "111110101",  "111011011",  "1011010101", "1010111011", "101111111",
    "11111011",   "11110111",   "101101111",  "111011111",  "1110101",    "110101",     "1010111",    "110101111",
    "10110111",   "10111101",   "11101101",   "11111111",   "101110111",  "101011011",  "101101011",  "110101101",
    "110101011",  "110110111",  "11110101",   "110111101",  "111101101",  "1010101",    "111010111",  "1010101111",
    "1010111101", "1111101",    "11101011",   "10101101",   "10110101",   "1110111",    "11011011",   "11111101",
    "101010101",  "1111111",    "111111101",  "101111101",  "11010111",   "10111011",   "11011101",   "10101011",
    "11010101",   "111011101",  "10101111",   "1101111",    "1101101",    "101010111",  "110110101",  "101011101",
    "101110101",  "101111011",  "1010101101", "111110111",  "111101111",  "111111011",  "1010111111", "101101101",
    "1011011111", "1011",       "1011111",    "101111",     "101101",     "11",         "111101",     "1011011",
    "101011",     "1101",       "111101011",  "10111111",   "11011",      "111011",     "1111",       "111",
    "111111",     "110111111",  "10101",      "10111",      "101",        "110111",     "1111011",    "1101011",
    "11011111",   "1011101",    "111010101",  "1010110111", "110111011",  "1010110101", "1011010111", "1110110101",
};

struct Table {
  Codeword cw[128];
  Table() {
    for (int i = 0; i < 128; ++i) {
      uint16_t v = 0;
      uint8_t n = 0;
      for (const char* p = kAlphabet[i]; *p; ++p, ++n) v = static_cast<uint16_t>(v << 1 | (*p == '1'));
      cw[i] = {v, n};
    }
  }
};
}  // namespace

const Codeword* varicode_table() {
  static const Table t;
  return t.cw;
}

Codeword varicode_encode(uint8_t byte) { return varicode_table()[byte >= 128 ? 0 : byte]; }

int varicode_decode(uint16_t bits, uint8_t len) {
  const Codeword* t = varicode_table();
  for (int i = 0; i < 128; ++i)
    if (t[i].len == len && t[i].bits == bits) return i;
  return -1;
}

void VaricodeEncoder::push_preamble(size_t n_bits) {
  pending_.insert(pending_.end(), n_bits, 0);
  first_ = true;
}

void VaricodeEncoder::push_byte(uint8_t b) {
  if (!first_) pending_.insert(pending_.end(), 2, 0);
  first_ = false;
  const Codeword c = varicode_encode(b);
  for (int i = c.len - 1; i >= 0; --i) pending_.push_back(static_cast<uint8_t>((c.bits >> i) & 1));
}

void VaricodeEncoder::push_postamble(size_t n_bits) {
  if (!first_) pending_.insert(pending_.end(), 2, 0);
  pending_.insert(pending_.end(), n_bits, 1);
}

int VaricodeEncoder::next_bit() {
  if (pending_.empty()) return -1;
  const int b = pending_.front();
  pending_.pop_front();
  return b;
}

std::vector<uint8_t> VaricodeEncoder::drain_bits() {
  std::vector<uint8_t> out(pending_.begin(), pending_.end());
  pending_.clear();
  return out;
}

void VaricodeDecoder::push_bit(uint8_t bit) {
  const bool is_zero = bit == 0;
  if (is_zero && prev_zero_) {
    // the first zero of the "00" went into shift_ with the previous call
    const uint16_t cw = len_ > 0 ? static_cast<uint16_t>(shift_ >> 1) : 0;
    const uint8_t cw_len = len_ > 0 ? static_cast<uint8_t>(len_ - 1) : 0;
    if (cw_len > 0) {
      const int ch = varicode_decode(cw, cw_len);
      if (ch >= 0) chars_.push_back(static_cast<uint8_t>(ch));
    }
    shift_ = 0;
    len_ = 0;
    prev_zero_ = false;
  } else {
    shift_ = static_cast<uint16_t>(shift_ << 1 | (bit & 1));
    if (len_ < kVaricodeMaxBits + 1) ++len_;
    prev_zero_ = is_zero;
  }
}

int VaricodeDecoder::pop_char() {
  if (chars_.empty()) return -1;
  const int c = chars_.front();
  chars_.pop_front();
  return c;
}

// ---- convolutional code ----------------------------------------------------------------
const float kDqpskExp[4][2] = {{1.0f, 0.0f}, {0.0f, -1.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}};

namespace {
constexpr float kInf = std::numeric_limits<float>::max() / 2.0f;  // psk31.rs:102

inline uint8_t parity(uint8_t x) {  // psk31.rs:33-37
  x ^= x >> 4;
  x ^= x >> 2;
  return (x ^ (x >> 1)) & 1;
}
// psk31.rs:63-66: the dibit c0 * 2 + c1 of state s taking input b
inline int branch_dibit(int s, int b) {
  const uint8_t window = static_cast<uint8_t>((b & 1) << 4 | (s & 0x0F));
  return parity(window & 0x15) * 2 + parity(window & 0x13);
}
inline int next_state(int s, int b) { return (s >> 1) | (b & 1) << 3; }  // psk31.rs:70-72

// One add-compare-select step, psk31.rs:113-135 = :296-316: prev_row entries that no
// predecessor writes keep what they held.
inline void acs(const float* pm, float s0, float s1, const float (*exp)[2], float* new_pm, uint8_t* prev_row) {
  for (int s = 0; s < kStates; ++s) new_pm[s] = kInf;
  for (int prev = 0; prev < kStates; ++prev) {
    const float pm_prev = pm[prev];
    if (pm_prev >= kInf) continue;
    for (int bit = 0; bit < 2; ++bit) {
      const float* e = exp[branch_dibit(prev, bit)];
      const float bm = (s0 - e[0]) * (s0 - e[0]) + (s1 - e[1]) * (s1 - e[1]);
      const int ns = next_state(prev, bit);
      const float cand = pm_prev + bm;
      if (cand < new_pm[ns]) {
        new_pm[ns] = cand;
        prev_row[ns] = static_cast<uint8_t>(prev);
      }
    }
  }
}
// Iterator::min_by with partial_cmp(..).unwrap_or(Equal), psk31.rs:139-144: the first of
// equal minima; an unordered pair keeps the earlier one.
inline int best_state(const float* pm) {
  int best = 0;
  for (int i = 1; i < kStates; ++i)
    if (pm[best] > pm[i]) best = i;
  return best;
}
}  // namespace

void conv_encode(const uint8_t* bits, size_t n, uint8_t* out) {
  ConvEncoder e;
  for (size_t i = 0; i < n; ++i) e.encode(bits[i], &out[2 * i], &out[2 * i + 1]);
}

void ConvEncoder::encode(uint8_t bit, uint8_t* c0, uint8_t* c1) {
  const uint8_t window = static_cast<uint8_t>((bit & 1) << 4 | (sr_ & 0x0F));
  *c0 = parity(window & 0x15);
  *c1 = parity(window & 0x13);
  sr_ = static_cast<uint8_t>(sr_ >> 1 | (bit & 1) << 3);
}

void viterbi_decode(const float* soft, size_t n_syms, uint8_t* bits) {
  if (n_syms == 0) return;
  float pm[kStates], new_pm[kStates];
  for (int s = 0; s < kStates; ++s) pm[s] = kInf;
  pm[0] = 0.0f;
  std::vector<uint8_t> table(n_syms * kStates, 0);
  for (size_t t = 0; t < n_syms; ++t) {
    acs(pm, soft[2 * t], soft[2 * t + 1], kDqpskExp, new_pm, &table[t * kStates]);
    for (int s = 0; s < kStates; ++s) pm[s] = new_pm[s];
  }
  int state = best_state(pm);
  for (size_t t = n_syms; t-- > 0;) {
    bits[t] = static_cast<uint8_t>((state >> 3) & 1);  // psk31.rs:154: the input bit is the state's MSB
    state = table[t * kStates + state];
  }
}

void viterbi_decode_hard(const uint8_t* coded, size_t n_syms, uint8_t* bits) {
  std::vector<float> soft(2 * n_syms);
  for (size_t i = 0; i < n_syms; ++i) {
    const int dibit = (coded[2 * i] & 1) * 2 + (coded[2 * i + 1] & 1);
    soft[2 * i] = kDqpskExp[dibit][0];
    soft[2 * i + 1] = kDqpskExp[dibit][1];
  }
  viterbi_decode(soft.data(), n_syms, bits);
}

StreamingViterbi::StreamingViterbi() {
  for (int s = 0; s < kStates; ++s) pm_[s] = kInf;
  pm_[0] = 0.0f;
  for (auto& row : history_)
    for (auto& v : row) v = 0;
}

int StreamingViterbi::feed_symbol(float s_re, float s_im) {
  float new_pm[kStates];
  acs(pm_, s_re, s_im, kDqpskExp, new_pm, history_[ptr_]);
  for (int s = 0; s < kStates; ++s) pm_[s] = new_pm[s];

  if (count_ % 256 == 255) {  // psk31.rs:319-333
    float min_pm = kInf;
    for (int s = 0; s < kStates; ++s)
      if (pm_[s] < kInf) min_pm = min_pm < pm_[s] ? min_pm : pm_[s];  // f32::min of two numbers
    if (min_pm > 0.0f)
      for (int s = 0; s < kStates; ++s)
        if (pm_[s] < kInf) pm_[s] -= min_pm;
  }
  ptr_ = (ptr_ + 1) % kPathMem;
  ++count_;
  if (count_ <= static_cast<size_t>(kTracebackDepth)) return -1;

  int state = best_state(pm_);
  size_t p = (ptr_ + kPathMem - 1) % kPathMem;
  for (int i = 0; i < kTracebackDepth; ++i) {
    state = history_[p][state];
    p = (p + kPathMem - 1) % kPathMem;
  }
  return (state >> 3) & 1;
}

std::vector<uint8_t> StreamingViterbi::flush() {
  std::vector<uint8_t> out;
  for (int i = 0; i < kTracebackDepth; ++i) {
    const int b = feed_symbol(0.0f, 0.0f);
    if (b >= 0) out.push_back(static_cast<uint8_t>(b));
  }
  return out;
}

// ---- modulators and demodulators --------------------------------------------------------
namespace {
constexpr float kPi = 3.14159265358979323846f, kTau = 6.28318530717958647692f;
constexpr size_t kMaxSps = 1u << 24;
constexpr float kLoopGain = 0.05f;  // demodulate/psk31.rs:52-53

// Rotator::next, dsp/rotator.rs:44-61
inline void rot_next(float& zr, float& zi, uint32_t& ctr, float wr, float wi) {
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
}
size_t checked_sps(float fs) {
  const size_t sps = psk31_sps(fs);
  if (sps == 0 || sps > kMaxSps) throw std::invalid_argument("psk31: 1 <= round(fs / 31.25) <= 2^24 samples per symbol");
  return sps;
}
int checked_mode(int mode) {
  if (mode != kBpsk && mode != kQpsk)
    throw std::invalid_argument("psk31: unknown mode (ORION_PSK31_BPSK / ORION_PSK31_QPSK)");
  return mode;
}
}  // namespace

size_t psk31_sps(float fs) {
  const float q = std::round(fs / 31.25f);
  if (!(q >= 1.0f)) return 0;
  if (q >= 1.8446744e19f) return std::numeric_limits<size_t>::max();
  return static_cast<size_t>(q);
}

std::vector<float> make_hann(size_t sps) {
  std::vector<float> h(sps);
  if (sps == 1) h[0] = 1.0f;
  if (sps < 2) return h;
  const float denom = static_cast<float>(sps - 1);
  for (size_t i = 0; i < sps; ++i) {
    const float t = kPi * static_cast<float>(i) / denom;
    h[i] = 0.5f - 0.5f * std::cos(t);
  }
  return h;
}

std::vector<uint8_t> text_bits(const uint8_t* text, size_t n, size_t preamble_bits, size_t postamble_bits) {
  VaricodeEncoder enc;
  enc.push_preamble(preamble_bits);
  for (size_t i = 0; i < n; ++i) enc.push_byte(text[i]);
  enc.push_postamble(postamble_bits);
  return enc.drain_bits();
}

void rotator_step(float freq_hz, float fs, float* w_re, float* w_im) {
  const float phi = kTau * freq_hz / fs;
  *w_re = std::cos(phi);
  *w_im = std::sin(phi);
}

Mod::Mod(int mode, float fs, float rf_hz, float gain)
    : mode_(checked_mode(mode)), fs_(fs), rf_hz_(rf_hz), gain_(gain), sps_(checked_sps(fs)), hann_(make_hann(sps_)) {}

void Mod::reset() {
  cur_re_ = 1.0f;
  cur_im_ = 0.0f;
  enc_.reset();
}

void rotator_table(float freq_hz, float fs, size_t n, float* out) {
  float wr, wi, zr = 1.0f, zi = 0.0f;
  uint32_t ctr = 0;
  rotator_step(freq_hz, fs, &wr, &wi);
  for (size_t i = 0; i < n; ++i) {
    rot_next(zr, zi, ctr, wr, wi);
    out[2 * i] = zr;
    out[2 * i + 1] = zi;
  }
}

uint64_t rotator_step_q64(float freq_hz, float fs) {
  float wr, wi;
  rotator_step(freq_hz, fs, &wr, &wi);
  const long double two_pi = 6.283185307179586476925286766559L, two64 = 18446744073709551616.0L;
  long double rev = atan2l(static_cast<long double>(wi), static_cast<long double>(wr)) / two_pi;
  if (!(rev == rev)) rev = 0.0L;
  if (rev < 0) rev += 1.0L;
  long double scaled = roundl(rev * two64);
  if (scaled >= two64) scaled -= two64;
  return static_cast<uint64_t>(scaled);
}

void Mod::symbol_phasors(const uint8_t* bits, size_t n, float* ph) {
  ph[0] = cur_re_;
  ph[1] = cur_im_;
  for (size_t k = 0; k < n; ++k) {
    if (mode_ == kBpsk) {
      if (bits[k] == 0) cur_re_ = -cur_re_;
    } else {
      uint8_t g0, g1;
      enc_.encode(bits[k], &g0, &g1);
      const float* step = kDqpskExp[g0 * 2 + g1];
      const float nr = cur_re_ * step[0] - cur_im_ * step[1];
      const float ni = cur_im_ * step[0] + cur_re_ * step[1];
      cur_re_ = nr;
      cur_im_ = ni;
    }
    ph[2 * (k + 1)] = cur_re_;
    ph[2 * (k + 1) + 1] = cur_im_;
  }
}

void Mod::modulate_bits(const uint8_t* bits, size_t n, float* iq) {
  float p0r = cur_re_, p0i = cur_im_;
  for (size_t k = 0; k < n; ++k) {
    if (mode_ == kBpsk) {
      if (bits[k] == 0) cur_re_ = -cur_re_;  // modulate/psk31.rs:171-173: only a zero byte flips
    } else {
      uint8_t g0, g1;
      enc_.encode(bits[k], &g0, &g1);
      const float* step = kDqpskExp[g0 * 2 + g1];  // QPSK31_PHASE_STEP (:234-239) is DQPSK_EXP
      const float nr = cur_re_ * step[0] - cur_im_ * step[1];
      const float ni = cur_im_ * step[0] + cur_re_ * step[1];
      cur_re_ = nr;
      cur_im_ = ni;
    }
    // write_symbol, :79-101
    const float dr = cur_re_ - p0r, di = cur_im_ - p0i;
    float* o = iq + 2 * k * sps_;
    for (size_t i = 0; i < sps_; ++i) {
      const float h = hann_[i];
      o[2 * i] = gain_ * (p0r + h * dr);
      o[2 * i + 1] = gain_ * (p0i + h * di);
    }
    p0r = cur_re_;
    p0i = cur_im_;
  }
  if (rf_hz_ != 0.0f) {
    float wr, wi, zr = 1.0f, zi = 0.0f;
    uint32_t ctr = 0;
    rotator_step(rf_hz_, fs_, &wr, &wi);
    for (size_t i = 0; i < n * sps_; ++i) {  // rotate_block, dsp/rotator.rs:74-84
      rot_next(zr, zi, ctr, wr, wi);
      const float a = iq[2 * i], b = iq[2 * i + 1];
      iq[2 * i] = std::fma(a, zr, -b * zi);
      iq[2 * i + 1] = std::fma(b, zr, a * zi);
    }
  }
}

void Mod::process(const uint8_t* bits, size_t n_bits, float* iq, size_t out_cap, size_t* in_read, size_t* out_written) {
  const size_t max_bits = out_cap / sps_;
  const size_t n = n_bits < max_bits ? n_bits : max_bits;
  if (n) modulate_bits(bits, n, iq);
  *in_read = n;
  *out_written = n * sps_;
}

Demod::Demod(int mode, float fs, float rf_hz, float gain, size_t offset)
    : mode_(checked_mode(mode)), gain_(gain), rot_(rf_hz != 0.0f), sps_(checked_sps(fs)), hann_(make_hann(sps_)) {
  w_re_ = 1.0f;
  w_im_ = 0.0f;
  if (rot_) rotator_step(-rf_hz, fs, &w_re_, &w_im_);
  hann_sq_sum_ = 0.0f;
  for (float h : hann_) hann_sq_sum_ += h * h;
  reset();
  st_.count = demod_start_count(sps_, offset);
}

void Demod::reset() { st_ = {0u, 0u, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.0f}; }

void Demod::process(const float* iq, size_t n, float* out, size_t out_cap, size_t* in_read, size_t* out_written) {
  size_t in_pos = 0, out_pos = 0;
  const size_t need = mode_ == kQpsk ? 2 : 1;
  DemodState& s = st_;
  while (in_pos < n && out_pos + need <= out_cap) {
    float xr = iq[2 * in_pos], xi = iq[2 * in_pos + 1];
    if (rot_) {
      rot_next(s.z_re, s.z_im, s.renorm_ctr, w_re_, w_im_);
      const float re = xr * s.z_re - xi * s.z_im;
      const float im = xi * s.z_re + xr * s.z_im;
      xr = re;
      xi = im;
    }
    const float h = hann_[s.count];
    const float one_minus_h = 1.0f - h;
    const float corr_re = xr - s.prev_re * one_minus_h;
    const float corr_im = xi - s.prev_im * one_minus_h;
    s.acc_re += h * corr_re;
    s.acc_im += h * corr_im;
    s.count += 1;
    in_pos += 1;
    if (s.count == sps_) {
      const float scale = gain_ / hann_sq_sum_;
      const float sr = s.acc_re * scale, si = s.acc_im * scale;
      s.acc_re = s.acc_im = 0.0f;
      s.count = 0;
      const float sin_pa = std::sin(s.phase_acc), cos_pa = std::cos(s.phase_acc);
      const float sym_re = sr * cos_pa + si * sin_pa;
      const float sym_im = si * cos_pa - sr * sin_pa;
      const float d_re = sym_re * s.prev_re + sym_im * s.prev_im;
      const float d_im = sym_im * s.prev_re - sym_re * s.prev_im;
      float cross_im;
      if (mode_ == kBpsk) {
        out[out_pos++] = d_re;
        const float dec_re = d_re >= 0.0f ? 1.0f : -1.0f;
        cross_im = d_im * dec_re;
      } else {
        out[out_pos] = d_re;
        out[out_pos + 1] = d_im;
        out_pos += 2;
        float dec_re, dec_im;  // hard_decide_dqpsk, :65-73
        if (std::fabs(d_re) >= std::fabs(d_im)) {
          dec_re = d_re >= 0.0f ? 1.0f : -1.0f;
          dec_im = 0.0f;
        } else {
          dec_re = 0.0f;
          dec_im = d_im >= 0.0f ? 1.0f : -1.0f;
        }
        cross_im = d_im * dec_re - d_re * dec_im;
      }
      const float mag_sq = d_re * d_re + d_im * d_im;
      const float phase_err = mag_sq > 1e-6f ? cross_im / std::sqrt(mag_sq) : 0.0f;
      s.phase_acc += kLoopGain * phase_err;
      if (s.phase_acc > kPi) s.phase_acc -= kTau;
      if (s.phase_acc < -kPi) s.phase_acc += kTau;
      s.prev_re = sym_re;
      s.prev_im = sym_im;
    }
  }
  *in_read = in_pos;
  *out_written = out_pos;
}

// ---- carrier search ----------------------------------------------------------------------
float median_f32(float* v, size_t n) {
  if (n == 0) return 0.0f;
  // partial_cmp(..).unwrap_or(Equal): any exact selection gives the same value for ordered
  // input (the median is one of the values or the mean of the two middle ones)
  // NaNs (not a waterfall's values) sort last, so the comparator stays a strict weak order
  std::sort(v, v + n, [](float a, float b) { return std::isnan(b) ? !std::isnan(a) : a < b; });
  const size_t mid = n / 2;
  return n % 2 == 0 ? (v[mid - 1] + v[mid]) * 0.5f : v[mid];
}

size_t sync_num_bins(float base_hz, float max_hz) {
  const float d = max_hz - base_hz;
  const float freq_range = d > 0.0f ? d : 0.0f;  // f32::max(0.0): a NaN gives 0
  const float bins = std::ceil(freq_range / 31.25f);
  if (!(bins < 16777216.0f)) throw std::invalid_argument("psk31 sync: frequency range above 2^24 bins");
  return static_cast<size_t>(bins) + 1;
}

std::vector<Carrier> find_carriers(const float* wf, size_t num_syms, size_t num_bins, size_t min_carrier_syms,
                                   float peak_margin_db, size_t max_cand) {
  std::vector<Carrier> out;
  if (num_syms == 0 || num_bins == 0) return out;
  const float ln_margin = peak_margin_db * 0.693147180559945309417f / 3.0f;
  const size_t min_run = min_carrier_syms > 1 ? min_carrier_syms : 1;
  const float neg_inf = -std::numeric_limits<float>::infinity();
  std::vector<float> bin_medians(num_bins), col(num_syms);
  for (size_t bin = 0; bin < num_bins; ++bin) {
    for (size_t s = 0; s < num_syms; ++s) col[s] = wf[s * num_bins + bin];
    bin_medians[bin] = median_f32(col.data(), num_syms);
  }
  std::vector<float> bm = bin_medians;
  const float noise_floor = median_f32(bm.data(), num_bins);
  const float global_threshold = noise_floor + ln_margin;

  for (size_t bin = 0; bin < num_bins; ++bin) {
    const float bin_median = bin_medians[bin];
    const float per_bin_threshold = bin_median + ln_margin;
    bool in_run = false;
    size_t run_start = 0, run_len = 0;
    float run_energy_sum = 0.0f;
    const auto record = [&] {
      out.push_back({static_cast<int32_t>(run_start), static_cast<uint32_t>(bin),
                     run_energy_sum / static_cast<float>(run_len)});
    };
    for (size_t sym = 0; sym < num_syms; ++sym) {
      const float e = wf[sym * num_bins + bin];
      const float e_left = bin > 0 ? wf[sym * num_bins + bin - 1] : neg_inf;
      const float e_right = bin + 1 < num_bins ? wf[sym * num_bins + bin + 1] : neg_inf;
      const bool is_peak = (e > per_bin_threshold || bin_median > global_threshold) && e >= e_left && e >= e_right;
      if (is_peak) {
        if (!in_run) {
          in_run = true;
          run_start = sym;
          run_energy_sum = 0.0f;
          run_len = 0;
        }
        run_energy_sum += e;
        run_len += 1;
      } else if (in_run) {
        in_run = false;
        if (run_len >= min_run) record();
        run_len = 0;
      }
    }
    if (in_run && run_len >= min_run) record();  // a run that reaches the end of the buffer
  }
  // score descending (an unordered pair compares Equal, psk31_sync.rs:198-202); equal scores
  // by freq_bin, then time_sym: the runs were recorded in exactly that order
  std::stable_sort(out.begin(), out.end(), [](const Carrier& a, const Carrier& b) { return b.score < a.score; });
  if (out.size() > max_cand) out.resize(max_cand);
  return out;
}

void bpsk31_decide(const float* soft, size_t n, uint8_t* bits) {
  for (size_t i = 0; i < n; ++i) bits[i] = soft[i] >= 0.0f ? 1 : 0;
}

}  // namespace psk31
}  // namespace orion
