// rs.cpp — the outer code of the COFDM / DVB-T chain, host side: see rs.hpp.
#include "rs.hpp"

#include <algorithm>
#include <stdexcept>

namespace orion {
namespace rs {

// ---- GF(2^8) --------------------------------------------------------------------------------
const Gf256& Gf256::shared() {
  static const Gf256 gf;
  return gf;
}
uint8_t Gf256::div(uint8_t a, uint8_t b) const {
  if (b == 0) throw std::invalid_argument("GF(2^8) division by zero");
  return a == 0 ? 0 : t_.exp[t_.log[a] + 255 - t_.log[b]];
}
uint8_t Gf256::inv(uint8_t a) const {
  if (a == 0) throw std::invalid_argument("GF(2^8) inverse of zero");
  return t_.exp[255 - t_.log[a]];
}
uint8_t Gf256::log_of(uint8_t a) const {
  if (a == 0) throw std::invalid_argument("GF(2^8) log of zero");
  return t_.log[a];
}

// ---- Reed-Solomon ---------------------------------------------------------------------------
namespace {
// low degree first, Horner from the top (poly_eval, reed_solomon.rs:276-282)
uint8_t poly_eval(const Gf256& gf, const std::vector<uint8_t>& p, uint8_t x) {
  uint8_t acc = 0;
  for (size_t i = p.size(); i-- > 0;) acc = gf.mul(acc, x) ^ p[i];
  return acc;
}

// sigma += coef x^shift b (apply_correction, reed_solomon.rs:321-331)
void apply_correction(const Gf256& gf, std::vector<uint8_t>& sigma, const std::vector<uint8_t>& b, uint8_t coef,
                      size_t shift) {
  if (sigma.size() < b.size() + shift) sigma.resize(b.size() + shift, 0);
  for (size_t i = 0; i < b.size(); ++i) sigma[i + shift] ^= gf.mul(coef, b[i]);
}

// reed_solomon.rs:286-318: 2 t iterations over s[0 .. 2 t)
std::vector<uint8_t> berlekamp_massey(const Gf256& gf, const std::vector<uint8_t>& s, size_t t) {
  std::vector<uint8_t> sigma{1}, b{1};
  size_t l = 0, m = 1;
  for (size_t n = 0; n < 2 * t; ++n) {
    uint8_t delta = s[n];
    for (size_t i = 1; i <= l; ++i)
      if (i < sigma.size()) delta ^= gf.mul(sigma[i], s[n - i]);
    if (delta == 0) {
      ++m;
    } else if (2 * l <= n) {
      const std::vector<uint8_t> t_sigma = sigma;
      apply_correction(gf, sigma, b, delta, m);
      l = n + 1 - l;
      b = t_sigma;
      const uint8_t inv = gf.inv(delta);
      for (auto& c : b) c = gf.mul(c, inv);
      m = 1;
    } else {
      apply_correction(gf, sigma, b, delta, m);
      ++m;
    }
  }
  return sigma;
}

// S_j = r(2^j), j < n_parity; position p has code degree n - 1 - p + (255 - n) = 254 - p
bool syndromes(const Gf256& gf, const uint8_t* word, size_t n, std::vector<uint8_t>& s) {
  bool nonzero = false;
  for (size_t j = 0; j < s.size(); ++j) {
    uint8_t acc = 0;
    for (size_t p = 0; p < n; ++p)
      if (word[p] != 0) acc ^= gf.mul(word[p], gf.pow(gf.exp_of(j), 254 - p));
    s[j] = acc;
    nonzero |= acc != 0;
  }
  return nonzero;
}
}  // namespace

ReedSolomon::ReedSolomon(size_t n, size_t n_parity) : n_(n), np_(n_parity) {
  if (n == 0 || n > 255 || n_parity >= n)
    throw std::invalid_argument("rs: code length n out of range 1..=255 or too short for the parity symbols");
  const Gf256& gf = Gf256::shared();
  gen_.assign(1, 1);
  for (size_t i = 0; i < np_; ++i) {  // times (x - 2^i)
    const uint8_t root = gf.exp_of(i);
    std::vector<uint8_t> out(gen_.size() + 1, 0);
    for (size_t d = 0; d < gen_.size(); ++d) {
      out[d + 1] ^= gen_[d];
      out[d] ^= gf.mul(gen_[d], root);
    }
    gen_ = out;
  }
}

void ReedSolomon::encode(const uint8_t* message, uint8_t* codeword) const {
  if (np_ == 0) throw std::invalid_argument("rs encode: a code without parity symbols has no shift register");
  const Gf256& gf = Gf256::shared();
  std::vector<uint8_t> reg(np_, 0);
  for (size_t p = 0; p < k(); ++p) {
    const uint8_t feedback = message[p] ^ reg[0];
    for (size_t i = 0; i + 1 < np_; ++i) reg[i] = reg[i + 1] ^ gf.mul(feedback, gen_[np_ - 1 - i]);
    reg[np_ - 1] = gf.mul(feedback, gen_[0]);
  }
  std::copy(message, message + k(), codeword);
  std::copy(reg.begin(), reg.end(), codeword + k());
}

int ReedSolomon::decode_counted(const uint8_t* received, uint8_t* message) const {
  const Gf256& gf = Gf256::shared();
  const size_t shift = 255 - n_;
  std::copy(received, received + k(), message);  // every path but a clean correction leaves this
  std::vector<uint8_t> s(np_, 0);
  if (!syndromes(gf, received, n_, s)) return 0;

  const std::vector<uint8_t> sigma = berlekamp_massey(gf, s, t());
  // Chien: the roots of sigma are 2^-i for an error of code degree i
  std::vector<size_t> error_degrees;
  for (size_t i = 0; i < 255; ++i) {
    const uint8_t x = gf.exp_of((255 - i) % 255);
    uint8_t val = 0;
    for (size_t d = 0; d < sigma.size(); ++d)
      if (sigma[d] != 0) val ^= gf.mul(sigma[d], gf.pow(x, d));
    if (val == 0) error_degrees.push_back(i);
  }
  size_t sigma_deg = 0;
  for (size_t d = 0; d < sigma.size(); ++d)
    if (sigma[d] != 0) sigma_deg = d;
  if (error_degrees.size() != sigma_deg || sigma_deg > t()) return -1;

  // omega = S sigma mod x^n_parity; sigma' keeps the odd-degree terms
  std::vector<uint8_t> omega(np_, 0);
  for (size_t i = 0; i < s.size(); ++i)
    for (size_t j = 0; j < sigma.size() && i + j < np_; ++j) omega[i + j] ^= gf.mul(s[i], sigma[j]);
  std::vector<uint8_t> deriv(sigma.size() > 1 ? sigma.size() - 1 : 1, 0);
  for (size_t d = 1; d < sigma.size(); d += 2) deriv[d - 1] = sigma[d];

  std::vector<uint8_t> corrected(received, received + n_);
  int n_corrected = 0;
  for (size_t i : error_degrees) {
    const uint8_t x = gf.exp_of(i), x_inv = gf.inv(x);
    const uint8_t omega_val = poly_eval(gf, omega, x_inv), deriv_val = poly_eval(gf, deriv, x_inv);
    if (deriv_val == 0) return -1;
    const uint8_t magnitude = gf.mul(x, gf.div(omega_val, deriv_val));
    if (i >= shift && magnitude != 0) {  // i <= 254 = n - 1 + shift always
      corrected[254 - i] ^= magnitude;
      ++n_corrected;
    }
  }
  if (syndromes(gf, corrected.data(), n_, s)) return -1;
  std::copy(corrected.begin(), corrected.begin() + static_cast<std::ptrdiff_t>(k()), message);
  return n_corrected;
}

// ---- the Forney interleaver -----------------------------------------------------------------
size_t conv_roundtrip_delay(size_t branches, size_t depth) {
  if (branches == 0 || depth == 0) throw std::invalid_argument("convolutional interleaver dimensions must be nonzero");
  if (branches > kMaxForney || depth > kMaxForney || branches * branches > kMaxForney ||
      branches * branches * depth > kMaxForney)
    throw std::invalid_argument("convolutional interleaver: branches^2 * depth above 2^24");
  return branches * (branches - 1) * depth;
}

ConvInterleaver::ConvInterleaver(size_t branches, size_t depth, bool inverse)
    : branches_(branches), depth_(depth), inverse_(inverse) {
  conv_roundtrip_delay(branches, depth);
  fifos_.resize(branches_);
  reset();
}

void ConvInterleaver::reset() {
  for (size_t j = 0; j < branches_; ++j) fifos_[j].assign(delay_of(j), 0);
  pos_ = 0;
}

void ConvInterleaver::feed(const uint8_t* in, size_t n, uint8_t* out) {
  for (size_t i = 0; i < n; ++i) {
    std::deque<uint8_t>& f = fifos_[pos_];
    uint8_t b = in[i];
    if (!f.empty()) {
      f.push_back(b);
      b = f.front();
      f.pop_front();
    }
    out[i] = b;
    if (++pos_ == branches_) pos_ = 0;
  }
}

std::vector<uint8_t> ConvInterleaver::flush() {
  std::vector<uint8_t> z(roundtrip_delay(), 0);
  feed(z.data(), z.size(), z.data());
  return z;
}

size_t forney_frame_len(size_t branches, size_t depth, size_t n) {
  const size_t d = conv_roundtrip_delay(branches, depth);
  if (n > (size_t(1) << 40)) throw std::invalid_argument("convolutional interleaver: n above 2^40");
  return (n + branches - 1) / branches * branches + d;
}

std::vector<uint8_t> forney_frame_interleave(size_t branches, size_t depth, const uint8_t* bytes, size_t n) {
  std::vector<uint8_t> out(forney_frame_len(branches, depth, n), 0);
  std::copy(bytes, bytes + n, out.begin());  // the padded payload, then the flush's zeros
  ConvInterleaver ci(branches, depth);
  ci.feed(out.data(), out.size(), out.data());
  return out;
}

std::vector<uint8_t> forney_frame_deinterleave(size_t branches, size_t depth, const uint8_t* bytes, size_t total) {
  const size_t d = conv_roundtrip_delay(branches, depth);
  if (total > (size_t(1) << 40)) throw std::invalid_argument("convolutional interleaver: n above 2^40");
  if (total <= d) return {};
  std::vector<uint8_t> all(total);
  ConvDeinterleaver di(branches, depth);
  di.feed(bytes, total, all.data());
  return std::vector<uint8_t>(all.begin() + static_cast<std::ptrdiff_t>(d), all.end());
}

void bytes_to_bits(const uint8_t* bytes, size_t n, uint8_t* bits) {
  for (size_t i = 0; i < n; ++i)
    for (int b = 0; b < 8; ++b) bits[8 * i + b] = (bytes[i] >> (7 - b)) & 1u;
}
void bits_to_bytes(const uint8_t* bits, size_t n_bytes, uint8_t* bytes) {
  for (size_t i = 0; i < n_bytes; ++i) {
    uint32_t v = 0;
    for (int b = 0; b < 8; ++b) v = v << 1 | (bits[8 * i + b] & 1u);
    bytes[i] = static_cast<uint8_t>(v);
  }
}

// ---- the PN scrambler -----------------------------------------------------------------------
PnScramblerStream::PnScramblerStream(uint32_t taps, uint32_t width, uint32_t seed)
    : taps_(taps), width_(width), seed_(seed), mask_(0), reg_(seed) {
  if (width < 2 || width > 32) throw std::invalid_argument("LFSR width must be in 2..=32");
  mask_ = width == 32 ? 0xFFFFFFFFu : (1u << width) - 1u;
  if (seed == 0) throw std::invalid_argument("LFSR seed must be nonzero");
  if (seed & ~mask_) throw std::invalid_argument("LFSR seed must fit in `width` bits");
  if (taps & ~mask_) throw std::invalid_argument("LFSR taps must fit in `width` bits");
}

void PnScramblerStream::feed_in_place(uint8_t* data, size_t n) {
  const uint32_t top = width_ - 1;
  for (size_t i = 0; i < n; ++i) {
    uint32_t pn = 0;
    for (int bit = 0; bit < 8; ++bit) {
      pn |= (reg_ & 1u) << bit;
      const uint32_t fb = static_cast<uint32_t>(__builtin_popcount(reg_ & taps_)) & 1u;
      reg_ = ((reg_ >> 1) | (fb << top)) & mask_;
    }
    data[i] ^= static_cast<uint8_t>(pn);
  }
}

// ---- the transport-stream layer -------------------------------------------------------------
size_t ts_energy_disperse(uint8_t* packets, size_t n) {
  if (n % kTsPacketLen) throw std::invalid_argument("TS energy dispersal needs whole 188-byte packets");
  DvbTEnergyDispersal prbs;
  for (size_t i = 0; i < n / kTsPacketLen; ++i) {
    uint8_t* packet = packets + i * kTsPacketLen;
    if (i % kTsDispersalGroup == 0) {
      prbs.reset();
      packet[0] ^= kTsSync ^ kTsSyncInverted;
    } else {
      prbs.advance_byte();
    }
    prbs.feed_in_place(packet + 1, kTsPayloadLen);
  }
  return n / kTsPacketLen;
}

const TsDispersalMask& ts_dispersal_mask() {
  static const TsDispersalMask mask = make_ts_dispersal_mask();
  return mask;
}

std::vector<uint8_t> ts_packetize(const uint8_t* payload, size_t n) {
  const size_t n_packets = std::max<size_t>((n + kTsPayloadLen - 1) / kTsPayloadLen, 1);
  std::vector<uint8_t> out(n_packets * kTsPacketLen, 0);
  out[0] = kTsSync;  // an empty payload still gives one packet
  for (size_t p = 0; p * kTsPayloadLen < n; ++p) {
    const size_t len = std::min(kTsPayloadLen, n - p * kTsPayloadLen);
    out[p * kTsPacketLen] = kTsSync;
    std::copy(payload + p * kTsPayloadLen, payload + p * kTsPayloadLen + len, out.begin() + static_cast<std::ptrdiff_t>(p * kTsPacketLen + 1));
  }
  return out;
}

std::vector<uint8_t> ts_depacketize(const uint8_t* packets, size_t n) {
  if (n == 0 || n % kTsPacketLen) throw std::invalid_argument("TS depacketize needs whole 188-byte packets, at least one");
  std::vector<uint8_t> out;
  out.reserve(n / kTsPacketLen * kTsPayloadLen);
  for (size_t p = 0; p < n; p += kTsPacketLen) out.insert(out.end(), packets + p + 1, packets + p + kTsPacketLen);
  return out;
}

void ts_null_packet(uint8_t out[kTsPacketLen]) {
  std::fill(out, out + kTsPacketLen, 0xFF);
  out[0] = kTsSync;
  out[1] = 0x1F;
  out[2] = 0xFF;
  out[3] = 0x10;
}

void ts_stuff_null_packets(std::vector<uint8_t>& ts, size_t target_packets) {
  if (ts.size() % kTsPacketLen) throw std::invalid_argument("ts_stuff_null_packets: ts must be whole TS packets");
  if (target_packets > (size_t(1) << 32)) throw std::invalid_argument("ts_stuff_null_packets: target above 2^32 packets");
  uint8_t null[kTsPacketLen];
  ts_null_packet(null);
  for (size_t have = ts.size() / kTsPacketLen; have < target_packets; ++have) ts.insert(ts.end(), null, null + kTsPacketLen);
}

}  // namespace rs
}  // namespace orion
