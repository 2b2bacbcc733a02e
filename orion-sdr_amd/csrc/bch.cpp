// bch.cpp — see bch.hpp.
#include "bch.hpp"

#include <algorithm>
#include <stdexcept>

namespace orion {
namespace bch {

using rs::Gf256;

namespace {
// times (x + alpha), low degree first (bch.rs:289-298)
std::vector<uint8_t> poly_mul_linear(const Gf256& gf, const std::vector<uint8_t>& p, uint8_t alpha) {
  std::vector<uint8_t> out(p.size() + 1, 0);
  for (size_t i = 0; i < p.size(); ++i) {
    out[i + 1] ^= p[i];
    out[i] ^= gf.mul(p[i], alpha);
  }
  return out;
}
std::vector<uint8_t> poly_mul(const Gf256& gf, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
  std::vector<uint8_t> out(a.size() + b.size() - 1, 0);
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i] == 0) continue;
    for (size_t j = 0; j < b.size(); ++j)
      if (b[j] != 0) out[i + j] ^= gf.mul(a[i], b[j]);
  }
  return out;
}

// bch.rs:233-285
std::vector<uint8_t> build_generator(const Gf256& gf, size_t t) {
  if (t == 0) throw std::invalid_argument("bch: design t = 0");
  // from 2 t = 255 on, the root 2^0 joins all the others: 256 coefficients, too many
  if (t > 127) throw std::invalid_argument("bch: design t is too large for GF(2^8) (parity would exceed the block)");
  std::vector<uint8_t> covered(2 * t + 1, 0);
  std::vector<uint8_t> g_lo(1, 1);
  for (size_t i = 1; i <= 2 * t; ++i) {
    if (covered[i]) continue;
    std::vector<uint8_t> min_poly(1, 1);
    size_t e = i % 255;
    do {  // the conjugacy class of 2^i
      if (e >= 1 && e <= 2 * t) covered[e] = 1;
      min_poly = poly_mul_linear(gf, min_poly, gf.exp_of(e));
      e = e * 2 % 255;
    } while (e != i % 255);
    g_lo = poly_mul(gf, g_lo, min_poly);
  }
  if (g_lo.size() > 255)
    throw std::invalid_argument("bch: design t is too large for GF(2^8) (parity would exceed the block)");
  std::vector<uint8_t> g(g_lo.rbegin(), g_lo.rend());
  for (uint8_t& c : g) c &= 1;
  while (g.size() > 1 && g[0] == 0) g.erase(g.begin());
  return g;
}

// sigma += coef x^shift b (bch.rs:359-369)
void apply_correction(const Gf256& gf, std::vector<uint8_t>& sigma, const std::vector<uint8_t>& b, uint8_t coef,
                      size_t shift) {
  if (sigma.size() < b.size() + shift) sigma.resize(b.size() + shift, 0);
  for (size_t i = 0; i < b.size(); ++i)
    if (b[i] != 0) sigma[i + shift] ^= gf.mul(coef, b[i]);
}

// bch.rs:318-356, s[1 ..= 2 t]
std::vector<uint8_t> berlekamp_massey(const Gf256& gf, const std::vector<uint8_t>& s, size_t t) {
  std::vector<uint8_t> sigma(1, 1), b(1, 1);
  size_t l = 0, m = 1;
  for (size_t n = 1; n <= 2 * t; ++n) {
    uint8_t delta = s[n];
    for (size_t i = 1; i <= l; ++i)
      if (i < sigma.size()) delta ^= gf.mul(sigma[i], s[n - i]);
    if (delta == 0) {
      ++m;
    } else if (2 * l < n) {
      const std::vector<uint8_t> t_sigma = sigma;
      apply_correction(gf, sigma, b, delta, m);
      l = n - l;
      b = t_sigma;
      const uint8_t inv = gf.inv(delta);
      for (uint8_t& c : b) c = gf.mul(c, inv);
      m = 1;
    } else {
      apply_correction(gf, sigma, b, delta, m);
      ++m;
    }
  }
  return sigma;
}
}  // namespace

Bch::Bch(size_t n, size_t t) : n_(n), t_(t) {
  if (n == 0 || n > 255) throw std::invalid_argument("bch: shortened length n out of range 1..=255");
  gen_ = build_generator(Gf256::shared(), t);
  if (parity_bits() >= n) throw std::invalid_argument("bch: shortened length n leaves no room for the parity bits");
}

Bch Bch::for_info_bits(size_t t, size_t info_bits) {
  const Bch full(255, t);
  if (info_bits == 0 || info_bits > 255) throw std::invalid_argument("bch: info_bits out of range");
  return Bch(info_bits + full.parity_bits(), t);
}

void Bch::encode(const uint8_t* message, uint8_t* codeword) const {
  const size_t pb = parity_bits(), kk = k();
  std::vector<uint8_t> reg(pb, 0);
  for (size_t p = 0; p < kk; ++p) {
    const uint8_t feedback = message[p] ^ reg[0];
    for (size_t i = 0; i + 1 < pb; ++i) reg[i] = reg[i + 1] ^ (gen_[i + 1] & feedback);
    reg[pb - 1] = gen_[pb] & feedback;
  }
  std::copy(message, message + kk, codeword);
  std::copy(reg.begin(), reg.end(), codeword + kk);
}

size_t Bch::residual_errors(const uint8_t* word) const {
  const Gf256& gf = Gf256::shared();
  const size_t shift = 255 - n_;
  size_t count = 0;
  for (size_t j = 1; j <= 2 * t_; ++j) {
    uint8_t acc = 0;
    for (size_t p = 0; p < n_; ++p)
      if (word[p] != 0) acc ^= gf.pow(gf.exp_of(j), n_ - 1 - p + shift);
    if (acc != 0) ++count;
  }
  return count;
}

int Bch::decode(const uint8_t* received, uint8_t* message, size_t* locator_len) const {
  const Gf256& gf = Gf256::shared();
  const size_t shift = 255 - n_, two_t = 2 * t_, kk = k();
  if (locator_len) *locator_len = 0;
  std::copy(received, received + kk, message);  // every path but a correction leaves this
  std::vector<uint8_t> syndromes(two_t + 1, 0);
  bool has_error = false;
  for (size_t j = 1; j <= two_t; ++j) {
    uint8_t acc = 0;
    for (size_t p = 0; p < n_; ++p)
      if (received[p] != 0) acc ^= gf.pow(gf.exp_of(j), n_ - 1 - p + shift);
    syndromes[j] = acc;
    if (acc != 0) has_error = true;
  }
  if (!has_error) return 0;

  const std::vector<uint8_t> sigma = berlekamp_massey(gf, syndromes, t_);
  if (locator_len) *locator_len = sigma.size();

  // Chien over all 255 degrees: sigma(2^-d) == 0 is an error at degree d
  std::vector<uint8_t> corrected(received, received + n_);
  size_t n_found = 0;
  for (size_t d = 0; d < 255; ++d) {
    const uint8_t x = gf.exp_of((255 - d % 255) % 255);
    uint8_t val = 0;
    for (size_t i = 0; i < sigma.size(); ++i)
      if (sigma[i] != 0) val ^= gf.mul(sigma[i], gf.pow(x, i));
    if (val == 0 && d >= shift && d <= n_ - 1 + shift) {  // below shift: never transmitted
      corrected[n_ - 1 + shift - d] ^= 1;
      ++n_found;
    }
  }
  const size_t residual = residual_errors(corrected.data());
  if (residual != 0 || n_found > t_) return -static_cast<int>(std::max(residual, n_found));
  std::copy(corrected.begin(), corrected.begin() + kk, message);
  return static_cast<int>(n_found);
}

size_t encoded_len(const Bch& code, size_t nbits) {
  if (nbits > (size_t(1) << 40)) throw std::invalid_argument("bch: nbits above 2^40");
  return (nbits + code.k() - 1) / code.k() * code.n();
}

void encode_stream(const Bch& code, const uint8_t* bits, size_t nbits, uint8_t* coded) {
  std::vector<uint8_t> msg(code.k());
  for (size_t off = 0, w = 0; off < nbits; off += code.k(), ++w) {
    const size_t len = std::min(code.k(), nbits - off);
    std::copy(bits + off, bits + off + len, msg.begin());
    std::fill(msg.begin() + len, msg.end(), 0);
    code.encode(msg.data(), coded + w * code.n());
  }
}

}  // namespace bch
}  // namespace orion
