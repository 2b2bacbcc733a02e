// bch.hpp — the outer BCH code of the COFDM frame chain, host side (no device): the binary
// BCH code over GF(2^8) (fec/bch.rs), primitive length 255, shortened to any n, correcting t
// bit errors; the frame's code is t = 8 over 120 information bits, 184 coded
// (shortened_bch_for, modulate/ofdm_frame.rs:485-552). The field is rs.hpp's. k_bch.hip's
// kernels are held to these functions byte for byte.
//
// Words are one bit per byte, index 0 the highest-degree term. The decoder takes an element
// as set when it is nonzero, corrects with ^= 1 and hands the other bits of an element back
// as they came.
//
// Everything here throws std::invalid_argument on a bad argument.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rs.hpp"

namespace orion {
namespace bch {

constexpr size_t kFrameInfoBits = 120;  // BCH_INFO_BITS

class Bch {
 public:
  // t >= 1, 1 <= n <= 255, parity bits < n (bch.rs:66-84)
  Bch(size_t n, size_t t);
  // shortened_bch_for: n = info_bits + the parity bits of t
  static Bch for_info_bits(size_t t, size_t info_bits);
  size_t n() const { return n_; }
  size_t k() const { return n_ - parity_bits(); }
  size_t t() const { return t_; }
  size_t parity_bits() const { return gen_.size() - 1; }
  // g(x), the product of the minimal polynomials of 2^1 .. 2^(2t), highest degree first, 0 / 1
  const std::vector<uint8_t>& generator() const { return gen_; }
  // message [k] -> codeword [n] = message | parity: the LFSR of bch.rs:105-125 (bit 0 of a
  // message element enters the parity, the element itself is copied)
  void encode(const uint8_t* message, uint8_t* codeword) const;
  // received [n] -> message [k] (bch.rs:131-207). Returns the number of bits flipped (parity
  // included) on success; on failure -max(residual, n_found) <= -1, the reference's error
  // payload, and message is then received[:k] (demodulate/ofdm_frame.rs:495-502).
  // locator_len (optional): entries of the locator vector Berlekamp-Massey returned, 0 for a
  // word without a nonzero syndrome.
  int decode(const uint8_t* received, uint8_t* message, size_t* locator_len = nullptr) const;

 private:
  size_t residual_errors(const uint8_t* word) const;
  size_t n_, t_;
  std::vector<uint8_t> gen_;
};

// The frame chain's drivers (outer_encode / outer_decode): ceil(nbits / k) words, the last
// message zero-padded.
size_t encoded_len(const Bch& code, size_t nbits);
void encode_stream(const Bch& code, const uint8_t* bits, size_t nbits, uint8_t* coded);

}  // namespace bch
}  // namespace orion
