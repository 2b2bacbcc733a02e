// ldpc_family.hpp — the inner LDPC family of the COFDM frame chain, host side (no device):
// the three constructed codes N512R12, N576R23 and N512R34 (fec/ldpc_codes.rs), their
// staircase encoder, the syndrome weight and the belief-propagation decoder under its three
// check rules. k_ldpc_family.hip's kernels are held to these functions in every output.
//
// H = [A | T]: the K message columns tap three rows each, chosen at construction by the
// seeded xorshift, the least-loaded row from a rotating offset and the A-block 4-cycle guard
// (ldpc_codes.rs:134-220); T is the lower-bidiagonal staircase. Within a check the message
// columns come ascending, then column K + i, then K + i - 1 (i > 0); within a bit the checks
// come ascending. Edge e of check c is entry e - check_start[c] of that check's list; every
// edge belongs to one check and one bit.
//
// Everything here throws std::invalid_argument on a bad argument.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orion {
namespace ldpcf {

enum : int { kN512R12 = 0, kN576R23 = 1, kN512R34 = 2, kNumCodes = 3 };
enum : int { kRuleSumProduct = 0, kRuleMinSum = 1, kRuleScaledMinSum = 2 };
constexpr int kColWeight = 3;      // rows tapped per message column
constexpr int kMaxN = 576, kMaxM = 256, kMaxEdges = 1535, kMaxCheckDeg = 11;
constexpr size_t kDefaultMaxIter = 50;  // demodulate/ofdm_frame.rs:448

struct DecodeResult {
  size_t unsat;       // the smallest unsatisfied-check count seen (0: a codeword was reached)
  size_t iterations;  // iterations run; 0 when the initial decision was a codeword
};

class Ldpc {
 public:
  // the code, built on first use and kept; code: kN512R12 .. kN512R34
  static const Ldpc& get(int code);
  int code() const { return code_; }
  size_t n() const { return n_; }
  size_t k() const { return k_; }
  size_t m() const { return m_; }
  size_t n_edges() const { return check_bits_.size(); }
  size_t max_check_degree() const { return max_deg_; }
  // picks for which no 4-cycle-free row was left and the guard was relaxed
  size_t relaxed_picks() const { return relaxed_; }
  // the graph as CSR: check_start [m + 1], check_bits [edges]; bit_start [n + 1], bit_checks
  // [edges] and, parallel to it, bit_edges [edges]: the edge (an index into check_bits) of that
  // bit in that check
  const std::vector<uint32_t>& check_start() const { return check_start_; }
  const std::vector<uint32_t>& check_bits() const { return check_bits_; }
  const std::vector<uint32_t>& bit_start() const { return bit_start_; }
  const std::vector<uint32_t>& bit_checks() const { return bit_checks_; }
  const std::vector<uint32_t>& bit_edges() const { return bit_edges_; }

  // message [k] -> codeword [n] = message | parity (ldpc_codes.rs:304-328): the message bytes
  // are copied as they are, bit 0 of each enters the parity.
  void encode(const uint8_t* message, uint8_t* codeword) const;
  // unsatisfied checks of hard [n] (bit 0 of each element)
  size_t syndrome_weight(const uint8_t* hard) const;
  // decode_soft_with (ldpc_codes.rs:366-540): llr [n], positive meaning bit 0 -> message [k].
  DecodeResult decode_soft(const float* llr, size_t max_iter, int rule, float scale, uint8_t* message) const;

 private:
  explicit Ldpc(int code);
  int code_;
  size_t n_, k_, m_, max_deg_ = 0, relaxed_ = 0;
  std::vector<uint32_t> check_start_, check_bits_, bit_start_, bit_checks_, bit_edges_;
};

// rule: kRuleSumProduct .. kRuleScaledMinSum; throws otherwise
void check_rule(int rule);

// The frame chain's drivers (modulate/ofdm_frame.rs:525-538, demodulate/ofdm_frame.rs:438-455).
// encode_stream: ceil(nbits / K) codewords, the last message zero-padded.
size_t encoded_len(int code, size_t nbits);
void encode_stream(int code, const uint8_t* bits, size_t nbits, uint8_t* coded);

}  // namespace ldpcf
}  // namespace orion
