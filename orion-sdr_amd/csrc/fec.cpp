// fec.cpp — host side of the inner code (fec.hpp): no device is touched.
#include "fec.hpp"

#include <limits>
#include <stdexcept>

namespace orion {
namespace fec {

namespace {
inline uint8_t parity(uint32_t x) { return static_cast<uint8_t>(__builtin_popcount(x) & 1); }

// conv.rs:112-120, (g0 row, g1 row) of each rate
constexpr int kPeriod[5] = {1, 2, 3, 5, 7};
constexpr uint8_t kG0[5][7] = {{1}, {1, 1}, {1, 1, 0}, {1, 1, 0, 1, 0}, {1, 1, 1, 1, 0, 1, 0}};
constexpr uint8_t kG1[5][7] = {{1}, {1, 0}, {1, 0, 1}, {1, 0, 1, 0, 1}, {1, 0, 0, 0, 1, 0, 1}};

void check_len(size_t info_bits) {
  if (info_bits > kMaxInfoBits) throw std::invalid_argument("fec: info_bits above 2^24");
}
}  // namespace

CodeSpec code_spec(int code) {
  if (code == kK5) return {4, 0x15u, 0x13u};       // 0b10101, 0b10011
  if (code == kDvbK7) return {6, 0x79u, 0x5Bu};    // 0b1111001, 0b1011011
  throw std::invalid_argument("fec: unknown code (ORION_FEC_K5 / ORION_FEC_DVB_K7)");
}

RateSpec rate_spec(int rate) {
  if (rate < kR1_2 || rate > kR7_8) throw std::invalid_argument("fec: unknown rate (ORION_FEC_RATE_1_2 .. _7_8)");
  RateSpec r{kPeriod[rate], 0, 0u};
  for (int col = 0; col < r.period; ++col) {
    if (kG0[rate][col]) r.keep |= 1u << (2 * col);
    if (kG1[rate][col]) r.keep |= 1u << (2 * col + 1);
  }
  r.kept = __builtin_popcount(r.keep);
  return r;
}

size_t punctured_coded_len(int code, size_t info_bits, int rate) {
  const CodeSpec c = code_spec(code);
  const RateSpec r = rate_spec(rate);
  check_len(info_bits);
  const size_t n_steps = info_bits + static_cast<size_t>(c.reg_bits);
  const size_t full = n_steps / static_cast<size_t>(r.period), rem = n_steps % static_cast<size_t>(r.period);
  return full * static_cast<size_t>(r.kept) +
         static_cast<size_t>(__builtin_popcount(r.keep & ((1u << (2 * rem)) - 1u)));
}

void conv_encode_punctured(int code, const uint8_t* info, size_t info_bits, int rate, uint8_t* out) {
  const CodeSpec c = code_spec(code);
  const RateSpec r = rate_spec(rate);
  check_len(info_bits);
  const size_t n_steps = info_bits + static_cast<size_t>(c.reg_bits);
  const uint32_t mask = (1u << c.reg_bits) - 1u;
  uint32_t state = 0;
  size_t at = 0;
  for (size_t t = 0; t < n_steps; ++t) {
    const uint32_t b = t < info_bits ? (info[t] & 1u) : 0u;  // the zero tail
    const uint32_t window = b << c.reg_bits | (state & mask);
    const int col = static_cast<int>(t % static_cast<size_t>(r.period));
    if (r.keep >> (2 * col) & 1u) out[at++] = parity(window & c.g0);
    if (r.keep >> (2 * col + 1) & 1u) out[at++] = parity(window & c.g1);
    state = state >> 1 | b << (c.reg_bits - 1);
  }
}

void viterbi_decode_soft(int code, const float* llr, size_t n_llr, size_t info_bits, int rate, uint8_t* bits) {
  const CodeSpec c = code_spec(code);
  const RateSpec r = rate_spec(rate);
  check_len(info_bits);
  if (info_bits == 0) return;
  const size_t n_steps = info_bits + static_cast<size_t>(c.reg_bits);
  const int num_states = 1 << c.reg_bits;
  const uint32_t mask = static_cast<uint32_t>(num_states) - 1u;

  // conv.rs:313-338: 0.0 where the puncturing deleted a bit and where the input has ended
  std::vector<float> full(2 * n_steps, 0.0f);
  size_t src = 0;
  for (size_t t = 0; t < n_steps; ++t) {
    const int col = static_cast<int>(t % static_cast<size_t>(r.period));
    for (int j = 0; j < 2; ++j)
      if (r.keep >> (2 * col + j) & 1u) {
        if (src < n_llr) full[2 * t + static_cast<size_t>(j)] = llr[src];
        ++src;
      }
  }

  // the trellis, conv.rs:141-152: branch (state, bit) -> the coded pair (c0 << 1 | c1), the next state
  uint8_t sym[64][2];
  uint8_t next[64][2];
  for (int s = 0; s < num_states; ++s)
    for (uint32_t b = 0; b < 2; ++b) {
      const uint32_t window = b << c.reg_bits | (static_cast<uint32_t>(s) & mask);
      sym[s][b] = static_cast<uint8_t>(parity(window & c.g0) << 1 | parity(window & c.g1));
      next[s][b] = static_cast<uint8_t>(static_cast<uint32_t>(s) >> 1 | b << (c.reg_bits - 1));
    }

  // conv.rs:343-383: correlations are maximised; states ascending, bit 0 then bit 1, a
  // survivor replaced on strict > only
  const float neg_inf = std::numeric_limits<float>::lowest() / 2.0f;
  float pm[64], new_pm[64];
  for (int s = 0; s < num_states; ++s) pm[s] = neg_inf;
  pm[0] = 0.0f;
  std::vector<uint8_t> prev_state(n_steps * static_cast<size_t>(num_states), 0);
  for (size_t t = 0; t < n_steps; ++t) {
    const float l0 = full[2 * t], l1 = full[2 * t + 1];
    const float corr[4] = {l0 + l1, l0 - l1, -l0 + l1, -l0 - l1};
    for (int s = 0; s < num_states; ++s) new_pm[s] = neg_inf;
    uint8_t* row = &prev_state[t * static_cast<size_t>(num_states)];
    for (int prev = 0; prev < num_states; ++prev) {
      const float pm_prev = pm[prev];
      if (pm_prev <= neg_inf) continue;
      for (int b = 0; b < 2; ++b) {
        const int ns = next[prev][b];
        const float cand = pm_prev + corr[sym[prev][b]];
        if (cand > new_pm[ns]) {
          new_pm[ns] = cand;
          row[ns] = static_cast<uint8_t>(prev);
        }
      }
    }
    for (int s = 0; s < num_states; ++s) pm[s] = new_pm[s];
  }

  // conv.rs:385-397: the zero tail ends the path in state 0; the tail's bits are dropped
  int state = 0;
  for (size_t t = n_steps; t-- > 0;) {
    if (t < info_bits) bits[t] = static_cast<uint8_t>(state >> (c.reg_bits - 1) & 1);
    state = prev_state[t * static_cast<size_t>(num_states) + static_cast<size_t>(state)];
  }
}

BlockInterleaver::BlockInterleaver(size_t rows, size_t cols) : rows_(rows), cols_(cols) {
  if (rows == 0 || cols == 0) throw std::invalid_argument("interleaver: rows and cols must be nonzero");
  if (rows > kMaxBlock || cols > kMaxBlock || rows * cols > kMaxBlock)
    throw std::invalid_argument("interleaver: rows * cols above 2^24");
}

std::vector<uint8_t> BlockInterleaver::interleave_bits(const uint8_t* bits, size_t n) const {
  const size_t block = block_len();
  std::vector<uint8_t> out(interleaved_len(n)), padded(block);
  for (size_t at = 0; at < n; at += block) {
    const size_t len = n - at < block ? n - at : block;
    for (size_t i = 0; i < block; ++i) padded[i] = i < len ? bits[at + i] : 0;
    interleave(padded.data(), out.data() + at);
  }
  return out;
}

std::vector<float> BlockInterleaver::deinterleave_llrs(const float* llr, size_t n) const {
  const size_t block = block_len();
  std::vector<float> out(n);
  size_t at = 0;
  for (; at + block <= n; at += block) deinterleave(llr + at, out.data() + at);
  for (; at < n; ++at) out[at] = llr[at];
  return out;
}

}  // namespace fec
}  // namespace orion
