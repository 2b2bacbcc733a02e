// ldpc_family.cpp — see ldpc_family.hpp. Every f32 operation is its own rounding
// (-ffp-contract=off), in the reference's order; / is the IEEE divide.
#include "ldpc_family.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

namespace orion {
namespace ldpcf {

namespace {
struct Dim {
  size_t n, k;
  uint64_t seed;
};
// ldpc_codes.rs:56-73, 552-558
constexpr Dim kDims[kNumCodes] = {{512, 256, 0x4C44504335313200ull},
                                  {576, 384, 0x4C44504335313201ull},
                                  {512, 384, 0x4C44504335313202ull}};

// ldpc_codes.rs:560-580
inline float fast_tanh(float x) {
  if (x < -4.97f) return -1.0f;
  if (x > 4.97f) return 1.0f;
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (105.0f + x2));
  const float b = 945.0f + x2 * (420.0f + x2 * 15.0f);
  return a / b;
}
inline float fast_atanh(float x) {
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (-735.0f + x2 * 64.0f));
  const float b = 945.0f + x2 * (-1050.0f + x2 * 225.0f);
  return a / b;
}
// f32::clamp(-1, 1): NaN passes through
inline float clamp1(float x) {
  if (x < -1.0f) x = -1.0f;
  if (x > 1.0f) x = 1.0f;
  return x;
}
}  // namespace

void check_rule(int rule) {
  if (rule < kRuleSumProduct || rule > kRuleScaledMinSum)
    throw std::invalid_argument("ldpc family: rule is sum_product, min_sum or scaled_min_sum");
}

const Ldpc& Ldpc::get(int code) {
  if (code < 0 || code >= kNumCodes) throw std::invalid_argument("ldpc family: code is n512r12, n576r23 or n512r34");
  static const Ldpc c0(kN512R12), c1(kN576R23), c2(kN512R34);  // built once, thread-safe
  return code == kN512R12 ? c0 : (code == kN576R23 ? c1 : c2);
}

// ldpc_codes.rs:134-280
Ldpc::Ldpc(int code) : code_(code), n_(kDims[code].n), k_(kDims[code].k), m_(n_ - k_) {
  const size_t m = m_, k = k_;
  std::vector<size_t> row_load(m, 0);
  std::vector<uint8_t> used_pairs(m * m, 0);  // [min * m + max]: two columns share this pair of rows
  auto pair_at = [&](size_t a, size_t b) -> uint8_t& { return used_pairs[std::min(a, b) * m + std::max(a, b)]; };
  uint64_t state = kDims[code].seed;
  auto next = [&] {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
  };
  std::vector<size_t> col_rows(k * kColWeight);
  for (size_t col = 0; col < k; ++col) {
    size_t rows[kColWeight], nrows = 0;
    auto has = [&](size_t r) { return std::find(rows, rows + nrows, r) != rows + nrows; };
    while (nrows < static_cast<size_t>(kColWeight)) {
      const size_t offset = static_cast<size_t>(next() % m);
      bool found = false;
      size_t best = 0, best_load = std::numeric_limits<size_t>::max();
      for (size_t step = 0; step < m; ++step) {
        const size_t r = (offset + step) % m;
        if (has(r)) continue;
        bool makes_cycle = false;
        for (size_t q = 0; q < nrows; ++q) makes_cycle = makes_cycle || pair_at(rows[q], r);
        if (makes_cycle) continue;
        if (row_load[r] < best_load) {
          best_load = row_load[r];
          best = r;
          found = true;
        }
      }
      if (!found) {  // no cycle-free row: the first free row from the offset
        ++relaxed_;
        for (size_t s = 0; s < m; ++s) {
          const size_t r = (offset + s) % m;
          if (!has(r)) {
            best = r;
            break;
          }
        }
      }
      rows[nrows++] = best;
    }
    for (size_t i = 0; i < nrows; ++i) {
      row_load[rows[i]] += 1;
      for (size_t j = i + 1; j < nrows; ++j) pair_at(rows[i], rows[j]) = 1;
    }
    std::sort(rows, rows + nrows);
    std::copy(rows, rows + nrows, col_rows.begin() + col * kColWeight);
  }

  // check -> bit and bit -> check incidence (ldpc_codes.rs:222-247)
  std::vector<std::vector<uint32_t>> cb(m), bc(n_);
  for (size_t col = 0; col < k; ++col)
    for (int j = 0; j < kColWeight; ++j) {
      const size_t r = col_rows[col * kColWeight + j];
      cb[r].push_back(static_cast<uint32_t>(col));
      bc[col].push_back(static_cast<uint32_t>(r));
    }
  for (size_t i = 0; i < m; ++i) {
    cb[i].push_back(static_cast<uint32_t>(k + i));
    bc[k + i].push_back(static_cast<uint32_t>(i));
    if (i > 0) {
      cb[i].push_back(static_cast<uint32_t>(k + i - 1));
      bc[k + i - 1].push_back(static_cast<uint32_t>(i));
    }
  }
  check_start_.assign(m + 1, 0);
  for (size_t c = 0; c < m; ++c) {
    check_start_[c + 1] = check_start_[c] + static_cast<uint32_t>(cb[c].size());
    check_bits_.insert(check_bits_.end(), cb[c].begin(), cb[c].end());
    max_deg_ = std::max(max_deg_, cb[c].size());
  }
  bit_start_.assign(n_ + 1, 0);
  for (size_t b = 0; b < n_; ++b) {
    bit_start_[b + 1] = bit_start_[b] + static_cast<uint32_t>(bc[b].size());
    for (uint32_t c : bc[b]) {
      const size_t idx = std::find(cb[c].begin(), cb[c].end(), static_cast<uint32_t>(b)) - cb[c].begin();
      bit_checks_.push_back(c);
      bit_edges_.push_back(check_start_[c] + static_cast<uint32_t>(idx));
    }
  }
}

void Ldpc::encode(const uint8_t* message, uint8_t* codeword) const {
  std::copy(message, message + k_, codeword);
  std::vector<uint8_t> s(m_, 0);
  for (size_t col = 0; col < k_; ++col)
    if (message[col] & 1)
      for (uint32_t j = bit_start_[col]; j < bit_start_[col + 1]; ++j) s[bit_checks_[j]] ^= 1;
  uint8_t prev = 0;
  for (size_t i = 0; i < m_; ++i) {
    const uint8_t p = s[i] ^ prev;
    codeword[k_ + i] = p;
    prev = p;
  }
}

size_t Ldpc::syndrome_weight(const uint8_t* hard) const {
  size_t unsat = 0;
  for (size_t c = 0; c < m_; ++c) {
    uint8_t x = 0;
    for (uint32_t e = check_start_[c]; e < check_start_[c + 1]; ++e) x ^= hard[check_bits_[e]] & 1;
    if (x != 0) ++unsat;
  }
  return unsat;
}

DecodeResult Ldpc::decode_soft(const float* llr, size_t max_iter, int rule, float scale, uint8_t* message) const {
  check_rule(rule);
  std::vector<uint8_t> hard(n_);
  for (size_t b = 0; b < n_; ++b) hard[b] = llr[b] <= 0.0f;
  const size_t init_unsat = syndrome_weight(hard.data());
  if (init_unsat == 0) {
    std::copy(hard.begin(), hard.begin() + k_, message);
    return {0, 0};
  }
  const size_t ne = n_edges();
  std::vector<float> msg(ne), ext(ne, 0.0f);
  for (size_t e = 0; e < ne; ++e) msg[e] = llr[check_bits_[e]];
  size_t min_unsat = init_unsat, iterations = 0;
  std::vector<uint8_t> best = hard;
  float tanh_half[kMaxCheckDeg];
  if (rule != kRuleScaledMinSum) scale = 1.0f;

  for (size_t iter = 0; iter < max_iter; ++iter) {
    iterations = iter + 1;
    for (size_t c = 0; c < m_; ++c) {
      const size_t base = check_start_[c], deg = check_start_[c + 1] - base;
      const float* msg_c = &msg[base];
      float* ext_c = &ext[base];
      if (rule == kRuleSumProduct) {
        for (size_t j = 0; j < deg; ++j) tanh_half[j] = fast_tanh(msg_c[j] / 2.0f);
        for (size_t i1 = 0; i1 < deg; ++i1) {
          float prod = 1.0f;
          for (size_t i2 = 0; i2 < deg; ++i2)
            if (i2 != i1) prod *= tanh_half[i2];
          ext_c[i1] = 2.0f * fast_atanh(clamp1(prod));
        }
      } else {
        float min1 = std::numeric_limits<float>::infinity(), min2 = min1, sign_parity = 1.0f;
        size_t argmin = 0;
        for (size_t j = 0; j < deg; ++j) {
          const float v = msg_c[j];
          if (v < 0.0f) sign_parity = -sign_parity;
          const float a = std::fabs(v);
          if (a < min1) {
            min2 = min1;
            min1 = a;
            argmin = j;
          } else if (a < min2) {
            min2 = a;
          }
        }
        for (size_t i1 = 0; i1 < deg; ++i1) {
          const float s_other = msg_c[i1] < 0.0f ? -sign_parity : sign_parity;
          const float mag = i1 == argmin ? min2 : min1;
          ext_c[i1] = (scale * s_other) * mag;
        }
      }
    }

    for (size_t b = 0; b < n_; ++b) {
      float l = llr[b];
      for (uint32_t j = bit_start_[b]; j < bit_start_[b + 1]; ++j) l += ext[bit_edges_[j]];
      hard[b] = l <= 0.0f;
    }
    const size_t unsat = syndrome_weight(hard.data());
    if (unsat < min_unsat) {
      min_unsat = unsat;
      best = hard;
      if (unsat == 0) break;
    }

    for (size_t b = 0; b < n_; ++b) {
      const uint32_t j0 = bit_start_[b], j1 = bit_start_[b + 1];
      float sum = ext[bit_edges_[j0]];  // every bit has at least one check
      for (uint32_t j = j0 + 1; j < j1; ++j) sum += ext[bit_edges_[j]];
      const float total = llr[b] + sum;
      for (uint32_t j = j0; j < j1; ++j) msg[bit_edges_[j]] = total - ext[bit_edges_[j]];
    }
  }
  std::copy(best.begin(), best.begin() + k_, message);
  return {min_unsat, iterations};
}

size_t encoded_len(int code, size_t nbits) {
  const Ldpc& c = Ldpc::get(code);
  if (nbits > (size_t(1) << 40)) throw std::invalid_argument("ldpc family: nbits above 2^40");
  return (nbits + c.k() - 1) / c.k() * c.n();
}

void encode_stream(int code, const uint8_t* bits, size_t nbits, uint8_t* coded) {
  const Ldpc& c = Ldpc::get(code);
  std::vector<uint8_t> msg(c.k());
  for (size_t off = 0, w = 0; off < nbits; off += c.k(), ++w) {
    const size_t len = std::min(c.k(), nbits - off);
    std::copy(bits + off, bits + off + len, msg.begin());
    std::fill(msg.begin() + len, msg.end(), 0);
    c.encode(msg.data(), coded + w * c.n());
  }
}

}  // namespace ldpcf
}  // namespace orion
