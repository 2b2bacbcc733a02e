// ldpc.cpp — host side of the FT8 / FT4 channel codec (ldpc.hpp). No HIP here.
#include "ldpc.hpp"

#include <cstring>
#include <stdexcept>

namespace orion {
namespace ldpc {

namespace {
// gray.rs:10,28: binary index -> tone
constexpr uint8_t kGray8[8] = {0, 1, 3, 2, 5, 6, 4, 7};
constexpr uint8_t kGray4[4] = {0, 1, 3, 2};

struct Row {  // one row of H as 174 bits
  uint64_t w[3] = {0, 0, 0};
  bool get(int i) const { return (w[i >> 6] >> (i & 63)) & 1u; }
  void flip(int i) { w[i >> 6] ^= 1ull << (i & 63); }
  void operator^=(const Row& o) {
    for (int k = 0; k < 3; ++k) w[k] ^= o.w[k];
  }
};

Tables derive() {
  Tables t;
  std::memset(&t, 0, sizeof t);
  int len[kM] = {};
  for (int k = 0; k < kEdges; ++k) ++len[kEdge[k][0]];
  for (int j = 0; j < kM; ++j) t.row_start[j + 1] = static_cast<uint16_t>(t.row_start[j] + len[j]);
  // the checks of each bit in ascending check order: the edge list is check-major
  int seen[kN] = {};
  for (int k = 0; k < kEdges; ++k) {
    const int i = kEdge[k][1];
    if (seen[i] >= 3) throw std::logic_error("ldpc: a bit in more than 3 checks");
    t.bit_check[i][seen[i]] = kEdge[k][0];
    t.bit_edge[i][seen[i]] = static_cast<uint16_t>(k);
    ++seen[i];
  }
  // H = [Hm | Hp] (83 x 91, 83 x 83) and H c = 0 with c = [m | p] give p = Hp^-1 Hm m:
  // reduce the last 83 columns to the identity, the first 91 are then the generator.
  Row h[kM];
  for (int k = 0; k < kEdges; ++k) h[kEdge[k][0]].flip(kEdge[k][1]);
  for (int r = 0; r < kM; ++r) {
    const int c = kK + r;
    int piv = r;
    while (piv < kM && !h[piv].get(c)) ++piv;
    if (piv == kM) throw std::logic_error("ldpc: the parity part of H is singular");
    if (piv != r) {
      const Row tmp = h[piv];
      h[piv] = h[r];
      h[r] = tmp;
    }
    for (int j = 0; j < kM; ++j)
      if (j != r && h[j].get(c)) h[j] ^= h[r];
  }
  for (int r = 0; r < kM; ++r)
    for (int i = 0; i < kK; ++i)
      if (h[r].get(i)) t.generator[r][i / 8] |= static_cast<uint8_t>(0x80 >> (i % 8));
  return t;
}

uint8_t parity8(uint8_t x) {
  x ^= x >> 4;
  x ^= x >> 2;
  x ^= x >> 1;
  return x & 1;
}

// ldpc.rs:644-663
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
}  // namespace

const Tables& tables() {
  static const Tables t = derive();
  return t;
}

uint16_t crc14(const uint8_t* message, int num_bits) {
  constexpr uint16_t kTop = 1u << 13;
  uint16_t rem = 0;
  int idx_byte = 0;
  for (int idx_bit = 0; idx_bit < num_bits; ++idx_bit) {
    if (idx_bit % 8 == 0) rem ^= static_cast<uint16_t>(message[idx_byte++] << 6);
    rem = (rem & kTop) ? static_cast<uint16_t>((rem << 1) ^ kCrcPoly) : static_cast<uint16_t>(rem << 1);
  }
  return rem & 0x3FFF;
}

void add_crc(const uint8_t payload[10], uint8_t a91[kKBytes]) {
  std::memcpy(a91, payload, 10);
  a91[9] &= 0xF8;
  a91[10] = 0;
  a91[11] = 0;
  const uint16_t c = crc14(a91, 96 - 14);
  a91[9] |= static_cast<uint8_t>(c >> 11);
  a91[10] = static_cast<uint8_t>(c >> 3);
  a91[11] = static_cast<uint8_t>(c << 5);
}

uint16_t extract_crc(const uint8_t a91[kKBytes]) {
  return static_cast<uint16_t>((a91[9] & 0x07) << 11 | a91[10] << 3 | a91[11] >> 5);
}

void encode(const uint8_t a91[kKBytes], uint8_t codeword[kNBytes]) {
  const Tables& t = tables();
  for (int j = 0; j < kNBytes; ++j) codeword[j] = j < kKBytes ? a91[j] : 0;
  uint8_t col_mask = 0x80 >> (kK % 8);
  int col_idx = kKBytes - 1;
  for (int r = 0; r < kM; ++r) {
    uint8_t nsum = 0;
    for (int j = 0; j < kKBytes; ++j) nsum ^= parity8(a91[j] & t.generator[r][j]);
    if (nsum & 1) codeword[col_idx] |= col_mask;
    col_mask >>= 1;
    if (col_mask == 0) {
      col_mask = 0x80;
      ++col_idx;
    }
  }
}

int count_errors(const uint8_t plain[kN]) {
  const Tables& t = tables();
  int errors = 0;
  for (int j = 0; j < kM; ++j) {
    uint8_t x = 0;
    for (int k = t.row_start[j]; k < t.row_start[j + 1]; ++k) x ^= plain[kEdge[k][1]];
    if (x) ++errors;
  }
  return errors;
}

int num_tones(int protocol) {
  if (protocol == kFt8) return kFt8Tones;
  if (protocol == kFt4) return kFt4Tones;
  throw std::invalid_argument("unknown protocol (ORION_COSTAS_FT8 / ORION_COSTAS_FT4)");
}

void check_args(int protocol, int rule, size_t max_iter) {
  num_tones(protocol);
  if (rule != kRuleReference && rule != kRuleSumProduct)
    throw std::invalid_argument("unknown check rule (ORION_LDPC_RULE_REFERENCE / ORION_LDPC_RULE_SUM_PRODUCT)");
  if (max_iter > 255) throw std::invalid_argument("max_iter above 255");
}

void encode_tones(int protocol, const uint8_t payload[10], uint8_t* tones, const uint8_t* a91_xor) {
  const int nt = num_tones(protocol), nb = protocol == kFt8 ? 3 : 2;
  uint8_t p[10];
  for (int i = 0; i < 10; ++i) p[i] = protocol == kFt4 ? payload[i] ^ kFt4Xor[i] : payload[i];
  uint8_t a91[kKBytes], cw[kNBytes];
  add_crc(p, a91);
  if (a91_xor)
    for (int i = 0; i < kKBytes; ++i) a91[i] ^= a91_xor[i];
  encode(a91, cw);
  int bit = 0;
  for (int s = 0; s < nt; ++s) {
    uint8_t v = 0;
    for (int b = 0; b < nb; ++b, ++bit) v = static_cast<uint8_t>(v << 1 | ((cw[bit / 8] >> (7 - bit % 8)) & 1));
    tones[s] = protocol == kFt8 ? kGray8[v] : kGray4[v];
  }
}

void frame_to_llr_hard(int protocol, const uint8_t* tones, float llr[kN]) {
  const int nt = num_tones(protocol), nb = protocol == kFt8 ? 3 : 2;
  for (int s = 0; s < nt; ++s) {
    uint8_t bin = 0;  // the inverse Gray map of the tone's low bits (gray.rs:46-66)
    if (protocol == kFt8) {
      for (uint8_t v = 0; v < 8; ++v)
        if (kGray8[v] == (tones[s] & 7)) bin = v;
    } else {
      for (uint8_t v = 0; v < 4; ++v)
        if (kGray4[v] == (tones[s] & 3)) bin = v;
    }
    for (int b = 0; b < nb; ++b) llr[s * nb + b] = ((bin >> (nb - 1 - b)) & 1) ? -10.0f : 10.0f;
  }
}

DecodeStat decode(const float llr[kN], int max_iter, int rule, uint8_t plain[kN]) {
  const Tables& t = tables();
  for (int i = 0; i < kN; ++i) plain[i] = llr[i] <= 0.0f;
  const int init_errors = count_errors(plain);
  if (init_errors == 0) return {0, 0};

  // One message per edge: m (bit -> check) and e (check -> bit). The reference's
  // m[check][bit] / e[check][bit] arrays are read and written at the edges only.
  float m[kEdges], tm[kEdges], e[kEdges];
  for (int k = 0; k < kEdges; ++k) m[k] = llr[kEdge[k][1]];
  int min_errors = init_errors, iterations = 0;
  uint8_t best[kN];
  std::memcpy(best, plain, kN);

  for (int iter = 0; iter < max_iter; ++iter) {
    ++iterations;
    // check update: the reference takes fast_tanh(-m / 2) anew for every pair; it is
    // one value per edge
    for (int k = 0; k < kEdges; ++k) tm[k] = fast_tanh(-m[k] / 2.0f);
    for (int j = 0; j < kM; ++j) {
      const int lo = t.row_start[j], hi = t.row_start[j + 1];
      const float factor = (rule == kRuleSumProduct && hi - lo == 7) ? 2.0f : -2.0f;
      for (int k1 = lo; k1 < hi; ++k1) {
        float a = 1.0f;
        for (int k2 = lo; k2 < hi; ++k2)
          if (k2 != k1) a *= tm[k2];
        e[k1] = factor * fast_atanh(a);
      }
    }
    // variable decision
    for (int i = 0; i < kN; ++i) {
      float l = llr[i];
      for (int ji = 0; ji < 3; ++ji) l += e[t.bit_edge[i][ji]];
      plain[i] = l <= 0.0f;
    }
    const int errors = count_errors(plain);
    if (errors < min_errors) {
      min_errors = errors;
      std::memcpy(best, plain, kN);
      if (errors == 0) break;
    }
    // variable -> check update
    for (int i = 0; i < kN; ++i)
      for (int ji1 = 0; ji1 < 3; ++ji1) {
        float l = llr[i];
        for (int ji2 = 0; ji2 < 3; ++ji2)
          if (ji2 != ji1) l += e[t.bit_edge[i][ji2]];
        m[t.bit_edge[i][ji1]] = l;
      }
  }
  std::memcpy(plain, best, kN);
  return {min_errors, iterations};
}

void finish(int protocol, const uint8_t plain[kN], DecodeStat st, Result* r) {
  std::memset(r, 0, sizeof *r);
  r->iterations = static_cast<uint8_t>(st.iterations);
  r->errors = static_cast<uint16_t>(st.errors);
  if (st.errors != 0) return;  // kParityFailed
  uint8_t a91[kKBytes] = {};
  for (int i = 0; i < kK; ++i)
    if (plain[i] == 1) a91[i / 8] |= static_cast<uint8_t>(0x80 >> (i % 8));
  const uint16_t extracted = extract_crc(a91);
  uint8_t buf[kKBytes];
  std::memcpy(buf, a91, kKBytes);
  buf[9] &= 0xF8;
  buf[10] = 0;
  buf[11] = 0;
  if (extracted != crc14(buf, 82)) {
    r->status = kCrcMismatch;
    return;
  }
  r->status = kDecoded;
  for (int i = 0; i < 10; ++i) r->payload[i] = protocol == kFt4 ? a91[i] ^ kFt4Xor[i] : a91[i];
  r->payload[9] &= 0xF8;
}

void decode_payload(int protocol, const float llr[kN], int max_iter, int rule, Result* r, uint8_t* plain) {
  uint8_t local[kN];
  uint8_t* p = plain ? plain : local;
  finish(protocol, p, decode(llr, max_iter, rule, p), r);
}

}  // namespace ldpc
}  // namespace orion
