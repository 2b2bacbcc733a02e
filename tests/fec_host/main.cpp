// A stand-alone host program over orion-sdr_amd/csrc/fec.cpp (test infrastructure):
// tests/test_fec_oracle.py builds it with the host compiler and -fsanitize=address,undefined
// and runs it as a subprocess. It runs encode -> decode round trips of both codes at all five
// rates from 1 to 300 information bits, the decoder on noisy half-integer, all-zero, short,
// empty, huge (metrics overflow) and NaN input, the length predictor against the encoder, the
// block interleaver and its two chain drivers on full blocks, tails and empty input, and the
// argument errors; it exits 0 when the results are the expected ones and the sanitizers saw
// nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "fec.hpp"

using namespace orion::fec;

static int g_fail = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                     \
    }                                                               \
  } while (0)

static uint32_t g_state = 0x2545F491u;
static uint32_t next_u32() {  // xorshift32
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return g_state;
}
template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}
static float noise() {  // a sum of four uniforms, deviation about 1
  float s = 0.0f;
  for (int i = 0; i < 4; ++i) s += static_cast<float>(next_u32() >> 8) / 16777216.0f - 0.5f;
  return s * 1.732f;
}

int main() {
  const size_t sizes[] = {1, 2, 3, 5, 8, 33, 120, 188, 300};
  for (int code = kK5; code <= kDvbK7; ++code)
    for (int rate = kR1_2; rate <= kR7_8; ++rate)
      for (size_t n : sizes) {
        std::vector<uint8_t> info(n), coded(punctured_coded_len(code, n, rate)), bits(n);
        for (auto& b : info) b = static_cast<uint8_t>(next_u32() & 1u);
        // the encoder writes exactly the predicted length (the vector's end is the sanitizer's check)
        conv_encode_punctured(code, info.data(), n, rate, coded.data());
        const size_t nl = coded.size();
        std::vector<float> llr(nl);
        for (size_t i = 0; i < nl; ++i) llr[i] = coded[i] ? -4.0f : 4.0f;
        viterbi_decode_soft(code, llr.data(), nl, n, rate, bits.data());
        CHECK(bits == info);
        // noisy, half-integers (ties): a result, whatever it is
        std::vector<float> noisy(nl);
        for (size_t i = 0; i < nl; ++i)
          noisy[i] = std::round(((coded[i] ? -1.0f : 1.0f) + noise()) * 2.0f) / 2.0f;
        viterbi_decode_soft(code, noisy.data(), nl, n, rate, bits.data());
        for (uint8_t b : bits) CHECK(b <= 1);
        // all zeros: every candidate ties, the first one seen wins everywhere: all-zero bits
        std::vector<float> zeros(nl, 0.0f);
        viterbi_decode_soft(code, zeros.data(), nl, n, rate, bits.data());
        for (uint8_t b : bits) CHECK(b == 0);
        // short and empty input (a heap slice of exactly that length), and a longer one
        std::vector<float> half(noisy.begin(), noisy.begin() + static_cast<long>(nl / 2));
        viterbi_decode_soft(code, half.data(), half.size(), n, rate, bits.data());
        viterbi_decode_soft(code, nullptr, 0, n, rate, bits.data());
        for (uint8_t b : bits) CHECK(b == 0);
        std::vector<float> longer(llr);
        longer.resize(nl + 9, -7.0f);
        viterbi_decode_soft(code, longer.data(), longer.size(), n, rate, bits.data());
        CHECK(bits == info);
        // metrics that overflow, infinities and NaN: no fault, bits that are bits
        std::vector<float> huge(noisy);
        for (auto& v : huge) v *= 1e38f;
        viterbi_decode_soft(code, huge.data(), nl, n, rate, bits.data());
        for (uint8_t b : bits) CHECK(b <= 1);
        huge[nl / 3] = std::numeric_limits<float>::quiet_NaN();
        huge[0] = std::numeric_limits<float>::infinity();
        viterbi_decode_soft(code, huge.data(), nl, n, rate, bits.data());
        for (uint8_t b : bits) CHECK(b <= 1);
      }

  // the impulse responses are the generators (tests/unit/fec.rs)
  {
    const uint8_t one = 1;
    uint8_t c[14];
    conv_encode_punctured(kDvbK7, &one, 1, kR1_2, c);
    const uint8_t g0[7] = {1, 1, 1, 1, 0, 0, 1}, g1[7] = {1, 0, 1, 1, 0, 1, 1};
    for (int i = 0; i < 7; ++i) CHECK(c[2 * i] == g0[i] && c[2 * i + 1] == g1[i]);
  }
  // info_bits == 0: nothing is written
  viterbi_decode_soft(kK5, nullptr, 0, 0, kR1_2, nullptr);
  CHECK(punctured_coded_len(kK5, 0, kR1_2) == 8 && punctured_coded_len(kDvbK7, 0, kR7_8) == 7);

  // the block interleaver
  const size_t dims[][2] = {{4, 4}, {3, 5}, {32, 32}, {1, 7}, {7, 1}};
  for (const auto& d : dims) {
    const BlockInterleaver bi(d[0], d[1]);
    const size_t n = bi.block_len();
    std::vector<uint8_t> x(n), y(n), z(n);
    for (auto& v : x) v = static_cast<uint8_t>(next_u32());
    bi.interleave(x.data(), y.data());
    for (size_t r = 0; r < d[0]; ++r)
      for (size_t c = 0; c < d[1]; ++c) CHECK(y[c * d[0] + r] == x[r * d[1] + c]);
    bi.deinterleave(y.data(), z.data());
    CHECK(x == z);
    std::vector<float> fx(n), fy(n), fz(n);
    for (auto& v : fx) v = noise();
    bi.interleave(fx.data(), fy.data());
    bi.deinterleave(fy.data(), fz.data());
    CHECK(fx == fz);
    // the chain drivers: every length from nothing to past two blocks
    for (size_t len = 0; len <= 2 * n + 3; len += (n > 100 ? 97 : 1)) {
      std::vector<uint8_t> b(len);
      for (auto& v : b) v = static_cast<uint8_t>(next_u32() & 1u);
      const std::vector<uint8_t> il = bi.interleave_bits(b.data(), len);
      CHECK(il.size() == bi.interleaved_len(len) && il.size() % n == 0 && il.size() >= len && il.size() < len + n);
      std::vector<float> fl(il.begin(), il.end());
      const std::vector<float> back = bi.deinterleave_llrs(fl.data(), fl.size());
      for (size_t i = 0; i < il.size(); ++i) CHECK(back[i] == (i < len ? static_cast<float>(b[i]) : 0.0f));
      std::vector<float> cut(len);
      for (auto& v : cut) v = noise();
      const std::vector<float> dc = bi.deinterleave_llrs(cut.data(), len);
      CHECK(dc.size() == len);
      for (size_t i = len / n * n; i < len; ++i) CHECK(dc[i] == cut[i]);  // the short tail as it is
    }
  }

  // argument errors
  uint8_t u[64] = {0};
  float f[64] = {0};
  CHECK(throws([&] { code_spec(2); }) && throws([&] { code_spec(-1); }));
  CHECK(throws([&] { rate_spec(5); }) && throws([&] { rate_spec(-1); }));
  CHECK(throws([&] { punctured_coded_len(kK5, kMaxInfoBits + 1, kR1_2); }));
  CHECK(throws([&] { conv_encode_punctured(3, u, 4, kR1_2, u); }));
  CHECK(throws([&] { viterbi_decode_soft(kK5, f, 8, 4, 9, u); }));
  CHECK(throws([&] { BlockInterleaver(0, 4); }) && throws([&] { BlockInterleaver(4, 0); }));
  CHECK(throws([&] { BlockInterleaver(size_t(1) << 40, size_t(1) << 40); }));

  if (g_fail) {
    std::printf("fec_host: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("fec_host: ok\n");
  return 0;
}
