// A stand-alone host program over orion-sdr_amd/csrc/ldpc.cpp (test infrastructure):
// tests/test_ldpc_oracle.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a subprocess. It encodes a few payloads for
// FT8 and FT4, decodes them clean, with one weak wrong bit, from noise and from the
// non-finite edge cases under both check rules, and exits 0 when the results are the
// expected ones and the sanitizers saw nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "ldpc.hpp"

using namespace orion::ldpc;

static int g_fail = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                 \
    }                                                           \
  } while (0)

static uint32_t g_state = 0x2545F491u;
static uint32_t next_u32() {  // xorshift32
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return g_state;
}

int main() {
  const Tables& t = tables();
  int sevens = 0;
  for (int j = 0; j < kM; ++j) sevens += t.row_start[j + 1] - t.row_start[j] == 7;
  CHECK(sevens == 24 && t.row_start[kM] == kEdges);

  for (int protocol = kFt8; protocol <= kFt4; ++protocol) {
    for (int trial = 0; trial < 4; ++trial) {
      uint8_t payload[10];
      for (int i = 0; i < 10; ++i) payload[i] = static_cast<uint8_t>(trial == 3 ? 0xFF : next_u32());
      uint8_t want[10];
      std::memcpy(want, payload, 10);
      want[9] &= 0xF8;
      uint8_t tones[kFt4Tones];
      encode_tones(protocol, payload, tones);
      float llr[kN];
      frame_to_llr_hard(protocol, tones, llr);
      for (int rule = kRuleReference; rule <= kRuleSumProduct; ++rule) {
        Result r;
        uint8_t plain[kN];
        decode_payload(protocol, llr, 20, rule, &r, plain);
        CHECK(r.status == kDecoded && r.iterations == 0 && r.errors == 0 && std::memcmp(r.payload, want, 10) == 0);
        CHECK(count_errors(plain) == 0);
        // one weak wrong bit in a check with 7 entries (bit 0): only sum_product corrects it
        float bad[kN];
        std::memcpy(bad, llr, sizeof bad);
        bad[0] = -0.3f * bad[0];
        decode_payload(protocol, bad, 20, rule, &r, nullptr);
        if (rule == kRuleSumProduct)
          CHECK(r.status == kDecoded && r.iterations >= 1 && std::memcmp(r.payload, want, 10) == 0);
        else
          CHECK(r.status == kParityFailed && r.iterations == 20 && r.errors > 0);
        // max_iter 0 and 1
        decode_payload(protocol, bad, 0, rule, &r, nullptr);
        CHECK(r.status == kParityFailed && r.iterations == 0 && r.errors > 0);
        decode_payload(protocol, bad, 1, rule, &r, nullptr);
        CHECK(r.iterations == 1);
        // non-finite input
        float odd[kN];
        for (int i = 0; i < kN; ++i) odd[i] = llr[i] > 0 ? std::numeric_limits<float>::infinity()
                                                         : -std::numeric_limits<float>::infinity();
        decode_payload(protocol, odd, 20, rule, &r, plain);
        CHECK(r.status == kDecoded);
        std::memcpy(odd, llr, sizeof odd);
        odd[3] = odd[90] = odd[171] = std::nanf("");
        decode_payload(protocol, odd, 20, rule, &r, plain);
        CHECK(r.iterations <= 20);
        // noise and zeros run to max_iter
        float noise[kN];
        for (int i = 0; i < kN; ++i) noise[i] = static_cast<float>(static_cast<int32_t>(next_u32())) * (1.0f / 268435456.0f);
        decode_payload(protocol, noise, 20, rule, &r, plain);
        CHECK(r.iterations <= 20 && r.errors == count_errors(plain));
        float zeros[kN] = {};
        decode_payload(protocol, zeros, 20, rule, &r, plain);
        CHECK(r.errors == 24 && r.iterations == 20 && r.status == kParityFailed);
      }
    }
  }
  const uint8_t msg[12] = {0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC, 0xDE, 0xF0, 0x11, 0x20, 0, 0};
  uint8_t a91[kKBytes];
  add_crc(msg, a91);
  CHECK(extract_crc(a91) == crc14(msg, 82));
  if (g_fail)
    std::printf("ldpc_host: %d checks failed\n", g_fail);
  else
    std::printf("ldpc_host: ok\n");
  return g_fail ? 1 : 0;
}
