// A stand-alone host program over orion-sdr_amd/csrc/psk31.cpp (test infrastructure):
// tests/test_psk31_oracle.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a subprocess. It runs the Varicode table,
// encoder and decoder (a text round trip, every byte, over-long runs of ones), the
// convolutional coder in one piece and bit by bit, the Viterbi decoders on clean, noisy,
// all-zero, NaN and huge input from 0 to 300 symbols, and the streaming decoder across its
// 256-symbol normalisation and around its 128-row ring, and a modulate -> demodulate -> decide
// -> Varicode round trip of both modes at two sample rates, with and without the RF stage,
// fed in ragged calls with a capacity that cuts calls short, and the carrier search on a small
// array with runs at both edges; it exits 0 when the results are the expected ones and the
// sanitizers saw nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "psk31.hpp"

using namespace orion::psk31;

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
template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}
static float noise() {  // a sum of four uniforms, deviation about 0.5
  float s = 0.0f;
  for (int i = 0; i < 4; ++i) s += static_cast<float>(next_u32() >> 8) / 16777216.0f - 0.5f;
  return s * 0.866f;
}

// memcmp's pointers may not be null even for n == 0 (an empty vector's data() is)
static bool same(const uint8_t* a, const uint8_t* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

static std::vector<float> dqpsk(const std::vector<uint8_t>& bits, float sigma) {
  std::vector<uint8_t> coded(2 * bits.size());
  conv_encode(bits.data(), bits.size(), coded.data());
  std::vector<float> soft(2 * bits.size());
  for (size_t i = 0; i < bits.size(); ++i) {
    const int d = coded[2 * i] * 2 + coded[2 * i + 1];
    soft[2 * i] = kDqpskExp[d][0] + sigma * noise();
    soft[2 * i + 1] = kDqpskExp[d][1] + sigma * noise();
  }
  return soft;
}

int main() {
  // ---- Varicode ----
  const Codeword* tab = varicode_table();
  for (int i = 0; i < 128; ++i) {
    CHECK(tab[i].len >= 1 && tab[i].len <= kVaricodeMaxBits);
    CHECK(varicode_decode(tab[i].bits, tab[i].len) == i);
    CHECK((tab[i].bits & 1) && (tab[i].bits >> (tab[i].len - 1)) == 1);
    for (int k = 0; k + 1 < tab[i].len; ++k) CHECK(((tab[i].bits >> k) & 3) != 0);  // no "00" inside
  }
  CHECK(varicode_encode(200).bits == tab[0].bits && varicode_decode(0, 3) == -1 && varicode_decode(1, 0) == -1);
  {
    const std::string text = "CQ CQ de TEST 599 ~\x7f";
    VaricodeEncoder enc;
    enc.push_preamble(32);
    for (char c : text) enc.push_byte(static_cast<uint8_t>(c));
    enc.push_postamble(32);
    const size_t pend = enc.pending();
    std::vector<uint8_t> bits = enc.drain_bits();
    CHECK(bits.size() == pend && enc.is_empty() && enc.next_bit() == -1);
    VaricodeDecoder dec;
    std::string back;
    for (uint8_t b : bits) dec.push_bit(b);
    dec.push_bit(0);
    dec.push_bit(0);
    for (int c; (c = dec.pop_char()) >= 0;) back.push_back(static_cast<char>(c));
    CHECK(back == text);  // the 32 ones of the postamble are no codeword
    // a run of ones far past the shift register's width, then a valid character
    for (int i = 0; i < 100; ++i) dec.push_bit(1);
    for (uint8_t b : {0, 0, 1, 1, 0, 0}) dec.push_bit(b);
    CHECK(dec.pending() == 1 && dec.pop_char() == 'e' && dec.pop_char() == -1);
  }

  // ---- the coder, whole and bit by bit ----
  std::vector<uint8_t> bits(300);
  for (auto& b : bits) b = static_cast<uint8_t>(next_u32() & 1);
  std::vector<uint8_t> coded(600), coded2(600);
  conv_encode(bits.data(), bits.size(), coded.data());
  ConvEncoder ce;
  for (size_t i = 0; i < bits.size(); ++i) ce.encode(bits[i] | 0xFE, &coded2[2 * i], &coded2[2 * i + 1]);  // bit 0 alone counts
  CHECK(coded == coded2);
  ce.reset();
  uint8_t c0, c1;
  ce.encode(1, &c0, &c1);
  CHECK(c0 == 1 && c1 == 1);  // a 1 into the zero register: both generators tap bit 4
  conv_encode(nullptr, 0, nullptr);

  // ---- Viterbi ----
  for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(5), size_t(33), size_t(300)}) {
    std::vector<uint8_t> in(bits.begin(), bits.begin() + n), out(n + 1, 7), hard(n + 1, 7);
    std::vector<uint8_t> cd(2 * n + 1);
    conv_encode(in.data(), n, cd.data());
    viterbi_decode_hard(cd.data(), n, hard.data());
    CHECK(same(hard.data(), in.data(), n) && hard[n] == 7);
    std::vector<float> soft = dqpsk(in, 0.0f);
    soft.push_back(0.0f);
    viterbi_decode(soft.data(), n, out.data());
    CHECK(same(out.data(), in.data(), n) && out[n] == 7);
    soft = dqpsk(in, 0.25f);
    soft.push_back(0.0f);
    viterbi_decode(soft.data(), n, out.data());
    if (n >= 33) CHECK(same(out.data(), in.data(), n - 8));  // the tail has no flush bits behind it
    // all-zero input: every comparison ties; NaN and huge input: defined, if meaningless
    std::vector<float> z(2 * n + 1, 0.0f);
    viterbi_decode(z.data(), n, out.data());
    for (size_t i = 0; i < n; ++i) CHECK(out[i] == 0);
    for (float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::max(),
                    std::numeric_limits<float>::infinity()}) {
      std::fill(z.begin(), z.end(), v);
      viterbi_decode(z.data(), n, out.data());
      for (size_t i = 0; i < n; ++i) CHECK(out[i] <= 1);
    }
  }

  // ---- the streaming decoder: 700 symbols cross the normalisation twice and the ring five times ----
  {
    std::vector<uint8_t> in(700);
    for (auto& b : in) b = static_cast<uint8_t>(next_u32() & 1);
    const std::vector<float> soft = dqpsk(in, 0.2f);
    StreamingViterbi sv;
    std::vector<uint8_t> got;
    for (size_t i = 0; i < in.size(); ++i) {
      const int b = sv.feed_symbol(soft[2 * i], soft[2 * i + 1]);
      CHECK((b < 0) == (i < static_cast<size_t>(kTracebackDepth)));
      if (b >= 0) got.push_back(static_cast<uint8_t>(b));
    }
    const std::vector<uint8_t> rest = sv.flush();
    CHECK(rest.size() == static_cast<size_t>(kTracebackDepth));
    got.insert(got.end(), rest.begin(), rest.end());
    CHECK(got.size() == in.size());
    CHECK(same(got.data(), in.data(), in.size() - 8));
  }

  // ---- modulate -> demodulate -> decide -> Varicode ----
  CHECK(psk31_sps(8000.0f) == 256 && psk31_sps(12000.0f) == 384 && psk31_sps(10.0f) == 0 && psk31_sps(-1.0f) == 0);
  CHECK(psk31_sps(std::numeric_limits<float>::quiet_NaN()) == 0 && make_hann(0).empty() && make_hann(1)[0] == 1.0f);
  CHECK(demod_start_count(256, 0) == 0 && demod_start_count(256, 256) == 0 && demod_start_count(256, 263) == 249);
  for (int mode = kBpsk; mode <= kQpsk; ++mode) {
    for (float fs : {8000.0f, 12000.0f}) {
      for (float rf : {0.0f, 1000.0f}) {
        const std::string text = "CQ de TEST";
        const std::vector<uint8_t> tb =
            text_bits(reinterpret_cast<const uint8_t*>(text.data()), text.size(), 8, mode == kQpsk ? 24 : 8);
        Mod mod(mode, fs, rf, 0.5f);
        const size_t sps = mod.sps();
        std::vector<float> iq(2 * tb.size() * sps);
        // two calls: the phasor and the coder's register carry over; process() reads whole symbols only
        const size_t half = tb.size() / 2;
        mod.modulate_bits(tb.data(), half, iq.data());
        size_t in_read = 0, out_written = 0;
        mod.process(tb.data() + half, tb.size() - half, iq.data() + 2 * half * sps, (tb.size() - half) * sps + 5, &in_read,
                    &out_written);
        CHECK(in_read == tb.size() - half && out_written == in_read * sps);
        for (size_t i = 0; i < tb.size() * sps; ++i) iq[2 * i] += 0.01f * noise(), iq[2 * i + 1] += 0.01f * noise();

        Demod dem(mode, fs, rf, 2.0f, 0);
        const size_t per = mode == kQpsk ? 2 : 1;
        std::vector<float> soft(per * tb.size());
        size_t at = 0, got = 0;
        for (size_t want : {size_t(1000), size_t(1), size_t(5000), tb.size() * sps}) {
          const size_t n = std::min(want, tb.size() * sps - at);
          // a capacity of 7 values cuts the longer calls short: feed the rest again, as a caller would
          size_t done = 0;
          while (done < n) {
            float out[7];
            size_t r = 0, w = 0;
            dem.process(iq.data() + 2 * (at + done), n - done, out, 7, &r, &w);
            CHECK(r > 0 && w <= 7 && got + w <= soft.size());
            std::memcpy(soft.data() + got, out, w * sizeof(float));
            got += w;
            done += r;
          }
          at += n;
        }
        CHECK(got == soft.size());
        std::vector<uint8_t> bits(tb.size());
        if (mode == kBpsk)
          bpsk31_decide(soft.data(), soft.size(), bits.data());
        else
          viterbi_decode(soft.data(), tb.size(), bits.data());
        VaricodeDecoder dec;
        for (uint8_t b : bits) dec.push_bit(b);
        std::string back;
        for (int c; (c = dec.pop_char()) >= 0;) back.push_back(static_cast<char>(c));
        CHECK(back == text);
        dem.reset();
        CHECK(dem.state().count == 0 && dem.state().prev_re == 1.0f && dem.state().z_re == 1.0f);
      }
    }
  }
  // ---- the carrier search on a small array with runs at both edges ----
  {
    const size_t ns = 20, nb = 5;
    std::vector<float> wf(ns * nb, -27.6f);
    for (size_t s = 0; s < 9; ++s) wf[s * nb + 0] = -2.0f;    // bin 0 from symbol 0
    for (size_t s = 12; s < ns; ++s) wf[s * nb + 4] = -1.0f;  // bin 4 to the end of the buffer
    for (size_t s = 5; s < 8; ++s) wf[s * nb + 2] = -2.0f;    // too short
    std::vector<Carrier> c = find_carriers(wf.data(), ns, nb, 8, 6.0f, 10);
    CHECK(c.size() == 2 && c[0].freq_bin == 4 && c[0].time_sym == 12 && c[0].score == -1.0f);
    CHECK(c.size() == 2 && c[1].freq_bin == 0 && c[1].time_sym == 0 && c[1].score == -2.0f);
    CHECK(find_carriers(wf.data(), ns, nb, 8, 6.0f, 1).size() == 1 && find_carriers(wf.data(), ns, nb, 8, 6.0f, 0).empty());
    CHECK(find_carriers(wf.data(), 0, nb, 8, 6.0f, 4).empty());
    // one constant bin: nothing exceeds its own median, and the cross-bin floor is that median
    const std::vector<float> flat(ns, -2.0f);
    CHECK(find_carriers(flat.data(), ns, 1, 1, 6.0f, 4).empty());
    std::fill(wf.begin(), wf.end(), std::numeric_limits<float>::quiet_NaN());
    CHECK(find_carriers(wf.data(), ns, nb, 1, 6.0f, 4).empty());  // no comparison holds
    float even[4] = {3.0f, 1.0f, 2.0f, 10.0f}, odd[3] = {3.0f, 1.0f, 2.0f};
    CHECK(median_f32(even, 4) == 2.5f && median_f32(odd, 3) == 2.0f && median_f32(odd, 0) == 0.0f);
    CHECK(sync_num_bins(900.0f, 1100.0f) == 8 && sync_num_bins(0.0f, 3000.0f) == 97 && sync_num_bins(5.0f, 1.0f) == 1);
  }
  CHECK(throws([] { Mod(2, 8000.0f, 0.0f, 1.0f); }) && throws([] { Demod(kBpsk, 10.0f, 0.0f, 1.0f, 0); }));

  if (g_fail)
    std::printf("psk31_host: %d checks failed\n", g_fail);
  else
    std::printf("psk31_host: ok\n");
  return g_fail ? 1 : 0;
}
