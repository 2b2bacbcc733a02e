// A stand-alone host program over orion-sdr_amd/csrc/ftmod.cpp (test infrastructure):
// tests/test_ftmod_oracle.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a subprocess. For FT8 and FT4 it modulates a
// frame with the scalar recurrence (with and without the RF stage), demodulates it back,
// checks the closed-form tables against the recurrence, and synthesises a small slot whose
// signals are clipped at both ends of their channel; it exits 0 when the results are the
// expected ones and the sanitizers saw nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "ftmod.hpp"

using namespace orion::ftmod;

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

int main() {
  for (int protocol = kFt8; protocol <= kFt4; ++protocol) {
    const Proto& m = proto(protocol);
    const size_t len = static_cast<size_t>(m.frame_len());
    uint8_t tones[kMaxData], back[kMaxData], syms[kMaxSyms];
    for (int k = 0; k < m.data; ++k) tones[k] = static_cast<uint8_t>(next_u32() % m.tones);
    symbol_sequence(protocol, tones, syms);
    int d = 0;
    for (int s = 0; s < m.total; ++s)
      if (is_data(protocol, s)) CHECK(syms[s] == tones[d++]);
    CHECK(d == m.data);

    // the recurrence, demodulated back; its distance from the closed form of the Q-steps
    std::vector<float> iq(2 * len + 2 * 11), en(static_cast<size_t>(m.total) * m.tones);
    modulate_host(protocol, 12000.0f, 1531.25f, 0.0f, 1.0f, tones, iq.data());
    demodulate_host(protocol, 12000.0f, 1531.25f, iq.data(), back, en.data());
    CHECK(std::memcmp(back, tones, m.data) == 0);
    const Signal one = {0u, 0u, 0, 1531.25f, 1.0f};
    SynthPlan plan = synth_plan(protocol, 12000.0f, &one, tones, 1, 1);
    CHECK(plan.rec.size() == 1 && plan.row.size() == 2 && plan.row[1] == 1);
    std::vector<float> cf(2 * len);
    synth_closed_form(protocol, plan, 1, len, false, cf.data());
    double worst = 0.0;
    for (size_t i = 0; i < 2 * len; ++i) worst = std::fmax(worst, std::fabs(static_cast<double>(cf[i]) - iq[i]));
    std::printf("protocol %d: max |closed form - recurrence| per component %.3e\n", protocol, worst);
    CHECK(worst < 1e-3);

    // the RF stage and a gain; a NaN sample leaves its symbol at tone 0 (a Costas or data tone)
    modulate_host(protocol, 12000.0f, 1000.0f, 1500.0f, 0.25f, tones, iq.data());
    demodulate_host(protocol, 12000.0f, 2500.0f, iq.data(), back, nullptr);
    CHECK(std::memcmp(back, tones, m.data) == 0);
    iq[2 * (40 * static_cast<size_t>(m.sps) + 3)] = std::numeric_limits<float>::quiet_NaN();
    demodulate_host(protocol, 12000.0f, 2500.0f, iq.data(), back, en.data());
    for (int k = 0; k < m.tones; ++k) CHECK(std::isnan(en[40 * m.tones + k]));

    // a slot of 3 symbols + 37 samples, 2 channels: one signal starts before sample 0, one
    // runs past the end, one lies wholly past the end; extreme offsets do not overflow
    const size_t n = 3 * static_cast<size_t>(m.sps) + 37;
    const Signal sig[5] = {{0u, 0u, -static_cast<int64_t>(m.sps + 5), 1000.0f, 1.0f},
                           {1u, 0u, static_cast<int64_t>(n) + 10, 1200.0f, 1.0f},
                           {0u, 0u, static_cast<int64_t>(m.sps), 1100.0f, 0.5f},
                           {1u, 0u, std::numeric_limits<int64_t>::max(), 900.0f, 1.0f},
                           {1u, 0u, std::numeric_limits<int64_t>::min(), 900.0f, 1.0f}};
    std::vector<uint8_t> st(5 * static_cast<size_t>(m.data));
    for (auto& t : st) t = static_cast<uint8_t>(next_u32() % m.tones);
    plan = synth_plan(protocol, 12000.0f, sig, st.data(), 5, 2);
    CHECK(plan.row[0] == 0 && plan.row[1] == 2 && plan.row[2] == 5);
    CHECK(plan.rec[0].offset == sig[0].offset && plan.rec[1].offset == sig[2].offset && plan.rec[2].offset == sig[1].offset);
    std::vector<float> slot(2 * 2 * n, 7.0f);
    synth_closed_form(protocol, plan, 2, n, false, slot.data());
    for (size_t i = 0; i < 2 * n; ++i) CHECK(slot[2 * n + i] == 0.0f);  // channel 1: nothing inside
    const double a0 = std::hypot(slot[0], slot[1]), a1 = std::hypot(slot[2 * (n - 1)], slot[2 * (n - 1) + 1]);
    CHECK(std::fabs(a0 - 1.0) < 1e-6 && a1 <= 1.5 + 1e-6 && a1 >= 0.5 - 1e-6);
    synth_closed_form(protocol, plan, 2, n, true, slot.data());
    CHECK(std::fabs(std::hypot(slot[0], slot[1]) - 2.0) < 1e-6);

    // errors
    st[7] = static_cast<uint8_t>(m.tones);
    CHECK(throws([&] { synth_plan(protocol, 12000.0f, sig, st.data(), 5, 2); }));
    CHECK(throws([&] { symbol_sequence(protocol, st.data(), syms); }));
    st[7] = 0;
    CHECK(throws([&] { synth_plan(protocol, 12000.0f, sig, st.data(), 5, 1); }));
  }
  CHECK(throws([] { proto(2); }));
  if (g_fail)
    std::printf("ftmod_host: %d checks failed\n", g_fail);
  else
    std::printf("ftmod_host: ok\n");
  return g_fail ? 1 : 0;
}
