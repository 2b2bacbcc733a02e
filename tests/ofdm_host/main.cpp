// A stand-alone program over csrc/ofdm.cpp for the sanitizers (tests/test_ofdm_oracle.py builds
// it with the host compiler and -fsanitize=address,undefined): a round trip per constellation
// with and without pilots, window and RF stage, both equalizer methods, plan edge cases and
// the rejected sizes. No Python, no device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "ofdm.hpp"

using namespace orion::ofdm;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("ofdm_host: FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static Config make(size_t n_fft, size_t cp, int order, bool pilots, float rf, size_t roll, size_t backoff) {
  Config c;
  c.plan.n_fft = n_fft;
  c.plan.cp_len = cp;
  if (pilots) {
    c.plan.pilot_idx = {-21, -7, 7, 21};
    c.plan.pilot_val = {1, 0, -1, 0, 0, 1, 1, 0};
  }
  plan_contiguous_data(c.plan, 4, false);
  c.plan.roll_off = roll;
  c.fs = 1e6f;
  c.rf_hz = rf;
  c.gain = 0.5f;
  c.constellation = order;
  c.rx_window_backoff = backoff;
  return c;
}

int main() {
  uint32_t lcg = 12345;
  auto bit = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return static_cast<uint8_t>((lcg >> 16) & 0xff); };

  for (int order = kBpsk; order <= kQam256; ++order) {
    for (int variant = 0; variant < 3; ++variant) {
      const size_t n_fft = variant == 2 ? 256 : 64, cp = variant == 1 ? 5 : 16;
      const Config c = make(n_fft, cp, order, variant != 2, 0.0f, variant == 1 ? 2 : 0, 0);
      Mod mod(c);
      Demod dem(c);
      dem.set_gain(2.0f);
      const size_t bps = c.bits_per_ofdm_symbol(), len = c.samples_per_ofdm_symbol(), nd = c.plan.data.size();
      std::vector<uint8_t> bits(3 * bps - 5);
      for (auto& b : bits) b = bit();
      const std::vector<float> iq = mod.modulate(bits.data(), bits.size());
      CHECK(iq.size() == 2 * 3 * len);
      std::vector<float> soft(2 * 3 * nd);
      size_t r = 0, w = 0;
      dem.process(iq.data(), iq.size() / 2, soft.data(), soft.size() / 2, nullptr, &r, &w);
      CHECK(r == 3 * len && w == 3 * nd);
      std::vector<uint8_t> got(3 * bps);
      std::vector<float> llr(3 * bps);
      decide(order, soft.data(), 3 * nd, got.data());
      soft_llr(order, soft.data(), 3 * nd, llr.data());
      // the window of variant 1 tapers samples inside the receiver's window (back-off 0, no
      // equalizer to undo a matched one): about -20 dB of distortion, which BPSK and QPSK bear
      const bool clean = variant != 1 || order <= kQpsk;
      for (size_t i = 0; i < bits.size() && clean; ++i) CHECK(got[i] == (bits[i] & 1));
      for (size_t i = bits.size(); i < got.size() && clean; ++i) CHECK(got[i] == 0);  // the zero padding
      for (size_t i = 0; i < got.size(); ++i) CHECK(llr[i] == 0 || (llr[i] < 0) == (got[i] == 1));
      float evm = 0;
      CHECK(evm_db(order, soft.data(), 3 * nd, got.data(), got.size(), 3, &evm) && evm < (variant == 1 ? -15.0f : -80.0f));
      CHECK(!evm_db(order, soft.data(), 3 * nd, got.data(), got.size() - bps, 3, &evm));
      // short input and output: a zero report
      dem.process(iq.data(), len - 1, soft.data(), soft.size() / 2, nullptr, &r, &w);
      CHECK(r == 0 && w == 0);
      mod.process(bits.data(), bps, soft.data(), len - 1, &r, &w);
      CHECK(r == 0 && w == 0);

      // both equalizers over the same symbols, the identity channel
      for (int method : {kEqTrainingSymbolHold, kEqPerSymbolPilotInterp}) {
        Equalizer eq(c, method);
        std::vector<float> tr(2 * n_fft);
        training_pattern(n_fft, tr.data());
        eq.estimate_from_training_symbol(tr.data(), n_fft);
        eq.estimate_from_training_symbol(tr.data(), n_fft - 1);  // too short: ignored
        // the pilots see the modulator's gain of 0.5, so their estimate already undoes it
        dem.set_gain(method == kEqPerSymbolPilotInterp && variant != 2 ? 1.0f : 2.0f);
        dem.process(iq.data(), iq.size() / 2, soft.data(), soft.size() / 2, &eq, &r, &w);
        CHECK(w == 3 * nd);
        decide(order, soft.data(), 3 * nd, got.data());
        for (size_t i = 0; i < bits.size() && clean; ++i) CHECK(got[i] == (bits[i] & 1));
      }
    }
  }

  {  // the RF stage and the window: finite, the right length, the phase carried
    const Config c = make(64, 16, kQam16, true, 125e3f, 3, 8);
    Mod mod(c);
    std::vector<uint8_t> bits(2 * c.bits_per_ofdm_symbol(), 1);
    const std::vector<float> a = mod.modulate(bits.data(), bits.size()), b = mod.modulate(bits.data(), bits.size());
    CHECK(a.size() == b.size() && a != b);
    for (float v : a) CHECK(std::isfinite(v));
    mod.reset();
    CHECK(mod.modulate(bits.data(), bits.size()) == a);
    Demod dem(c);
    CHECK(dem.window_start() == 8);
    CHECK(window_ramp(10, 99).size() == 5 && window_ramp(80, 0).empty());
    CHECK(max_pilot_safe_backoff(2048, 12) == 85 && max_pilot_safe_backoff(64, 0) == 32);
  }

  {  // plan edge cases
    Plan p;
    p.n_fft = 64;
    int32_t bad = 0;
    CHECK(plan_validate(p, &bad) == kPlanEmptyData);
    p.data = {1, 32};
    CHECK(plan_validate(p, &bad) == kPlanOutOfRange && bad == 32);
    p.data = {-32, 31};
    CHECK(plan_validate(p, nullptr) == kPlanOk);
    CHECK(plan_validate_edge_guard(p, 1, &bad) == kPlanInGuardBand && bad == -32);
    p.pilot_idx = {31};
    p.pilot_val = {1, 0};
    CHECK(plan_validate(p, &bad) == kPlanOverlap && bad == 31);
    CHECK(throws([&] { grid_from_plan(p); }));
    p.pilot_idx = {-1};
    const Grid g = grid_from_plan(p);
    CHECK(g.data_bins[0] == 32 && g.data_bins[1] == 31 && g.pilot_bins[0] == 63);
    CHECK(plan_occupied_half_carriers(p) == 32 && plan_occupied_bins(p).size() == 3);
    Plan q;
    q.n_fft = 8;
    plan_contiguous_data(q, 0, true);
    CHECK(q.data.size() == 7 && q.data.front() == -3 && q.data.back() == 3);
    Plan e;
    e.n_fft = 8;
    plan_contiguous_data(e, 100, false);  // a guard wider than the band: nothing
    CHECK(e.data.empty() && plan_occupied_bins(Plan{}).empty());
    const uint32_t pb[3] = {3, 9, 40};
    const float ratios[6] = {1, 0, 0, 1, -1, 0};
    float re, im;
    interpolate_at(pb, ratios, 3, 0, &re, &im);
    CHECK(re == 1 && im == 0);
    interpolate_at(pb, ratios, 3, 63, &re, &im);
    CHECK(re == -1 && im == 0);
    interpolate_at(pb, ratios, 3, 6, &re, &im);
    CHECK(re == 0.5f && im == 0.5f);
    interpolate_at(pb, ratios, 1, 50, &re, &im);
    CHECK(re == 1 && im == 0);
    equalizer_weight(1e-4f, 0, &re, &im);
    CHECK(re == 0 && im == 0);
  }

  // rejected sizes and configurations
  for (size_t n : {size_t{0}, size_t{6}, size_t{8192}, size_t{4}, size_t{100}}) {
    CHECK(!fft_size_ok(n));
    CHECK(throws([&] { Fft f(n, false); }));
    CHECK(throws([&] { Mod m(make(n, 0, kQpsk, false, 0, 0, 0)); }));
  }
  CHECK(throws([] { Mod m(make(64, 65, kQpsk, false, 0, 0, 0)); }));
  CHECK(throws([] { Demod d(make(64, 16, 7, false, 0, 0, 0)); }));
  CHECK(throws([] { Equalizer e(make(64, 16, kQpsk, true, 0, 0, 0), 5); }));
  CHECK(throws([] {
    float t[4] = {0}, o[4];
    cp_insert(t, 2, 3, o);
  }));
  {
    Fft f(8, false), fi(8, true);
    float x[16], y[16];
    for (int i = 0; i < 16; ++i) x[i] = static_cast<float>(i % 5) - 2.0f;
    size_t r, w;
    f.process(x, 7, y, 8, &r, &w);
    CHECK(r == 0 && w == 0);
    f.process(x, 8, y, 8, &r, &w);
    fi.process(y, 8, y, 8, &r, &w);
    for (int i = 0; i < 16; ++i) CHECK(std::fabs(x[i] - y[i]) < 1e-5f);
  }
  std::printf("ofdm_host: ok\n");
  return 0;
}
