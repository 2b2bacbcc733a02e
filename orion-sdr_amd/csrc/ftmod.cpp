// ftmod.cpp — host side of the FT8 / FT4 modulators and demodulators (ftmod.hpp). Built
// with -ffp-contract=off: every FMA of the reference is an explicit std::fma here.
#include "ftmod.hpp"

#include <array>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <unordered_map>

namespace orion {
namespace ftmod {

namespace {
constexpr float kTau = 6.28318530717958647692f;
// modulate/ft8.rs:9-20; modulate/ft4.rs:9-24
const Proto kProto[2] = {{1920, 79, 58, 8, 6.25f}, {576, 105, 87, 4, 20.833334f}};
const uint8_t kFt8Costas[7] = {3, 1, 4, 0, 6, 5, 2};
const int kFt8Pos[3] = {0, 36, 72};
const uint8_t kFt4Costas[4][4] = {{0, 1, 3, 2}, {1, 0, 2, 3}, {2, 3, 1, 0}, {3, 2, 0, 1}};
const int kFt4Pos[4] = {1, 34, 67, 100};

// One step of the phasor recurrence (ft8.rs:110-112, rotator.rs:46-48).
inline void step(float& zr, float& zi, float wr, float wi) {
  const float r = std::fma(zr, wr, -(zi * wi));
  const float i = std::fma(zi, wr, zr * wi);
  zr = r;
  zi = i;
}
inline void renorm(float& zr, float& zi) {  // ft8.rs:133-136, rotator.rs:54-58
  const float r2 = zr * zr + zi * zi;
  const float inv = 1.0f / std::sqrt(r2);
  zr *= inv;
  zi *= inv;
}
}  // namespace

const Proto& proto(int protocol) {
  if (protocol != kFt8 && protocol != kFt4)
    throw std::invalid_argument("unknown protocol (ORION_COSTAS_FT8 / ORION_COSTAS_FT4)");
  return kProto[protocol];
}

bool is_data(int protocol, int s) {
  if (protocol == kFt8) return !((s >= 0 && s < 7) || (s >= 36 && s < 43) || (s >= 72 && s < 79));
  if (s == 0 || s == 104) return false;
  for (int p : kFt4Pos)
    if (s >= p && s < p + 4) return false;
  return true;
}

void symbol_sequence(int protocol, const uint8_t* tones, uint8_t* syms) {
  const Proto& m = proto(protocol);
  for (int k = 0; k < m.data; ++k)
    if (tones[k] >= m.tones) throw std::invalid_argument("a data tone is out of range (FT8: < 8, FT4: < 4)");
  for (int s = 0; s < m.total; ++s) syms[s] = 0;
  if (protocol == kFt8) {
    for (int p : kFt8Pos)
      for (int c = 0; c < 7; ++c) syms[p + c] = kFt8Costas[c];
  } else {
    for (int b = 0; b < 4; ++b)
      for (int c = 0; c < 4; ++c) syms[kFt4Pos[b] + c] = kFt4Costas[b][c];
  }
  int k = 0;
  for (int s = 0; s < m.total; ++s)
    if (is_data(protocol, s)) syms[s] = tones[k++];
}

void tone_steps(int protocol, float fs, float base_hz, float* w, uint64_t* step_q64) {
  const Proto& m = proto(protocol);
  constexpr long double kTwoPi = 6.283185307179586476925286766559005768L;
  constexpr long double kTwo64 = 18446744073709551616.0L;
  for (int k = 0; k < m.tones; ++k) {
    const float f = base_hz + static_cast<float>(k) * m.spacing;
    const float phi = kTau * f / fs;
    const float wr = std::cos(phi), wi = std::sin(phi);
    w[2 * k] = wr;
    w[2 * k + 1] = wi;
    long double rev = atan2l(static_cast<long double>(wi), static_cast<long double>(wr)) / kTwoPi;
    if (!(rev == rev)) rev = 0.0L;  // a non-finite fs or base_hz: the reference gives NaN samples
    if (rev < 0) rev += 1.0L;
    long double scaled = roundl(rev * kTwo64);
    if (scaled >= kTwo64) scaled -= kTwo64;
    step_q64[k] = static_cast<uint64_t>(scaled);
  }
}

void enter_phases(int protocol, const uint8_t* syms, const uint64_t* step_q64, uint64_t* enter) {
  const Proto& m = proto(protocol);
  uint64_t ph = 0;
  for (int s = 0; s < m.total; ++s) {
    enter[s] = ph;
    ph += static_cast<uint64_t>(m.sps) * step_q64[syms[s]];
  }
}

void rotator_table(float freq_hz, float fs, size_t n, float* out) {
  const float phi = kTau * freq_hz / fs;
  const float wr = std::cos(phi), wi = std::sin(phi);
  float zr = 1.0f, zi = 0.0f;
  uint32_t ctr = 0;
  for (size_t i = 0; i < n; ++i) {
    step(zr, zi, wr, wi);
    if ((++ctr & 0x3FFu) == 0) renorm(zr, zi);
    out[2 * i] = zr;
    out[2 * i + 1] = zi;
  }
}

void modulate_host(int protocol, float fs, float base_hz, float rf_hz, float gain, const uint8_t* tones, float* iq) {
  const Proto& m = proto(protocol);
  uint8_t syms[kMaxSyms];
  symbol_sequence(protocol, tones, syms);
  float zr = 1.0f, zi = 0.0f;
  uint32_t ctr = 0;
  const int nn = m.sps & ~3;
  for (int s = 0; s < m.total; ++s) {
    const float f = base_hz + static_cast<float>(syms[s]) * m.spacing;
    const float phi = kTau * f / fs;
    const float wi = std::sin(phi), wr = std::cos(phi);
    float* o = iq + 2 * static_cast<size_t>(s) * m.sps;
    int i = 0;
    while (i < nn) {
      for (int u = 0; u < 4; ++u) {
        step(zr, zi, wr, wi);
        o[2 * (i + u)] = gain * zr;
        o[2 * (i + u) + 1] = gain * zi;
      }
      i += 4;
      ctr += 4;
      if ((ctr & 0x3FFu) < 4) renorm(zr, zi);
    }
    for (; i < m.sps; ++i) {
      step(zr, zi, wr, wi);
      o[2 * i] = gain * zr;
      o[2 * i + 1] = gain * zi;
      ctr += 1;
    }
  }
  if (rf_hz != 0.0f) {  // ft8.rs:150-153: a fresh Rotator over the whole frame
    const size_t n = static_cast<size_t>(m.frame_len());
    std::vector<float> p(2 * n);
    rotator_table(rf_hz, fs, n, p.data());
    for (size_t i = 0; i < n; ++i) {
      const float a = iq[2 * i], b = iq[2 * i + 1];
      iq[2 * i] = std::fma(a, p[2 * i], -(b * p[2 * i + 1]));
      iq[2 * i + 1] = std::fma(b, p[2 * i], a * p[2 * i + 1]);
    }
  }
}

void demod_steps(int protocol, float fs, float base_hz, float* w) {
  const Proto& m = proto(protocol);
  for (int k = 0; k < m.tones; ++k) {  // demodulate/ft8.rs:39-44
    const float f = base_hz + static_cast<float>(k) * m.spacing;
    const float phi = -kTau * f / fs;
    w[2 * k] = std::cos(phi);
    w[2 * k + 1] = std::sin(phi);
  }
}

void demodulate_host(int protocol, float fs, float base_hz, const float* iq, uint8_t* tones, float* energies) {
  const Proto& m = proto(protocol);
  float w[2 * kMaxTones];
  demod_steps(protocol, fs, base_hz, w);
  int d = 0;
  for (int s = 0; s < m.total; ++s) {
    const float* x = iq + 2 * static_cast<size_t>(s) * m.sps;
    float best_e = -1.0f;  // detect_tone, demodulate/ft8.rs:74-126
    uint8_t best_k = 0;
    for (int k = 0; k < m.tones; ++k) {
      const float wr = w[2 * k], wi = w[2 * k + 1];
      float ar = 0.0f, ai = 0.0f, pr = 1.0f, pi = 0.0f;
      for (int i = 0; i < m.sps; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        ar += a * pr - b * pi;  // num-complex Mul (no FMA), AddAssign
        ai += a * pi + b * pr;
        step(pr, pi, wr, wi);
      }
      const float e = ar * ar + ai * ai;  // norm_sqr
      if (energies) energies[s * m.tones + k] = e;
      if (e > best_e) {
        best_e = e;
        best_k = static_cast<uint8_t>(k);
      }
    }
    if (is_data(protocol, s)) tones[d++] = best_k;
  }
}

void check_signals(int protocol, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch) {
  const Proto& m = proto(protocol);
  if (nsig > 0x7fffffffull || nch > 0x7fffffffull) throw std::invalid_argument("synth: nsig, nch <= 2^31 - 1");
  for (size_t j = 0; j < nsig; ++j)
    if (signals[j].channel >= nch) throw std::invalid_argument("synth: a signal's channel is >= nch");
  for (size_t k = 0; k < nsig * m.data; ++k)
    if (tones[k] >= m.tones) throw std::invalid_argument("a data tone is out of range (FT8: < 8, FT4: < 4)");
}

void synth_plan_into(int protocol, float fs, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                     SynthRecord* rec, uint32_t* row) {
  const Proto& m = proto(protocol);
  check_signals(protocol, signals, tones, nsig, nch);
  for (size_t c = 0; c <= nch; ++c) row[c] = 0;
  for (size_t j = 0; j < nsig; ++j) row[signals[j].channel + 1] += 1;
  for (size_t c = 0; c < nch; ++c) row[c + 1] += row[c];
  std::vector<uint32_t> next(row, row + nch);
  // the tone steps depend on base_hz alone: signals sharing one (a batch of frames from one
  // modulator, a band plan on a grid) share its eight arctangents
  std::unordered_map<uint32_t, std::array<uint64_t, kMaxTones>> steps;
  for (size_t j = 0; j < nsig; ++j) {
    uint8_t syms[kMaxSyms];
    symbol_sequence(protocol, tones + j * m.data, syms);
    uint32_t key;
    std::memcpy(&key, &signals[j].base_hz, sizeof key);
    auto it = steps.find(key);
    if (it == steps.end()) {
      float w[2 * kMaxTones];
      std::array<uint64_t, kMaxTones> q{};
      tone_steps(protocol, fs, signals[j].base_hz, w, q.data());
      it = steps.emplace(key, q).first;
    }
    const uint64_t* q = it->second.data();
    SynthRecord& r = rec[next[signals[j].channel]++];
    r.offset = signals[j].offset;
    r.gain = signals[j].gain;
    r.pad = 0;
    enter_phases(protocol, syms, q, r.enter);
    for (int s = 0; s < m.total; ++s) r.step[s] = q[syms[s]];
    for (int s = m.total; s < kMaxSyms; ++s) r.enter[s] = r.step[s] = 0;
  }
}

SynthPlan synth_plan(int protocol, float fs, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch) {
  check_signals(protocol, signals, tones, nsig, nch);
  SynthPlan p;
  p.rec.resize(nsig);
  p.row.resize(nch + 1);
  synth_plan_into(protocol, fs, signals, tones, nsig, nch, p.rec.data(), p.row.data());
  return p;
}

void synth_closed_form(int protocol, const SynthPlan& plan, size_t nch, size_t n, bool accumulate, float* iq) {
  const Proto& m = proto(protocol);
  constexpr double kTurn = 6.283185307179586476925286766559 / 18446744073709551616.0;
  const int64_t len = m.frame_len();
  for (size_t ch = 0; ch < nch; ++ch) {
    float* o = iq + 2 * ch * n;
    if (!accumulate)
      for (size_t i = 0; i < 2 * n; ++i) o[i] = 0.0f;
    for (uint32_t j = plan.row[ch]; j < plan.row[ch + 1]; ++j) {
      const SynthRecord& r = plan.rec[j];
      // the part of the frame inside [0, n)
      const int64_t lo = r.offset > 0 ? r.offset : 0;
      const int64_t end = r.offset > static_cast<int64_t>(n) - len ? static_cast<int64_t>(n) : r.offset + len;
      for (int64_t i = lo; i < end; ++i) {
        const int64_t t = i - r.offset;
        const int s = static_cast<int>(t / m.sps), k = static_cast<int>(t % m.sps);
        const uint64_t ph = r.enter[s] + static_cast<uint64_t>(k + 1) * r.step[s];
        const double a = static_cast<double>(ph) * kTurn;
        o[2 * i] += r.gain * static_cast<float>(std::cos(a));
        o[2 * i + 1] += r.gain * static_cast<float>(std::sin(a));
      }
    }
  }
}

}  // namespace ftmod
}  // namespace orion
