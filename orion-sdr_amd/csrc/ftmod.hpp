// ftmod.hpp — FT8 / FT4 modulator and hard demodulator, host side (no HIP: ftmod.cpp
// builds with the host compiler alone, tests/ftmod_host).
//
// Reference: modulate/ft8.rs:48-156 (Ft8Mod), modulate/ft4.rs:51-173 (Ft4Mod),
// demodulate/ft8.rs:25-126 (Ft8Demod), demodulate/ft4.rs (Ft4Demod). The scalar
// modulator and demodulator here are the reference's f32 operation order; the kernels
// of k_ftmod.hip are held to them: the demodulator bit for bit, the modulator (whose
// phasor recurrence is one serial chain over the frame) through the closed form of the
// reference's own f32 steps, as Q0.64 turn counts.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orion {
namespace ftmod {

enum : int { kFt8 = 0, kFt4 = 1 };  // include/orion_sdr_amd.h ORION_COSTAS_*
constexpr int kMaxTones = 8, kMaxSyms = 105, kMaxData = 87;

struct Proto {
  int sps, total, data, tones;
  float spacing;
  int frame_len() const { return sps * total; }
};
// Throws std::invalid_argument for an unknown protocol.
const Proto& proto(int protocol);
// Frame symbol s carries data (not a Costas tone, not an FT4 ramp symbol).
bool is_data(int protocol, int s);

// build_symbol_sequence (ft8.rs:65-85, ft4.rs:73-103): tones [58 | 87] -> syms [79 | 105].
// A tone >= 8 | 4 throws std::invalid_argument.
void symbol_sequence(int protocol, const uint8_t* tones, uint8_t* syms);

// Per tone k < tones: the reference's step w = (cos phi, sin phi), phi = f32(TAU * f /
// fs), f = base_hz + f32(k) * spacing (ft8.rs:98-101), and its angle as a Q0.64 fraction
// of a turn: atan2l(w.im, w.re) / 2 pi * 2^64, rounded, in long double. w: [tones][2].
void tone_steps(int protocol, float fs, float base_hz, float* w, uint64_t* step_q64);
// The phase entering each symbol: enter[0] = 0, enter[s + 1] = enter[s] + sps *
// step[syms[s]] as wrapping uint64 sums (exact integers). enter: [total].
void enter_phases(int protocol, const uint8_t* syms, const uint64_t* step_q64, uint64_t* enter);

// Rotator(freq_hz, fs)::next n times from a fresh oscillator (rotator.rs:16-62): out [n][2].
void rotator_table(float freq_hz, float fs, size_t n, float* out);

// Ft8Mod / Ft4Mod::modulate in the reference's operation order: iq [frame_len][2].
void modulate_host(int protocol, float fs, float base_hz, float rf_hz, float gain, const uint8_t* tones, float* iq);

// Ft8Demod / Ft4Demod::demodulate of the first frame_len samples of iq: tones [58 | 87];
// energies (may be null) [total][tones], every correlator energy of detect_tone.
void demodulate_host(int protocol, float fs, float base_hz, const float* iq, uint8_t* tones, float* energies);
// The demodulator's step phasors (-phi), [tones][2].
void demod_steps(int protocol, float fs, float base_hz, float* w);

// ---- slot synthesis -----------------------------------------------------------------
struct Signal {  // include/orion_sdr_amd.h orion_ft_signal
  uint32_t channel, pad;
  int64_t offset;  // the channel sample at which the frame starts (may be negative)
  float base_hz, gain;
};
// What the synthesis kernel reads for one signal (k_ftmod.hip k_ft_synth).
struct SynthRecord {
  int64_t offset;
  float gain;
  uint32_t pad;
  uint64_t enter[kMaxSyms];  // phase entering symbol s
  uint64_t step[kMaxSyms];   // step of symbol s's tone
};
struct SynthPlan {
  std::vector<SynthRecord> rec;  // sorted by channel, list order kept within a channel
  std::vector<uint32_t> row;     // [nch + 1]: channel ch owns rec[row[ch] .. row[ch + 1])
};
// signals [nsig], tones [nsig][58 | 87]. Throws std::invalid_argument for a channel >=
// nch, a tone out of range, or nsig / nch above 2^31 - 1 (check_signals: those checks alone).
void check_signals(int protocol, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch);
SynthPlan synth_plan(int protocol, float fs, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch);
// The same plan written into caller memory: rec [nsig], row [nch + 1].
void synth_plan_into(int protocol, float fs, const Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                     SynthRecord* rec, uint32_t* row);
// The kernel's sum on the host, with the phasor in f64 rounded to f32 (what the device's
// phasor_at approximates): iq [nch][n][2], accumulate as the kernel.
void synth_closed_form(int protocol, const SynthPlan& plan, size_t nch, size_t n, bool accumulate, float* iq);

}  // namespace ftmod
}  // namespace orion
