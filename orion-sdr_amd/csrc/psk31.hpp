// psk31.hpp — PSK31 channel code and modems, host side (no HIP: psk31.cpp builds with the
// host compiler alone, tests/psk31_host).
//
// Reference: codec/varicode.rs (the Varicode table, VaricodeEncoder, VaricodeDecoder),
// codec/psk31.rs (conv_encode, viterbi_decode, viterbi_decode_hard, StreamingViterbi),
// modulate/psk31.rs (psk31_sps, make_hann, Bpsk31Mod, Qpsk31Mod and the stateful coder of
// :368-385), demodulate/psk31.rs (Bpsk31Demod, Qpsk31Demod, Bpsk31Decider) and the search of
// sync/psk31_sync.rs over a waterfall given to it. Everything
// here is the reference's operation order in f32 (-ffp-contract=off: every * and + is its
// own rounding; fused multiply-adds only where the reference writes mul_add, in the
// Rotator). k_psk31.hip's k_psk31_viterbi is held to viterbi_decode bit for bit, and its
// k_psk31_demod to Demod::process up to the sine and cosine of the phase correction.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <vector>

#include "trellis.hpp"

namespace orion {
namespace psk31 {

// ---- Varicode (codec/varicode.rs) ------------------------------------------------------
constexpr int kVaricodeMaxBits = 10;  // varicode.rs:20
struct Codeword {
  uint16_t bits;  // MSB first: bit len - 1 is transmitted first
  uint8_t len;
};
// The 128-entry table (varicode.rs:27-156; G3PLX, "PSK31: A New Radio-Teletype Mode").
const Codeword* varicode_table();
// varicode_encode, varicode.rs:163-169: a byte >= 128 gives the NUL entry.
Codeword varicode_encode(uint8_t byte);
// varicode_decode, varicode.rs:176-183: the byte, or -1 for a codeword not in the table.
int varicode_decode(uint16_t bits, uint8_t len);

// VaricodeEncoder, varicode.rs:192-267. push_preamble sets first = true again, so the byte
// after a preamble gets no "00" gap of its own (varicode.rs:216-223).
class VaricodeEncoder {
 public:
  void push_preamble(size_t n_bits);
  void push_byte(uint8_t b);
  void push_postamble(size_t n_bits);
  int next_bit();  // -1 when the queue is empty
  bool is_empty() const { return pending_.empty(); }
  size_t pending() const { return pending_.size(); }
  std::vector<uint8_t> drain_bits();

 private:
  std::deque<uint8_t> pending_;
  bool first_ = true;
};

// VaricodeDecoder, varicode.rs:277-320. len stops at kVaricodeMaxBits + 1 while shift keeps
// shifting (varicode.rs:308-311).
class VaricodeDecoder {
 public:
  void push_bit(uint8_t bit);
  int pop_char();  // -1 when the queue is empty
  size_t pending() const { return chars_.size(); }

 private:
  uint16_t shift_ = 0;
  uint8_t len_ = 0;
  bool prev_zero_ = false;
  std::deque<uint8_t> chars_;
};

// ---- rate 1/2, K = 5 convolutional code (codec/psk31.rs) -------------------------------
constexpr int kStates = 16;          // psk31.rs:59
constexpr int kTracebackDepth = 32;  // psk31.rs:267
constexpr int kPathMem = 128;        // psk31.rs:269
// DQPSK_EXP, psk31.rs:80-85: the expected phasor of dibit c0 * 2 + c1.
extern const float kDqpskExp[4][2];

// conv_encode, psk31.rs:45-55: bits [n] -> out [2 n], (g0, g1) per bit from a zero register.
void conv_encode(const uint8_t* bits, size_t n, uint8_t* out);
// The coder that keeps its register between calls, modulate/psk31.rs:368-385.
class ConvEncoder {
 public:
  void encode(uint8_t bit, uint8_t* c0, uint8_t* c1);
  void reset() { sr_ = 0; }

 private:
  uint8_t sr_ = 0;
};

// viterbi_decode, psk31.rs:95-160: soft [2 n_syms] (re, im per symbol) -> bits [n_syms].
// Start metric f32::MAX / 2 with state 0 at 0; a predecessor at or above it is skipped;
// predecessors in ascending order, replaced on strict < only; the first minimum wins the
// final-state search; an entry of the survivor table that no predecessor wrote reads 0.
void viterbi_decode(const float* soft, size_t n_syms, uint8_t* bits);
// viterbi_decode_hard, psk31.rs:384-396: coded [2 n_syms] bits -> DQPSK_EXP phasors -> decode.
void viterbi_decode_hard(const uint8_t* coded, size_t n_syms, uint8_t* bits);

// StreamingViterbi, psk31.rs:257-377: a fixed lag of kTracebackDepth symbols over a ring
// of kPathMem survivor rows; metrics lose their minimum after every 256th symbol.
class StreamingViterbi {
 public:
  StreamingViterbi();
  int feed_symbol(float s_re, float s_im);  // the decoded bit, or -1 while the lag fills
  std::vector<uint8_t> flush();             // feeds kTracebackDepth (0, 0) symbols

 private:
  float pm_[kStates];
  uint8_t history_[kPathMem][kStates];
  size_t ptr_ = 0, count_ = 0;
};

// ---- modulators and demodulators (modulate/psk31.rs, demodulate/psk31.rs) ---------------
enum : int { kBpsk = 0, kQpsk = 1 };  // include/orion_sdr_amd.h ORION_PSK31_BPSK / _QPSK
// psk31_sps, modulate/psk31.rs:42-44: round(fs / 31.25) (half away from zero; a NaN or
// negative quotient gives 0, as Rust's saturating cast does).
size_t psk31_sps(float fs);
// make_hann, modulate/psk31.rs:53-67 = demodulate/psk31.rs:39-50: 0.5 - 0.5 cosf(pi i / (sps - 1)).
std::vector<float> make_hann(size_t sps);
// The bits modulate_text sends (modulate/psk31.rs:146-159): preamble, the bytes, postamble.
std::vector<uint8_t> text_bits(const uint8_t* text, size_t n, size_t preamble_bits, size_t postamble_bits);

// Bpsk31Mod (modulate/psk31.rs:110-216) and Qpsk31Mod (:248-362). The phasor is carried as
// the f32 pair the reference's own arithmetic gives (QPSK31's products hold -0.0). With
// rf_hz != 0 every modulate_bits call runs a fresh Rotator over its output (:186-189).
// A sample rate whose psk31_sps is 0 throws std::invalid_argument.
class Mod {
 public:
  Mod(int mode, float fs, float rf_hz, float gain);
  size_t sps() const { return sps_; }
  void set_gain(float g) { gain_ = g; }
  void reset();
  // bits [n] -> iq [n * sps][2]
  void modulate_bits(const uint8_t* bits, size_t n, float* iq);
  // What the device modulator reads (k_psk31.hip k_psk31_mod): ph [n + 1][2], ph[0] the
  // phasor before the first symbol, ph[k + 1] the phasor of symbol k, each the f32 pair the
  // reference's arithmetic gives. Advances the phasor (and the coder) as modulate_bits does.
  void symbol_phasors(const uint8_t* bits, size_t n, float* ph);
  int mode() const { return mode_; }
  float fs() const { return fs_; }
  float rf_hz() const { return rf_hz_; }
  float gain() const { return gain_; }
  const std::vector<float>& hann() const { return hann_; }
  // Block::process (:199-215): n = min(n_bits, out_cap / sps) bits -> n * sps samples.
  void process(const uint8_t* bits, size_t n_bits, float* iq, size_t out_cap, size_t* in_read, size_t* out_written);

 private:
  int mode_;
  float fs_, rf_hz_, gain_;
  size_t sps_;
  float cur_re_ = 1.0f, cur_im_ = 0.0f;
  std::vector<float> hann_;
  ConvEncoder enc_;
};

// What a demodulator carries from call to call (the device bank keeps one per stream).
struct DemodState {
  uint32_t count, renorm_ctr;
  float acc_re, acc_im, prev_re, prev_im, phase_acc, z_re, z_im;
};
// Bpsk31Demod (demodulate/psk31.rs:83-220, new_with_offset :104-130) and Qpsk31Demod
// (:271-397): the reference's loop sample by sample, glibc sinf / cosf at each symbol.
// BPSK writes one soft value per symbol and stops when out_pos == out_cap; QPSK writes
// (re, im) and stops when out_pos + 1 >= out_cap.
class Demod {
 public:
  Demod(int mode, float fs, float rf_hz, float gain, size_t offset);
  size_t sps() const { return sps_; }
  void set_gain(float g) { gain_ = g; }
  void reset();
  void process(const float* iq, size_t n, float* out, size_t out_cap, size_t* in_read, size_t* out_written);
  const DemodState& state() const { return st_; }
  float hann_sq_sum() const { return hann_sq_sum_; }
  const std::vector<float>& hann() const { return hann_; }

 private:
  int mode_;
  float gain_, w_re_, w_im_, hann_sq_sum_;
  bool rot_;
  size_t sps_;
  std::vector<float> hann_;
  DemodState st_;
};
// One stream of the device bank as the caller states it (include/orion_sdr_amd.h
// orion_psk31_stream) and as the kernel reads it (k_psk31.hip k_psk31_demod).
struct Stream {
  uint32_t mode, channel;
  float rf_hz, gain;
  uint64_t start;    // the channel sample at which the stream's first sample lies
  uint32_t offset;   // as in new_with_offset
  uint32_t out_cap;  // soft values per call (the reference's output.len())
};
struct BankRecord {
  uint64_t start;
  uint32_t mode, channel, slot, out_cap, rot;
  float w_re, w_im, scale;  // the Rotator's step; gain / hann_sq_sum
};
// new_with_offset's starting count, demodulate/psk31.rs:111-115.
inline uint32_t demod_start_count(size_t sps, size_t offset) {
  return offset % sps == 0 ? 0u : static_cast<uint32_t>(sps - offset % sps);
}
// Rotator::new's step phasor (dsp/rotator.rs:16-24): (cosf, sinf) of f32(TAU * freq_hz / fs).
void rotator_step(float freq_hz, float fs, float* w_re, float* w_im);
// Rotator(freq_hz, fs)::next n times from a fresh oscillator (dsp/rotator.rs:16-61): out [n][2].
void rotator_table(float freq_hz, float fs, size_t n, float* out);
// Bpsk31Decider, demodulate/psk31.rs:236-261: bit = soft >= 0.
void bpsk31_decide(const float* soft, size_t n, uint8_t* bits);

// ---- band synthesis (no reference counterpart; k_psk31.hip k_psk31_synth) ----------------
struct Signal {  // include/orion_sdr_amd.h orion_psk31_signal
  uint32_t channel, mode;
  int64_t offset;  // the channel sample at which the signal starts (may be negative)
  float rf_hz, gain;
  uint64_t n_bits;  // its bits follow the previous signal's in the bits array
};
struct SynthRecord {  // what the kernel reads, sorted by channel, list order kept within one
  int64_t offset, len;  // len = n_bits * sps samples
  uint64_t ph0;         // its n_bits + 1 symbol phasors start here in the phasor array
  uint64_t step_q64;    // the Rotator's f32 step phasor's angle as a Q0.64 turn count
  float gain;
  uint32_t rot;
};
// The angle of Rotator(freq_hz, fs)'s f32 step phasor (cosf, sinf of f32(TAU f / fs)) as a
// Q0.64 fraction of a turn, rounded, in long double (as ftmod.hpp tone_steps).
uint64_t rotator_step_q64(float freq_hz, float fs);

// ---- carrier search (sync/psk31_sync.rs) -------------------------------------------------
// One detected carrier run: include/orion_sdr_amd.h orion_candidate.
struct Carrier {
  int32_t time_sym;   // the run's first symbol
  uint32_t freq_bin;  // carrier_hz = base_hz + f32(freq_bin) * 31.25
  float score;        // run_energy_sum / run_len, the sum in symbol order
};
// median_f32, psk31_sync.rs:242-253: the middle value, or the f32 mean of the two middle
// ones ((a + b) * 0.5); 0 for an empty slice. v is sorted in place.
float median_f32(float* v, size_t n);
// The number of bins psk31_sync searches, psk31_sync.rs:70-71: ceil(max(max_hz - base_hz,
// 0) / 31.25) + 1 (a NaN range gives 1).
size_t sync_num_bins(float base_hz, float max_hz);
// The search of psk31_sync (psk31_sync.rs:82-203) over a log waterfall wf [num_syms][num_bins]
// given to it: per-bin medians over time and their median over the bins; ln_margin =
// peak_margin_db * LN_2 / 3; a symbol is a peak when (e > bin_median + ln_margin ||
// bin_median > noise_floor + ln_margin) && e >= e_left && e >= e_right (missing neighbours
// are -inf); runs of at least max(min_carrier_syms, 1) peaks are kept, a run that reaches the
// end of the buffer included. Returns the max_cand best runs, score descending.
// The reference sorts with sort_unstable_by on the score alone, so the order of runs of equal
// score is open there; here it is defined: equal scores are ordered by freq_bin, then
// time_sym, both ascending, which is one of the orders the reference may produce.
std::vector<Carrier> find_carriers(const float* wf, size_t num_syms, size_t num_bins, size_t min_carrier_syms,
                                   float peak_margin_db, size_t max_cand);

// ---- the batched decode's scratch (k_psk31.hip): the survivor words of K = 5, trellis.hpp ----
inline size_t viterbi_work_bytes(size_t nstreams, size_t n_syms) { return trellis::work_bytes(4, nstreams, n_syms); }

}  // namespace psk31
}  // namespace orion
