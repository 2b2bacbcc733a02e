// ofdm.hpp — the OFDM symbol layer, host side (no HIP): carrier plans and grids, the
// constellation mappers, hard deciders and max-log LLRs, the radix-2 transform, cyclic
// prefix, symbol window, OfdmMod / OfdmDemod, the per-bin equalizer and the EVM figure.
// A restatement of the reference in scalar f32 (built with -ffp-contract=off; fmaf only
// where the reference writes mul_add); the kernels of k_ofdm.hip are held to it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orion {
namespace ofdm {

// ---- constellations (modulate/ofdm.rs:20-39) ------------------------------------------
enum : int { kBpsk = 0, kQpsk = 1, kQam16 = 2, kQam64 = 3, kQam256 = 4 };
// bits_per_symbol (modulate/ofdm.rs:30-38); 0 for an unknown order.
size_t bits_per_symbol(int order);
// axis_scale (modulate/qam.rs:27-31): 1 / sqrt(2 (M^2 - 1) / 3) in f64, cast to f32.
float axis_scale(size_t bits);
// build_axis_table (modulate/qam.rs:45-57): table[g ^ (g >> 1)] = f32(2 g + 1 - M) * scale; 16 entries.
void axis_table(size_t bits, float* table16);
// build_threshold_table (demodulate/qam.rs:28-41): f32(2 j - (M - 2)) * scale, j < M - 1; 15 entries.
void threshold_table(size_t bits, float* table15);
// The mappers (modulate/bpsk.rs, qpsk.rs:33-45, qam.rs:92-101): bits [n_syms * bps] u8 (LSB
// counts) -> syms [n_syms][2].
void map_bits(int order, const uint8_t* bits, size_t n_syms, float* syms);
// The hard deciders (demodulate/bpsk.rs:74, qpsk.rs:79-91, qam.rs:120-140).
void decide(int order, const float* syms, size_t n_syms, uint8_t* bits);
// Max-log LLRs, positive = 0 (demodulate/ofdm.rs:588-638): llr [n_syms * bps].
void soft_llr(int order, const float* syms, size_t n_syms, float* llr);

// ---- CarrierPlan (multicarrier/config.rs:50-279) --------------------------------------
enum : int { kPlanOk = 0, kPlanOutOfRange = 1, kPlanOverlap = 2, kPlanEmptyData = 3, kPlanInGuardBand = 4 };
struct Plan {
  size_t n_fft = 0, cp_len = 0;
  std::vector<int32_t> data;       // signed carrier indices, the caller's order
  std::vector<int32_t> pilot_idx;  // signed carrier indices
  std::vector<float> pilot_val;    // [n_pilots][2]
  size_t roll_off = 0;             // window_roll_off
};
// validate (config.rs:223-252); bad (may be null) receives the offending index.
int plan_validate(const Plan& p, int32_t* bad);
// validate_edge_guard (config.rs:262-278).
int plan_validate_edge_guard(const Plan& p, size_t edge_guard, int32_t* bad);
// with_contiguous_data (config.rs:128-149): appends to p.data.
void plan_contiguous_data(Plan& p, size_t edge_guard, bool include_dc);
// occupied_half_carriers (config.rs:167-174), occupied_bins (config.rs:188-203).
size_t plan_occupied_half_carriers(const Plan& p);
std::vector<size_t> plan_occupied_bins(const Plan& p);

// CarrierGrid::from_plan (grid.rs:40-66): bin = idx.rem_euclid(n_fft). Throws
// std::invalid_argument for a plan that does not validate (the reference panics).
struct Grid {
  size_t n_fft = 0;
  std::vector<uint32_t> data_bins;   // the plan's order
  std::vector<uint32_t> pilot_bins;  // the plan's order
  std::vector<float> pilot_val;      // [n_pilots][2]
};
Grid grid_from_plan(const Plan& p);

// ---- the transform (multicarrier/fft.rs) ----------------------------------------------
// Powers of two from 8 to 4096 (rustfft takes any length: a stated divergence).
bool fft_size_ok(size_t n);
// W_n^k = (f32 cos(2 pi k / n), f32 -sin(2 pi k / n)), k < n / 2, each computed in f64 and
// rounded once; the kernels read the same values.
std::vector<float> fft_twiddles(size_t n);
// Radix-2 decimation in time in place: the bit reversal, then stages of size 2, 4, .. n with
// t = b w as re = b.re w.re - b.im w.im, im = b.re w.im + b.im w.re (no FMA), a' = a + t,
// b' = a - t; every stage multiplies (W^0 included). inverse: conj(w), and the result times
// f32(1 / n) per component (fft.rs:77, :101-113). x [n][2] in place.
void fft_inplace(float* x, size_t n, const float* tw, bool inverse);

class Fft {  // FftBlock / IfftBlock (fft.rs:16-120)
 public:
  Fft(size_t n, bool inverse);  // throws std::invalid_argument unless fft_size_ok(n)
  size_t n() const { return n_; }
  bool inverse() const { return inv_; }
  const std::vector<float>& twiddles() const { return tw_; }
  // One symbol per call; a short input or output is a no-op (fft.rs:42-46).
  void process(const float* in, size_t n_in, float* out, size_t out_cap, size_t* in_read, size_t* out_written) const;

 private:
  size_t n_;
  bool inv_;
  std::vector<float> tw_;
};

// SymbolWindow::new's ramp (symbol_window.rs:47-59): 0.5 (1 - cosf(PI (i + 0.5) / L)), L =
// min(roll_off, symbol_len / 2).
std::vector<float> window_ramp(size_t symbol_len, size_t roll_off);
// SymbolWindow::process (symbol_window.rs:80-98) on one symbol in place.
void window_apply(float* sym, size_t symbol_len, const std::vector<float>& ramp);
// SymbolFft::max_pilot_safe_backoff (symbol_fft.rs:90-92).
size_t max_pilot_safe_backoff(size_t n_fft, size_t pilot_spacing);
// CyclicPrefixInsert / CyclicPrefixRemove (multicarrier/cyclic_prefix.rs) on one symbol.
void cp_insert(const float* time, size_t n_fft, size_t cp_len, float* out);
void cp_remove(const float* sym, size_t n_fft, size_t cp_len, float* out);

// ---- OfdmConfig (modulate/ofdm.rs:57-117, :139-166, :240-259, :359-365) ---------------
struct Config {
  Plan plan;
  float fs = 1.0f, rf_hz = 0.0f, gain = 1.0f;
  int constellation = kQpsk;
  size_t rx_window_backoff = 0;
  size_t bits_per_ofdm_symbol() const { return plan.data.size() * bits_per_symbol(constellation); }
  size_t samples_per_ofdm_symbol() const { return plan.n_fft + plan.cp_len; }
};
// Throws std::invalid_argument: the plan (validate), the transform size, cp_len > n_fft
// (the reference's CyclicPrefixInsert would panic), the constellation.
void config_check(const Config& c);

// Rotator (dsp/rotator.rs:16-61).
struct Rotator {
  float zr = 1.0f, zi = 0.0f, wr = 1.0f, wi = 0.0f;
  uint32_t ctr = 0;
  Rotator() = default;
  Rotator(float freq_hz, float fs);
  void next(float* re, float* im);
};

// OfdmMod (modulate/ofdm.rs:422-544). The symbol window (symbol_window.rs), when the plan
// has a roll-off, is applied per symbol before the gain, as the frame modulator does.
class Mod {
 public:
  explicit Mod(const Config& c);
  const Config& config() const { return cfg_; }
  const Grid& grid() const { return grid_; }
  const Fft& ifft() const { return ifft_; }
  const std::vector<float>& ramp() const { return ramp_; }
  void set_gain(float g) { cfg_.gain = g; }
  float gain() const { return cfg_.gain; }
  void reset() { rot_ = Rotator(cfg_.rf_hz, cfg_.fs); }
  // One symbol, at gain g, through the rotator when rf_hz != 0 (modulate/ofdm.rs:500-543).
  void symbol(const uint8_t* bits, float* out);
  // As many whole symbols as fit (the reference's process takes one; k calls of it equal this).
  void process(const uint8_t* bits, size_t n_bits, float* out, size_t out_cap, size_t* in_read, size_t* out_written);
  // modulate (modulate/ofdm.rs:469-493): every bit, the last symbol zero-padded.
  std::vector<float> modulate(const uint8_t* bits, size_t n_bits);

 private:
  Config cfg_;
  Grid grid_;
  Fft ifft_;
  std::vector<float> ramp_, syms_, freq_;
  Rotator rot_;
};

// ---- OfdmEqualizer (demodulate/ofdm.rs:296-569) ---------------------------------------
enum : int { kEqNone = -1, kEqTrainingSymbolHold = 0, kEqPerSymbolPilotInterp = 1 };
constexpr float kEqualizerFloor = 1e-6f;  // demodulate/ofdm.rs:386, on |h|^2
// training_symbol_freq_pattern (sync/ofdm_sync.rs:270-272, :335-352): out [n_fft][2].
void training_pattern(size_t n_fft, float* out);
// num-complex a / b: re = (a.re b.re + a.im b.im) / |b|^2, im = (a.im b.re - a.re b.im) / |b|^2,
// |b|^2 = b.re b.re + b.im b.im (num-complex 0.4 src/lib.rs, impl Div for Complex<T>), no FMA.
void cdiv(float ar, float ai, float br, float bi, float* re, float* im);
// equalizer_weight (demodulate/ofdm.rs:495-502): conj(h) / |h|^2, or 0 under the floor.
void equalizer_weight(float hr, float hi, float* wr, float* wi);
// interpolate_at (demodulate/ofdm.rs:514-537) over n bin-sorted ratios.
void interpolate_at(const uint32_t* bins, const float* ratios, size_t n, uint32_t bin, float* re, float* im);

class Equalizer {
 public:
  Equalizer(const Config& c, int method);
  int method() const { return method_; }
  size_t n_fft() const { return n_fft_; }
  // set_pilot_bins (demodulate/ofdm.rs:426-432).
  void set_pilot_bins(const uint32_t* bins, const float* vals, size_t n, const uint32_t* data_bins, size_t n_data);
  // estimate_from_training_symbol (demodulate/ofdm.rs:440-448): received [n_fft][2].
  void estimate_from_training_symbol(const float* received, size_t n);
  // process (demodulate/ofdm.rs:543-568): one n_fft-bin vector per call.
  void process(const float* in, size_t n_in, float* out, size_t out_cap, size_t* in_read, size_t* out_written);
  // What the kernels read: the held coefficients [n_fft][2], the held estimates [n_fft][2],
  // the bin-sorted pilots and the data bins.
  const std::vector<float>& weight() const { return weight_; }
  const std::vector<float>& estimate() const { return est_; }
  const std::vector<uint32_t>& pilot_bins() const { return pbin_; }
  const std::vector<float>& pilot_val() const { return pval_; }
  const std::vector<uint32_t>& data_bins() const { return dbin_; }

 private:
  int method_;
  size_t n_fft_;
  std::vector<float> est_, weight_, pval_, ratios_;
  std::vector<uint32_t> pbin_, dbin_;
};

// OfdmDemod (demodulate/ofdm.rs:26-95) over SymbolFft (symbol_fft.rs:67-126): the window
// starts at cp_len - min(backoff, cp_len); the gain applies only when |g - 1| > f32::EPSILON.
// eq (may be null) runs between the transform and the gather, as the reference composes it.
class Demod {
 public:
  explicit Demod(const Config& c);
  const Config& config() const { return cfg_; }
  const Grid& grid() const { return grid_; }
  const Fft& fft() const { return fft_; }
  size_t window_start() const { return start_; }
  void set_gain(float g) { gain_ = g; }
  float gain() const { return gain_; }
  // The transform of one symbol's window: freq [n_fft][2].
  void symbol_freq(const float* sym, float* freq) const;
  // As many whole symbols as fit: iq [n][2] -> soft [.. num_data][2].
  void process(const float* iq, size_t n, float* soft, size_t out_cap, Equalizer* eq, size_t* in_read,
               size_t* out_written);

 private:
  Config cfg_;
  Grid grid_;
  Fft fft_;
  size_t start_;
  float gain_ = 1.0f;
  std::vector<float> freq_, eqd_;
};

// evm_db (demodulate/ofdm.rs:263-293): f64 sums; false where the reference returns None.
bool evm_db(int order, const float* soft, size_t n_soft, const uint8_t* bits, size_t n_bits, size_t num_symbols,
            float* out);

}  // namespace ofdm
}  // namespace orion
