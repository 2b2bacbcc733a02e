// dvbt.hpp — the DVB-T 2K frame, host side (no HIP): the Figure-9a constellation, the
// four-phase continual / scattered / TPS carrier grid, the TPS word with its BCH(67,53), the
// guard-interval (van de Beek) acquisition, the continual-pilot integer CFO search and the
// per-symbol modulator and demodulator that the frame classes compose. A restatement of the
// reference (waveform/dvb_t.rs, waveform/dvb_t_tps.rs, sync/dvb_t_gi_sync.rs,
// modulate/dvb_t_frame.rs, demodulate/dvb_t_frame.rs) in scalar f32, built with
// -ffp-contract=off; the kernels of k_dvbt.hip are held to it.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orion {
namespace dvbt {

constexpr size_t kNFft = 2048, kKmax = 1704, kActive = kKmax + 1, kData = 1512, kPhases = 4;
constexpr size_t kContinual = 45, kTps = 17, kTpsSymbols = 68, kPilotSpacing = 12;
constexpr size_t kMaxRefPilots = 193;                                // continual + one phase's scattered, at most
constexpr size_t kMaxRxWindowBackoff = kNFft / (2 * kPilotSpacing);  // 85
constexpr size_t kTpsCodeword = 67, kTpsInfo = 53, kTpsParity = 14;
extern const uint16_t kContinualPilots2k[kContinual];
extern const uint16_t kTpsCarriers2k[kTps];

// Bin roles of the per-phase table: >= 0 the data index, or one of these.
enum : int32_t { kRoleNull = -1, kRolePilotPos = -2, kRolePilotNeg = -3, kRoleTps0 = -4 };  // TPS carrier j: kRoleTps0 - j

// wk_prbs (dvb_t.rs:390-402): X^11 + X^2 + 1 from all ones, one bit per active carrier.
std::vector<uint8_t> wk_prbs(size_t len);
// boosted_pilot_value (dvb_t.rs:408-410): (4/3) * 2 * (0.5 - w) in f32, in that order.
float boosted_pilot_value(uint8_t wk);
// scattered_pilot_indices (dvb_t.rs:439-444).
std::vector<uint32_t> scattered_pilot_indices(size_t phase);
// (active - 852).rem_euclid(2048).
uint32_t active_to_bin(size_t a);

// What dvb_t_2k_plans and ScatteredGridCycle hold of one phase (dvb_t.rs:494-575).
struct Phase {
  std::vector<uint32_t> data_bins;   // [1512] in active-carrier order
  std::vector<uint32_t> pilot_bins;  // every reserved carrier (continual + scattered + TPS) in active order
  std::vector<float> pilot_val;      // their boosted values (real)
  std::vector<uint32_t> ref_bins;    // the channel references: pilots minus TPS, sorted by bin
  std::vector<float> ref_val;        // real
  std::vector<int32_t> role;         // [2048]
  // Per data index: the reference pilots that interpolate_at would pick, lo == hi where it
  // takes one ratio as it is.
  std::vector<uint16_t> br_lo, br_hi;  // [1512]
};
struct Tables {
  std::array<Phase, kPhases> phase;
  std::array<uint32_t, kTps> tps_bins;
  std::array<float, kTps> tps_sign;  // 2 (0.5 - w_k)
  std::array<uint32_t, kContinual> continual_bins;
};
// Built once; throws std::logic_error unless every phase has exactly 1512 data carriers.
const Tables& tables();

// ---- Figure 9a (dvb_t.rs:138-266); v = 2, 4, 6, false otherwise ------------------------
bool map_symbol(const uint8_t* bits, size_t v, float* re, float* im);
bool demap_symbol(float re, float im, size_t v, uint8_t* bits);
bool soft_llr(float re, float im, size_t v, float* llr);

// ---- TPS (dvb_t_tps.rs) -------------------------------------------------------------------
uint32_t tps_bch_parity(const uint8_t* info53);
void tps_bch_encode(const uint8_t* info53, uint8_t* cw67);
bool tps_bch_decode(const uint8_t* cw67, uint8_t* info53);
struct TpsWord {
  int frame_number = 0;   // 0..3
  int constellation = 1;  // ofdm::kQpsk / kQam16 / kQam64
  int code_rate = 0;      // fec::kR1_2 .. kR7_8
  int guard = 0;          // 0..3
  int cell_id = 0;        // one byte
};
void tps_pack(const TpsWord& w, uint8_t* bits68);
bool tps_unpack(const uint8_t* bits68, TpsWord* w);
// TpsEncoder over n_symbols from symbol 0 (reset after every 68th, as the frame modulator
// does): signs [n_symbols], the common factor of the 17 reference signs.
void tps_symbol_signs(const uint8_t* bits68, size_t n_symbols, float* signs);
// TpsDecoder::feed_symbol over the first min(n_symbols, 68) symbols of cells [n_symbols][17][2]:
// bits [68], returns how many were written.
size_t tps_decide(const float* cells, size_t n_symbols, uint8_t* bits68);

// ---- guard-interval acquisition (dvb_t_gi_sync.rs) ------------------------------------------
// |z| as this library defines it for the acquisition: the f32 rounding of the f64 square root
// of the f64 sum of the two exact f64 squares (a stated divergence from libm's hypotf).
float norm32(float re, float im);
struct GiConfig {
  float rho = 0.95f;
  size_t max_symbols = 4;
  float origin_score_ratio = 0.5f;
};
struct GiResult {
  size_t start = 0;
  float cfo_hz = 0.0f, score = 0.0f, gamma_re = 0.0f, gamma_im = 0.0f, phi = 0.0f;
};
// The sums of one offset: gamma and phi (halved) over up to max_symbols symbols that fit.
void gi_sums(const float* iq, size_t n, size_t n_fft, size_t cp, size_t d, size_t max_symbols, float* gre, float* gim,
             float* phi);
// dvb_t_gi_sync_with; false where the reference returns None. metric (may be null) [search_len].
bool gi_sync(const float* iq, size_t n, size_t n_fft, size_t cp, float fs, size_t search_len, const GiConfig& cfg,
             GiResult* out, float* metric);
// dvb_t_integer_cfo (dvb_t_gi_sync.rs:380-417) over freq [n_fft][2].
bool integer_cfo(const float* freq, size_t n_freq, size_t n_fft, int max_bins, int32_t* bins, float* confidence);

// ---- the per-symbol modulator and demodulator ----------------------------------------------
// modulate/dvb_t_frame.rs:213-261 from the coded bits on: bits [n_bits] u8 -> iq [n_symbols *
// (2048 + cp)][2]. A data carrier whose v bits do not lie inside n_bits is zero.
void mod_symbols(const uint8_t* bits, size_t n_bits, size_t v, size_t cp, const uint8_t* tps68, size_t n_symbols,
                 size_t roll_off, float* iq);
// demodulate/dvb_t_frame.rs:497-583 over n_symbols from iq (the acquired start): llr
// [n_symbols][1512 v], cells [n_symbols][17][2] (raw bins), syms (may be null) [n_symbols][1512][2].
void demod_symbols(const float* iq, size_t n_symbols, size_t cp, size_t backoff, size_t v, float* llr, float* cells,
                   float* syms);

}  // namespace dvbt
}  // namespace orion
