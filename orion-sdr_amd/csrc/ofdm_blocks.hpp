// ofdm_blocks.hpp — the OFDM symbol layer on the device over k_ofdm.hip (host side): the
// batched transform and one engine per OfdmConfig that runs the fused modulator and
// demodulator, the RF stage and the elementwise blocks. The scalar code they are held to is
// ofdm.hpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "blocks.hpp"
#include "hip_common.hpp"
#include "ofdm.hpp"
#include "osc.hpp"

namespace orion {

constexpr int kOfdmThreads = 256;  // lanes per workgroup of the per-symbol kernels
// Lanes that share one symbol: min(n / 4, kOfdmThreads) — one radix-4 butterfly per lane and
// pass up to n = 1024, then 2 (n = 2048) and 4 (n = 4096); kOfdmThreads / T symbols share a
// workgroup (128 at n = 8, 16 at n = 64, 1 from n = 1024).
int ofdm_threads_per_symbol(size_t n);

// What the kernels read of one configuration (device pointers).
struct OfdmDev {
  int n, log2n, cp, T, order, bps, nd, np, roll;
  const f2* tw;               // [n / 2] ofdm::fft_twiddles
  const int32_t* map;         // [n] per bin: >= 0 the data index, -1 null, -2 - p pilot p (plan order)
  const f2* pilot_val;        // [np] plan order
  const uint32_t* data_bins;  // [nd]
  const uint32_t* spbin;      // [np] pilots sorted by bin
  const f2* spval;            // [np]
  const int32_t* emap;        // [n] k_ofdm_equalize's roles
  const f2* weight;           // [n] the held coefficients (TrainingSymbolHold)
  const f2* hold;             // [n] the held estimates
  const float* ramp;          // [roll]
  const float* axis;          // [16]
  const float* thr;           // [15]
};

void launch_fft(const f2* in, long long in_stride, f2* out, long long out_stride, long long batch, int n, int log2n,
                const f2* tw, bool inverse, hipStream_t s);
void launch_ofdm_mod(const uint8_t* bits, f2* out, long long batch, const OfdmDev& c, float gain, bool apply_gain,
                     hipStream_t s);
void launch_ofdm_rf(f2* iq, long long per_ch, long long nch, uint64_t k0, const OscDev& o, float gain, hipStream_t s);
void launch_ofdm_demod(const f2* iq, f2* soft, uint8_t* bits, float* llr, long long batch, const OfdmDev& c, int start,
                       float gain, bool apply_gain, int eq, hipStream_t s);
void launch_ofdm_decide(const f2* soft, long long n, int order, const float* thr, uint8_t* bits, hipStream_t s);
void launch_ofdm_llr(const f2* soft, long long n, int order, const float* axis, float* llr, hipStream_t s);
void launch_ofdm_equalize(const f2* in, f2* out, long long nsym, const OfdmDev& c, int eq, hipStream_t s);
// k_acquire.hip: raw [frames][nsym][nd] soft symbols (no equalizer, no gain) times each frame's
// weights [frames][n] at the data bins, then remove_common_phase_error per frame -> out.
void launch_frame_eq_cpe(const f2* raw, const f2* weights, long long frames, int nsym, const OfdmDev& c, f2* out,
                         hipStream_t s);

// FftBlock / IfftBlock (multicarrier/fft.rs) on the device. Constructing one touches no
// device; the twiddles are uploaded by the first call.
class FftDev {
 public:
  FftDev(size_t n, bool inverse) : host_(n, inverse) {}
  const ofdm::Fft& host() const { return host_; }
  // batch transforms: symbol b reads in + b * in_stride and writes out + b * out_stride (in
  // cf32 values; a stride >= n). Device pointers, asynchronous on s.
  void batch(const void* in, size_t in_stride, void* out, size_t out_stride, size_t batch, hipStream_t s);
  // One symbol per call from and to host memory (fft.rs:42-54), synchronous.
  WorkReport process_host(const void* in, size_t n_in, void* out, size_t out_cap);

 private:
  ofdm::Fft host_;
  DevTable tw_;
  DevBuf h_in_, h_out_;
};

// One OfdmConfig on the device. Constructing it touches no device; the tables are uploaded
// by the first call, and again after estimate_channel changed the held coefficients.
class OfdmEngine {
 public:
  // eq: ofdm::kEqNone, kEqTrainingSymbolHold or kEqPerSymbolPilotInterp (OfdmDemod / OfdmEqualizer).
  OfdmEngine(const ofdm::Config& c, int eq);
  const ofdm::Config& config() const { return mod_.config(); }
  ofdm::Mod& mod() { return mod_; }
  ofdm::Demod& demod() { return demod_; }
  ofdm::Equalizer* equalizer() { return eq_.get(); }
  int eq_method() const { return eq_ ? eq_->method() : ofdm::kEqNone; }
  size_t num_data() const { return demod_.grid().data_bins.size(); }

  // OfdmMod: bits [nch][nsym * bits_per_ofdm_symbol] u8 -> iq [nch][nsym * (n_fft + cp_len)]
  // cf32, one launch (two with rf_hz != 0: every channel continues the engine's oscillator
  // from the same output index, which then advances by one channel's samples).
  void modulate(const uint8_t* bits, size_t nch, size_t nsym, void* iq, hipStream_t s);
  // OfdmDemod (+ OfdmEqualizer + OfdmDecider / OfdmSoftDemod): iq [nch][nsym * (n_fft +
  // cp_len)] -> soft [nch][nsym * nd] cf32; bits (u8) and llr (f32) [nch][nsym * nd * bps]
  // may be null. One launch.
  void demodulate(const void* iq, size_t nch, size_t nsym, void* soft, uint8_t* bits, float* llr, hipStream_t s);
  // OfdmDecider / OfdmSoftDemod over n soft symbols.
  void decide(const void* soft, size_t n, uint8_t* bits, hipStream_t s);
  void soft_demod(const void* soft, size_t n, float* llr, hipStream_t s);
  // OfdmEqualizer::process over nsym n_fft-bin vectors (not in place).
  void equalize(const void* in, size_t nsym, void* out, hipStream_t s);
  // The equalizer branch of the frame demodulator's soft_demap for frames of nsym symbols each:
  // raw [frames][nsym * nd] (this engine's demodulate with no equalizer and no gain) and
  // weights [frames][n_fft] -> syms [frames][nsym * nd] after the phase tracker, and llr
  // [frames][nsym * nd * bps] (may be null) from them.
  void equalize_track(const void* raw, const void* weights, size_t frames, size_t nsym, void* syms, float* llr,
                      hipStream_t s);
  // estimate_from_training_symbol: received [n_fft] cf32 in host memory.
  void estimate_channel(const float* received, size_t n);
  // set_pilot_bins: the equalizer stage's tables are rebuilt by the next call.
  void set_pilot_bins(const uint32_t* bins, const float* vals, size_t n, const uint32_t* data_bins, size_t n_data);
  void set_demod_gain(float g) { demod_.set_gain(g); }
  void set_mod_gain(float g) { mod_.set_gain(g); }
  void reset();

  // The Block contract from and to host memory, synchronous: as many whole symbols as fit.
  WorkReport mod_host(const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap);
  WorkReport demod_host(const void* iq, size_t n, void* soft, size_t out_cap);
  WorkReport decide_host(const void* soft, size_t n, uint8_t* bits, size_t out_cap);
  WorkReport soft_demod_host(const void* soft, size_t n, float* llr, size_t out_cap);
  WorkReport equalize_host(const void* in, size_t n, void* out, size_t out_cap);

 private:
  const OfdmDev& dev(hipStream_t s);
  ofdm::Mod mod_;
  ofdm::Demod demod_;
  std::unique_ptr<ofdm::Equalizer> eq_;
  std::unique_ptr<RefOsc> osc_;
  OfdmDev d_{};
  bool up_ = false, weight_dirty_ = false;
  DevTable tw_, map_, pval_, dbin_, spbin_, spval_, emap_, weight_, hold_, ramp_, axis_, thr_;
  DevBuf h_in_, h_out_;
};

}  // namespace orion
