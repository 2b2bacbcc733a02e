// acquire.hpp — OFDM burst acquisition: the Schmidl & Cox packet search with its fractional
// and integer carrier-offset estimates (sync/ofdm_sync.rs:354-589), on the host in the
// reference's f32 operation order (built with -ffp-contract=off), and the batched search of
// k_acquire.hip that is held to it: one independent search per capture, one lane per
// candidate offset.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "blocks.hpp"
#include "hip_common.hpp"
#include "ofdm_blocks.hpp"

namespace orion {
namespace acquire {

// OfdmPreamble (sync/ofdm_sync.rs:45-75): num_repeats segments of repeat_len samples, then
// the training symbol of tn_fft + tcp samples when training is set.
struct Preamble {
  size_t num_repeats = 0, repeat_len = 0;
  bool training = false;
  size_t tn_fft = 0, tcp = 0;
  size_t lead() const { return num_repeats * repeat_len; }
  size_t total_len() const { return lead() + (training ? tn_fft + tcp : 0); }
};

// OfdmSyncResult (sync/ofdm_sync.rs:94-107).
struct SyncResult {
  int64_t start_sample;
  float cfo_hz;
  int32_t integer_cfo_bins;
  float score;
  uint32_t reserved;
};

constexpr size_t kTopN = 5;  // the integer search runs for this many ranked results

// The clamped end of a search, min(search_end, n - total_len) (saturating); a search is empty
// unless search_start < end, repeat_len > 0, num_repeats >= 2 and fs > 0 (ofdm_sync.rs:368-378).
size_t search_end(size_t n, const Preamble& pre, size_t search_end);
bool search_ok(size_t n, float fs, const Preamble& pre, size_t search_start, size_t search_end);

// P(d) and R(d) for d in [start, end) (ofdm_sync.rs:393-403, :567-589): every segment's sums
// start from zero and are added to p and r in segment order; the plain complex product and
// norm_sqr. iq [n][2]; p [end - start][2], r [end - start]. end <= n - num_repeats * repeat_len.
void sc_metric(const float* iq, const Preamble& pre, size_t start, size_t end, float* p, float* r);
// clamp(|p|^2 / (r r), 0, 1) and atan2(p.im, p.re) / (TAU repeat_len / fs) (ofdm_sync.rs:410-411).
float sc_score(float pr, float pi, float r);
float sc_cfo_den(size_t repeat_len, float fs);

// ofdm_sync (ofdm_sync.rs:361-463): the ranked candidates. r_peak (may be null) receives the
// largest r of the kept offsets.
std::vector<SyncResult> ofdm_sync(const float* iq, size_t n, float fs, const Preamble& pre, size_t search_start,
                                  size_t search_end, float* r_peak = nullptr);
// earliest_accepted (ofdm_sync.rs:488-503): the index into results, or -1.
long long earliest_accepted(const SyncResult* results, size_t n, float score_threshold, size_t cluster_len);
// estimate_integer_cfo_bins (ofdm_sync.rs:513-562). corr2 (may be null, [tn_fft + 1]) receives
// |corr|^2 per shift, -tn_fft / 2 first.
int32_t estimate_integer_cfo_bins(const float* iq, size_t n, float fs, size_t tn_fft, size_t tcp, size_t training_start,
                                  float fractional_cfo_hz, float* corr2 = nullptr);


// ---- the burst receiver's body (demodulate/ofdm_frame.rs:55-274, :1486-1592) --------------
// Rotator::new(freq_hz, fs).rotate_block (dsp/rotator.rs:74-84): in, out [n][2].
void rotate_block(float freq_hz, float fs, const float* in, size_t n, float* out);
// remove_common_phase_error (demodulate/ofdm_frame.rs:200-274) over syms [n_sym][n_data][2] in
// place: nothing below 4 symbols; the decision-directed loop (ALPHA 0.5, BETA 0.05, bit 1 where
// the LLR <= 0, the ideal mapper, err = 0 for an accumulator that is exactly zero), then the
// least-squares line through the measured phases in closed form, guarded on its denominator.
void remove_common_phase_error(int order, float* syms, size_t n_sym, size_t n_data);
// The equalizer branch of soft_demap (:95-134) for c's constellation: per symbol SymbolFft at
// c's window back-off, times the weights of estimate_from_training_symbol(training_freq
// [n_fft][2]) (the 1e-6 floor), the data bins; then the phase tracker over all of them.
// iq [n_sym * (n_fft + cp_len)][2] -> syms [n_sym * n_data][2], llr [n_sym * n_data * bps] (may
// be null). No gain is divided out: the estimate absorbs it.
void soft_demap_equalized(const ofdm::Config& c, const float* iq, size_t n_sym, const float* training_freq, float* syms,
                          float* llr);

}  // namespace acquire

// ---- the device side (k_acquire.hip) --------------------------------------------------------
constexpr int kScThreads = 256;         // candidate offsets per workgroup of k_sc_metric
constexpr int kScLdsSamples = 4096;     // k_sc_metric stages 256 + num_repeats repeat_len samples up to this (32 KiB)

// What one batched search writes (device pointers): per offset p [ncap][nd] cf32, r, score
// (-1 at a skipped offset), cfo_hz [ncap][nd]; per capture r_peak, top_start / top_bins
// [ncap][5] (-1 / 0 padded), accepted_start (-1: none), accepted_in_top (-1: not among the
// five), accepted_bins, accepted_score, accepted_cfo_hz.
struct SyncOut {
  f2* p;
  float *r, *score, *cfo_hz, *r_peak;
  int32_t *top_start, *top_bins, *accepted_start, *accepted_in_top, *accepted_bins;
  float *accepted_score, *accepted_cfo_hz;
};

void launch_sc_metric(const f2* iq, long long ncap, long long n, int num_repeats, int repeat_len, long long start,
                      long long nd, float cfo_den, const SyncOut& o, hipStream_t s);
void launch_sc_select(long long ncap, long long nd, long long start, float threshold, long long cluster_len,
                      const SyncOut& o, hipStream_t s);
// sym [ncap * 5][n_fft]: each candidate's training symbol from the CP boundary, times the
// closed-form phasor of -cfo_hz (phase index k + 1 at sample k of the symbol); zeros for a
// padded candidate.
void launch_icfo_gather(const f2* iq, long long ncap, long long n, long long nd, long long start, int lead, int n_fft,
                        int cp, float fs, const SyncOut& o, f2* sym, hipStream_t s);
void launch_icfo_corr(const f2* freq, const f2* known, long long ncap, long long n, int lead, int n_fft, int cp,
                      const SyncOut& o, hipStream_t s);

// rows [ncap][n]: capture c from accepted_start[c] on, times the closed-form phasor of
// -total_cfo[c] = -(accepted_cfo_hz + accepted_bins spacing), zero past the capture's end (and
// everywhere without an accepted candidate); avail [ncap] the samples a row holds, total_cfo [ncap].
void launch_acq_correct(const f2* iq, long long ncap, long long n, float spacing, float fs, const SyncOut& o, f2* rows,
                        int32_t* avail, float* total_cfo, hipStream_t s);
// weights [count] = equalizer_weight(freq / known[i mod n_fft]) (demodulate/ofdm.rs:440-502).
void launch_acq_weights(const f2* freq, const f2* known, long long count, int n_fft, f2* weights, hipStream_t s);

// One preamble's batched search. Constructing it touches no device.
class AcquireEngine {
 public:
  explicit AcquireEngine(const acquire::Preamble& pre);
  const acquire::Preamble& preamble() const { return pre_; }
  // iq [ncap][n] cf32 on the device; the range is ofdm_sync's, clamped the same way, and must
  // not be empty (acquire::search_ok). Asynchronous on s.
  void sync_batch(const void* iq, size_t ncap, size_t n, float fs, size_t search_start, size_t search_end,
                  float threshold, const SyncOut& o, hipStream_t s);
  // The accepted candidates' corrected rows (launch_acq_correct; spacing = fs / n_fft in f32).
  void correct(const void* iq, size_t ncap, size_t n, float fs, size_t n_fft, const SyncOut& o, void* rows, int32_t* avail,
               float* total_cfo, hipStream_t s);
  // Per-capture equalizer weights [ncap][n_fft] from the training symbol of the corrected rows,
  // transformed at window (samples into the symbol: cp_len - back-off). Needs a training symbol.
  void weights(const void* rows, size_t ncap, size_t n, size_t window, void* weights, hipStream_t s);

 private:
  acquire::Preamble pre_;
  std::unique_ptr<FftDev> fft_;
  const f2* known(hipStream_t s);  // the training pattern on the device, uploaded by the first use
  DevTable known_;
  DevBuf sym_, freq_;
};

}  // namespace orion
