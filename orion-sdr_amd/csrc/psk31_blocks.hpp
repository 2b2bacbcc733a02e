// psk31_blocks.hpp — PSK31 on the device over k_psk31.hip (host side): the batched Viterbi
// decode (the wave engine of trellis_wave.hpp) and the demodulator bank. The scalar code they
// are held to is psk31.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "blocks.hpp"
#include "psk31.hpp"
#include "sync_blocks.hpp"

namespace orion {

// viterbi_decode (codec/psk31.rs:95-160) of nstreams streams in one launch: soft [nstreams][2 *
// n_syms] f32 -> bits [nstreams][n_syms] u8. Device pointers, asynchronous on s; work is the
// caller's scratch of at least psk31::viterbi_work_bytes(nstreams, n_syms) bytes.
void psk31_viterbi(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits, void* work, size_t work_bytes,
                   hipStream_t s);
// Host slices: synchronous, the scratch is allocated for the call.
void psk31_viterbi_host(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits);

// The PSK31 demodulator bank (k_psk31.hip k_psk31_demod): nstreams independent Bpsk31Demod /
// Qpsk31Demod (demodulate/psk31.rs) over nch channels, advanced by one launch per call. The
// streams keep the caller's order in every output; the kernel's copy is sorted by channel
// and start. Constructing a bank touches no device; its tables are uploaded by the first call.
class Psk31DemodBank {
 public:
  Psk31DemodBank(float fs, const psk31::Stream* streams, size_t nstreams, size_t nch);
  size_t nstreams() const { return rec_.size(); }
  size_t max_out_cap() const { return max_cap_; }
  // iq [nch][n] cf32, the channels' next n samples; soft [nstreams][out_stride] f32
  // (out_stride >= max_out_cap()), bits (may be null) the same shape u8, reports
  // [nstreams][2] u64 {in_read, out_written}. Device pointers, asynchronous on s.
  void process(const void* iq, size_t nch, size_t n, float* soft, size_t out_stride, uint8_t* bits, uint64_t* reports,
               hipStream_t s);
  // Host slices: synchronous.
  void process_host(const void* iq, size_t nch, size_t n, float* soft, size_t out_stride, uint8_t* bits,
                    uint64_t* reports);
  void reset();
  // set_gain (demodulate/psk31.rs:132-134) of the stream the caller listed at index slot;
  // takes effect with the next call.
  void set_gain(size_t slot, float gain);

 private:
  size_t nch_, sps_, max_cap_ = 0;
  float hann_sq_sum_ = 1.0f;
  bool rec_dirty_ = false;
  uint64_t base_ = 0;
  bool fresh_ = true;  // the device tables and states are not (or no longer) the initial ones
  std::vector<psk31::BankRecord> rec_;
  std::vector<psk31::DemodState> st0_;
  std::vector<float> hann_;
  DevTable d_rec_, d_st_, d_hann_;
  DevBuf h_iq_, h_soft_, h_bits_, h_rep_;
};

// Bpsk31Mod / Qpsk31Mod with a device path (k_psk31_mod). host() is the scalar modulator
// (and the state: the phasor and QPSK31's coder register); the device calls build each
// stream's symbol phasors on the host with the same arithmetic and launch one kernel.
// Constructing one touches no device.
class Psk31ModDev {
 public:
  Psk31ModDev(int mode, float fs, float rf_hz, float gain) : host_(mode, fs, rf_hz, gain) {}
  psk31::Mod& host() { return host_; }
  // One stream from the modulator's current state, which advances as modulate_bits' does:
  // bits [n] (host) -> iq [n * sps] cf32 (device), asynchronous on s: a call waits only for
  // the handle's previous launch (blocks.hpp PlanUpload).
  void modulate(const uint8_t* bits, size_t n, void* iq_dev, hipStream_t s);
  // nstreams independent streams, each from a fresh modulator of these parameters (the
  // state is not touched): bits [nstreams][n] (host) -> iq [nstreams][n * sps] (device).
  void modulate_batch(const uint8_t* bits, size_t nstreams, size_t n, void* iq_dev, hipStream_t s);
  // The batch into host memory (synchronous).
  void modulate_batch_host(const uint8_t* bits, size_t nstreams, size_t n, void* iq);

 private:
  void run(const std::vector<float>& ph, size_t nstreams, size_t n, void* iq_dev, hipStream_t s);
  psk31::Mod host_;
  PlanUpload ph_;  // a call's symbol phasors
  DevTable hann_, rot_;
  DevBuf h_out_;
  size_t rot_n_ = 0;
};

// Band synthesis (k_psk31_synth): signals [nsig] and their bits concatenated (host memory) ->
// iq [nch][n] cf32 on the device. The plan (records sorted by channel, symbol phasors from
// fresh modulators) is built on the host; its copy and the launch are queued on s (blocks.hpp
// PlanUpload, one per device). One call at a time, process-wide. Throws
// std::invalid_argument for a channel >= nch, an unknown mode, or sizes above the limits.
void psk31_synth(float fs, const psk31::Signal* signals, const uint8_t* bits, size_t nsig, size_t nch, size_t n,
                 bool accumulate, void* iq_dev, hipStream_t s);
void psk31_synth_host(float fs, const psk31::Signal* signals, const uint8_t* bits, size_t nsig, size_t nch, size_t n,
                      bool accumulate, void* iq);

// psk31_sync (sync/psk31_sync.rs:50-239) on the device, batched over channels, with no trip
// to the host between its stages: the waterfall (Sync::waterfall, one bin per 31.25 Hz), the
// carrier search (k_psk31_medians / _floor / _runs / _merge), the candidates' bank records
// written on the device (k_psk31_cand_records) and one launch of the demodulator bank over
// them. Owns the scratch the stages share; buffers grow to the geometry (growing allocates).
class Psk31Sync {
 public:
  // The search alone on a caller's log waterfall wf [nch][num_syms][num_bins] (device):
  // cand [nch][max_cand] (unused slots zeroed), count [nch]. Asynchronous on s.
  void find_carriers(const float* wf, size_t nch, size_t num_syms, size_t num_bins, size_t min_carrier_syms,
                     float peak_margin_db, size_t max_cand, SyncCandidate* cand, uint32_t* count, hipStream_t s);
  // iq [nch][n] cf32 (device) -> cand, count as above (time_sym the run's first symbol), soft
  // [nch][max_cand][n_bits + 2] f32 (zeroed, then each candidate's soft bits from its start),
  // reports [nch][max_cand][2] u64 {in_read, out_written}: record_candidate keeps the first
  // min(out_written, n_bits) values. Asynchronous on s.
  void sync(Sync& eng, const void* iq, size_t nch, size_t n, float fs, float base_hz, float max_hz,
            size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand, SyncCandidate* cand,
            uint32_t* count, float* soft, uint64_t* reports, hipStream_t s);
  // Host slices: uploaded, run as above, downloaded (synchronous).
  void find_carriers_host(const float* wf, size_t nch, size_t num_syms, size_t num_bins, size_t min_carrier_syms,
                          float peak_margin_db, size_t max_cand, SyncCandidate* cand, uint32_t* count);
  void sync_host(Sync& eng, const void* iq, size_t nch, size_t n, float fs, float base_hz, float max_hz,
                 size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand, SyncCandidate* cand,
                 uint32_t* count, float* soft, uint64_t* reports);

 private:
  DevBuf wf_, med_, floor_, runs_, nruns_, head_, rec_, st_;
  DevTable hann_, steps_;
  DevBuf h_in_, h_cand_, h_soft_, h_rep_;
  float st_fs_ = 0, st_base_ = 0, hann_fs_ = 0, hann_sq_sum_ = 1.0f;
  size_t st_bins_ = 0;
};

}  // namespace orion
