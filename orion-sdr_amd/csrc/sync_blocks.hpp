// sync_blocks.hpp — the FT8 / FT4 sync front end over k_sync.hip (host side).
//
// Reference: sync/waterfall.rs (compute_waterfall), sync/costas.rs (find_candidates),
// sync/ft8_sync.rs and sync/ft4_sync.rs (ft8_sync / ft4_sync). Not a Block: a sync call
// has no streaming state and several outputs, so it has a handle of its own that owns
// what the calls reuse (the step table, the scratch waterfall, the score map).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "blocks.hpp"

namespace orion {

enum : int { kWfLog = 0, kWfEnergy = 1 };       // include/orion_sdr_amd.h ORION_WF_*
enum : int { kCostasFt8 = 0, kCostasFt4 = 1 };  // ORION_COSTAS_*

// waterfall.rs:84-91: w_k = (cos phi, sin phi), phi = (-TAU * f) / fs, f = base + k *
// spacing, all f32, libm sinf / cosf. Interleaved (re, im).
std::vector<float> waterfall_steps(float fs, float base_hz, float tone_spacing_hz, size_t num_tones);

// ft8_sync.rs:99-131 / ft4_sync.rs:74-98: the geometry a sync call derives.
struct SyncGeometry {
  size_t num_bins, wf_syms, wf_sample_start;
  int sym_offset_adj, wf_t_max;
};
SyncGeometry sync_geometry(int pattern, float base_hz, float max_hz, int t_min, int t_max);

// A host entry stages cand [nch][max_cand] and count [nch] in one device buffer: count's offset.
inline size_t cand_count_offset(size_t nch, size_t max_cand) {
  return (nch * max_cand * sizeof(SyncCandidate) + 15) / 16 * 16;
}

class Sync {
 public:
  // Symbol rows per lane of the waterfall kernel: 1, 2, 4 or 8; 0 = chosen per call
  // from the number of waves the call spreads over (1, 2 or 4).
  void set_rows_per_lane(int s);
  // All device pointers; asynchronous on s once the handle's buffers have grown to the
  // geometry (growing frees and allocates, which synchronises the device).
  void waterfall(const void* iq, float fs, float base_hz, float tone_spacing_hz, size_t samples_per_sym,
                 size_t num_syms, size_t num_tones, size_t time_offset, size_t nch, size_t n_per_ch, int mode,
                 float* mag, hipStream_t s);
  void find_candidates(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern, int t_min,
                       int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, hipStream_t s);
  void sync(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz, int t_min,
            int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, float* llr, hipStream_t s);
  // sync, then the LDPC + CRC decode of every candidate (ldpc_decode below) and the pick
  // of each channel's first decoded one, all on s with no host round trip. results
  // [nch][max_cand] records, pick [nch].
  void decode(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz, int t_min,
              int t_max, size_t max_cand, int rule, size_t max_iter, SyncCandidate* cand, uint32_t* count, float* llr,
              void* results, DecodePick* pick, hipStream_t s);
  void decode_host(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                   int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, SyncCandidate* cand, uint32_t* count,
                   float* llr, void* results, DecodePick* pick);
  // Host slices: uploaded, run as one device call, downloaded (synchronous).
  void waterfall_host(const void* iq, float fs, float base_hz, float tone_spacing_hz, size_t samples_per_sym,
                      size_t num_syms, size_t num_tones, size_t time_offset, size_t nch, size_t n_per_ch, int mode,
                      float* mag);
  void sync_host(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                 int t_min, int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, float* llr);

 private:
  int rows_for(size_t num_syms, size_t num_tones, size_t nch) const;
  int rows_ = 0;
  // the step table on the device and the geometry it was built for
  DevTable steps_;
  float st_fs_ = 0, st_base_ = 0, st_spacing_ = 0;
  size_t st_tones_ = 0;
  DevBuf wf_, score_;             // sync()'s waterfall; the score map
  DevBuf h_iq_, h_out_, h_cand_, h_res_;  // staging of the host entries
};

// LLRs of caller-supplied candidates on a caller-supplied waterfall (device pointers).
void sync_llr(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern, const SyncCandidate* cand,
              const uint32_t* count, size_t max_cand, float* llr, hipStream_t s);


// LDPC(174,91) + CRC-14 decode (k_ldpc.hip; ldpc.hpp for the rule and the record) of n
// codewords, llr [n][174] -> results [n] (16-byte records), plain [n][174] u8 or null;
// device pointers, asynchronous on s. count non-null: the layout sync() writes, n = nch *
// max_cand, and the slots past a channel's count give all-zero records without a decode.
void ldpc_decode(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                 size_t max_iter, void* results, uint8_t* plain, hipStream_t s);
// Host slices (count: nch = n / max_cand entries, or null): synchronous.
void ldpc_decode_host(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                      size_t max_iter, void* results, uint8_t* plain);

// ---- FT8 / FT4 modulators, slot synthesis and hard demodulators (ftmod.hpp, k_ftmod.hip) ----
// The device copy of a synthesis plan and the launch over it. A call waits for the handle's
// previous launch, builds the plan on the host in pinned memory (signals and tones are host
// memory), and queues the copy and the launch on s: asynchronous once the buffers have grown
// to the plan. iq is device memory [nch][n] cf32. rot: kernels.hpp launch_ft_synth.
// The mechanism is what blocks.hpp PlanUpload holds for the PSK31 entries. It stays spelt out
// here: the time of orion_ft_synth_device is the host's plan build (ftmod::synth_plan_into),
// which moves by tens of per cent with where a build places it (profiles/HISTORY.md), so an
// A/B of this path against PlanUpload has not been able to show that the two are equal.
class FtSynth {
 public:
  FtSynth() = default;
  ~FtSynth();
  FtSynth(const FtSynth&) = delete;
  FtSynth& operator=(const FtSynth&) = delete;
  void run(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
           size_t n, bool accumulate, void* iq, const f2* rot, hipStream_t s);

 private:
  DevBuf tab_;
  void* pin_ = nullptr;  // the plan as the host builds it (pinned: copied by DMA, no staging)
  size_t pin_n_ = 0;
  hipEvent_t done_ = nullptr;  // the last copy out of pin_ and launch over tab_
};
// Ft8Mod / Ft4Mod (modulate/ft8.rs:48-156, ft4.rs:51-173): nframes frames per call, tones
// [nframes][58 | 87] (host) -> iq [nframes][frame_len] cf32. With rf_hz != 0 the Rotator's
// phasors over one frame (a fresh Rotator per frame, ft8.rs:150-153: the reference's own,
// from its recurrence on the host) are tabulated once, at the first device call: constructing
// a modulator touches no device.
class FtMod {
 public:
  FtMod(int protocol, float fs, float base_hz, float rf_hz, float gain);
  size_t frame_len() const { return static_cast<size_t>(ftmod::proto(protocol_).frame_len()); }
  void modulate(const uint8_t* tones, size_t nframes, void* iq_dev, hipStream_t s);
  void modulate_host(const uint8_t* tones, size_t nframes, void* iq);

 private:
  int protocol_;
  float fs_, base_hz_, rf_hz_, gain_;
  DevTable rot_;
  DevBuf h_out_;
  FtSynth synth_;
  std::vector<ftmod::Signal> sig_;
};
// Slot synthesis on a shared FtSynth, one per device (one call at a time, process-wide).
void ft_synth(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
              size_t n, bool accumulate, void* iq_dev, hipStream_t s);
void ft_synth_host(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                   size_t n, bool accumulate, void* iq);
// Ft8Demod / Ft4Demod (demodulate/ft8.rs:25-126, ft4.rs): iq [nframes] rows of n_per_frame
// >= frame_len samples -> tones [nframes][58 | 87], energies (may be null) [nframes][79 |
// 105][8 | 4]. Device pointers, asynchronous on s / host slices, synchronous.
void ft_demod(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame, uint8_t* tones,
              float* energies, hipStream_t s);
void ft_demod_host(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                   uint8_t* tones, float* energies);

}  // namespace orion
