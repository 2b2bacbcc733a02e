// kernels.hpp — launch interfaces of the gfx950 kernels (host side).
// Every pointer named *_dev is device memory; every launch is asynchronous on
// the given stream and allocation-free (graph-capturable).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ftmod.hpp"
#include "hip_common.hpp"
#include "psk31.hpp"

namespace orion {

// ---------------------------------------------------------------- NCO --
// Rotator / Nco kernel tile (k_fir.hip k_rotator): samples per workgroup tile.
constexpr int kRotTile = 4096;
// ---- analog modulators (k_mod.hip; modulate/am.rs, fm.rs, ssb.rs) ----
// Every oscillator: o (hip_common.hpp OscDev), sample i of a call = output k0 + i.
void launch_am_mod(const float* x, f2* y, long long n, uint64_t k0, const OscDev& o, float cl, float mi, float g,
                   bool clamp, hipStream_t s);
// pm.rs:36-47: out = mix_with_nco((cos kp x, sin kp x) * g, rf phasor)
void launch_pm_mod(const float* x, f2* y, long long n, uint64_t k0, const OscDev& o, float kp, float g, hipStream_t s);
// u = [x p.re | x p.im] (planar, 2n floats), p = audio NCO phasor
void launch_ssb_mod_front(const float* x, float* u, long long n, uint64_t k0, const OscDev& o, hipStream_t s);
// y = (v[i], side v[n + i]) * rf phasor
void launch_ssb_mod_back(const float* v, f2* y, long long n, uint64_t k0, const OscDev& o, float side, hipStream_t s);
// FM phase accumulator: sums = fm_mod_chunks(n) uint64 of workspace; carry_in /
// carry_out: the running phase as a Q0.64 turn count (one uint64 each, ping-pong
// between calls; zero = phase 0); o: the RF Nco.
long long fm_mod_chunks(long long n);
// Single-pass form: rec = fm_mod_chunks(n) * 8 u32 look-back records (zeroed when
// allocated), epoch = this launch's tag (never reused while a record may hold it).
// err: the handle's host-visible error word (a look-back wait that timed out).
void launch_fm_mod_sp(const float* x, f2* y, long long n, float kf, float gain, uint32_t* rec, uint32_t epoch,
                      const uint64_t* carry_in, uint64_t* carry_out, uint64_t k0, const OscDev& o, int* err,
                      hipStream_t s);
void launch_fm_mod(const float* x, f2* y, long long n, float kf, float gain, uint64_t* sums,
                   const uint64_t* carry_in, uint64_t* carry_out, uint64_t k0, const OscDev& o, hipStream_t s);
// Oscillator blocks (k_fir.hip k_rotator): output i of a call is oscillator output
// k0 + i. mode: 0 Rotator::rotate_block (rotator.rs:74-85, cf32 -> cf32), 1
// Rotator::mix_usb_block (rotator.rs:88-94, cf32 -> f32), 2 mix_with_nco (nco.rs:63-66,
// cf32 -> cf32, non-FMA), 3 Nco::next_cs / Rotator::next (no input, cf32 phasors out).
void launch_osc(int mode, const f2* x_dev, void* y_dev, long long n, uint64_t k0, const OscDev& o, hipStream_t s);

// ---------------------------------------------------------- FIR family --
// Decimating FIR at the kept outputs only: out[j] = sum_k g[k] * x[M*j - k],
// j < n_out, with x[P<0] from hist (hist_len samples ending at x[-1]).
struct Taps256 { float g[256]; };
void launch_decim(const f2* x_dev, long long n, const f2* hist_dev, int hist_len, f2* out_dev,
                  long long n_out, int M, int K, const Taps256& g, const float* g_dev,
                  hipStream_t s);
// Batched over channels: x[ch*x_stride + i], out[ch*out_stride + j], shared taps.
// hist_out (optional): each channel's next history, written by the launch itself.
void launch_decim_batch(const f2* x_dev, long long x_stride, long long n, const f2* hist_dev,
                        int hist_len, f2* out_dev, long long out_stride, long long n_out, int nch,
                        int M, int K, const Taps256& g, const float* g_dev, hipStream_t s,
                        f2* hist_out = nullptr);
// Real FIR y[i] = sum_k g[k] x[i-k] (x[P<0] from hist).
// hist_out (optional): the next call's history (last hist_len of [hist | x]), written by
// the FIR launch itself (no separate k_hist_update launch).
void launch_fir_real(const float* x_dev, long long n, const float* hist_dev, int hist_len,
                     float* y_dev, int K, const Taps256& g, const float* g_dev, hipStream_t s,
                     float* hist_out = nullptr);
// Complex-sample real-tap FIR y[i] = sum_k g[k] x[i + off - k], i < n_out
// (x[P<0] from hist, x[P>=n] = 0). off = 0: streaming; off = (K-1)/2 with an
// all-zero history: FirLowpassIq::filter_aligned.
// nch > 1: independent channels, channel ch at x + ch x_stride / y + ch y_stride, its
// histories at ch hist_len of hist_dev / hist_out (batched FirLowpassIq).
void launch_fir_iq(const f2* x_dev, long long n, const f2* hist_dev, int hist_len, f2* y_dev,
                   long long n_out, long long off, int K, const Taps256& g, const float* g_dev,
                   hipStream_t s, f2* hist_out = nullptr, int nch = 1, long long x_stride = 0,
                   long long y_stride = 0);
// Copy the last hist_len samples of [old_hist | x[0..n)] into new_hist.
// FirLowpassIq::filter_aligned in place (k_fir_iq8 INPLACE + boundary copies);
// writes the history the reference leaves (last hist_len of [x | 0^d]) to
// hist_out first. false: K > 256 or edges too small (fir_iq_aligned_edges f2).
bool launch_fir_iq_aligned_inplace(f2* io, long long n, long long d, int K, const Taps256& g, f2* edges,
                                   long long edges_cap, f2* hist_out, int hist_len, hipStream_t s);
long long fir_iq_aligned_edges(long long n, int K);
void launch_hist_update_c(const f2* x_dev, long long n, const f2* old_dev, f2* new_dev,
                          int hist_len, hipStream_t s, int nch = 1, long long x_stride = 0);
void launch_hist_update_r(const float* x_dev, long long n, const float* old_dev, float* new_dev,
                          int hist_len, hipStream_t s);
// out[k] = e^{j 2 pi k step / 2^64}, k < n (device-built oscillator model step table)
void launch_phasor_table_q64(f2* out, uint64_t step_q64, int n, hipStream_t s);

// ------------------------------------------------------------ WBFM chain --
// Default: one launch per call (k_wbfm_seg, see k_wbfm.hip). The two-kernel path
// (any IIR design):
//  front: NCO mix -> polyphase decim x8 (<= 128 taps) -> FM discriminator,
//         writing phi (f32, 1/8 rate) — 8 B in, 0.5 B out per input sample;
//  back : LpCascade (wave scan, f64 carries, warm-up across workgroups) ->
//         audio FIR (<= 128 taps) — 0.59 B in, 0.5 B out per input sample.
constexpr int kWbfmM = 8;
constexpr int kWbfmQ = 16;
constexpr int kWbfmT = 512;                          // decimated outputs per front workgroup
constexpr int kWbfmPhi = kWbfmT - 1;                 // discriminator outputs per front workgroup
constexpr int kWbfmNS = kWbfmM * (kWbfmT + kWbfmQ);  // staged input samples per front workgroup
constexpr int kWbfmHist = kWbfmM * kWbfmQ;           // raw input history (128)
constexpr int kBackA = 4096;                         // audio outputs per back workgroup
constexpr int kBackC = 10;                           // IIR samples per lane and half
constexpr int kBackW = 510;                          // zero-state warm-up per half (51 chunks)
constexpr int kBackSpan = 256 * kBackC;              // 2560 = kBackA / 2 + warm-up (+2)
constexpr int kWbfmCarry = 8 + 128;                  // iir[4], prev[2], pad[2], fhist[128]
struct WbfmFrontConst {
  float g[128];  // decimator taps g[8q+c] phase-major at [c*16+q]; quirk-mapped
                 // (g[0]=h[L-1], g[k]=h[k-1], dsp/fir.rs:57-66), zero padded
  float k;       // 1/dev (fm.rs:23)
};
struct WbfmBackConst {
  float a[128];               // audio taps, quirk-mapped, zero padded
  float b0, b1, b2, a1, a2;   // LpCascade biquad (iir.rs:49-71)
  double pw[6 * 16];          // (A^C)^(2^s), s = 0..5 (C = kBackC)
  double mw[16];              // A^(64 C): one wave's span
};
// Segmented single-kernel chain (k_wbfm_seg): sub-range backs of kSgL outputs.
constexpr int kFuTail = 128;                         // IIR outputs handed to the next segment (FIR history)
constexpr int kFuSlot = 144;                         // u32 words of a segment's end-state record
// record layout (u32 words): [2,10) end state of the IIR (4 f64), [16,144) last
// 128 IIR outputs. Flags: 3 u32 per segment (the epoch of the last publish).
struct WbfmFusedConst {
  float b0, b1, b2, a1, a2;   // LpCascade biquad (iir.rs:49-71)
  float tscale;               // audio FIR on the matrix cores: 2^-st (taps scaled by 2^st; f per sub-range)
  // device memory, read with scalar loads where used (kWbfmMats doubles): (A^kSgC)^(2^s)
  // for s = 0..5, then A^(kSgL/2) (one half sub-range, read by iir16 as step 6)
  const double* mats;
};
constexpr int kWbfmMats = 7 * 16;
struct WbfmArgs {
  const f2* x;  long long x_stride;  long long n;
  float* phi;   long long phi_stride;               // workspace [nch][>= n_dec]
  float* y;     long long y_stride;  long long n_dec;
  long long k0;                                     // samples consumed by earlier calls
  const uint64_t* step;                             // [nch] Q0.64 oscillator step
  const f2* tab;                                    // [nch][kWbfmNS] e^{j theta p}
  const float* carry_in; float* carry_out;          // [nch][kWbfmCarry]
  const f2* hist_in; f2* hist_out;                  // [nch][kWbfmHist]
  const double* lanemats;                           // A^(C L), L = 0..63 (16 doubles each; k_wbfm_back)
  // segmented chain only
  uint32_t* hand;                                   // [slots][kSeg4Slot] hand-off records
  uint32_t* flags;                                  // [slots][3] epoch of the last publish
  int* err;                                         // host-visible error word: a hand-off wait timed out
  uint32_t spin;                                    // polls before a wait times out (kernels.hpp kSpinDefault)
  uint32_t epoch;                                   // this launch's tag (never 0)
  long long* trace;                                 // debug: per-wave phase timestamps (or null)
  const void* afrag;                                // audio FIR reversed f16 tap words (k_wbfm.hip sg::back)
};
// The audio FIR's taps as the A operand source: r[m] = a[127 - m] 2^st (zero outside
// [0, 128)) as f16 hi and lo parts, each in two parity copies of 96 words (copy p, word w:
// halves r[2w - 16 - p], r[2w - 15 - p]), so that any 8 consecutive halves are 4 aligned
// words of one copy (k_wbfm.hip sg::back keeps them in LDS).
constexpr int kAudTapWords = 96;
constexpr int kAudFragBytes = 2 * 2 * kAudTapWords * 4;  // (hi, lo) x 2 parity copies
constexpr int kFuTracePoints = 16;
void launch_wbfm(const WbfmArgs& a, const WbfmFrontConst& f, const WbfmBackConst& b, int nch,
                 hipStream_t s);
// Segmented single-kernel chain (k_wbfm_seg): sub-ranges of kSgL outputs, one round
// of waves. Requires ||A^(kSgL - 128)|| negligible (the block checks it).
constexpr int kSgL = 1024;                           // outputs per sub-range
constexpr int kSgC = kSgL / 128;                     // IIR samples per lane and half (8)
constexpr int kSeg4Slot = kFuSlot + kSgL;            // u32 words per segment: end-state record, then sub-range 0's phi
long long wbfm_seg_slots(long long n_dec, int nch);
// max_segments > 0 caps the waves (default: the resident capacity).
void launch_wbfm_seg(const WbfmArgs& a, const WbfmFrontConst& f, const WbfmFusedConst& b, int nch,
                     int max_segments, hipStream_t s);

// On-box bandwidth probe (k_diag.hip): a streaming read of the first
// stream_read_bytes(bytes) bytes of x (16-B aligned) with the WBFM front's load shape.
long long stream_read_bytes(long long bytes);
void launch_stream_read(const void* x, long long bytes, float* sink, hipStream_t s);
// Residency tests: `workgroups` one-wave workgroups holding lds_bytes of LDS each for
// `seconds` of wall clock (bounded; every wave exits).
void launch_spin(int workgroups, int lds_bytes, double seconds, hipStream_t s);

// ------------------------------------------------- FT8 / FT4 sync (k_sync.hip) --
// Waterfall (sync/waterfall.rs:73-151): x [nch][n] cf32, steps [num_tones] cf32 (the
// per-tone step phasors, host libm), out [nch][num_syms][num_tones] f32. mode 0:
// ln(e + 1e-12); 1: the energy e. rows_per_lane: 1, 2, 4 or 8 symbol rows per lane.
void launch_waterfall(const f2* x_dev, const f2* steps_dev, float* out_dev, int nch, long long n, int sps, int num_syms,
                      int num_tones, long long time_offset, int mode, int rows_per_lane, hipStream_t s);
// A Costas search pattern: nblk blocks of len tones, block b at frame symbol pos[b];
// tones: the FSK tones of a frame (bins it spans).
struct CostasPattern {
  int nblk, len, tones;
  int pos[4];
  int tone[4][7];
};
struct SyncCandidate {  // include/orion_sdr_amd.h orion_candidate
  int32_t time_sym;
  uint32_t freq_bin;
  float score;
};
constexpr int kSyncLlr = 174;  // codec/ldpc.rs N
// Candidate search (sync/costas.rs:125-174, sync/ft4_sync.rs:122-163) over wf
// [nch][num_syms][num_tones]: score_dev holds nch * (t_max - t_min + 1) * (num_tones -
// pat.tones + 1) floats of scratch; cand_dev [nch][max_cand] (unused slots zeroed),
// count_dev [nch]. max_cand >= 1.
void launch_costas_search(const float* wf_dev, float* score_dev, int nch, int num_syms, int num_tones,
                          const CostasPattern& pat, int t_min, int t_max, int max_cand, SyncCandidate* cand_dev,
                          uint32_t* count_dev, hipStream_t s);
// Normalised LLRs (sync/ft8_sync.rs:170-246, sync/ft4_sync.rs:227-292): llr_dev
// [nch][max_cand][174] (slots past a channel's count zeroed). cand_out_dev (optional, may
// be cand_dev): the records with time_sym - sym_adj.
void launch_sync_llr(const float* wf_dev, int nch, int num_syms, int num_tones, bool ft4, const SyncCandidate* cand_dev,
                     const uint32_t* count_dev, int max_cand, float* llr_dev, SyncCandidate* cand_out_dev, int sym_adj,
                     hipStream_t s);

// ------------------------------------------ LDPC(174,91) + CRC-14 decode (k_ldpc.hip) --
// n codewords, llr_dev [n][174] -> res_dev [n] records of 16 bytes (ldpc.hpp Result, 4-byte
// aligned), plain_dev [n][174] u8 or null. count_dev (optional): the sync layout, codeword
// w is slot w % max_cand of channel w / max_cand; slots at or past count[channel] give an
// all-zero record and are not decoded. rule / max_iter: ldpc.hpp (max_iter <= 255).
void launch_ldpc_decode(const float* llr_dev, long long n, const uint32_t* count_dev, int max_cand, bool ft4, int rule,
                        int max_iter, void* res_dev, uint8_t* plain_dev, hipStream_t s);
struct DecodePick {  // include/orion_sdr_amd.h orion_decode_pick
  int32_t first_ok;  // the first candidate with status 2, or -1
  float carrier_hz, snr_db;
  uint32_t pad;
};
void launch_decode_pick(const SyncCandidate* cand_dev, const uint32_t* count_dev, const void* res_dev, int nch,
                        int max_cand, float base_hz, float spacing, DecodePick* pick_dev, hipStream_t s);

// ------------------------- FT8 / FT4 modulators and hard demodulators (k_ftmod.hip) --
// Slot synthesis: out [nch][n] cf32 = (accumulate ? out : 0) + the sum, in table order, of
// every signal of the channel (rec_dev sorted by channel, rows_dev [nch + 1]: ftmod.hpp
// SynthPlan), clipped to [0, n). rot_dev (optional, >= n phasors): the RF Rotator stage,
// applied to each finished sample (Ft8Mod with rf_hz != 0: offset 0, n = the frame length).
using FtSynthRecord = ftmod::SynthRecord;
void launch_ft_synth(bool ft4, const FtSynthRecord* rec_dev, const uint32_t* rows_dev, f2* out_dev, int nch, long long n,
                     bool accumulate, const f2* rot_dev, hipStream_t s);
// Hard demodulator: x [nframes] rows of stride n >= the frame length (only the first
// frame length of a row is read); steps: the tones' step phasors (host memory, [8 | 4][2],
// ftmod.hpp demod_steps); tones_dev uint8 [nframes][58 | 87]; energies_dev (optional)
// f32 [nframes][79 | 105][8 | 4].
void launch_ft_demod(bool ft4, const f2* x_dev, int nframes, long long n, const float* steps, uint8_t* tones_dev,
                     float* energies_dev, hipStream_t s);

// ------------------------------------- PSK31 channel code: batched Viterbi (k_psk31.hip) --
// viterbi_decode (codec/psk31.rs:95-160) of nstreams soft streams: soft_dev [nstreams][2 *
// n_syms] f32 -> bits_dev [nstreams][n_syms] u8. work_dev: psk31::viterbi_work_bytes bytes of
// scratch (the survivor words of trellis_wave.hpp), 4-byte aligned. nstreams <= 2^31 - 4,
// n_syms <= 2^31 - 1.
void launch_psk31_viterbi(const float* soft_dev, long long nstreams, long long n_syms, uint8_t* bits_dev,
                          uint32_t* work_dev, hipStream_t s);
// The demodulator bank: one launch advances nstreams demodulators over x_dev [nch][n] cf32,
// whose first sample is the channels' sample base. rec_dev [nstreams] sorted by channel
// (every channel < nch, every out_cap <= out_stride), st_dev [nstreams] carried from call to
// call, hann_dev [sps]. soft_dev [nstreams][out_stride] and bits_dev (optional; soft >= 0, BPSK31 streams only)
// are indexed by the record's slot; report_dev [nstreams][2] = {in_read, out_written}.
void launch_psk31_demod(const f2* x_dev, long long n, unsigned long long base, const psk31::BankRecord* rec_dev,
                        psk31::DemodState* st_dev, int nstreams, const float* hann_dev, uint32_t sps, float* soft_dev,
                        long long out_stride, uint8_t* bits_dev, unsigned long long* report_dev, hipStream_t s);
// psk31_sync's carrier search (sync/psk31_sync.rs:82-203) on wf_dev [nch][num_syms][num_bins]
// (log waterfall): cand_dev [nch][max_cand] in the order psk31.hpp find_carriers defines
// (unused slots zeroed), count_dev [nch]. Scratch: med_dev [nch][num_bins] f32, floor_dev [nch]
// f32, runs_dev [nch][num_bins][max_cand], nruns_dev and head_dev [nch][num_bins] u32.
// ln_margin = peak_margin_db * LN_2 / 3 in f32; min_run >= 1; max_cand >= 1.
void launch_psk31_carriers(const float* wf_dev, int nch, int num_syms, int num_bins, int min_run, float ln_margin,
                           int max_cand, float* med_dev, float* floor_dev, SyncCandidate* runs_dev, uint32_t* nruns_dev,
                           uint32_t* head_dev, SyncCandidate* cand_dev, uint32_t* count_dev, hipStream_t s);
// The candidates' bank records and initial states, written on the device (record_candidate,
// psk31_sync.rs:209-239): rec_dev / st_dev [nch * max_cand], slot = channel * max_cand + k.
// steps_dev [num_bins][3]: each bin's Rotator step (w_re, w_im) and 1 if it has a rotator.
void launch_psk31_cand_records(const SyncCandidate* cand_dev, const uint32_t* count_dev, int nch, int max_cand,
                               const float* steps_dev, uint32_t sps, uint32_t out_cap, float scale,
                               psk31::BankRecord* rec_dev, psk31::DemodState* st_dev, hipStream_t s);
// The PSK31 modulator for a batch of streams: ph_dev [nstreams][n_syms + 1] symbol phasors
// (psk31.hpp Mod::symbol_phasors), hann_dev [sps], rot_dev (optional) >= n_syms * sps Rotator
// phasors from a fresh start; out_dev [nstreams][n_syms * sps] cf32.
void launch_psk31_mod(const f2* ph_dev, const float* hann_dev, const f2* rot_dev, int nstreams, long long n_syms,
                      uint32_t sps, float gain, f2* out_dev, hipStream_t s);
// PSK31 band synthesis: out_dev [nch][n] cf32 = (accumulate ? out : 0) + the signals of each
// channel in table order. rec_dev sorted by channel, rows_dev [nch + 1], ph_dev the signals'
// symbol phasors concatenated (n_bits + 1 each), hann_dev [sps].
void launch_psk31_synth(const psk31::SynthRecord* rec_dev, const uint32_t* rows_dev, const f2* ph_dev,
                        const float* hann_dev, uint32_t sps, int nch, long long n, bool accumulate, f2* out_dev,
                        hipStream_t s);
}  // namespace orion
