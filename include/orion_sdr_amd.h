/*
 * orion_sdr_amd.h — C ABI of the MI355X (gfx950) streaming DSP engine.
 *
 * Drop-in boundary for skynavga/orion-sdr's analog sample-stream path. Every
 * entry point replaces one reference interface (cited file:line, reference
 * v0.0.63). Plain pointers and sizes only: no HIP or torch types cross this
 * boundary (streams are passed as `void*` = hipStream_t, NULL = default stream).
 *
 * Contract (src/core.rs:6-22, trait Block):
 *  - A handle is one stateful Block instance; it keeps its streaming state
 *    (delay lines, oscillator phase, IIR state, discriminator history) across
 *    calls, so k calls on consecutive chunks equal one call on the whole.
 *  - orion_block_process*: 1:1 blocks consume n = min(n_in, out_cap) samples;
 *    FirDecimator and the WBFM chain consume all n_in and write
 *    min(ceil(n_in/m), out_cap) (dsp/decim.rs:66-75). The decimation phase
 *    restarts at every call, as in the reference (decim.rs:68-71).
 *  - Return 0 on success, a negative ORION_E_* code otherwise (the reference
 *    never fails on lengths; errors here are HIP/argument failures only).
 *  - Types: cf32 = interleaved {float re, im} (num_complex::Complex32), f32.
 *  - Multi-channel handles (nch > 1) read in[ch*n_in + i] and write
 *    out[ch*out_cap + j]; channels are independent streams.
 */
#ifndef ORION_SDR_AMD_H
#define ORION_SDR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORION_OK 0
#define ORION_E_NULL (-1)
#define ORION_E_HIP (-2)
#define ORION_E_ARG (-3)
#define ORION_E_TYPE (-4)
#define ORION_E_UNSUPPORTED (-5)

#define ORION_DT_C32 0
#define ORION_DT_F32 1

/* core.rs:6-10 */
typedef struct {
  size_t in_read;
  size_t out_written;
} orion_work_report;

typedef struct orion_block orion_block;

/* ---- library ---------------------------------------------------------- */
const char* orion_version(void);
const char* orion_last_error(void);          /* thread-local message of the last failure */
int orion_device_count(void);
int orion_set_device(int device);
int orion_synchronize(void* stream);
/* Pinned (page-locked) host memory for the host-buffer path (no reference counterpart):
 * orion_block_process DMAs it without staging copies. NULL on failure. */
void* orion_host_alloc(size_t bytes);
int orion_host_free(void* p);
int orion_device_cus(void);                 /* compute units of the current device (< 0: error) */
/* On-box bandwidth probe (no reference counterpart; bench.py's measured read
 * peak): one streaming read of the first orion_diag_stream_read_bytes(bytes)
 * bytes of the 16-B aligned device buffer `dev`, asynchronous on `stream`. */
size_t orion_diag_stream_read_bytes(size_t bytes);
int orion_diag_stream_read(const void* dev, size_t bytes, void* stream);
/* Residency tests (no reference counterpart): `workgroups` one-wave workgroups that
 * each hold lds_bytes of LDS (256 .. 160 KiB) for `seconds` (<= 10) of wall clock on
 * `stream`, asynchronous; and a stream restricted to the first n_cus CUs (0: an
 * ordinary non-blocking stream), destroyed with orion_diag_stream_destroy. */
int orion_diag_spin(void* stream, uint32_t workgroups, uint32_t lds_bytes, double seconds);
void* orion_diag_stream_create(uint32_t n_cus);
int orion_diag_stream_destroy(void* stream);

/* ---- constructors (one per reference constructor) ---------------------- */
/* dsp/rotator.rs:16-26 Rotator::new(freq_hz, fs); Block-like rotate_block (:74-85). cf32->cf32
 * The oscillator tracks the reference's own f32 recurrence (z <- z w, renormalised
 * every 1024 steps, :44-62), not the ideal phasor it drifts from: at construction and
 * every set_freq / reset_phase the host runs that recurrence from the current state
 * for up to ORION_OPT_NCO_TABLE outputs (default 2^20, a few ms) and the device reads
 * its phasors. The finite-state recurrence falls into a cycle; when the cycle closes
 * within the budget (-1.5 MHz / 10 MHz: after 21504 steps) every output is the
 * reference's, bit for bit, forever. Otherwise outputs past the budget follow a drift
 * model (the fitted mean step and a magnitude linear in the renorm position).
 * Construction fails (NULL, orion_last_error) if TAU * freq_hz / fs is not finite. */
orion_block* orion_rotator_new(float freq_hz, float fs);
/* dsp/rotator.rs:35-39 Rotator::set_freq(freq_hz, fs): a new step phasor; z and the
 * renorm counter carry on (the reference keeps them). Synchronizes the device
 * (kernels in flight read the oscillator table). ORION_E_ARG if TAU * freq_hz / fs is
 * not finite (e.g. fs = 0: the reference would produce NaN forever). */
int orion_rotator_set_freq(orion_block* b, float freq_hz, float fs);
/* dsp/rotator.rs:44-68 Rotator::next / next_cs, n times: out[i] = the phasor after each
 * step (cf32 pairs), advancing the same oscillator as rotate_block. Host buffer
 * (synchronous) / device buffer. */
int orion_rotator_next_cs_block(orion_block* b, void* out, size_t n);
int orion_rotator_next_cs_block_device(orion_block* b, void* out_dev, size_t n, void* stream);
/* dsp/rotator.rs:28-31 Rotator::reset_phase: phasor back to 1 + j0 (the step stays);
 * the same as orion_block_reset on a Rotator. */
int orion_rotator_reset_phase(orion_block* b);
/* dsp/rotator.rs:88-94 Rotator::mix_usb_block(input, out): out[i] = fma(I, cos, Q*sin)
 * with the phasor of the next step, on the same oscillator as rotate_block; n =
 * min(n_in, out_cap). cf32 -> f32. Host buffers (synchronous) / device buffers. */
int orion_rotator_mix_usb_block(orion_block* b, const void* in, size_t n_in, float* out, size_t out_cap,
                                orion_work_report* wr);
int orion_rotator_mix_usb_block_device(orion_block* b, const void* in_dev, size_t n_in, float* out_dev, size_t out_cap,
                                       void* stream, orion_work_report* wr);
/* Host only (no device; tests and diagnostics, no reference counterpart): the first n
 * phasors of Rotator::new(freq_hz, fs) as the engine tabulates them with a budget of
 * max_out outputs (the reference recurrence, its cycle, or the drift model past the
 * budget) into out (cf32); cyc_len = 0 when no cycle closed within the budget. */
int orion_osc_table_phasors(float freq_hz, float fs, uint64_t max_out, void* out, size_t n, uint64_t* cyc_start,
                            uint64_t* cyc_len, uint64_t* n_tab);
/* dsp/nco.rs:20-31 Nco::new(freq_hz, fs) as a block: process = mix_with_nco per sample
 * (nco.rs:63-66, the non-FMA product (x.re c - x.im s, x.re s + x.im c)). cf32->cf32
 * The oscillator tracks the reference recurrence (nco.rs:42-58) as the Rotator's does. */
orion_block* orion_nco_new(float freq_hz, float fs);
/* dsp/nco.rs:33-38 Nco::set_freq(freq_hz) (fs from orion_nco_new): the phase continues.
 * Synchronizes the device. */
int orion_nco_set_freq(orion_block* b, float freq_hz);
/* dsp/nco.rs:42-58 next_cs, n times: out[i] = (cos, sin) of the phasor after each step
 * (cf32 pairs). Host buffer (synchronous) / device buffer. */
int orion_nco_next_cs_block(orion_block* b, void* out, size_t n);
int orion_nco_next_cs_block_device(orion_block* b, void* out_dev, size_t n, void* stream);
/* dsp/decim.rs:24-37 FirDecimator::new(fs, m, cutoff_hz, trans_hz). cf32->cf32 */
orion_block* orion_fir_decimator_new(float fs, size_t m, float cutoff_hz, float trans_hz);
/* Batched FirDecimator: nch independent channels sharing one design. */
orion_block* orion_fir_decimator_batch_new(float fs, size_t m, float cutoff_hz, float trans_hz,
                                           size_t nch);
/* dsp/fir.rs:16-44 FirLowpass::design(fs, pass_hz, trans_hz); process :47-54. f32->f32 */
orion_block* orion_fir_lowpass_new(float fs, float pass_hz, float trans_hz);
/* dsp/fir.rs:186-188 FirLowpassIq::design(num_taps, cutoff_norm, stopband_db). cf32->cf32 */
orion_block* orion_fir_lowpass_iq_design(size_t num_taps, float cutoff_norm, float stopband_db);
/* dsp/fir.rs:193-204 FirLowpassIq::from_taps(taps) (empty -> [1.0]). */
orion_block* orion_fir_lowpass_iq_from_taps(const float* taps, size_t n);
/* Batched FirLowpassIq: nch independent channels sharing the taps (a channel filter in
 * front of a batched demodulator, BASELINE C5), [nch][n] in and out; filter_aligned is
 * single-channel only (ORION_E_ARG here). */
orion_block* orion_fir_lowpass_iq_batch_from_taps(const float* taps, size_t n, size_t nch);
/* dsp/fir.rs:210-212 FirLowpassIq::num_taps, :216-218 group_delay = (num_taps - 1) / 2.
 * ORION_E_TYPE if b is not a FirLowpassIq. */
int orion_fir_lowpass_iq_num_taps(const orion_block* b, size_t* num_taps);
int orion_fir_lowpass_iq_group_delay(const orion_block* b, size_t* group_delay);
/* dsp/fir.rs:260-276 FirLowpassIq::filter_aligned(io) on device memory (resets state). */
int orion_fir_lowpass_iq_filter_aligned_device(orion_block* b, void* io_dev, size_t n, void* stream);
/* Host-memory variant of filter_aligned (synchronous). */
int orion_fir_lowpass_iq_filter_aligned(orion_block* b, void* io, size_t n);
/* dsp/iir.rs:49-71 LpCascade::design(fs, fc) as a f32->f32 block (:79-83). */
orion_block* orion_lp_cascade_new(float fs, float fc);
/* dsp/iir.rs:15-41 Biquad::new(b0, b1, b2, a1, a2) (TDF-II, process :34-40) as an f32->f32
 * block; orion_block_reset = Biquad::reset. Any coefficients: a design whose state
 * decays within 8192 samples runs one pass, any other (a pole near the unit circle)
 * the three-kernel state-carry scan with f64 carries. */
orion_block* orion_biquad_new(float b0, float b1, float b2, float a1, float a2);
/* dsp/iir.rs:111-137 LpDcCascade::design(fs, lp_fc, dc_cut_hz); process :151-165 (LP4 then
 * the DC blocker). f32->f32 */
orion_block* orion_lp_dc_cascade_new(float fs, float lp_fc, float dc_cut_hz);
/* LpDcCascade::process_mapped(x, f) (iir.rs:170-186: f between the LP4 and the DC blocker)
 * instead of process (:151-165), for the maps a C caller can name: ORION_MAP_IDENTITY
 * (|v| v, the same as process), ORION_MAP_SQRT (f32::sqrt, the AM-PowerSqrt use,
 * demodulate/am.rs:55) or ORION_MAP_ABS (f32::abs). Set before the first call.
 * ORION_E_ARG for another value, ORION_E_TYPE for another block. */
#define ORION_MAP_IDENTITY 0
#define ORION_MAP_SQRT 1
#define ORION_MAP_ABS 2
int orion_lp_dc_cascade_set_map(orion_block* b, int map);
/* on = 1: orion_lp_dc_cascade_set_map(b, ORION_MAP_SQRT); on = 0: ORION_MAP_IDENTITY. */
int orion_lp_dc_cascade_set_sqrt_map(orion_block* b, int on);
/* dsp/dc.rs:15-21 DcBlocker::new(fs, cut_hz); Block impl :40-58. f32->f32 */
orion_block* orion_dc_blocker_new(float fs, float cut_hz);
/* demodulate/fm.rs:22-32 FmQuadratureDemod::new(fs, dev_hz, audio_bw_hz). cf32->f32 */
orion_block* orion_fm_quadrature_demod_new(float fs, float dev_hz, float audio_bw_hz);
/* demodulate/fm.rs:34-37 with_translate(freq_hz) (before the first process call). */
int orion_fm_quadrature_demod_with_translate(orion_block* b, float freq_hz);
/* demodulate/pm.rs:22-32 PmQuadratureDemod::new(fs, k, audio_bw_hz). cf32->f32 */
orion_block* orion_pm_quadrature_demod_new(float fs, float k, float audio_bw_hz);
/* demodulate/ssb.rs:15-20 SsbProductDemod::new(fs, bfo_hz, audio_bw_hz). cf32->f32 */
orion_block* orion_ssb_product_demod_new(float fs, float bfo_hz, float audio_bw_hz);
/* Batched SsbProductDemod: nch independent channels. */
orion_block* orion_ssb_product_demod_batch_new(float fs, float bfo_hz, float audio_bw_hz, size_t nch);
/* demodulate/am.rs:24-30 AmEnvelopeDemod::new(fs, audio_bw_hz). cf32->f32 */
orion_block* orion_am_envelope_demod_new(float fs, float audio_bw_hz);
/* demodulate/am.rs:33-36 with_abs_approx(k1, k2). */
int orion_am_envelope_demod_with_abs_approx(orion_block* b, float k1, float k2);
/* demodulate/cw.rs:15-25 CwEnvelopeDemod::new(fs, tone_hz, env_bw_hz); set_gain :26-28. */
orion_block* orion_cw_envelope_demod_new(float fs, float tone_hz, float env_bw_hz);
int orion_cw_envelope_demod_set_gain(orion_block* b, float g);

/* ---- analog modulators: f32 audio -> cf32 IQ ---- */
/* modulate/am.rs:20-30 AmDsbMod::new(fs, rf_hz, carrier_level, modulation_index);
 * set_gain :31-33, set_clamp :34-36 (ORION_E_TYPE on another block). */
orion_block* orion_am_dsb_mod_new(float fs, float rf_hz, float carrier_level, float modulation_index);
/* dsp/agc.rs:20-31 AgcRms::new(fs, attack_ms, release_ms, target_rms); process :48-75. f32->f32 */
orion_block* orion_agc_rms_new(float fs, float attack_ms, float release_ms, float target_rms);
/* dsp/agc.rs:93-106 AgcRmsIq::new(fs, attack_ms, release_ms, target_rms); process :124-150. cf32->cf32 */
orion_block* orion_agc_rms_iq_new(float fs, float attack_ms, float release_ms, float target_rms);
int orion_am_dsb_mod_set_gain(orion_block* b, float g);
int orion_am_dsb_mod_set_clamp(orion_block* b, int on);
/* modulate/fm.rs:21-32 FmPhaseAccumMod::new(sample_rate, deviation_hz, rf_hz);
 * set_deviation :33-35, set_gain :36-38. The running phase is summed on the device as
 * exact Q0.64 turn counts of the reference's own f32 step pairs (associative: any
 * summation order gives the same bits), then the reference's f32 recurrence is re-run
 * over each thread's 16 samples; the RF Nco is the reference's recurrence (tabulated). */
orion_block* orion_fm_phase_accum_mod_new(float fs, float deviation_hz, float rf_hz);
int orion_fm_phase_accum_mod_set_deviation(orion_block* b, float deviation_hz);
int orion_fm_phase_accum_mod_set_gain(orion_block* b, float g);
/* modulate/pm.rs:17-29 PmDirectPhaseMod::new(sample_rate, kp_rad_per_unit, rf_hz); set_gain,
 * set_sensitivity. process :36-47: (cos kp x, sin kp x) * gain, mixed with the RF Nco. */
orion_block* orion_pm_direct_phase_mod_new(float fs, float kp_rad_per_unit, float rf_hz);
int orion_pm_direct_phase_mod_set_gain(orion_block* b, float g);
int orion_pm_direct_phase_mod_set_sensitivity(orion_block* b, float kp_rad_per_unit);
/* modulate/cw.rs:21-41 CwKeyedMod::new(sample_rate, tone_hz, rise_ms, fall_ms); set_gain.
 * process :45-87: keying input clamped to [0, 1], rise/fall one-pole envelope, mixed with
 * the tone Nco. The envelope is a data-dependent recurrence: chunked warm-ups whose
 * exactness is checked bitwise, in-order re-runs where it fails (as AgcRms). */
orion_block* orion_cw_keyed_mod_new(float fs, float tone_hz, float rise_ms, float fall_ms);
int orion_cw_keyed_mod_set_gain(orion_block* b, float g);
/* modulate/ssb.rs:22-35 SsbPhasingMod::new(fs, audio_bw_hz, audio_if_hz, rf_hz, usb). */
orion_block* orion_ssb_phasing_mod_new(float fs, float audio_bw_hz, float audio_if_hz, float rf_hz, int usb);

/* The WBFM chain composed per docs/demodulate.md:128-133 (no single reference
 * type): Rotator(-f_off, fs) -> FirDecimator(fs, m, dec_cutoff, dec_trans) ->
 * FmQuadratureDemod(fs/m, dev_hz, audio_bw) -> FirLowpass(fs/m, audio_pass,
 * audio_trans). Any design the reference's constructors accept. cf32 -> f32 in one
 * gfx950 kernel per call for m = 8 with <= 128 decimator and audio taps and an
 * LpCascade that forgets within 896 outputs (the WBFM defaults): NCO + polyphase
 * decimation + discriminator + LpCascade + audio FIR, intermediates on chip; other
 * designs run the four blocks stage by stage (see configure). */
typedef struct {
  float fs, f_off, dec_cutoff, dec_trans, dev_hz, audio_bw, audio_pass, audio_trans;
  size_t m;
} orion_wbfm_params;
orion_block* orion_wbfm_chain_new(const orion_wbfm_params* p);
/* nch channels sharing the design, each with its own tuning offset f_off[ch]. */
orion_block* orion_wbfm_chain_batch_new(const orion_wbfm_params* p, const float* f_off, size_t nch);
/* Engine tuning and tests (no reference counterpart): the kernel path of a WBFM
 * chain handle, chosen before its first call. ORION_WBFM_AUTO picks the segmented
 * single kernel when the design allows it, else the two-kernel path when its
 * LpCascade warm-up suffices, else the four blocks (ORION_WBFM_GRAPH);
 * max_segments > 0 sets the segmented kernel's segments (waves; more than the
 * resident capacity runs several rounds), 0 = one round at the resident capacity.
 * ORION_E_TYPE if b is not a WBFM chain, ORION_E_ARG if the design cannot run on
 * that path.
 * Residency: the segmented kernel launches one round of waves (at most the
 * device's resident capacity) and each segment waits, bounded, for the end state
 * its predecessor publishes. A predecessor is always the previous workgroup in
 * dispatch order, so the wait ends even when other streams hold most CUs; a wait
 * that still outlasts its bound (~0.5 s) makes the handle report ORION_E_HIP (see
 * orion_block_status) instead of returning the audio as valid. */
#define ORION_WBFM_AUTO 0
#define ORION_WBFM_SEGMENTED 1  /* one kernel, one round of segments (k_wbfm_seg) */
#define ORION_WBFM_SPLIT 3      /* two kernels (front, back): m = 8, <= 128 taps, ||A^510|| < 1e-7 */
#define ORION_WBFM_GRAPH 4      /* Rotator, FirDecimator, FmQuadratureDemod, FirLowpass blocks: any design */
int orion_wbfm_chain_configure(orion_block* b, int path, int max_segments);
/* Time-sharded streams (no reference counterpart): the absolute
 * index of the next input sample, i.e. the NCO phase origin (rotator.rs:44-62
 * advances the phase once per sample from index 0). A shard of one stream is
 * processed by a fresh handle sought to its halo start, fed the halo and then
 * the shard (orion_sdr.stream_shard). A seek in the middle of a stream moves only the
 * NCO phase: the decimator, discriminator, IIR and FIR state carry on, on every path.
 * orion_block_reset on a chain returns to the last seek origin, not to index 0.
 * ORION_E_TYPE if b is not a WBFM chain. */
int orion_wbfm_chain_seek(orion_block* b, uint64_t index);

/* ---- Block contract (core.rs:12-22) ------------------------------------ */
/* Host buffers (synchronous): the path Block::process with host slices takes.
 * Pinned host memory (orion_host_alloc, or hipHostRegister'ed) moves by DMA directly;
 * pageable memory through the handle's pinned staging buffers, the CPU copy of one
 * chunk overlapping the DMA of the next. Blocks whose output does not depend on how a
 * call is cut (Rotator, Nco, FirLowpass, FirLowpassIq, FirDecimator at multiples of m,
 * the AM / PM / FM modulators, AgcRms(Iq), CwKeyedMod) run calls >= 2^21 samples as a
 * pipeline of chunks on three streams (H2D, kernel, D2H overlapped); the others upload,
 * run one device call and download. Either way the output equals one
 * orion_block_process_device call on the same input, bit for bit. */
int orion_block_process(orion_block* b, const void* in, size_t n_in, void* out, size_t out_cap,
                        orion_work_report* wr);
/* Device buffers (asynchronous on `stream`). Overlapping in/out ranges are
 * ORION_E_ARG, except for AgcRms / AgcRmsIq, which work in place (through an
 * internal copy of the input). */
int orion_block_process_device(orion_block* b, const void* in_dev, size_t n_in, void* out_dev,
                               size_t out_cap, void* stream, orion_work_report* wr);
/* The batched entry SURVEY §8(b) names (no reference counterpart: the reference runs one
 * channel per Block): n_ch channels of n_per_ch samples laid out [n_ch][n_per_ch] on the
 * device, outputs [n_ch][out_cap]; the handle must have been built for n_ch channels
 * (the *_batch_new constructors), else ORION_E_ARG. Equals orion_block_process_device
 * on the same buffers; wr reports per-channel counts. */
int orion_batch_process(orion_block* b, const void* in_dev, size_t n_ch, size_t n_per_ch, void* out_dev,
                        size_t out_cap, void* stream, orion_work_report* wr);
/* Device-side failures (no reference counterpart; the reference never fails on the
 * path, core.rs:12-22): kernels that wait on other workgroups (the WBFM segment
 * hand-off, the single-pass scans' decoupled look-back, FmPhaseAccumMod's phase
 * look-back) bound every wait and flag a timeout in the handle's host-visible
 * error word instead of hanging. orion_block_status returns ORION_E_HIP once if a
 * kernel of this handle flagged one since the last check (non-blocking; it sees
 * every kernel that has finished: orion_synchronize(stream) first to cover all).
 * orion_block_process checks after its own sync; orion_block_process_device
 * checks at entry, so an error of call k fails call k+1 at the latest. */
int orion_block_status(orion_block* b);
/* Test-only: polls a cross-workgroup wait makes before it times out (process-wide;
 * default 1 << 22; 0 makes every such wait time out at once). */
void orion_debug_set_spin_limit(uint32_t polls);
uint32_t orion_debug_spin_limit(void);
int orion_block_reset(orion_block* b);
void orion_block_free(orion_block* b);
int orion_block_in_type(const orion_block* b);
int orion_block_out_type(const orion_block* b);
size_t orion_block_out_len(const orion_block* b, size_t n_in);
size_t orion_block_channels(const orion_block* b);
const char* orion_block_name(const orion_block* b);
/* Engine options (no reference counterpart; tests and timing comparisons).
 * ORION_E_TYPE if the block has no such option, ORION_E_ARG for a bad value. */
#define ORION_OPT_SCAN_PATH 1   /* IIR-based blocks (LpCascade, DcBlocker, Biquad, LpDcCascade, the FM/PM/SSB/
                                   AM/CW demods): 0 single pass where the design allows (default), 1 the
                                   three-kernel scan */
#define ORION_OPT_MOD_PASSES 2  /* FmPhaseAccumMod, SsbPhasingMod: 0 single pass (default), 3 three passes */
#define ORION_OPT_NCO_TABLE 3   /* Rotator, Nco: outputs of the reference recurrence tabulated per (re)tune,
                                   0 .. 2^28 (default 2^20; 0 = the closed-form ideal phasor of the f32 step).
                                   The oscillator state carries on across the change. */
int orion_block_configure(orion_block* b, int option, long long value);
/* Designed coefficients, for parity tests: which = 0 primary taps, 1 audio taps.
 * AgcRms, AgcRmsIq, CwKeyedMod: which = 2 is a diagnostic of the last device call (waits for
 * the device): {its chunks, how many of them entered with an envelope that was not their
 * predecessor's recorded exit and were re-walked}. */
int orion_block_taps(const orion_block* b, int which, float* out, size_t cap, size_t* n);

/* ---- designs (host only; bit-exact with the reference constructors) ----- */
size_t orion_fir_lowpass_design(float fs, float pass_hz, float trans_hz, float* taps, size_t cap); /* fir.rs:16-44 */
size_t orion_kaiser_lowpass_taps(size_t num_taps, float cutoff_norm, float stopband_db, float* taps,
                                 size_t cap);                                                     /* fir.rs:113-141 */
float orion_kaiser_transition_norm(size_t num_taps, float stopband_db);                           /* fir.rs:147-150 */
size_t orion_kaiser_num_taps(float transition_norm, float stopband_db);                           /* fir.rs:154-157 */
void orion_lp_cascade_design(float fs, float fc, float out5[5]);                                  /* iir.rs:49-71 */

/* ---- multicarrier/tx_lowpass.rs:88-195 TxLowpass (the TX mask) ----
 * The spec and its host-side sizing helpers (the reference's f32 arithmetic); the
 * filter itself is FirLowpassIq::design(num_taps, cutoff_norm, stopband_db), applied
 * by filter_aligned (TxLowpass::apply = orion_tx_lowpass_filter +
 * orion_fir_lowpass_iq_filter_aligned[_device]). */
typedef struct {
  float cutoff_norm;
  size_t num_taps;
  float stopband_db;
} orion_tx_lowpass;
orion_tx_lowpass orion_tx_lowpass_for_null_band(size_t n_fft, size_t occupied_half, size_t num_taps,
                                                float stopband_db);                              /* :118-134 */
size_t orion_tx_lowpass_taps_for_null_band(size_t n_fft, size_t occupied_half, float stopband_db); /* :141-144 */
size_t orion_tx_lowpass_group_delay(const orion_tx_lowpass* t);                                  /* :148-150 */
float orion_tx_lowpass_transition_norm(const orion_tx_lowpass* t);                               /* :154-156 */
int orion_tx_lowpass_transition_fits(const orion_tx_lowpass* t, size_t n_fft, size_t occupied_half); /* :162-165 */
float orion_tx_lowpass_stopband_edge_norm(const orion_tx_lowpass* t);                            /* :171-173 */
int orion_tx_lowpass_fits_guard(const orion_tx_lowpass* t, size_t cp_len, size_t roll_off, size_t backoff); /* :179-182 */
orion_block* orion_tx_lowpass_filter(const orion_tx_lowpass* t);                                 /* :185-187 */

/* ---- FT8 / FT4 frame sync (src/sync; docs/demodulate.md:297-336) ----------------
 * The search half of the reference's digital side: a symbol-rate Goertzel waterfall, the
 * Costas candidate search and max-log LLRs, batched over nch independent channels
 * ([nch][n_per_ch] cf32, channel-major; nch = 1 is the reference's call). Every cell,
 * score and LLR is computed in the reference's f32 operation order: energies, scores,
 * candidate lists (ties included) and LLRs equal the reference's bit for bit on the same
 * waterfall; the waterfall's ln() is the device's (within 2 ulp of libm's).
 * A sync handle owns what calls reuse (step table, scratch waterfall, score map) and is
 * not a Block: there is no streaming state. One call at a time per handle.
 * Limits (ORION_E_ARG beyond them): nch <= 65535, num_syms <= 65535, num_tones <= 2^20,
 * nch * num_syms * num_tones < 2^31, max_cand <= 65536.
 *
 * Streams and the digital handles (orion_sync, orion_ft_mod, the orion_psk31_*, orion_fft,
 * orion_ofdm, orion_ofdm_acquire): a handle keeps two kinds of device memory.
 * - Its tables (step phasors, windows, rotator phasors, twiddles, the OFDM grid and equalizer
 *   coefficients) may be replaced by a call, a setter or a reset whatever streams the handle's
 *   earlier calls used: replacing a table waits for the device first.
 * - Its scratch (a sync's waterfall and score map, a search's run lists, staging) is shared
 *   by its calls: calls that use it are ordered by the caller, on one stream or with events.
 * The *_device entries are asynchronous on their stream except while a table is uploaded
 * (a handle's first call and every replacement; a replacement waits for the whole device),
 * while a buffer grows, or while the previous call's plan is still in use (the synthesisers
 * and modulators, whose plan is built on the host: a call waits for the handle's previous
 * launch). The entries that take host memory are synchronous and return with the result in
 * place. The slot synthesisers without a
 * handle (orion_ft_synth_*, orion_psk31_synth_*) share one plan per device: one call at a
 * time, process-wide. */
typedef struct orion_sync orion_sync;
typedef struct {
  int32_t time_sym;  /* costas.rs:29-36 Candidate (freq_bin: usize there) */
  uint32_t freq_bin;
  float score;
} orion_candidate;
#define ORION_SYNC_LLR 174  /* codec/ldpc.rs N: LLRs per candidate */
#define ORION_WF_LOG 0      /* ln(e + 1e-12), waterfall.rs:114 */
#define ORION_WF_ENERGY 1   /* e itself (goertzel_energy, waterfall.rs:126-151): bit-exact with the reference */
#define ORION_COSTAS_FT8 0  /* [3,1,4,0,6,5,2] at frame symbols 0, 36, 72 (ft8_sync.rs:44-45) */
#define ORION_COSTAS_FT4 1  /* four 4-tone patterns at 1, 34, 67, 100 (ft4_sync.rs:44-47) */
orion_sync* orion_sync_new(void);
void orion_sync_free(orion_sync* h);
/* Engine tuning (no reference counterpart): symbol rows per lane of the waterfall kernel,
 * 1, 2, 4 or 8; 0 (default) picks per call. Results do not depend on it. */
int orion_sync_set_rows_per_lane(orion_sync* h, int rows);
/* compute_waterfall, waterfall.rs:73-119. mag: [nch][num_syms][num_tones] f32. A row
 * that starts at or past the end of the buffer stays 0.0 (in both modes); a row the
 * buffer ends inside uses the samples it has; time_offset is any sample offset. */
int orion_waterfall_compute(orion_sync* h, const void* iq, float fs, float base_hz, float tone_spacing_hz,
                            size_t samples_per_sym, size_t num_syms, size_t num_tones, size_t time_offset,
                            size_t nch, size_t n_per_ch, int mode, float* mag);
int orion_waterfall_compute_device(orion_sync* h, const void* iq, float fs, float base_hz, float tone_spacing_hz,
                                   size_t samples_per_sym, size_t num_syms, size_t num_tones, size_t time_offset,
                                   size_t nch, size_t n_per_ch, int mode, float* mag, void* stream);
/* find_candidates, costas.rs:125-174 (ORION_COSTAS_FT8) / find_ft4_candidates,
 * ft4_sync.rs:122-163 (ORION_COSTAS_FT4) on a device waterfall [nch][num_syms][num_tones]:
 * time_sym in t_min ..= t_max. cand: [nch][max_cand] records, best first, in the
 * reference's order among equal scores; count: [nch] (slots past it are zeroed; 0 when
 * num_tones <= the frame's tones). max_cand == 0 is ORION_E_ARG (the reference indexes an
 * empty heap, costas.rs:159). */
int orion_costas_find_candidates_device(orion_sync* h, const float* wf, size_t nch, size_t num_syms,
                                        size_t num_tones, int pattern, int t_min, int t_max, size_t max_cand,
                                        orion_candidate* cand, uint32_t* count, void* stream);
/* extract_ft8_llr + normalise_llr, ft8_sync.rs:170-246 (extract_ft4_llr, ft4_sync.rs:227-292)
 * for the first count[ch] candidates of each channel, on a device waterfall.
 * llr: [nch][max_cand][ORION_SYNC_LLR] f32 (unused slots zeroed). */
int orion_sync_llr_device(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern,
                          const orion_candidate* cand, const uint32_t* count, size_t max_cand, float* llr,
                          void* stream);
/* ft8_sync, ft8_sync.rs:90-159, and ft4_sync, ft4_sync.rs:65-117: waterfall -> search ->
 * LLRs, with the reference's num_bins, wf_syms, wf_sample_start and sym_offset_adj
 * (ft8_sync.rs:99-131). cand [nch][max_cand] (time_sym relative to the buffer, as the
 * reference returns it), count [nch], llr [nch][max_cand][ORION_SYNC_LLR]. Host slices
 * (uploaded, one device call, downloaded; synchronous) or device buffers on a stream. */
int orion_ft8_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                   int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr);
int orion_ft8_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                          float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand,
                          uint32_t* count, float* llr, void* stream);
int orion_ft4_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                   int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr);
int orion_ft4_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                          float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand,
                          uint32_t* count, float* llr, void* stream);
/* The geometry orion_ft8_sync / orion_ft4_sync derive (ft8_sync.rs:99-131), host only:
 * geom[5] = num_bins, wf_syms, wf_sample_start, sym_offset_adj, wf_t_max. */
int orion_sync_geometry(int pattern, float base_hz, float max_hz, int t_min, int t_max, size_t geom[5]);

/* ---- FT8 / FT4 channel codec: LDPC(174,91) + CRC-14 (src/codec) -------------------
 * The decode half of the receive path: 174 LLRs (positive: the bit is more likely 0) ->
 * belief propagation (ldpc_decode_soft, ldpc.rs:673-757) -> CRC-14 over the 77-bit payload
 * (ft8.rs:91-130, ft4.rs:91-127). protocol: ORION_COSTAS_FT8 / ORION_COSTAS_FT4 (FT4
 * un-XORs the payload, ft4.rs:22).
 * rule: ORION_LDPC_RULE_REFERENCE is the reference's arithmetic bit for bit, plain word,
 * error count and iterations included. Its check -> bit message has the wrong sign for a
 * check with 7 entries (24 of the 83), so it does not correct errors: it decodes a word
 * whose initial hard decision is already valid. ORION_LDPC_RULE_SUM_PRODUCT differs in
 * that one constant (+2 atanh(a) for those checks) and does correct errors. DESIGN.md 8.1.
 * max_iter <= 255; 20 is the reference's. A bad protocol, rule or max_iter: ORION_E_ARG. */
#define ORION_LDPC_N 174
#define ORION_LDPC_RULE_REFERENCE 0
#define ORION_LDPC_RULE_SUM_PRODUCT 1
#define ORION_LDPC_PARITY_FAILED 0 /* status: unsatisfied checks remain */
#define ORION_LDPC_CRC_MISMATCH 1  /* all checks satisfied, the CRC is not */
#define ORION_LDPC_DECODED 2
typedef struct {
  uint8_t payload[10]; /* status 2: the 77 bits MSB first, byte 9 & 0xF8; else zeros */
  uint8_t status;
  uint8_t iterations;  /* 0: the initial decision was valid (or max_iter == 0); else iterations started */
  uint16_t errors;     /* unsatisfied checks of the best word */
  uint16_t pad;
} orion_ldpc_result;
/* Each channel's pick, as Ft8StreamDecoder::decode_buf makes it (ft8.rs:302-320). */
typedef struct {
  int32_t first_ok;  /* index of the first candidate with status 2, or -1 */
  float carrier_hz;  /* base_hz + freq_bin * tone spacing in f32; 0 when first_ok < 0 */
  float snr_db;      /* that candidate's score */
  uint32_t pad;
} orion_decode_pick;
/* n codewords, llr [n][174] -> results [n], plain [n][174] (the best hard decision; may be
 * NULL). count non-NULL: llr is the [nch][max_cand][174] layout of orion_ft*_sync with
 * n = nch * max_cand, and slots at or past count[ch] give all-zero records (and plain)
 * without being decoded; count NULL: max_cand is ignored. One kernel, one wave64
 * workgroup per codeword. Host slices (synchronous) / device buffers (asynchronous). */
int orion_ldpc_decode(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                      size_t max_iter, orion_ldpc_result* results, uint8_t* plain);
int orion_ldpc_decode_device(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                             size_t max_iter, orion_ldpc_result* results, uint8_t* plain, void* stream);
/* orion_ft*_sync, then the decode of every candidate and each channel's pick, on one
 * stream with no host round trip. cand, count, llr as orion_ft*_sync writes them (llr may
 * be NULL in the host-slice calls); results [nch][max_cand]; pick [nch]. */
int orion_ft8_decode(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                     uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick);
int orion_ft8_decode_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter,
                            orion_candidate* cand, uint32_t* count, float* llr, orion_ldpc_result* results,
                            orion_decode_pick* pick, void* stream);
int orion_ft4_decode(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                     uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick);
int orion_ft4_decode_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter,
                            orion_candidate* cand, uint32_t* count, float* llr, orion_ldpc_result* results,
                            orion_decode_pick* pick, void* stream);
/* Host only (no device is touched). */
/* Ft8Codec::encode, ft8.rs:29-59: tones[58]; Ft4Codec::encode, ft4.rs:29-65: tones[87].
 * a91_xor (12 bytes, may be NULL) is XORed into the 91-bit block after the CRC is
 * appended: test frames whose parity passes and whose CRC does not. */
int orion_ft8_encode(const uint8_t payload[10], uint8_t tones[58], const uint8_t* a91_xor);
int orion_ft4_encode(const uint8_t payload[10], uint8_t tones[87], const uint8_t* a91_xor);
/* frame_to_llr_hard, ft8.rs:79-89 / ft4.rs:79-89: +-10 per bit. */
int orion_ft_frame_to_llr_hard(int protocol, const uint8_t* tones, float llr[174]);
/* The scalar decoder the device kernel is held to: one codeword, same record. plain may be NULL. */
int orion_ldpc_decode_host(const float llr[174], int protocol, int rule, size_t max_iter, orion_ldpc_result* result,
                           uint8_t* plain);
/* ft8_crc14, crc.rs:37-54, over the first num_bits bits of message (MSB first). */
uint16_t orion_ft_crc14(const uint8_t* message, size_t num_bits);
/* The code's tables: the edge list as stated (edges [522][2]: check, bit; 0-based) and what
 * is derived from it: row_start [84], bit_check [174][3] (ascending), generator [83][12]
 * (rows bit-packed MSB first). Any pointer may be NULL. */
int orion_ldpc_tables(uint8_t* edges, uint16_t* row_start, uint8_t* bit_check, uint8_t* generator);

/* ---- FT8 / FT4 modulators, slot synthesis and hard demodulators -------------------
 * protocol: ORION_COSTAS_FT8 / ORION_COSTAS_FT4. A frame is 79 x 1920 = 151680 (FT8) or
 * 105 x 576 = 60480 (FT4) cf32 samples; data tones are uint8 [58] (< 8) or [87] (< 4).
 * The device modulator generates the closed form of the reference's own f32 tone steps
 * (each step's exact angle as a Q0.64 turn count, phases as wrapping integer sums): it
 * follows the reference's phasor recurrence to its rounding drift (1e-4 over a frame,
 * DESIGN.md 3.3), not bit for bit; orion_ft_mod_host is the recurrence itself. The
 * demodulator's energies and tones are the reference's bit for bit.
 * Errors: ORION_E_ARG for an unknown protocol, a tone out of range, n_per_frame below the
 * frame length or a signal's channel >= nch; ORION_E_NULL for a null pointer. */
#define ORION_FT8_FRAME_LEN 151680
#define ORION_FT4_FRAME_LEN 60480
typedef struct orion_ft_mod orion_ft_mod;
/* Ft8Mod::new / Ft4Mod::new, modulate/ft8.rs:55-62, ft4.rs:58-65. No device is touched here.
 * rf_hz != 0: the phasors of a fresh Rotator(rf_hz, fs) over one frame (ft8.rs:150-153) are
 * tabulated once, by the handle's first modulate call. */
orion_ft_mod* orion_ft_mod_new(int protocol, float fs, float base_hz, float rf_hz, float gain);
void orion_ft_mod_free(orion_ft_mod* h);
/* Ft8Mod::modulate, ft8.rs:88-156 / Ft4Mod::modulate, ft4.rs:106-173, of nframes frames:
 * tones [nframes][58 | 87] (host memory in both calls) -> iq [nframes][frame_len] cf32,
 * host memory (synchronous) / device memory (launched on stream). */
int orion_ft_mod_modulate(orion_ft_mod* h, const uint8_t* tones, size_t nframes, void* iq);
int orion_ft_mod_modulate_device(orion_ft_mod* h, const uint8_t* tones, size_t nframes, void* iq, void* stream);
/* The same frame by the reference's scalar recurrence (ft8.rs:94-153), bit for bit. Host
 * only: no device is touched. iq [frame_len] cf32. */
int orion_ft_mod_host(int protocol, float fs, float base_hz, float rf_hz, float gain, const uint8_t* tones, void* iq);
/* build_symbol_sequence, ft8.rs:65-85 / ft4.rs:73-103: syms [79 | 105]. Host only. */
int orion_ft_symbol_sequence(int protocol, const uint8_t* tones, uint8_t* syms);
/* What the device modulator is built from (host only; any output may be NULL): w [8 | 4][2]
 * the f32 step phasors (ft8.rs:98-101), step [8 | 4] their angles as Q0.64 turns, enter
 * [79 | 105] the phase entering each symbol of the frame with these data tones. */
int orion_ft_mod_tables(int protocol, float fs, float base_hz, const uint8_t* tones, float* w, uint64_t* step,
                        uint64_t* enter);
/* Slot synthesis: iq [nch][n_per_ch] cf32 = (accumulate ? iq : 0) + every signal's frame
 * (what orion_ft_mod_modulate gives at fs, the signal's base_hz and gain, rf_hz 0) placed
 * at its offset in its channel, clipped to the channel; the signals of a channel are summed
 * in list order with plain f32 adds, so a call is bit-reproducible. signals [nsig] and tones
 * [nsig][58 | 87] are host memory in both calls. */
typedef struct {
  uint32_t channel;
  uint32_t pad;
  int64_t offset; /* the channel sample at which the frame starts; may be negative */
  float base_hz;
  float gain;
} orion_ft_signal;
int orion_ft_synth(int protocol, float fs, const orion_ft_signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                   size_t n_per_ch, int accumulate, void* iq);
int orion_ft_synth_device(int protocol, float fs, const orion_ft_signal* signals, const uint8_t* tones, size_t nsig,
                          size_t nch, size_t n_per_ch, int accumulate, void* iq, void* stream);
/* Ft8Demod::demodulate, demodulate/ft8.rs:33-126 / Ft4Demod::demodulate, ft4.rs:35-74, of
 * nframes rows of n_per_frame >= frame_len samples (the first frame_len of a row are
 * read): tones [nframes][58 | 87]; energies (may be NULL) [nframes][79 | 105][8 | 4], every
 * correlator energy of detect_tone (ft8.rs:74-126). nframes <= 65535 (ORION_E_ARG above).
 * Host slices / device buffers. */
int orion_ft_demod(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                   uint8_t* tones, float* energies);
int orion_ft_demod_device(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                          uint8_t* tones, float* energies, void* stream);
/* The scalar demodulator the kernel is held to, one frame (iq: >= frame_len samples). Host only. */
int orion_ft_demod_host(int protocol, float fs, float base_hz, const void* iq, uint8_t* tones, float* energies);

/* ---- PSK31 channel code: Varicode and QPSK31's rate 1/2, K = 5 code (src/codec) ---
 * Bits are uint8, one per byte, 0 or 1 (only bit 0 of an input byte is read). Everything
 * in this section but orion_psk31_viterbi and orion_psk31_viterbi_device is host only: no
 * device is touched. Errors: ORION_E_NULL for a null pointer or handle, ORION_E_ARG for a
 * count above its limit or an output capacity below what the call produces. */
#define ORION_VARICODE_MAX_BITS 10    /* codec/varicode.rs:20 */
#define ORION_PSK31_TRACEBACK_DEPTH 32 /* codec/psk31.rs:267 */
/* The tables as the library holds them (any pointer may be NULL): the Varicode alphabet
 * (varicode.rs:27-156) as codewords [128], MSB first, and their lengths [128]; DQPSK_EXP
 * (psk31.rs:80-85) as dqpsk_exp [4][2]. */
int orion_psk31_tables(uint16_t* varicode_bits, uint8_t* varicode_len, float* dqpsk_exp);
/* varicode_encode, varicode.rs:163-169 (a byte >= 128 gives the NUL entry), and
 * varicode_decode, varicode.rs:176-183: the byte, or -1 for a codeword not in the table. */
int orion_varicode_encode(uint8_t byte, uint16_t* bits, uint8_t* len);
int orion_varicode_decode(uint16_t bits, uint8_t len);
/* VaricodeEncoder, varicode.rs:192-267. push_preamble leaves the next byte without a "00"
 * gap of its own (varicode.rs:216-223). pending: the bits queued; drain copies and removes
 * them all (cap below pending: ORION_E_ARG, nothing removed). */
typedef struct orion_varicode_encoder orion_varicode_encoder;
orion_varicode_encoder* orion_varicode_encoder_new(void);
void orion_varicode_encoder_free(orion_varicode_encoder* e);
int orion_varicode_encoder_push_preamble(orion_varicode_encoder* e, size_t n_bits);
int orion_varicode_encoder_push_byte(orion_varicode_encoder* e, uint8_t byte);
int orion_varicode_encoder_push_postamble(orion_varicode_encoder* e, size_t n_bits);
size_t orion_varicode_encoder_pending(const orion_varicode_encoder* e);
int orion_varicode_encoder_drain(orion_varicode_encoder* e, uint8_t* bits, size_t cap, size_t* n_bits);
/* VaricodeDecoder, varicode.rs:277-320 (its length counter stops at ORION_VARICODE_MAX_BITS
 * + 1). push_bits feeds n bits; pending: the characters decoded and not yet popped;
 * pop_bytes copies and removes them all (cap below pending: ORION_E_ARG, nothing removed). */
typedef struct orion_varicode_decoder orion_varicode_decoder;
orion_varicode_decoder* orion_varicode_decoder_new(void);
void orion_varicode_decoder_free(orion_varicode_decoder* d);
int orion_varicode_decoder_push_bits(orion_varicode_decoder* d, const uint8_t* bits, size_t n);
size_t orion_varicode_decoder_pending(const orion_varicode_decoder* d);
int orion_varicode_decoder_pop_bytes(orion_varicode_decoder* d, uint8_t* bytes, size_t cap, size_t* n_bytes);
/* conv_encode, psk31.rs:45-55: bits [n] -> coded [2 n], (g0, g1) per bit, G0 = 25, G1 = 23
 * octal, from a zero register. */
int orion_conv_encode(const uint8_t* bits, size_t n, uint8_t* coded);
/* viterbi_decode, psk31.rs:95-160, of nstreams streams in one launch: soft [nstreams][2 *
 * n_syms] f32 (re, im of each differential symbol) -> bits [nstreams][n_syms]. Sixteen lanes
 * per stream, four streams per wave; the bits are those of orion_psk31_viterbi_host for every
 * input (the start metric f32::MAX / 2, the skip of predecessors at it, strict < on the
 * second predecessor, the first minimum at the end). NaN input is outside the contract; it
 * neither faults nor hangs. nstreams <= 2^31 - 4, n_syms <= 2^31 - 1 (ORION_E_ARG above).
 * Host slices (uploaded, one launch, downloaded; synchronous) or device buffers on a stream;
 * the device call needs work, device memory of at least orion_psk31_viterbi_work_bytes
 * (nstreams, n_syms) bytes (4 bytes per stream, rounded up to 4 streams, and symbol), which
 * it may overwrite wholly. */
int orion_psk31_viterbi(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits);
int orion_psk31_viterbi_device(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits, void* work,
                               size_t work_bytes, void* stream);
size_t orion_psk31_viterbi_work_bytes(size_t nstreams, size_t n_syms);
/* The scalar decoder the kernel is held to, one stream: soft [2 n_syms] -> bits [n_syms];
 * and viterbi_decode_hard, psk31.rs:384-396: coded [2 n_syms] bits -> bits [n_syms]. */
int orion_psk31_viterbi_host(const float* soft, size_t n_syms, uint8_t* bits);
int orion_psk31_viterbi_hard_host(const uint8_t* coded, size_t n_syms, uint8_t* bits);
/* StreamingViterbi, psk31.rs:257-377, on DQPSK_EXP: feed takes n_syms symbols (soft [2
 * n_syms]) and writes the bits that come out, none for the first 32 symbols of a decoder
 * and one per symbol after (bits holds n_syms); flush feeds 32 (0, 0) symbols (bits holds
 * 32). *n_bits: how many were written. */
typedef struct orion_psk31_streaming_viterbi orion_psk31_streaming_viterbi;
orion_psk31_streaming_viterbi* orion_psk31_streaming_viterbi_new(void);
void orion_psk31_streaming_viterbi_free(orion_psk31_streaming_viterbi* v);
int orion_psk31_streaming_viterbi_feed(orion_psk31_streaming_viterbi* v, const float* soft, size_t n_syms,
                                       uint8_t* bits, size_t* n_bits);
int orion_psk31_streaming_viterbi_flush(orion_psk31_streaming_viterbi* v, uint8_t* bits, size_t* n_bits);

/* ---- PSK31 modulators and demodulators (src/modulate/psk31.rs, src/demodulate/psk31.rs)
 * 31.25 baud; a symbol is round(fs / 31.25) samples (psk31_sps, modulate/psk31.rs:42-44: 256
 * at 8 kHz, 384 at 12 kHz; 0 or above 2^24: ORION_E_ARG). mode: ORION_PSK31_BPSK /
 * ORION_PSK31_QPSK, another value is ORION_E_ARG. The scalar modulators and demodulators
 * of this section run on the host, in the reference's f32 operation order (glibc sinf /
 * cosf); the demodulator bank is the device path. */
#define ORION_PSK31_BPSK 0
#define ORION_PSK31_QPSK 1
size_t orion_psk31_sps(float fs);
/* The bits modulate_text sends (modulate/psk31.rs:146-159): preamble zeros, the Varicode of
 * the bytes, "00" and postamble ones. cap below the count: ORION_E_ARG with *n_bits set to
 * the count (bits may then be NULL: a size query). */
int orion_psk31_text_bits(const uint8_t* text, size_t n, size_t preamble_bits, size_t postamble_bits, uint8_t* bits,
                          size_t cap, size_t* n_bits);
/* Bpsk31Mod, modulate/psk31.rs:110-216 (bit 0 flips the phase: only a zero byte is a 0), and
 * Qpsk31Mod, :248-362 (the coder's register and the phasor are kept between calls; the
 * phasor is the f32 pair the reference's products give, -0.0 included). Host only.
 * modulate_bits: bits [n] -> iq [n * sps] cf32; with rf_hz != 0 a fresh Rotator runs over
 * each call's output (:186-189). */
typedef struct orion_psk31_mod orion_psk31_mod;
orion_psk31_mod* orion_psk31_mod_new(int mode, float fs, float rf_hz, float gain);
void orion_psk31_mod_free(orion_psk31_mod* m);
int orion_psk31_mod_set_gain(orion_psk31_mod* m, float gain);
int orion_psk31_mod_reset(orion_psk31_mod* m);
int orion_psk31_mod_modulate_bits(orion_psk31_mod* m, const uint8_t* bits, size_t n, void* iq);
/* The device modulator (k_psk31_mod, one lane per output sample): the symbol phasors are
 * built on the host with the reference's arithmetic, the Hann cross-fade and the RF stage
 * (the phasors of a fresh Rotator, tabulated from the reference's own recurrence and kept on
 * the device) run in the kernel, operation for operation as the host modulator: the output
 * equals orion_psk31_mod_modulate_bits byte for byte at any length. bits are host memory.
 * _bits_device: one stream from the handle's state, which advances; iq [n * sps] device.
 * _batch / _batch_device: nstreams independent streams bits [nstreams][n], each from a fresh
 * modulator of the handle's parameters (the handle's state is not touched) -> iq [nstreams]
 * [n * sps], host memory (synchronous) / device memory. nstreams <= 2^24. */
int orion_psk31_mod_modulate_bits_device(orion_psk31_mod* m, const uint8_t* bits, size_t n, void* iq, void* stream);
int orion_psk31_mod_modulate_batch(orion_psk31_mod* m, const uint8_t* bits, size_t nstreams, size_t n, void* iq);
int orion_psk31_mod_modulate_batch_device(orion_psk31_mod* m, const uint8_t* bits, size_t nstreams, size_t n, void* iq,
                                          void* stream);
/* Band synthesis (k_psk31_synth; no reference counterpart): iq [nch][n_per_ch] cf32 =
 * (accumulate ? iq : 0) + every signal, what a fresh Bpsk31Mod / Qpsk31Mod(fs, rf_hz, gain)
 * gives for its bits, placed at its offset in its channel and clipped to the channel; the
 * signals of a channel are summed in list order with plain f32 adds, so a call is
 * bit-reproducible. The RF stage is the closed form of the Rotator's f32 step (its angle as
 * a Q0.64 turn count, orion_psk31_rotator_q64): it follows the reference's recurrence to its
 * rounding drift, 2 d0 + 2e-6 per unit gain with d0 the distance between the recurrence and
 * that closed form, not bit for bit; with rf_hz == 0 a signal is the host
 * modulator's bytes. signals [nsig] and bits (signal k's n_bits bits follow signal k - 1's)
 * are host memory in both calls. ORION_E_ARG: channel >= nch, an unknown mode, nsig > 2^24. */
typedef struct {
  uint32_t channel;
  uint32_t mode;   /* ORION_PSK31_BPSK / ORION_PSK31_QPSK */
  int64_t offset;  /* the channel sample at which the signal starts; may be negative */
  float rf_hz;
  float gain;
  uint64_t n_bits;
} orion_psk31_signal;
int orion_psk31_synth(float fs, const orion_psk31_signal* signals, const uint8_t* bits, size_t nsig, size_t nch,
                      size_t n_per_ch, int accumulate, void* iq);
int orion_psk31_synth_device(float fs, const orion_psk31_signal* signals, const uint8_t* bits, size_t nsig, size_t nch,
                             size_t n_per_ch, int accumulate, void* iq, void* stream);
/* The angle of Rotator(freq_hz, fs)'s f32 step phasor as a Q0.64 fraction of a turn. Host only. */
uint64_t orion_psk31_rotator_q64(float freq_hz, float fs);
/* Block::process, :199-215: min(n_bits, out_cap / sps) bits are read. */
int orion_psk31_mod_process(orion_psk31_mod* m, const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap,
                            orion_work_report* report);
/* Bpsk31Demod, demodulate/psk31.rs:83-220 (offset: new_with_offset, :104-130), and
 * Qpsk31Demod, :271-397, on the host: the scalar demodulators the bank is held to. BPSK
 * writes one soft value per symbol and stops when out_written == out_cap; QPSK writes (re,
 * im) of the differential product and stops when out_written + 1 >= out_cap. */
typedef struct orion_psk31_demod orion_psk31_demod;
orion_psk31_demod* orion_psk31_demod_new(int mode, float fs, float rf_hz, float gain, size_t offset);
void orion_psk31_demod_free(orion_psk31_demod* d);
int orion_psk31_demod_set_gain(orion_psk31_demod* d, float gain);
int orion_psk31_demod_reset(orion_psk31_demod* d);
int orion_psk31_demod_process(orion_psk31_demod* d, const void* iq, size_t n, float* soft, size_t out_cap,
                              orion_work_report* report);
/* Bpsk31Decider, demodulate/psk31.rs:236-261: bits[i] = soft[i] >= 0. Host only. */
int orion_bpsk31_decide(const float* soft, size_t n, uint8_t* bits);
/* What a bank stream (below) or a sync candidate read and wrote in a call. */
typedef struct {
  uint64_t in_read;
  uint64_t out_written;
} orion_psk31_report;
/* The carrier search of psk31_sync (sync/psk31_sync.rs:82-203) on the host, over log
 * waterfalls given to it: wf [nch][num_syms][num_bins] as orion_waterfall_compute writes it
 * with ORION_WF_LOG, one bin per 31.25 Hz. Per bin the median over time, per channel the
 * median of those (median_f32: even counts average the two middle values); ln_margin =
 * peak_margin_db * LN_2 / 3; a symbol is a peak when (e > bin_median + ln_margin ||
 * bin_median > noise_floor + ln_margin) && e >= e_left && e >= e_right; runs of at least
 * max(min_carrier_syms, 1) peaks count, a run that reaches the end of the buffer included;
 * score = run_energy_sum / run_len. cand [nch][max_cand] (time_sym the run's first symbol;
 * unused slots zeroed), count [nch]: the max_cand best runs per channel, score descending.
 * The reference sorts with sort_unstable_by on the score alone, which leaves the order of
 * runs of equal score open; here it is defined: equal scores are ordered by freq_bin, then
 * time_sym, both ascending, one of the orders the reference may produce.
 * max_cand == 0 is ORION_E_ARG, as for the FT entries; nch * num_syms * num_bins < 2^31. */
int orion_psk31_find_carriers_host(const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                                   size_t min_carrier_syms, float peak_margin_db, size_t max_cand,
                                   orion_candidate* cand, uint32_t* count);
/* The same search on the device, on the orion_sync handle (which owns its scratch): four
 * small kernels (medians over time by exact selection, each channel's noise floor, one
 * serial scan per channel and bin with the f32 run sum in symbol order, a merge of the bins'
 * lists); no list is appended to in arrival order, so the output does not depend on
 * scheduling and equals orion_psk31_find_carriers_host on the same waterfall, order and
 * scores included. Host slices (uploaded, run, downloaded; synchronous) / device buffers on
 * a stream. Limits (ORION_E_ARG): those of the host entry, nch * num_bins * max_cand <= 2^26,
 * num_bins * max_cand <= 2^22. */
int orion_psk31_find_carriers(orion_sync* h, const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                              size_t min_carrier_syms, float peak_margin_db, size_t max_cand, orion_candidate* cand,
                              uint32_t* count);
int orion_psk31_find_carriers_device(orion_sync* h, const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                                     size_t min_carrier_syms, float peak_margin_db, size_t max_cand,
                                     orion_candidate* cand, uint32_t* count, void* stream);
/* psk31_sync, sync/psk31_sync.rs:50-239, batched over channels, all on the device with no
 * trip to the host between its stages: iq [nch][n_per_ch] cf32 -> the waterfall (one bin per
 * 31.25 Hz from base_hz, round(fs / 31.25) samples per symbol, n_per_ch / sps symbols) -> the
 * search above -> for every kept candidate a BPSK31 stream as record_candidate starts it
 * (:209-239: carrier base_hz + f32(freq_bin) * 31.25, from sample time_sym * sps, gain 1,
 * capacity n_bits + 2), written as bank records on the device and demodulated by one launch
 * of the demodulator bank. cand [nch][max_cand], count [nch]; soft [nch][max_cand][n_bits +
 * 2] f32 (zeroed first), reports [nch][max_cand] {in_read, out_written}: the reference keeps
 * the first min(out_written, n_bits) values of a candidate. A buffer under one symbol gives
 * count 0. The soft values follow the host demodulator's as the bank's do.
 * Limits as above, n_bits <= 2^30 - 2, nch * max_cand * (n_bits + 2) <= 2^32. */
int orion_psk31_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand,
                     orion_candidate* cand, uint32_t* count, float* soft, orion_psk31_report* reports);
int orion_psk31_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand,
                            orion_candidate* cand, uint32_t* count, float* soft, orion_psk31_report* reports,
                            void* stream);
/* psk31_sync's bin count, psk31_sync.rs:70-71: ceil(max(max_hz - base_hz, 0) / 31.25) + 1;
 * 0 when the range is above 2^24 bins. */
size_t orion_psk31_sync_num_bins(float base_hz, float max_hz);
/* The demodulator bank: nstreams independent demodulators over nch channels, all advanced
 * by one kernel launch per call, one lane per stream (a stream is one serial chain in time:
 * every sample's correction uses the previous symbol's decision-feedback sum). Each call
 * takes iq [nch][n] cf32, the next n samples of every channel. A stream reads its channel
 * from the channel sample `start` on (counted from the bank's first call or last reset),
 * with the symbol clock of new_with_offset(.., offset), and writes at most out_cap soft
 * values per call (the reference's output.len(): BPSK stops at out_cap, QPSK when fewer
 * than two slots are left); a stream that stops early has in_read < the samples offered,
 * and the next call still brings every stream its channel's next samples.
 * soft [nstreams][out_stride] f32 with out_stride >= every out_cap; bits (may be NULL) the
 * same shape: for a BPSK31 stream bits = soft >= 0 (Bpsk31Decider); the rows of QPSK31
 * streams are not written (a pair's quadrature component is noise about zero, and QPSK31's
 * decisions are the Viterbi decoder's: orion_psk31_viterbi on the soft pairs); reports
 * [nstreams] {in_read, out_written} of this call.
 * State is carried between calls, so chunked calls give one call's bytes. Against the host
 * demodulator the soft values agree to a few ulp, not bit for bit: phase_acc's sine and
 * cosine are glibc's there and a correctly-rounded-but-for-near-ties pair here (DESIGN.md
 * 3.3). Limits (ORION_E_ARG): nch <= 65535, nstreams <= 2^24, out_cap <= 2^30, channel < nch. */
typedef struct {
  uint32_t mode;    /* ORION_PSK31_BPSK / ORION_PSK31_QPSK */
  uint32_t channel;
  float rf_hz;      /* the carrier to mix down from; 0: no rotator at all */
  float gain;
  uint64_t start;   /* first channel sample the stream reads */
  uint32_t offset;  /* new_with_offset's offset */
  uint32_t out_cap; /* soft values per call */
} orion_psk31_stream;
typedef struct orion_psk31_demod_bank orion_psk31_demod_bank;
/* No device is touched here: the bank's tables are uploaded by its first process call. */
orion_psk31_demod_bank* orion_psk31_demod_bank_new(float fs, const orion_psk31_stream* streams, size_t nstreams,
                                                   size_t nch);
void orion_psk31_demod_bank_free(orion_psk31_demod_bank* b);
/* Host slices (synchronous) / device buffers (launched on stream). */
int orion_psk31_demod_bank_process(orion_psk31_demod_bank* b, const void* iq, size_t nch, size_t n, float* soft,
                                   size_t out_stride, uint8_t* bits, orion_psk31_report* reports);
int orion_psk31_demod_bank_process_device(orion_psk31_demod_bank* b, const void* iq, size_t nch, size_t n, float* soft,
                                          size_t out_stride, uint8_t* bits, orion_psk31_report* reports, void* stream);
/* Every stream back to its initial state and the sample count to 0 (waits for the device). */
int orion_psk31_demod_bank_reset(orion_psk31_demod_bank* b);
/* set_gain (demodulate/psk31.rs:132-134) of stream `index` of the list the bank was built
 * from; takes effect with the next call (which waits for the device once). */
int orion_psk31_demod_bank_set_gain(orion_psk31_demod_bank* b, size_t index, float gain);

/* ---- the OFDM symbol layer (src/multicarrier, modulate/ofdm.rs, demodulate/ofdm.rs) ----
 * Two stated divergences from the reference: the transform takes powers of two from 8 to
 * 4096 only (rustfft takes any length; ORION_E_ARG / NULL otherwise), and its rounding is
 * this library's radix-2 transform's, not rustfft's. The handles keep the
 * Block contract's shape (host pointers, orion_work_report) through their own process
 * entries: the bit and LLR streams are not orion_block sample types. */
#define ORION_OFDM_BPSK 0
#define ORION_OFDM_QPSK 1
#define ORION_OFDM_QAM16 2
#define ORION_OFDM_QAM64 3
#define ORION_OFDM_QAM256 4
/* CarrierPlanError (multicarrier/config.rs:17-26) as orion_ofdm_config_validate returns it. */
#define ORION_OFDM_PLAN_OK 0
#define ORION_OFDM_PLAN_OUT_OF_RANGE 1
#define ORION_OFDM_PLAN_OVERLAP 2
#define ORION_OFDM_PLAN_EMPTY_DATA 3
#define ORION_OFDM_PLAN_IN_GUARD_BAND 4
/* EqualizerMethod (demodulate/ofdm.rs:297-321); NONE: no equalizer stage. */
#define ORION_OFDM_EQ_NONE (-1)
#define ORION_OFDM_EQ_TRAINING_SYMBOL_HOLD 0
#define ORION_OFDM_EQ_PER_SYMBOL_PILOT_INTERP 1

/* OfdmConfig::new over CarrierPlan::new(..).with_data_carriers(..).with_pilot_carriers(..)
 * (modulate/ofdm.rs:139-166, multicarrier/config.rs:51-69): signed carrier indices, pilot_val
 * [n_pilots] cf32. Nothing is validated here (orion_ofdm_config_validate does; the block
 * constructors refuse an invalid configuration). */
typedef struct orion_ofdm_config orion_ofdm_config;
orion_ofdm_config* orion_ofdm_config_new(size_t n_fft, size_t cp_len, const int32_t* data_carriers, size_t n_data,
                                         const int32_t* pilot_idx, const float* pilot_val, size_t n_pilots, float fs,
                                         float rf_hz, float gain, int constellation);
void orion_ofdm_config_free(orion_ofdm_config* c);
/* with_contiguous_data (config.rs:128-149): appends to the data carriers. */
int orion_ofdm_config_contiguous_data(orion_ofdm_config* c, size_t edge_guard, int include_dc);
/* with_rx_window_backoff / with_symbol_window (modulate/ofdm.rs:240-259). */
int orion_ofdm_config_set_rx_window_backoff(orion_ofdm_config* c, size_t backoff);
int orion_ofdm_config_set_symbol_window(orion_ofdm_config* c, size_t roll_off);
/* validate (config.rs:223-252), or validate_edge_guard (:262-278) when edge_guard >= 0:
 * returns ORION_OFDM_PLAN_* (>= 0); bad_index (may be NULL) receives the offending carrier. */
int orion_ofdm_config_validate(const orion_ofdm_config* c, long long edge_guard, int32_t* bad_index);
/* info [8]: n_fft, cp_len, data carriers, pilots, bits_per_ofdm_symbol, samples_per_ofdm_symbol
 * (modulate/ofdm.rs:359-365), occupied_half_carriers (config.rs:167-174), the window roll-off. */
int orion_ofdm_config_info(const orion_ofdm_config* c, size_t* info);
/* The data carriers (cap >= their count) and occupied_bins (config.rs:188-203; cap >= n_fft). */
int orion_ofdm_config_data_carriers(const orion_ofdm_config* c, int32_t* out, size_t cap);
int orion_ofdm_config_occupied_bins(const orion_ofdm_config* c, uint32_t* out, size_t cap, size_t* n);
/* CarrierGrid::from_plan (grid.rs:40-66): data_bins [data carriers], pilot_bins [pilots]. */
int orion_ofdm_config_grid(const orion_ofdm_config* c, uint32_t* data_bins, uint32_t* pilot_bins);
/* SymbolFft::max_pilot_safe_backoff (symbol_fft.rs:90-92). */
size_t orion_ofdm_max_pilot_safe_backoff(size_t n_fft, size_t pilot_spacing);

/* Host only. The tables as the library holds them: axis [16] (build_axis_table,
 * modulate/qam.rs:45-57) and thresholds [15] (build_threshold_table, demodulate/qam.rs:28-41)
 * of a QAM order (zeros for BPSK / QPSK), the training pattern [n_fft] cf32
 * (training_symbol_freq_pattern, sync/ofdm_sync.rs:270-272, :335-352), the transform's
 * twiddles [n_fft / 2] cf32 and the window ramp [min(roll_off, symbol_len / 2)]
 * (symbol_window.rs:47-59). Any output may be NULL. */
int orion_ofdm_tables(int constellation, float* axis, float* thresholds, size_t n_fft, float* training,
                      float* twiddles, size_t symbol_len, size_t roll_off, float* ramp);
/* Host only: the mappers, hard deciders and max-log LLRs on n_syms symbols
 * (modulate/qpsk.rs:33-45, qam.rs:92-101; demodulate/qam.rs:120-140, ofdm.rs:588-638). */
int orion_ofdm_map_host(int constellation, const uint8_t* bits, size_t n_syms, void* syms);
int orion_ofdm_decide_host(int constellation, const void* syms, size_t n_syms, uint8_t* bits);
int orion_ofdm_llr_host(int constellation, const void* syms, size_t n_syms, float* llr);
/* Host only: the scalar radix-2 transform of n_sym n_fft-point symbols, in place allowed. */
int orion_fft_host(size_t n_fft, int inverse, const void* in, size_t n_sym, void* out);
/* Host only: SymbolWindow (symbol_window.rs:80-98) over n_sym symbols in place. */
int orion_ofdm_window_host(size_t symbol_len, size_t roll_off, void* iq, size_t n_sym);
/* Host only: Rotator::next n times from a fresh oscillator (dsp/rotator.rs:16-61). */
int orion_ofdm_rotator_host(float freq_hz, float fs, size_t n, void* out);
/* Host only: evm_db (demodulate/ofdm.rs:263-293); *valid 0 where the reference gives None. */
int orion_ofdm_evm_db_host(int constellation, const void* soft, size_t n_soft, const uint8_t* bits, size_t n_bits,
                           size_t num_symbols, float* evm_db, int* valid);
/* Host only: equalizer_weight (demodulate/ofdm.rs:495-502) of n channel estimates, and
 * interpolate_at (:514-537) over n_pilots bin-sorted ratios at n_bins bins. */
int orion_ofdm_equalizer_weight_host(const void* h, size_t n, void* w);
int orion_ofdm_interpolate_host(const uint32_t* pilot_bins, const void* ratios, size_t n_pilots, const uint32_t* bins,
                                size_t n_bins, void* out);

/* FftBlock / IfftBlock (multicarrier/fft.rs:16-120). NULL (and a message) for a size that is
 * not a power of two from 8 to 4096. No device is touched here. */
typedef struct orion_fft orion_fft;
orion_fft* orion_fft_new(size_t n_fft);
orion_fft* orion_ifft_new(size_t n_fft);
void orion_fft_free(orion_fft* f);
/* One symbol per call, host pointers; a short input or output gives a zero report (fft.rs:42-46). */
int orion_fft_process(orion_fft* f, const void* in, size_t n_in, void* out, size_t out_cap, orion_work_report* report);
/* batch symbols over resident buffers: symbol b reads in + b * in_stride and writes out + b *
 * out_stride (strides in cf32 values, >= n_fft; any 8-byte aligned address). */
int orion_fft_batch(orion_fft* f, const void* in, size_t in_stride, void* out, size_t out_stride, size_t batch,
                    void* stream);

/* OfdmMod, OfdmDemod (+ an optional OfdmEqualizer stage), OfdmDecider, OfdmSoftDemod and
 * OfdmEqualizer (modulate/ofdm.rs:422-544, demodulate/ofdm.rs:26-166, :333-569, :693-731) of
 * one configuration, which is copied. NULL (and a message) for a configuration that does not
 * validate, a transform size outside 8..4096, cp_len > n_fft or an unknown constellation.
 * No device is touched here. */
typedef struct orion_ofdm orion_ofdm;
orion_ofdm* orion_ofdm_mod_new(const orion_ofdm_config* c);
orion_ofdm* orion_ofdm_demod_new(const orion_ofdm_config* c, int equalizer);
orion_ofdm* orion_ofdm_decider_new(const orion_ofdm_config* c);
orion_ofdm* orion_ofdm_soft_demod_new(const orion_ofdm_config* c);
orion_ofdm* orion_ofdm_equalizer_new(const orion_ofdm_config* c, int method);
void orion_ofdm_free(orion_ofdm* h);
/* set_gain of the modulator or demodulator (modulate/ofdm.rs:463-465, demodulate/ofdm.rs:50-52);
 * reset: the RF rotator back to phase 0. */
int orion_ofdm_set_gain(orion_ofdm* h, float gain);
int orion_ofdm_reset(orion_ofdm* h);
/* estimate_from_training_symbol (demodulate/ofdm.rs:440-448) of a demodulator's or an
 * equalizer's TrainingSymbolHold stage: received [n_fft] cf32, host memory. */
int orion_ofdm_estimate_channel(orion_ofdm* h, const void* received_freq, size_t n);
/* The Block contract, host pointers, on the device: as many whole symbols as fit in both
 * buffers (the reference's process takes one; k calls of it equal one call here); a short
 * input or output gives a zero report. Modulator: bits u8 -> cf32; demodulator: cf32 ->
 * cf32 soft symbols; decider: cf32 -> bits u8; soft demodulator: cf32 -> f32 LLRs;
 * equalizer: cf32 n_fft-bin vectors -> the same. Sizes count elements. */
int orion_ofdm_process(orion_ofdm* h, const void* in, size_t n_in, void* out, size_t out_cap,
                       orion_work_report* report);
/* Resident buffers, n_channels x n_symbols symbols in one launch, asynchronous on stream.
 * Modulator: bits [n_channels][n_symbols * bits_per_ofdm_symbol] -> iq [n_channels][n_symbols
 * * samples_per_ofdm_symbol]; with rf_hz != 0 every channel continues the handle's rotator
 * from the same phase, which then advances by one channel's samples. */
int orion_ofdm_mod_device(orion_ofdm* h, const uint8_t* bits, size_t n_channels, size_t n_symbols, void* iq,
                          void* stream);
/* Demodulator: iq -> soft [n_channels][n_symbols * data carriers] cf32 and, from the same
 * launch where not NULL, bits (u8) and llr (f32) [n_channels][n_symbols * bits_per_ofdm_symbol]. */
int orion_ofdm_demod_device(orion_ofdm* h, const void* iq, size_t n_channels, size_t n_symbols, void* soft,
                            uint8_t* bits, float* llr, void* stream);
/* Decider / soft demodulator over n_channels * n_symbols * data carriers soft symbols;
 * equalizer over n_channels * n_symbols n_fft-bin vectors. */
int orion_ofdm_decider_device(orion_ofdm* h, const void* soft, size_t n_channels, size_t n_symbols, uint8_t* bits,
                              void* stream);
int orion_ofdm_soft_demod_device(orion_ofdm* h, const void* soft, size_t n_channels, size_t n_symbols, float* llr,
                                 void* stream);
int orion_ofdm_equalizer_device(orion_ofdm* h, const void* in, size_t n_channels, size_t n_symbols, void* out,
                                void* stream);
/* Host only, the scalar restatement the kernels are held to: OfdmMod::process over whole
 * symbols from the handle's state, OfdmDemod::process (through the handle's equalizer
 * stage, when it has one), OfdmEqualizer::process. Reports as orion_ofdm_process. */
int orion_ofdm_mod_host(orion_ofdm* h, const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap,
                        orion_work_report* report);
int orion_ofdm_demod_host(orion_ofdm* h, const void* iq, size_t n, void* soft, size_t out_cap,
                          orion_work_report* report);
int orion_ofdm_equalize_host(orion_ofdm* h, const void* in, size_t n, void* out, size_t out_cap,
                             orion_work_report* report);
/* Host only: set_pilot_bins (demodulate/ofdm.rs:426-432) of an equalizer's host stage. */
int orion_ofdm_set_pilot_bins_host(orion_ofdm* h, const uint32_t* pilot_bins, const void* pilot_val, size_t n_pilots,
                                   const uint32_t* data_bins, size_t n_data);

/* ---- the inner code: punctured convolutional code, soft Viterbi, block interleaver
 * (src/fec/conv.rs, src/fec/interleaver.rs:53-120) --------------------------------------
 * A rate 1/2 mother code, terminated by K - 1 zero tail bits and punctured to rate 2/3, 3/4,
 * 5/6 or 7/8 (matrices of conv.rs:112-120; step t uses column t % period). Bits are uint8,
 * one per byte, 0 or 1 (only bit 0 of an input byte is read). LLRs are f32 in punctured
 * order, positive meaning bit 0: what orion_ofdm_demod_device writes as llr.
 *
 * A batched call works on nstreams streams, one frame each; all streams of a call share code,
 * rate, info_bits and interleaver. The interleaver of the frame chain is given as rows, cols
 * (0, 0: none): the encoder's output goes through interleave_bits (modulate/ofdm_frame.rs:
 * row-in, column-out blocks of rows * cols, the last one zero-padded, so a whole number of
 * blocks: orion_fec_encoded_len), the decoder's input through deinterleave_llrs
 * (demodulate/ofdm_frame.rs: full blocks are permuted back; a short last chunk of the n_llr
 * values is NOT permuted, it passes through as it is).
 *
 * Layouts: llr [nstreams][n_llr] f32, bits [nstreams][info_bits] u8, coded
 * [nstreams][orion_fec_encoded_len] u8. The decoder reads 0.0 where the puncturing deleted a
 * bit and at every index at or past n_llr or the coded length (n_llr may be shorter or longer
 * than the coded length).
 *
 * Limits: 1 <= info_bits <= 2^24, nstreams <= 2^24, n_llr <= 2^31 - 1, rows * cols <= 2^24,
 * nstreams * orion_fec_encoded_len <= 2^38. Errors: ORION_E_NULL for a null pointer,
 * ORION_E_ARG for an unknown code or rate, info_bits == 0, a count above its limit, one of
 * rows, cols zero and the other not, or a workspace that is too small or not 8-byte aligned
 * (nothing is launched). nstreams == 0 does nothing. The functions that return a size return 0
 * for such arguments.
 *
 * Only orion_fec_viterbi, orion_fec_viterbi_device, orion_fec_conv_encode_batch and
 * orion_fec_conv_encode_batch_device touch a device. */
#define ORION_FEC_K5 0     /* K = 5, G0 = 25, G1 = 23 octal: orion_conv_encode's code */
#define ORION_FEC_DVB_K7 1 /* K = 7, G0 = 171, G1 = 133 octal (ETSI EN 300 744 4.3.3) */
#define ORION_FEC_RATE_1_2 0
#define ORION_FEC_RATE_2_3 1
#define ORION_FEC_RATE_3_4 2
#define ORION_FEC_RATE_5_6 3
#define ORION_FEC_RATE_7_8 4
/* punctured_coded_len_with, conv.rs:274-288; and that length after interleave_bits. */
size_t orion_fec_punctured_coded_len(int code, size_t info_bits, int rate);
size_t orion_fec_encoded_len(int code, size_t info_bits, int rate, size_t rows, size_t cols);
/* conv_encode_punctured_with, conv.rs:234-263, host only: info [info_bits] -> coded
 * [orion_fec_punctured_coded_len] (no interleaver). */
int orion_fec_conv_encode(int code, int rate, const uint8_t* info, size_t info_bits, uint8_t* coded);
/* The scalar decoder the kernel is held to, one stream, host only: viterbi_decode_soft_with
 * (conv.rs:304-398) of deinterleave_llrs(llr [n_llr]) -> bits [info_bits]. The start metric
 * is f32::MIN / 2 with state 0 at 0; a predecessor at or below it is skipped; a survivor is
 * replaced on strict > only, states visited ascending; the traceback starts at state 0. */
int orion_fec_viterbi_host(int code, int rate, const float* llr, size_t n_llr, size_t info_bits, size_t rows,
                           size_t cols, uint8_t* bits);
/* The same decode of nstreams streams in one launch: one lane per trellis state (K = 7: one
 * stream per wave; K = 5: sixteen lanes per stream, four streams per wave), depuncturing and
 * deinterleaving fused into the LLR fetch. The bits are those of orion_fec_viterbi_host for
 * every input, ties, all-zero input, short input and metrics that overflow included. NaN
 * input is outside the contract; it neither faults nor hangs. Host slices (uploaded, one
 * launch, downloaded; synchronous) or device buffers on a stream; the device call needs work,
 * device memory of at least orion_fec_viterbi_work_bytes(code, nstreams, info_bits) bytes,
 * 8-byte aligned (K = 5: 4 bytes per stream, rounded up to 4 streams, and trellis step;
 * K = 7: 16 bytes per stream and step; info_bits + K - 1 steps), which it may overwrite wholly. */
int orion_fec_viterbi(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                      size_t rows, size_t cols, uint8_t* bits);
int orion_fec_viterbi_device(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                             size_t rows, size_t cols, uint8_t* bits, void* work, size_t work_bytes, void* stream);
size_t orion_fec_viterbi_work_bytes(int code, size_t nstreams, size_t info_bits);
/* Encode, puncture and interleave nstreams streams in one launch, one thread per output bit:
 * info [nstreams][info_bits] -> coded [nstreams][orion_fec_encoded_len]; the bytes are those
 * of orion_fec_conv_encode followed by orion_fec_interleave_bits. Host slices (synchronous)
 * or device buffers on a stream. */
int orion_fec_conv_encode_batch(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits,
                                size_t rows, size_t cols, uint8_t* coded);
int orion_fec_conv_encode_batch_device(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits,
                                       size_t rows, size_t cols, uint8_t* coded, void* stream);
/* BlockInterleaver, interleaver.rs:53-120, host only, rows and cols nonzero. One block of
 * rows * cols elements: interleave out[c rows + r] = in[r cols + c], deinterleave its inverse. */
int orion_fec_interleave_u8(size_t rows, size_t cols, const uint8_t* in, uint8_t* out);
int orion_fec_interleave_f32(size_t rows, size_t cols, const float* in, float* out);
int orion_fec_deinterleave_u8(size_t rows, size_t cols, const uint8_t* in, uint8_t* out);
int orion_fec_deinterleave_f32(size_t rows, size_t cols, const float* in, float* out);
/* The chain drivers, host only: interleave_bits, bits [n] -> out [orion_fec_interleaved_len
 * (rows, cols, n)], n rounded up to whole blocks; deinterleave_llrs, llr [n] -> out [n]. */
size_t orion_fec_interleaved_len(size_t rows, size_t cols, size_t n);
int orion_fec_interleave_bits(size_t rows, size_t cols, const uint8_t* bits, size_t n, uint8_t* out);
int orion_fec_deinterleave_llrs(size_t rows, size_t cols, const float* llr, size_t n, float* out);

/* ---- the outer code: Reed-Solomon over GF(2^8), the Forney byte interleaver, the PN scrambler,
 * DVB-T energy dispersal and the transport-stream packet layer (src/fec/gf.rs,
 * reed_solomon.rs, interleaver.rs:122-305, scrambler.rs; src/waveform/dvb_t.rs:30-110,
 * dvb_t_ts.rs) --------------------------------------------------------------------------------
 * A code is (n, n_parity): n codeword bytes, k = n - n_parity message bytes, byte 0 the
 * highest-degree symbol, first consecutive root 0, field polynomial 0x11D; n < 255 is the
 * shortened code. 1 <= n <= 255 and n_parity < n (the reference's check); t = n_parity / 2,
 * rounded down. DVB-T's outer code is (204, 16).
 *
 * The decoder is the reference's decode_counted step for step: the Chien search runs over all
 * 255 degrees; a root on a degree that is never transmitted counts as a root and is not
 * applied; a zero magnitude is not counted; the syndromes of the corrected word decide. Its
 * status is the number of codeword bytes it changed (parity bytes included), or -1 for an
 * uncorrectable word, whose message is then the systematic prefix received[:k].
 *
 * The Forney interleaver has I = branches and M = depth (DVB-T: 12, 17), both nonzero and
 * I * I * M <= 2^24; its round-trip delay is D = I (I - 1) M bytes. Frame mode: the payload is
 * zero-padded to a multiple of I bytes, fed through a fresh interleaver and followed by the
 * flush, round_up(n, I) + D bytes (orion_rs_forney_frame_len); the deinterleaver returns bytes
 * D .. total of a fresh deinterleaver's output.
 *
 * Only orion_rs_decode_batch / _device, orion_rs_encode_batch / _device and
 * orion_rs_forney_interleave_batch / _device touch a device; nstreams == 0 does nothing.
 * Device limits: 1 <= n_parity <= 32, 1 <= ncw <= 2^20, nstreams <= 2^24, nstreams * ncw <=
 * 2^30, the interleaver's input 1 <= len <= 2^27 bytes and at most 2^38 output elements.
 * Errors: ORION_E_NULL for a null pointer or handle, ORION_E_ARG for everything else that is
 * out of range (nothing is launched). The functions that return a size return 0 for such
 * arguments. */
typedef struct orion_rs_forney orion_rs_forney;
typedef struct orion_rs_pn_stream orion_rs_pn_stream;
typedef struct orion_rs_dispersal orion_rs_dispersal;
/* Gf256: the tables exp [512] (2^i, the cycle of 255 repeated) and log [256]; mul, div, inv,
 * pow (n reduced modulo 255; 0^0 = 1) and exp_of (i modulo 255) return the element 0..255, or
 * ORION_E_ARG for an operand above 255, a division by zero or the inverse of zero. */
int orion_rs_gf_tables(uint8_t* exp, uint8_t* log);
int orion_rs_gf_mul(unsigned a, unsigned b);
int orion_rs_gf_div(unsigned a, unsigned b);
int orion_rs_gf_inv(unsigned a);
int orion_rs_gf_pow(unsigned a, size_t n);
int orion_rs_gf_exp_of(size_t i);
/* The generator polynomial, low degree first: out [n_parity + 1]. */
int orion_rs_generator(size_t n, size_t n_parity, uint8_t* out);
/* Host only, nwords words one after another: msgs [nwords][k] -> cws [nwords][n] (n_parity ==
 * 0: ORION_E_ARG, the reference's shift register has no cell); words [nwords][n] -> msgs
 * [nwords][k], status [nwords]. */
int orion_rs_encode(size_t n, size_t n_parity, const uint8_t* msgs, size_t nwords, uint8_t* cws);
int orion_rs_decode_counted(size_t n, size_t n_parity, const uint8_t* words, size_t nwords, uint8_t* msgs,
                            int32_t* status);
/* ConvInterleaver (inverse == 0) / ConvDeinterleaver (inverse != 0) as streaming blocks: feed
 * is 1:1 in length (in [n] -> out [n], in == out allowed) and carries the delay lines across
 * calls; flush feeds D zeros (out [D]); reset clears the lines and the commutator. */
orion_rs_forney* orion_rs_forney_new(size_t branches, size_t depth, int inverse);
void orion_rs_forney_free(orion_rs_forney* f);
int orion_rs_forney_feed(orion_rs_forney* f, const uint8_t* in, size_t n, uint8_t* out);
int orion_rs_forney_flush(orion_rs_forney* f, uint8_t* out);
int orion_rs_forney_reset(orion_rs_forney* f);
size_t orion_rs_forney_delay(size_t branches, size_t depth); /* 0 for bad dimensions, and for I == 1 */
/* Frame mode, host only: bytes [n] -> out [orion_rs_forney_frame_len(branches, depth, n)];
 * bytes [total] -> out [total - D] (total <= D: nothing is written). */
size_t orion_rs_forney_frame_len(size_t branches, size_t depth, size_t n);
int orion_rs_forney_frame_interleave(size_t branches, size_t depth, const uint8_t* bytes, size_t n, uint8_t* out);
int orion_rs_forney_frame_deinterleave(size_t branches, size_t depth, const uint8_t* bytes, size_t total,
                                       uint8_t* out);
/* PnScrambler: a Fibonacci LFSR of width bits (2..=32) from seed (nonzero; seed and taps fit in
 * width bits); the scrambling bit is bit 0, the feedback the parity of reg & taps, inserted at
 * bit width - 1; data bits LSB first. orion_rs_pn_scramble restarts from seed (in place,
 * self-inverse); a stream carries the register across feeds (in place) until reset. */
int orion_rs_pn_scramble(uint32_t taps, uint32_t width, uint32_t seed, uint8_t* data, size_t n);
orion_rs_pn_stream* orion_rs_pn_stream_new(uint32_t taps, uint32_t width, uint32_t seed);
void orion_rs_pn_stream_free(orion_rs_pn_stream* s);
int orion_rs_pn_stream_feed(orion_rs_pn_stream* s, uint8_t* data, size_t n);
int orion_rs_pn_stream_reset(orion_rs_pn_stream* s);
/* DvbTEnergyDispersal: PRBS 1 + X^14 + X^15 from 100101010000000, data bits MSB first, the
 * register carried across feeds (in place); advance_byte clocks eight steps without output. */
orion_rs_dispersal* orion_rs_dispersal_new(void);
void orion_rs_dispersal_free(orion_rs_dispersal* d);
int orion_rs_dispersal_feed(orion_rs_dispersal* d, uint8_t* data, size_t n);
int orion_rs_dispersal_advance_byte(orion_rs_dispersal* d);
int orion_rs_dispersal_reset(orion_rs_dispersal* d);
/* The transport-stream layer, host only. ts_energy_disperse: in place over n bytes, a multiple
 * of 188 (ORION_E_ARG otherwise): the PRBS restarts every eight packets, the first sync byte
 * of a group is flipped 0x47 <-> 0xB8, the other seven are clocked over, every payload byte
 * is whitened; self-inverse. ts_dispersal_mask: what that XORs onto a group, out [1504], the
 * kernels' table. ts_packetize: payload [n] -> out [orion_rs_ts_packetized_len(n)], max(1,
 * ceil(n / 187)) packets of 0x47 and 187 payload bytes. ts_depacketize: packets [n], n a
 * nonzero multiple of 188 -> out [n / 188 * 187]. ts_null_packet: out [188] = 47 1F FF 10 and
 * 0xFF. ts_stuff_null_packets: ts [n], whole packets -> out [max(n / 188, target_packets) *
 * 188], ts followed by null packets. */
int orion_rs_ts_energy_disperse(uint8_t* packets, size_t n);
int orion_rs_ts_dispersal_mask(uint8_t* out);
size_t orion_rs_ts_packetized_len(size_t n);
int orion_rs_ts_packetize(const uint8_t* payload, size_t n, uint8_t* out);
int orion_rs_ts_depacketize(const uint8_t* packets, size_t n, uint8_t* out);
int orion_rs_ts_null_packet(uint8_t* out);
int orion_rs_ts_stuff_null_packets(const uint8_t* ts, size_t n, size_t target_packets, uint8_t* out);
/* The batched decoder, one wave per codeword: nstreams streams of ncw words each. A stream is
 * ncw * n bytes; with branches, depth nonzero it is the frame-mode interleaved payload, ncw *
 * n + D bytes, deinterleaved in the fetch (ncw * n must be a multiple of branches); with bits
 * nonzero every byte of it is given as eight elements of one bit each, MSB first, as
 * orion_fec_viterbi_device writes them (only bit 0 of an element is read):
 * orion_rs_decode_stream_len elements in all. msgs [nstreams][ncw][k], status [nstreams][ncw];
 * both equal orion_rs_decode_counted of the words, for every input. With derandomize nonzero
 * (k = 188 only) the messages, those of uncorrectable words included, go through
 * orion_rs_ts_energy_disperse per stream. Host slices (synchronous) or device buffers on a
 * stream (status 4-byte aligned). */
size_t orion_rs_decode_stream_len(size_t n, size_t n_parity, size_t ncw, int bits, size_t branches, size_t depth);
int orion_rs_decode_batch(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, int bits,
                          size_t branches, size_t depth, int derandomize, uint8_t* msgs, int32_t* status);
int orion_rs_decode_batch_device(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, int bits,
                                 size_t branches, size_t depth, int derandomize, uint8_t* msgs, int32_t* status,
                                 void* stream);
/* The batched encoder: msgs [nstreams][ncw][k] -> cws [nstreams][ncw][n], the bytes of
 * orion_rs_encode; with disperse nonzero (k = 188 only) of orion_rs_ts_energy_disperse of each
 * stream's messages. */
int orion_rs_encode_batch(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw, int disperse,
                          uint8_t* cws);
int orion_rs_encode_batch_device(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw,
                                 int disperse, uint8_t* cws, void* stream);
/* The frame-mode interleaver, one thread per output element: in [nstreams][len] -> out
 * [nstreams][orion_rs_forney_interleave_len], the bytes of orion_rs_forney_frame_interleave,
 * with bits nonzero unpacked to one bit per element, MSB first (what
 * orion_fec_conv_encode_batch_device reads). */
size_t orion_rs_forney_interleave_len(size_t branches, size_t depth, size_t len, int bits);
int orion_rs_forney_interleave_batch(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len,
                                     int bits, uint8_t* out);
int orion_rs_forney_interleave_batch_device(size_t branches, size_t depth, const uint8_t* in, size_t nstreams,
                                            size_t len, int bits, uint8_t* out, void* stream);

/* ---- the COFDM frame chain's codes: the constructed LDPC family and the shortened binary BCH
 * code (src/fec/ldpc_codes.rs, src/fec/bch.rs; ldpc_family.hpp, bch.hpp, k_ldpc_family.hip,
 * k_bch.hip). A bad argument is ORION_E_ARG, before anything is launched. ---- */
#define ORION_LDPCF_N512R12 0 /* N = 512, K = 256 */
#define ORION_LDPCF_N576R23 1 /* N = 576, K = 384 */
#define ORION_LDPCF_N512R34 2 /* N = 512, K = 384 */
#define ORION_LDPCF_SUM_PRODUCT 0
#define ORION_LDPCF_MIN_SUM 1
#define ORION_LDPCF_SCALED_MIN_SUM 2 /* the message times scale */
/* The code, built on first use and kept. dims: out [6] = N, K, M, edges, the largest check
 * degree, the picks for which the 4-cycle guard was relaxed. graph: the Tanner graph as CSR:
 * check_start [M + 1], check_bits [edges] (within a check the message columns ascending, then
 * K + i, then K + i - 1), bit_start [N + 1], bit_checks [edges] (ascending) and bit_edges
 * [edges], the index into check_bits of that bit in that check. */
int orion_ldpcf_dims(int code, uint32_t* out);
int orion_ldpcf_graph(int code, uint32_t* check_start, uint32_t* check_bits, uint32_t* bit_start,
                      uint32_t* bit_checks, uint32_t* bit_edges);
/* Host only, nwords words each. encode: msgs [nwords][K] -> cws [nwords][N], message | parity
 * (the message elements as they are, bit 0 of each in the parity). syndrome_weight: hard
 * [nwords][N] -> unsat [nwords]. decode_soft: llr [nwords][N], positive meaning bit 0 -> bits
 * [nwords][K], unsat [nwords] (the smallest unsatisfied-check count seen, 0: decoded),
 * iterations [nwords] (0: the initial decision was a codeword). */
int orion_ldpcf_encode(int code, const uint8_t* msgs, size_t nwords, uint8_t* cws);
int orion_ldpcf_syndrome_weight(int code, const uint8_t* hard, size_t nwords, int32_t* unsat);
int orion_ldpcf_decode_soft(int code, const float* llr, size_t nwords, size_t max_iter, int rule, float scale,
                            uint8_t* bits, int32_t* unsat, int32_t* iterations);
/* The batched decoder, one wave per codeword: llr [nstreams][n_llr]; with rows, cols nonzero a
 * stream is whole interleaver blocks and is deinterleaved in the fetch (as
 * orion_fec_deinterleave_llrs); its nblocks = orion_ldpcf_decode_blocks words are elements 0 ..
 * nblocks * N of that, the rest is not read. bits [nstreams][nblocks * K], unsat and iterations
 * [nstreams][nblocks]; all equal orion_ldpcf_decode_soft of the words, for every input. Host
 * slices (synchronous) or device buffers on a stream. */
size_t orion_ldpcf_decode_blocks(int code, size_t n_llr, size_t rows, size_t cols);
int orion_ldpcf_decode_batch(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                             size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat,
                             int32_t* iterations);
int orion_ldpcf_decode_batch_device(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows,
                                    size_t cols, size_t max_iter, int rule, float scale, uint8_t* bits,
                                    int32_t* unsat, int32_t* iterations, void* stream);
/* The batched encoder: bits [nstreams][nbits] -> coded [nstreams][orion_ldpcf_encoded_len]:
 * ceil(nbits / K) codewords, the last message zero-padded, then with rows, cols nonzero the
 * block interleaver, zero-padded to whole blocks (as orion_fec_interleave_bits). */
size_t orion_ldpcf_encoded_len(int code, size_t nbits, size_t rows, size_t cols);
int orion_ldpcf_encode_batch(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                             uint8_t* coded);
int orion_ldpcf_encode_batch_device(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows,
                                    size_t cols, uint8_t* coded, void* stream);
/* The binary BCH code over GF(2^8) correcting t bit errors, shortened to n elements of one bit
 * each, index 0 the highest degree; host only. parity_bits: of the code of t, 0 on a bad t.
 * generator: out [parity_bits + 1], highest degree first. encode: msgs [nwords][k] -> cws
 * [nwords][n]. decode: words [nwords][n] -> msgs [nwords][k], status [nwords]: the bits flipped
 * (an element is set when nonzero, a flip is ^= 1), or -max(residual syndromes, roots found)
 * <= -1 for an uncorrectable word, whose message is then words[:k]; locator_len (optional)
 * [nwords]: entries of the Berlekamp-Massey locator vector, 0 for a clean word. */
size_t orion_bch_parity_bits(size_t t);
int orion_bch_generator(size_t n, size_t t, uint8_t* out);
int orion_bch_encode(size_t n, size_t t, const uint8_t* msgs, size_t nwords, uint8_t* cws);
int orion_bch_decode(size_t n, size_t t, const uint8_t* words, size_t nwords, uint8_t* msgs, int32_t* status,
                     int32_t* locator_len);
/* The batched coder of the frame chain, one wave per word, for the code of t (1 .. 31) over
 * info_bits information bits, n = info_bits + parity_bits. decode: in [nstreams][nb], ncw = nb
 * / n >= 1 words per stream, the tail ignored -> msgs [nstreams][ncw * info_bits], status
 * [nstreams][ncw], both equal to orion_bch_decode of the words. encode: bits [nstreams][nbits]
 * -> coded [nstreams][ceil(nbits / info_bits) * n], the last message zero-padded. Host slices
 * (synchronous) or device buffers on a stream (status 4-byte aligned). */
int orion_bch_decode_batch(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                           int32_t* status);
int orion_bch_decode_batch_device(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb,
                                  uint8_t* msgs, int32_t* status, void* stream);
int orion_bch_encode_batch(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                           uint8_t* coded);
int orion_bch_encode_batch_device(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                                  uint8_t* coded, void* stream);

/* ---- the coding chain of the COFDM frame layer (modulate/ofdm_frame.rs:204-682,
 * demodulate/ofdm_frame.rs:351-779, codec/crc.rs:89-130, fec/frame.rs) ----
 *   payload -> CRC -> [scramble] -> outer FEC -> outer interleave -> inner FEC ->
 *              inner interleave -> [scramble] -> coded bits            (reversed on receive)
 * Bits are one per byte, MSB first within a byte. */
#define ORION_FRAME_CRC_NONE 0
#define ORION_FRAME_CRC16 1 /* CCITT-FALSE */
#define ORION_FRAME_CRC32 2 /* ISO-HDLC */
#define ORION_FRAME_OUTER_NONE 0
#define ORION_FRAME_OUTER_BCH 1 /* a = t, over 120 information bits */
#define ORION_FRAME_OUTER_RS 2  /* a = n, b = n_parity */
#define ORION_FRAME_INNER_NONE 0
#define ORION_FRAME_INNER_LDPC 1 /* a = the orion_ldpcf code */
#define ORION_FRAME_INNER_CONV 2 /* a = ORION_FEC_K5 / ORION_FEC_DVB_K7, b = ORION_FEC_RATE_* */
#define ORION_FRAME_IL_NONE 0
#define ORION_FRAME_IL_BLOCK 1  /* a = rows, b = cols */
#define ORION_FRAME_IL_FORNEY 2 /* a = branches, b = depth (frame mode) */
#define ORION_FRAME_SCR_NONE 0
#define ORION_FRAME_SCR_ADDITIVE 1
#define ORION_FRAME_SCR_DVBT 2 /* DVB-T energy dispersal: before the outer code only */
#define ORION_FRAME_SCR_BEFORE_OUTER 0
#define ORION_FRAME_SCR_AFTER_INNER 1
#define ORION_FRAME_HEADER_FIELD_BYTES 14
/* RxError, fec/frame.rs:59-77; 0 is no error */
#define ORION_RX_PREAMBLE_TIMEOUT 1
#define ORION_RX_MALFORMED_HEADER 2
#define ORION_RX_HEADER_CRC_MISMATCH 3
#define ORION_RX_CRC_MISMATCH 4
#define ORION_RX_FEC_UNCORRECTABLE 5
typedef struct {
  int32_t crc;
  int32_t outer;
  uint32_t outer_a, outer_b;
  int32_t inner;
  uint32_t inner_a, inner_b;
  int32_t outer_il;
  uint32_t outer_il_a, outer_il_b;
  int32_t inner_il;
  uint32_t inner_il_a, inner_il_b;
  int32_t scrambler;
  uint32_t scr_poly, scr_width;
  int32_t scr_per_frame; /* SeedMode::PerFrameRandom: the seed is the call's, not scr_seed */
  uint32_t scr_seed;     /* SeedMode::Fixed */
  int32_t scrambler_pos;
} orion_frame_scheme;
uint32_t orion_frame_crc16(const uint8_t* data, size_t n);
uint32_t orion_frame_crc32(const uint8_t* data, size_t n);
/* out [n + 0 | 2 | 4] = data | crc, big-endian */
int orion_frame_append_crc(int crc, const uint8_t* data, size_t n, uint8_t* out);
/* data = payload | crc: *ok = 1 when it checks. ORION_E_ARG when n is shorter than the CRC. */
int orion_frame_check_crc(int crc, const uint8_t* data, size_t n, int32_t* ok);
/* fields [5]: mcs_index, payload_len, sequence_num, flags, scrambler_seed <-> the 14 bytes */
int orion_frame_pack_header(const uint32_t* fields, uint8_t* out14);
int orion_frame_unpack_header(const uint8_t* in14, uint32_t* fields);
/* build_scrambler's seed: raw reduced to width bits (all 32 when width >= 32), 0 mapped to 1 */
uint32_t orion_frame_reduce_seed(uint32_t width, uint32_t raw);
/* scramble_bytes / scramble_bits / apply_pn_to_llrs of the scheme's scrambler, in place,
 * whatever its position. Bit i meets PN step 8 (i / 8) + 7 - i % 8. */
int orion_frame_scramble_bytes(const orion_frame_scheme* s, uint32_t per_frame_seed, uint8_t* bytes, size_t n);
int orion_frame_scramble_bits(const orion_frame_scheme* s, uint32_t per_frame_seed, uint8_t* bits, size_t n);
int orion_frame_apply_pn_to_llrs(const orion_frame_scheme* s, uint32_t per_frame_seed, float* llr, size_t n);
/* plan [6]: info_bytes, framed_bytes, outer_coded_bits, outer_il_bits, inner_coded_bits, coded_bits */
int orion_frame_block_plan(const orion_frame_scheme* s, size_t info_bytes, size_t* plan);
/* encode_chain_stages: coded [plan.coded_bits], outer_il_bits [plan.outer_il_bits] (may be NULL) */
int orion_frame_encode_chain(const orion_frame_scheme* s, const uint8_t* bytes, size_t n, uint32_t per_frame_seed,
                             uint8_t* coded, uint8_t* outer_il_bits);
/* decode_chain under block_plan(info_bytes): bytes [info_bytes]; outcome [8] = the RxError (0,
 * or ORION_RX_MALFORMED_HEADER and nothing else is written), inner_ok, outer_ok, crc_ok,
 * crc_present, outer_present, outer_corrected_bytes (-1: none reported), is_valid;
 * inner_out_bits [inner_cap] (may be NULL) takes the untrimmed inner decoder output,
 * *inner_out_len its length (ORION_E_ARG when it does not fit). LDPC runs 50 iterations. */
int orion_frame_decode_chain(const orion_frame_scheme* s, const float* llr, size_t n_llr, size_t info_bytes,
                             uint32_t per_frame_seed, int ldpc_rule, float ldpc_scale, uint8_t* bytes,
                             int32_t* outcome, uint8_t* inner_out_bits, size_t inner_cap, size_t* inner_out_len);
/* The glue kernels between the batched codes, one wave per frame (k_frame.hip). Host slices
 * (synchronous) or device buffers on a stream. seeds [nframes] i64 (per-frame seeds) or NULL
 * for the scheme's fixed seed. nframes <= 2^24, info_len <= 2^16, rows <= 2^24 elements.
 * pack: payload [nframes][info_len], or fields [nframes][5] i64 for a header (info_len 14)
 * -> out [nframes][framed * 8] bits or (out_bytes) [nframes][framed] bytes: append_crc, then
 * scramble_bytes when the scrambler sits before the outer code.
 * unpack: the first framed * 8 bits (or, in_bytes, framed bytes) of each row of in
 * [nframes][in_stride]; unsat [nframes][n_inner] and status [nframes][n_outer] i32 (either may
 * be NULL) are the decoders' per-word outputs -> payload [nframes][info_len], flags
 * [nframes][4] = inner_ok, outer_ok, crc_ok, is_valid, corrected [nframes] i32 (the sum of
 * the non-negative status entries), fields [nframes][5] i64 (header; else NULL).
 * coded_bits: out [nframes][out_len] = the first nbits of in [nframes][in_stride],
 * scramble_bits applied when the Additive scrambler sits after the inner code, then zeros.
 * llr_prepare: out [nframes][n] = the first n LLRs of in [nframes][in_stride],
 * apply_pn_to_llrs applied under the same condition. */
int orion_frame_pack_batch(const orion_frame_scheme* s, const uint8_t* payload, const int64_t* fields,
                           const int64_t* seeds, size_t nframes, size_t info_len, int out_bytes, uint8_t* out);
int orion_frame_pack_batch_device(const orion_frame_scheme* s, const uint8_t* payload, const int64_t* fields,
                                  const int64_t* seeds, size_t nframes, size_t info_len, int out_bytes, uint8_t* out,
                                  void* stream);
int orion_frame_unpack_batch(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, int in_bytes,
                             const int64_t* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                             size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                             int32_t* corrected, int64_t* fields);
int orion_frame_unpack_batch_device(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, int in_bytes,
                                    const int64_t* seeds, const int32_t* unsat, size_t n_inner,
                                    const int32_t* status, size_t n_outer, size_t nframes, size_t info_len,
                                    uint8_t* payload, uint8_t* flags, int32_t* corrected, int64_t* fields,
                                    void* stream);
int orion_frame_coded_bits_batch(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, size_t nbits,
                                 const int64_t* seeds, size_t nframes, size_t out_len, uint8_t* out);
int orion_frame_coded_bits_batch_device(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride,
                                        size_t nbits, const int64_t* seeds, size_t nframes, size_t out_len,
                                        uint8_t* out, void* stream);
int orion_frame_llr_prepare_batch(const orion_frame_scheme* s, const float* in, size_t in_stride, size_t n,
                                  const int64_t* seeds, size_t nframes, float* out);
int orion_frame_llr_prepare_batch_device(const orion_frame_scheme* s, const float* in, size_t in_stride, size_t n,
                                         const int64_t* seeds, size_t nframes, float* out, void* stream);
/* The frames' IQ on the device (cf32): out [nframes][lead_len + hdr_len + pay_len] = the shared
 * lead (S&C repeats and training symbol), then each frame's header and payload symbols. With
 * ramp [ramp_len] f32 (SymbolWindow's ramp, 2 ramp_len <= sps; NULL / 0 for none) every whole
 * symbol of sps samples from win_start on is tapered, the frame modulator's window post-pass. */
int orion_frame_assemble_batch_device(const void* lead, size_t lead_len, const void* hdr, size_t hdr_len,
                                      const void* pay, size_t pay_len, size_t nframes, size_t sps, size_t win_start,
                                      const float* ramp, size_t ramp_len, void* out, void* stream);
/* in [nframes][nbytes] -> out [nframes][nbytes * 8], MSB first */
int orion_frame_bytes_to_bits_batch(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out);
int orion_frame_bytes_to_bits_batch_device(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out,
                                           void* stream);

/* ---- OFDM burst acquisition: Schmidl & Cox packet search, fractional and integer carrier
 * offset (sync/ofdm_sync.rs:354-589). The host entries are the reference in its f32 operation
 * order; the batched search runs one independent search per capture on the GPU. ---- */
/* OfdmPreamble (sync/ofdm_sync.rs:45-75): training != 0 adds a training symbol of
 * training_n_fft + training_cp_len samples after the repeats. */
typedef struct {
  size_t num_repeats, repeat_len;
  int32_t training;
  size_t training_n_fft, training_cp_len;
} orion_ofdm_preamble;
/* OfdmSyncResult (sync/ofdm_sync.rs:94-107). */
typedef struct {
  int64_t start_sample;
  float cfo_hz;
  int32_t integer_cfo_bins;
  float score;
  uint32_t reserved;
} orion_ofdm_sync_result;
#define ORION_OFDM_SYNC_TOP 5 /* the integer search runs for this many ranked results */
/* The number of candidate offsets of a search, end - search_start with end = min(search_end,
 * n - total_len); 0 where ofdm_sync returns nothing whatever the samples. */
size_t orion_ofdm_sync_offsets(size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                               size_t search_end);
/* ofdm_sync on the host: iq [n] cf32 -> results [cap] ranked, *count of them (cap >=
 * orion_ofdm_sync_offsets(..)); r_peak (may be NULL) the largest window energy of a kept offset. */
int orion_ofdm_sync_host(const void* iq, size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                         size_t search_end, orion_ofdm_sync_result* results, size_t cap, size_t* count, float* r_peak);
/* The sums ofdm_sync ranks, per offset of the same range: p [offsets] cf32, r [offsets] f32. */
int orion_ofdm_sc_metric_host(const void* iq, size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                              size_t search_end, void* p, float* r);
/* earliest_accepted (sync/ofdm_sync.rs:488-503): *index into results, or -1. */
int orion_ofdm_earliest_accepted(const orion_ofdm_sync_result* results, size_t n, float score_threshold,
                                 size_t cluster_len, int64_t* index);
/* estimate_integer_cfo_bins (sync/ofdm_sync.rs:513-562) of the training symbol at
 * training_start; corr2 (may be NULL) [training_n_fft + 1] receives |corr|^2 per shift from
 * -training_n_fft / 2 on. */
int orion_ofdm_integer_cfo_host(const void* iq, size_t n, float fs, size_t training_n_fft, size_t training_cp_len,
                                size_t training_start, float fractional_cfo_hz, int32_t* bins, float* corr2);
/* Rotator::new(freq_hz, fs).rotate_block (dsp/rotator.rs:74-84) from a fresh oscillator: in,
 * out [n] cf32. */
int orion_ofdm_rotate_block_host(float freq_hz, float fs, const void* in, size_t n, void* out);
/* remove_common_phase_error (demodulate/ofdm_frame.rs:200-274) in place over syms
 * [n_sym][n_data] cf32 of a constellation (ORION_OFDM_*); nothing below 4 symbols. */
int orion_ofdm_cpe_host(int constellation, void* syms, size_t n_sym, size_t n_data);
/* The equalizer branch of soft_demap (demodulate/ofdm_frame.rs:95-134) on the host: n_sym
 * symbols of iq at the configuration's plan and RX window back-off, equalized by the weights
 * of training_freq [n_fft] cf32 (the received training symbol's transform at the same window),
 * the phase tracker, then the LLRs of constellation. syms [n_sym * n_data] cf32, llr [n_sym *
 * n_data * bits] f32 (may be NULL). No gain is divided out. */
int orion_ofdm_soft_demap_equalized_host(const orion_ofdm_config* cfg, int constellation, const void* iq, size_t n_sym,
                                         const void* training_freq, void* syms, float* llr);
/* What the batched search writes, device pointers: per offset p [ncap][offsets] cf32, r, score
 * (-1 at an offset ofdm_sync skips), cfo_hz [ncap][offsets] f32; per capture r_peak [ncap],
 * top_start / top_bins [ncap][5] i32 (the first five of ofdm_sync's ranking; -1 / 0 padded),
 * accepted_start [ncap] (earliest_accepted's choice at the call's threshold with cluster_len =
 * the preamble's total length; -1: none), accepted_in_top [ncap] (which of the five it is, or
 * -1), accepted_bins (its top-five entry, or 0), accepted_score, accepted_cfo_hz. */
typedef struct {
  void* p;
  float *r, *score, *cfo_hz, *r_peak;
  int32_t *top_start, *top_bins, *accepted_start, *accepted_in_top, *accepted_bins;
  float *accepted_score, *accepted_cfo_hz;
} orion_ofdm_sync_out;
/* NULL (and a message) for a training symbol the transform does not take. No device is touched. */
typedef struct orion_ofdm_acquire orion_ofdm_acquire;
orion_ofdm_acquire* orion_ofdm_acquire_new(const orion_ofdm_preamble* pre);
void orion_ofdm_acquire_free(orion_ofdm_acquire* a);
/* iq [ncap][n] cf32 on the device, finite; the range must hold an offset
 * (orion_ofdm_sync_offsets > 0). Asynchronous on stream. */
int orion_ofdm_sync_batch_device(orion_ofdm_acquire* a, const void* iq, size_t ncap, size_t n, float fs,
                                 size_t search_start, size_t search_end, float score_threshold,
                                 const orion_ofdm_sync_out* out, void* stream);
/* rows [ncap][n] cf32: capture c from sync->accepted_start[c] on, times the closed-form phasor
 * of -(accepted_cfo_hz + accepted_bins fs / n_fft) with the Rotator's phase index (k + 1 at
 * sample k), zero past the capture's end and in a capture with no accepted candidate; avail
 * [ncap] i32 the samples a row holds (0: none), total_cfo [ncap] f32. Only the three accepted_*
 * arrays named here are read. Asynchronous on stream. */
int orion_ofdm_acquire_correct_device(orion_ofdm_acquire* a, const void* iq, size_t ncap, size_t n, float fs, size_t n_fft,
                                      const orion_ofdm_sync_out* sync, void* rows, int32_t* avail, float* total_cfo,
                                      void* stream);
/* weights [ncap][training_n_fft] cf32: the corrected rows' training symbol transformed window
 * samples into the symbol (cp_len - RX window back-off), divided by the known pattern, then
 * equalizer_weight (demodulate/ofdm.rs:440-502). The preamble must carry a training symbol. */
int orion_ofdm_acquire_weights_device(orion_ofdm_acquire* a, const void* rows, size_t ncap, size_t n, size_t window,
                                      void* weights, void* stream);
/* The equalizer branch of the frame demodulator's soft_demap on the device, for frames of
 * n_symbols symbols of a demodulator handle's constellation: raw [frames][n_symbols * n_data]
 * cf32 (orion_ofdm_demod_device with no equalizer and gain 1) times weights [frames][n_fft] at
 * the data bins, remove_common_phase_error per frame (one wave each) -> syms, then their LLRs
 * -> llr [frames][n_symbols * n_data * bits] (may be NULL). */
int orion_ofdm_equalize_track_device(orion_ofdm* h, const void* raw, const void* weights, size_t frames, size_t n_symbols,
                                     void* syms, float* llr, void* stream);

/* ---- The DVB-T 2K frame (src/waveform/dvb_t.rs, dvb_t_tps.rs, src/sync/dvb_t_gi_sync.rs,
 * src/modulate/dvb_t_frame.rs, src/demodulate/dvb_t_frame.rs) -------------------------------
 * n_fft = 2048, 1705 active carriers, 1512 data carriers in each of the four scattered-pilot
 * phases (symbol mod 4). guard: 0..3 = 1/32, 1/16, 1/8, 1/4 (cp_len 64 .. 512). Bits are uint8,
 * one per byte; v is the bits per carrier (2, 4, 6). The *_host entries touch no device and
 * run the reference's f32 operation order; the *_device entries take device pointers, are
 * asynchronous on stream, keep no state between calls and give the host entries' bits
 * (cfo_hz: the device's atan2f). ORION_E_ARG for a value outside these ranges. */
#define ORION_DVBT_N_FFT 2048
#define ORION_DVBT_DATA_CARRIERS 1512
#define ORION_DVBT_TPS_CARRIERS 17
#define ORION_DVBT_CONTINUAL_PILOTS 45
#define ORION_DVBT_TPS_SYMBOLS 68
#define ORION_DVBT_MAX_REF_PILOTS 193
#define ORION_DVBT_MAX_RX_WINDOW_BACKOFF 85
/* The constants: continual [45] and tps [17] active-carrier indices (Tables 7 and 8), their
 * transform bins, wk [1705] the reference sequence; any pointer may be NULL. */
int orion_dvbt_constants(uint32_t* continual, uint32_t* tps, uint32_t* continual_bins, uint32_t* tps_bins, uint8_t* wk);
float orion_dvbt_boosted_pilot_value(uint8_t wk);
/* One phase of dvb_t_2k_plans: data_bins [1512] (active-carrier order), pilot_bins / pilot_vals
 * [n_pilots] every reserved carrier with its boosted value (real), ref_bins / ref_vals [n_ref]
 * the channel references (pilots minus TPS) sorted by bin; role [2048] (>= 0 the data index,
 * -1 null, -2 / -3 a pilot + / -, -4 - j TPS carrier j). Arrays hold 1512 / 256 / 256 / 2048. */
int orion_dvbt_phase(int phase, uint32_t* data_bins, uint32_t* pilot_bins, float* pilot_vals, size_t* n_pilots,
                     uint32_t* ref_bins, float* ref_vals, size_t* n_ref, int32_t* role);
/* dvb_t_map_symbol / dvb_t_demap_symbol / dvb_t_soft_llr over n symbols: bits and llr
 * [n][v], syms [n] cf32. */
int orion_dvbt_map_host(const uint8_t* bits, size_t n, size_t v, void* syms);
int orion_dvbt_demap_host(const void* syms, size_t n, size_t v, uint8_t* bits);
int orion_dvbt_llr_host(const void* syms, size_t n, size_t v, float* llr);
/* tps_bch_encode: info [53] -> codeword [67]; tps_bch_decode: codeword [67] -> info [53],
 * *ok = 0 where the reference returns None. */
int orion_dvbt_tps_bch_encode(const uint8_t* info, uint8_t* codeword);
int orion_dvbt_tps_bch_decode(const uint8_t* codeword, uint8_t* info, int* ok);
/* TpsWord::pack / unpack: fields [5] = frame_number, constellation (ORION_OFDM_QPSK / QAM16 /
 * QAM64), code rate (ORION_FEC_RATE_*), guard, cell_id; bits [68] s0 .. s67. */
int orion_dvbt_tps_pack(const int32_t* fields, uint8_t* bits);
int orion_dvbt_tps_unpack(const uint8_t* bits, int32_t* fields, int* ok);
/* TpsEncoder over n_symbols (reset after every 68th): cells [n_symbols][17] cf32.
 * TpsDecoder::feed_symbol over the first min(n_symbols, 68) symbols: bits [68], *n_bits. */
int orion_dvbt_tps_encode_host(const uint8_t* bits, size_t n_symbols, void* cells);
int orion_dvbt_tps_decide_host(const void* cells, size_t n_symbols, uint8_t* bits, size_t* n_bits);
/* dvb_t_gi_sync_with. |gamma| is defined as the f32 rounding of the f64 square root of the f64
 * sum of the two exact f64 squares (not libm's hypotf). out [5] f32: cfo_hz, score, gamma.re,
 * gamma.im, phi; *found = 0 where the reference returns None. metric (may be NULL) [search_len]. */
int orion_dvbt_gi_sync_host(const void* iq, size_t n, size_t n_fft, size_t cp_len, float fs, size_t search_len, float rho,
                            size_t max_symbols, float origin_score_ratio, int64_t* start, float* out, int* found,
                            float* metric);
/* dvb_t_integer_cfo over one symbol's bins freq [n_fft] cf32. */
int orion_dvbt_integer_cfo_host(const void* freq, size_t n_freq, size_t n_fft, int max_bins, int32_t* bins,
                                float* confidence, int* found);
/* The frame modulator from the coded bits on (modulate/dvb_t_frame.rs:213-261): bits [n_bits],
 * tps [68] -> iq [n_symbols (2048 + cp_len)] cf32; a data carrier whose bits lie past n_bits is
 * zero. The frame demodulator's symbol loop (demodulate/dvb_t_frame.rs:497-583) from the
 * acquired start: iq [n_symbols (2048 + cp_len)] -> llr [n_symbols][1512 v], cells
 * [n_symbols][17] cf32 (raw bins), syms (may be NULL) [n_symbols][1512] cf32. */
int orion_dvbt_mod_symbols_host(const uint8_t* bits, size_t n_bits, size_t v, size_t cp_len, const uint8_t* tps,
                                size_t n_symbols, size_t roll_off, void* iq);
int orion_dvbt_demod_symbols_host(const void* iq, size_t n_symbols, size_t cp_len, size_t backoff, size_t v, float* llr,
                                  void* cells, void* syms);
/* k_dvbt_mod, one workgroup per (frame, symbol): bits [frames][row_bits], nbits [frames] i32
 * (NULL: row_bits each), tps [frames][3] u32 (bit l of the 68-bit word is s_l) -> iq
 * [frames][n_symbols (2048 + cp_len)]. frames <= 65535. */
int orion_dvbt_mod_symbols_device(const uint8_t* bits, size_t frames, size_t row_bits, const int32_t* nbits,
                                  const uint32_t* tps, size_t v, size_t cp_len, size_t n_symbols, size_t roll_off,
                                  void* iq, void* stream);
/* k_gi_metric + k_gi_select, one independent search per capture of iq [ncap][n]: per capture
 * start, found (i32), score, cfo_hz, phi (f32), gamma (cf32); per offset metric, phi_all (f32)
 * and gamma_all (cf32), each [ncap][search_len]. ncap <= 65535, n < 2^31. */
typedef struct {
  int32_t* start;
  int32_t* found;
  float* score;
  float* cfo_hz;
  void* gamma;
  float* phi;
  float* metric;
  void* gamma_all;
  float* phi_all;
} orion_dvbt_gi_out;
int orion_dvbt_gi_sync_batch_device(const void* iq, size_t ncap, size_t n, size_t n_fft, size_t cp_len, float fs,
                                    size_t search_len, float rho, size_t max_symbols, float origin_score_ratio,
                                    const orion_dvbt_gi_out* out, void* stream);
/* k_dvbt_demod: iq [ncap][n] from start[c]; a capture with found[c] == 0 or whose frame does
 * not fit is skipped and its outputs are left as they are. Shapes as the host entry's per capture. */
int orion_dvbt_demod_symbols_device(const void* iq, size_t ncap, size_t n, const int32_t* start, const int32_t* found,
                                    size_t n_symbols, size_t cp_len, size_t backoff, size_t v, float* llr, void* cells,
                                    void* syms, void* stream);
/* k_tps_decode, one wave per frame: cells [frames][n_symbols][17] -> fields [frames][5] i32 (as
 * orion_dvbt_tps_unpack) and status [frames] i32 (0 decoded, 1 not). */
int orion_dvbt_tps_decode_device(const void* cells, size_t frames, size_t n_symbols, int32_t* fields, int32_t* status,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORION_SDR_AMD_H */
