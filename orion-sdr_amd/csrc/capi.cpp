// capi.cpp — extern "C" boundary (include/orion_sdr_amd.h) over the Block layer.
#include "../../include/orion_sdr_amd.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "acquire.hpp"
#include "bch.hpp"
#include "bch_blocks.hpp"
#include "blocks.hpp"
#include "dvbt.hpp"
#include "dvbt_blocks.hpp"
#include "fec.hpp"
#include "fec_blocks.hpp"
#include "frame.hpp"
#include "frame_blocks.hpp"
#include "ldpc.hpp"
#include "ldpc_family.hpp"
#include "ldpc_family_blocks.hpp"
#include "ofdm.hpp"
#include "ofdm_blocks.hpp"
#include "osc.hpp"
#include "psk31.hpp"
#include "psk31_blocks.hpp"
#include "rs.hpp"
#include "rs_blocks.hpp"
#include "scan_blocks.hpp"
#include "sync_blocks.hpp"

struct orion_block {
  std::unique_ptr<orion::Block> impl;
};
struct orion_sync {
  orion::Sync impl;
  orion::Psk31Sync psk;
};
struct orion_ft_mod {
  orion::FtMod impl;
  orion_ft_mod(int protocol, float fs, float base_hz, float rf_hz, float gain) : impl(protocol, fs, base_hz, rf_hz, gain) {}
};
struct orion_varicode_encoder {
  orion::psk31::VaricodeEncoder impl;
};
struct orion_varicode_decoder {
  orion::psk31::VaricodeDecoder impl;
};
struct orion_psk31_streaming_viterbi {
  orion::psk31::StreamingViterbi impl;
};
struct orion_psk31_mod {
  orion::Psk31ModDev dev;
  orion::psk31::Mod& impl;
  orion_psk31_mod(int mode, float fs, float rf_hz, float gain) : dev(mode, fs, rf_hz, gain), impl(dev.host()) {}
};
struct orion_psk31_demod {
  orion::psk31::Demod impl;
  orion_psk31_demod(int mode, float fs, float rf_hz, float gain, size_t offset) : impl(mode, fs, rf_hz, gain, offset) {}
};
struct orion_psk31_demod_bank {
  orion::Psk31DemodBank impl;
  orion_psk31_demod_bank(float fs, const orion::psk31::Stream* streams, size_t nstreams, size_t nch)
      : impl(fs, streams, nstreams, nch) {}
};
struct orion_rs_forney {
  orion::rs::ConvInterleaver impl;
};
struct orion_rs_pn_stream {
  orion::rs::PnScramblerStream impl;
};
struct orion_rs_dispersal {
  orion::rs::DvbTEnergyDispersal impl;
};
struct orion_ofdm_config {
  orion::ofdm::Config impl;
};
struct orion_fft {
  orion::FftDev impl;
  orion_fft(size_t n, bool inverse) : impl(n, inverse) {}
};
struct orion_ofdm_acquire {
  orion::AcquireEngine impl;
  explicit orion_ofdm_acquire(const orion::acquire::Preamble& p) : impl(p) {}
};
static_assert(sizeof(orion_ofdm_sync_result) == sizeof(orion::acquire::SyncResult) && sizeof(orion_ofdm_sync_result) == 24 &&
                  sizeof(orion_ofdm_sync_out) == sizeof(orion::SyncOut) && ORION_OFDM_SYNC_TOP == orion::acquire::kTopN,
              "orion_ofdm_sync_result / orion_ofdm_sync_out are acquire.hpp's records");
enum { kOfdmMod = 0, kOfdmDemod = 1, kOfdmDecider = 2, kOfdmSoftDemod = 3, kOfdmEqualizer = 4 };
struct orion_ofdm {
  int kind;
  orion::OfdmEngine impl;
  orion_ofdm(int k, const orion::ofdm::Config& c, int eq) : kind(k), impl(c, eq) {}
};
static_assert(ORION_OFDM_BPSK == orion::ofdm::kBpsk && ORION_OFDM_QAM256 == orion::ofdm::kQam256 &&
                  ORION_OFDM_PLAN_IN_GUARD_BAND == orion::ofdm::kPlanInGuardBand &&
                  ORION_OFDM_EQ_NONE == orion::ofdm::kEqNone &&
                  ORION_OFDM_EQ_PER_SYMBOL_PILOT_INTERP == orion::ofdm::kEqPerSymbolPilotInterp,
              "the header's OFDM constants are ofdm.hpp's");
static_assert(sizeof(orion_psk31_signal) == sizeof(orion::psk31::Signal) && sizeof(orion_psk31_signal) == 32,
              "orion_psk31_signal is psk31.hpp's record");
static_assert(sizeof(orion_psk31_stream) == sizeof(orion::psk31::Stream) && sizeof(orion_psk31_stream) == 32 &&
                  sizeof(orion_psk31_report) == 16 && ORION_PSK31_BPSK == orion::psk31::kBpsk &&
                  ORION_PSK31_QPSK == orion::psk31::kQpsk,
              "orion_psk31_stream is psk31.hpp's record");
static_assert(ORION_VARICODE_MAX_BITS == orion::psk31::kVaricodeMaxBits &&
                  ORION_PSK31_TRACEBACK_DEPTH == orion::psk31::kTracebackDepth,
              "the header's constants are psk31.hpp's");
static_assert(sizeof(orion_ft_signal) == sizeof(orion::ftmod::Signal) && sizeof(orion_ft_signal) == 24 &&
                  ORION_FT8_FRAME_LEN == 79 * 1920 && ORION_FT4_FRAME_LEN == 105 * 576,
              "orion_ft_signal is ftmod.hpp's record");
static_assert(sizeof(orion_candidate) == sizeof(orion::SyncCandidate) && sizeof(orion_candidate) == 12,
              "orion_candidate is the kernels' record");
static_assert(sizeof(orion_ldpc_result) == sizeof(orion::ldpc::Result) && sizeof(orion_ldpc_result) == 16 &&
                  sizeof(orion_decode_pick) == sizeof(orion::DecodePick) && sizeof(orion_decode_pick) == 16,
              "orion_ldpc_result / orion_decode_pick are the kernels' records");
static_assert(ORION_FEC_K5 == orion::fec::kK5 && ORION_FEC_DVB_K7 == orion::fec::kDvbK7 &&
                  ORION_FEC_RATE_1_2 == orion::fec::kR1_2 && ORION_FEC_RATE_7_8 == orion::fec::kR7_8,
              "the header's constants are fec.hpp's");
static_assert(ORION_LDPC_N == orion::ldpc::kN && ORION_LDPC_RULE_SUM_PRODUCT == orion::ldpc::kRuleSumProduct &&
                  ORION_LDPC_DECODED == orion::ldpc::kDecoded && ORION_COSTAS_FT4 == orion::ldpc::kFt4,
              "the header's constants are ldpc.hpp's");
static_assert(ORION_LDPCF_N512R12 == orion::ldpcf::kN512R12 && ORION_LDPCF_N512R34 == orion::ldpcf::kN512R34 &&
                  ORION_LDPCF_SUM_PRODUCT == orion::ldpcf::kRuleSumProduct &&
                  ORION_LDPCF_SCALED_MIN_SUM == orion::ldpcf::kRuleScaledMinSum,
              "the header's constants are ldpc_family.hpp's");

namespace {
thread_local std::string g_err;

int fail(int code, const char* what) {
  g_err = what ? what : "unknown error";
  return code;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const orion::HipError& e) {
    return fail(ORION_E_HIP, e.what());
  } catch (const std::invalid_argument& e) {
    return fail(ORION_E_ARG, e.what());
  } catch (const std::exception& e) {
    return fail(ORION_E_HIP, e.what());
  }
}

template <class F>
orion_block* make(F&& f) {
  try {
    auto b = new orion_block;
    b->impl = f();
    return b;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

// one block through a BlockInterleaver (orion_fec_interleave_* / orion_fec_deinterleave_*)
template <class T>
int fec_block(size_t rows, size_t cols, const T* in, T* out, bool inverse) {
  if (!in || !out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::fec::BlockInterleaver bi(rows, cols);
    if (inverse)
      bi.deinterleave(in, out);
    else
      bi.interleave(in, out);
    return ORION_OK;
  });
}

// a handle from a constructor that may throw
template <class F>
auto make_handle(F&& f) -> decltype(f()) {
  try {
    return f();
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
template <class F>
size_t size_or_zero(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    fail(ORION_E_ARG, e.what());
    return 0;
  }
}
orion::RsFusion rs_fusion(int bits, size_t branches, size_t depth, int disperse) {
  orion::RsFusion f;
  f.bits = bits != 0;
  f.branches = branches;
  f.depth = depth;
  f.disperse = disperse != 0;
  return f;
}
constexpr size_t kRsMaxHostWords = size_t(1) << 32;
}  // namespace

extern "C" {

const char* orion_version(void) { return "orion-sdr-amd 0.1.0 (gfx950)"; }
const char* orion_last_error(void) { return g_err.c_str(); }

int orion_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int orion_set_device(int d) {
  return guarded([&] {
    ORION_HIP(hipSetDevice(d));
    return ORION_OK;
  });
}
size_t orion_diag_stream_read_bytes(size_t bytes) {
  try {
    return static_cast<size_t>(orion::stream_read_bytes(static_cast<long long>(bytes)));
  } catch (...) {
    return 0;
  }
}
int orion_diag_stream_read(const void* dev, size_t bytes, void* stream) {
  if (!dev) return fail(ORION_E_NULL, "null buffer");
  if (reinterpret_cast<uintptr_t>(dev) % 16) return fail(ORION_E_ARG, "buffer not 16-B aligned");
  return guarded([&] {
    static orion::DevBuf sink(256);
    orion::launch_stream_read(dev, static_cast<long long>(bytes), sink.as<float>(),
                              static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
void* orion_host_alloc(size_t bytes) {
  try {
    return orion::host_alloc(bytes);
  } catch (const std::exception& e) {
    fail(ORION_E_HIP, e.what());
    return nullptr;
  }
}
int orion_host_free(void* p) {
  return guarded([&] {
    orion::host_free(p);
    return ORION_OK;
  });
}
int orion_device_cus(void) {
  try {
    return orion::device_cus();
  } catch (const std::exception& e) {
    return fail(ORION_E_HIP, e.what());
  }
}
int orion_diag_spin(void* stream, uint32_t workgroups, uint32_t lds_bytes, double seconds) {
  return guarded([&] {
    orion::launch_spin(static_cast<int>(workgroups), static_cast<int>(lds_bytes), seconds,
                       static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
void* orion_diag_stream_create(uint32_t n_cus) {
  hipStream_t st = nullptr;
  try {
    if (n_cus == 0) {
      ORION_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    } else {
      const int ncu = orion::device_cus();
      std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
      for (uint32_t c = 0; c < n_cus && c < static_cast<uint32_t>(ncu); ++c) mask[c / 32] |= 1u << (c % 32);
      ORION_HIP(hipExtStreamCreateWithCUMask(&st, static_cast<uint32_t>(mask.size()), mask.data()));
    }
  } catch (const std::exception& e) {
    fail(ORION_E_HIP, e.what());
    return nullptr;
  }
  return st;
}
int orion_diag_stream_destroy(void* stream) {
  if (!stream) return fail(ORION_E_NULL, "null stream");
  return guarded([&] {
    ORION_HIP(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return ORION_OK;
  });
}
int orion_synchronize(void* stream) {
  return guarded([&] {
    ORION_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return ORION_OK;
  });
}

orion_block* orion_rotator_new(float freq_hz, float fs) {
  return make([&] { return orion::make_rotator(freq_hz, fs); });
}
orion_block* orion_nco_new(float freq_hz, float fs) {
  return make([&] { return orion::make_nco(freq_hz, fs); });
}
int orion_rotator_set_freq(orion_block* b, float freq_hz, float fs) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::osc_set_freq(b->impl.get(), "Rotator", freq_hz, fs)) return fail(ORION_E_TYPE, "not a Rotator");
    return ORION_OK;
  });
}
int orion_rotator_reset_phase(orion_block* b) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::osc_reset_phase(b->impl.get())) return fail(ORION_E_TYPE, "not a Rotator");
    return ORION_OK;
  });
}
int orion_rotator_mix_usb_block_device(orion_block* b, const void* in, size_t n_in, float* out, size_t out_cap,
                                       void* stream, orion_work_report* wr) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((!in && n_in) || (!out && out_cap)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    b->impl->check_device_errors();
    const size_t n = std::min(n_in, out_cap);  // rotator.rs:89
    if (orion::osc_mix_usb(b->impl.get(), in, n, out, static_cast<hipStream_t>(stream)))
      return fail(ORION_E_TYPE, "not a Rotator");
    if (wr) { wr->in_read = n; wr->out_written = n; }
    return ORION_OK;
  });
}
int orion_rotator_mix_usb_block(orion_block* b, const void* in, size_t n_in, float* out, size_t out_cap,
                                orion_work_report* wr) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((!in && n_in) || (!out && out_cap)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const size_t n = std::min(n_in, out_cap);
    orion::DevBuf di(n * 8 + 16), dout(n * 4 + 16);
    if (n) ORION_HIP(hipMemcpy(di.as<void>(), in, n * 8, hipMemcpyHostToDevice));
    if (orion::osc_mix_usb(b->impl.get(), di.as<void>(), n, dout.as<float>(), nullptr))
      return fail(ORION_E_TYPE, "not a Rotator");
    if (n) ORION_HIP(hipMemcpy(out, dout.as<void>(), n * 4, hipMemcpyDeviceToHost));
    ORION_HIP(hipDeviceSynchronize());
    if (wr) { wr->in_read = n; wr->out_written = n; }
    return ORION_OK;
  });
}
int orion_nco_set_freq(orion_block* b, float freq_hz) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::osc_set_freq(b->impl.get(), "Nco", freq_hz, 0.0f)) return fail(ORION_E_TYPE, "not an Nco");
    return ORION_OK;
  });
}
namespace {
int next_cs_device(orion_block* b, const char* kind, void* out, size_t n, void* stream) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (!out && n) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    b->impl->check_device_errors();
    if (orion::osc_next_cs(b->impl.get(), kind, out, n, static_cast<hipStream_t>(stream)))
      return fail(ORION_E_TYPE, "wrong oscillator kind");
    return ORION_OK;
  });
}
int next_cs_host(orion_block* b, const char* kind, void* out, size_t n) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (!out && n) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::DevBuf d(n * 8 + 16);
    if (orion::osc_next_cs(b->impl.get(), kind, d.as<void>(), n, nullptr)) return fail(ORION_E_TYPE, "wrong oscillator kind");
    if (n) ORION_HIP(hipMemcpy(out, d.as<void>(), n * 8, hipMemcpyDeviceToHost));
    ORION_HIP(hipDeviceSynchronize());
    return ORION_OK;
  });
}
}  // namespace
int orion_nco_next_cs_block_device(orion_block* b, void* out, size_t n, void* stream) {
  return next_cs_device(b, "Nco", out, n, stream);
}
int orion_nco_next_cs_block(orion_block* b, void* out, size_t n) { return next_cs_host(b, "Nco", out, n); }
int orion_rotator_next_cs_block_device(orion_block* b, void* out, size_t n, void* stream) {
  return next_cs_device(b, "Rotator", out, n, stream);
}
int orion_rotator_next_cs_block(orion_block* b, void* out, size_t n) { return next_cs_host(b, "Rotator", out, n); }
orion_block* orion_fir_decimator_new(float fs, size_t m, float cutoff_hz, float trans_hz) {
  return make([&] { return orion::make_fir_decimator(fs, m, cutoff_hz, trans_hz, 1); });
}
orion_block* orion_fir_decimator_batch_new(float fs, size_t m, float cutoff_hz, float trans_hz, size_t nch) {
  return make([&] { return orion::make_fir_decimator(fs, m, cutoff_hz, trans_hz, static_cast<int>(nch)); });
}
orion_block* orion_fir_lowpass_new(float fs, float pass_hz, float trans_hz) {
  return make([&] { return orion::make_fir_lowpass(fs, pass_hz, trans_hz); });
}
orion_block* orion_fir_lowpass_iq_design(size_t num_taps, float cutoff_norm, float stopband_db) {
  return make([&] { return orion::make_fir_lowpass_iq(orion::kaiser_lowpass_taps(num_taps, cutoff_norm, stopband_db)); });
}
orion_block* orion_fir_lowpass_iq_from_taps(const float* taps, size_t n) {
  return make([&] { return orion::make_fir_lowpass_iq(std::vector<float>(taps, taps + (taps ? n : 0))); });
}
orion_block* orion_fir_lowpass_iq_batch_from_taps(const float* taps, size_t n, size_t nch) {
  return make([&] {
    if (nch < 1 || nch > (1u << 16)) throw std::invalid_argument("FirLowpassIq batch: 1 <= nch <= 65536");
    return orion::make_fir_lowpass_iq(std::vector<float>(taps, taps + (taps ? n : 0)), static_cast<int>(nch));
  });
}
int orion_osc_table_phasors(float freq_hz, float fs, uint64_t max_out, void* out, size_t n, uint64_t* cyc_start,
                            uint64_t* cyc_len, uint64_t* n_tab) {
  if (!out && n) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (max_out > orion::kNcoTableMax) return fail(ORION_E_ARG, "budget above 2^28");
    const orion::Oscillator o = orion::oscillator(freq_hz, fs);
    const orion::RecTable t = orion::rec_table(o.w_re, o.w_im, orion::RecState{}, max_out, orion::kOscSpan, o.step_q64);
    float* z = static_cast<float*>(out);
    for (size_t k = 0; k < n; ++k) {
      const orion::RecState st = orion::rec_state_after(t, k);
      z[2 * k] = st.zr;
      z[2 * k + 1] = st.zi;
    }
    if (cyc_start) *cyc_start = t.cyc_start;
    if (cyc_len) *cyc_len = t.cyc_len;
    if (n_tab) *n_tab = t.n;
    return ORION_OK;
  });
}
int orion_fir_lowpass_iq_num_taps(const orion_block* b, size_t* n) {
  if (!b || !n) return fail(ORION_E_NULL, "null argument");
  if (std::strcmp(b->impl->name(), "FirLowpassIq") != 0) return fail(ORION_E_TYPE, "not a FirLowpassIq");
  *n = b->impl->taps(0).size();  // fir.rs:210-212 taps.len()
  return ORION_OK;
}
int orion_fir_lowpass_iq_group_delay(const orion_block* b, size_t* d) {
  size_t n = 0;
  const int rc = orion_fir_lowpass_iq_num_taps(b, &n);
  if (rc) return rc;
  *d = (n - 1) / 2;  // fir.rs:216-218 (taps.len() - 1) / 2; from_taps keeps len >= 1
  return ORION_OK;
}
int orion_fir_lowpass_iq_filter_aligned_device(orion_block* b, void* io, size_t n, void* stream) {
  if (!b || (!io && n)) return fail(ORION_E_NULL, "null argument");
  return guarded([&] { return orion::fir_lowpass_iq_filter_aligned(b->impl.get(), io, n, static_cast<hipStream_t>(stream)); });
}
int orion_fir_lowpass_iq_filter_aligned(orion_block* b, void* io, size_t n) {
  if (!b || (!io && n)) return fail(ORION_E_NULL, "null argument");
  return guarded([&] {
    orion::DevBuf d(n * 8 + 8);
    if (n) ORION_HIP(hipMemcpy(d.as<void>(), io, n * 8, hipMemcpyHostToDevice));
    const int rc = orion::fir_lowpass_iq_filter_aligned(b->impl.get(), d.as<void>(), n, nullptr);
    if (rc) return rc;
    if (n) ORION_HIP(hipMemcpy(io, d.as<void>(), n * 8, hipMemcpyDeviceToHost));
    ORION_HIP(hipDeviceSynchronize());
    return ORION_OK;
  });
}
orion_block* orion_agc_rms_new(float fs, float attack_ms, float release_ms, float target_rms) {
  return make([&] { return orion::make_agc(false, fs, attack_ms, release_ms, target_rms); });
}
orion_block* orion_agc_rms_iq_new(float fs, float attack_ms, float release_ms, float target_rms) {
  return make([&] { return orion::make_agc(true, fs, attack_ms, release_ms, target_rms); });
}
orion_block* orion_am_dsb_mod_new(float fs, float rf_hz, float carrier_level, float modulation_index) {
  return make([&] { return orion::make_am_mod(fs, rf_hz, carrier_level, modulation_index); });
}
int orion_am_dsb_mod_set_gain(orion_block* b, float g) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (std::strcmp(b->impl->name(), "AmDsbMod") != 0) return fail(ORION_E_TYPE, "not an AmDsbMod");
  return guarded([&] { return orion::mod_set_gain(b->impl.get(), g); });
}
int orion_am_dsb_mod_set_clamp(orion_block* b, int on) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::am_mod_set_clamp(b->impl.get(), on != 0)) return fail(ORION_E_TYPE, "not an AmDsbMod");
    return ORION_OK;
  });
}
orion_block* orion_fm_phase_accum_mod_new(float fs, float deviation_hz, float rf_hz) {
  return make([&] { return orion::make_fm_mod(fs, deviation_hz, rf_hz); });
}
int orion_fm_phase_accum_mod_set_deviation(orion_block* b, float deviation_hz) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::fm_mod_set_deviation(b->impl.get(), deviation_hz)) return fail(ORION_E_TYPE, "not an FmPhaseAccumMod");
    return ORION_OK;
  });
}
int orion_fm_phase_accum_mod_set_gain(orion_block* b, float g) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (std::strcmp(b->impl->name(), "FmPhaseAccumMod") != 0) return fail(ORION_E_TYPE, "not an FmPhaseAccumMod");
  return guarded([&] { return orion::mod_set_gain(b->impl.get(), g); });
}
orion_block* orion_pm_direct_phase_mod_new(float fs, float kp_rad_per_unit, float rf_hz) {
  return make([&] { return orion::make_pm_mod(fs, kp_rad_per_unit, rf_hz); });
}
int orion_pm_direct_phase_mod_set_gain(orion_block* b, float g) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (std::strcmp(b->impl->name(), "PmDirectPhaseMod") != 0) return fail(ORION_E_TYPE, "not a PmDirectPhaseMod");
  return guarded([&] { return orion::mod_set_gain(b->impl.get(), g); });
}
int orion_pm_direct_phase_mod_set_sensitivity(orion_block* b, float kp_rad_per_unit) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::pm_mod_set_sensitivity(b->impl.get(), kp_rad_per_unit)) return fail(ORION_E_TYPE, "not a PmDirectPhaseMod");
    return ORION_OK;
  });
}
orion_block* orion_cw_keyed_mod_new(float fs, float tone_hz, float rise_ms, float fall_ms) {
  return make([&] { return orion::make_cw_mod(fs, tone_hz, rise_ms, fall_ms); });
}
int orion_cw_keyed_mod_set_gain(orion_block* b, float g) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::cw_mod_set_gain(b->impl.get(), g)) return fail(ORION_E_TYPE, "not a CwKeyedMod");
    return ORION_OK;
  });
}
orion_block* orion_ssb_phasing_mod_new(float fs, float audio_bw_hz, float audio_if_hz, float rf_hz, int usb) {
  return make([&] { return orion::make_ssb_mod(fs, audio_bw_hz, audio_if_hz, rf_hz, usb != 0); });
}
orion_block* orion_lp_cascade_new(float fs, float fc) {
  return make([&] { return orion::make_lp_cascade(fs, fc); });
}
orion_block* orion_biquad_new(float b0, float b1, float b2, float a1, float a2) {
  return make([&] { return orion::make_biquad(b0, b1, b2, a1, a2); });
}
orion_block* orion_lp_dc_cascade_new(float fs, float lp_fc, float dc_cut_hz) {
  return make([&] { return orion::make_lp_dc_cascade(fs, lp_fc, dc_cut_hz); });
}
int orion_lp_dc_cascade_set_map(orion_block* b, int map) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    const int rc = orion::lp_dc_cascade_set_map(b->impl.get(), map);
    if (rc == -4) return fail(ORION_E_TYPE, "not an LpDcCascade");
    if (rc == -3) return fail(ORION_E_ARG, "unknown process_mapped map (ORION_MAP_IDENTITY / SQRT / ABS)");
    return ORION_OK;
  });
}
int orion_lp_dc_cascade_set_sqrt_map(orion_block* b, int on) {
  return orion_lp_dc_cascade_set_map(b, on ? ORION_MAP_SQRT : ORION_MAP_IDENTITY);
}
orion_block* orion_dc_blocker_new(float fs, float cut_hz) {
  return make([&] { return orion::make_dc_blocker(fs, cut_hz); });
}
orion_block* orion_fm_quadrature_demod_new(float fs, float dev_hz, float audio_bw_hz) {
  return make([&] { return orion::make_fm_demod(fs, dev_hz, audio_bw_hz); });
}
int orion_fm_quadrature_demod_with_translate(orion_block* b, float freq_hz) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] { return orion::fm_demod_with_translate(b->impl.get(), freq_hz); });
}
orion_block* orion_pm_quadrature_demod_new(float fs, float k, float audio_bw_hz) {
  return make([&] { return orion::make_pm_demod(fs, k, audio_bw_hz); });
}
orion_block* orion_ssb_product_demod_new(float fs, float bfo_hz, float audio_bw_hz) {
  return make([&] { return orion::make_ssb_demod(fs, bfo_hz, audio_bw_hz, 1); });
}
orion_block* orion_ssb_product_demod_batch_new(float fs, float bfo_hz, float audio_bw_hz, size_t nch) {
  return make([&] { return orion::make_ssb_demod(fs, bfo_hz, audio_bw_hz, static_cast<int>(nch)); });
}
orion_block* orion_am_envelope_demod_new(float fs, float audio_bw_hz) {
  return make([&] { return orion::make_am_demod(fs, audio_bw_hz); });
}
int orion_am_envelope_demod_with_abs_approx(orion_block* b, float k1, float k2) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] { return orion::am_demod_with_abs_approx(b->impl.get(), k1, k2); });
}
orion_block* orion_cw_envelope_demod_new(float fs, float tone_hz, float env_bw_hz) {
  return make([&] { return orion::make_cw_demod(fs, tone_hz, env_bw_hz); });
}
int orion_cw_envelope_demod_set_gain(orion_block* b, float g) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] { return orion::cw_demod_set_gain(b->impl.get(), g); });
}

static orion::WbfmParams wbfm_params(const orion_wbfm_params* p) {
  return {p->fs, p->dec_cutoff, p->dec_trans, p->dev_hz, p->audio_bw, p->audio_pass, p->audio_trans, p->m};
}
orion_block* orion_wbfm_chain_new(const orion_wbfm_params* p) {
  if (!p) { g_err = "null params"; return nullptr; }
  return make([&] { return orion::make_wbfm_chain(wbfm_params(p), {p->f_off}); });
}
orion_block* orion_wbfm_chain_batch_new(const orion_wbfm_params* p, const float* f_off, size_t nch) {
  if (!p || !f_off || nch == 0) { g_err = "null params / no channels"; return nullptr; }
  return make([&] { return orion::make_wbfm_chain(wbfm_params(p), std::vector<float>(f_off, f_off + nch)); });
}

int orion_wbfm_chain_configure(orion_block* b, int path, int max_segments) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    const int rc = orion::wbfm_chain_configure(b->impl.get(), path, max_segments);
    if (rc == -4) return fail(ORION_E_TYPE, "not a WBFM chain");
    if (rc != 0) return fail(ORION_E_ARG, "WBFM path unavailable for this design (or bad arguments)");
    return ORION_OK;
  });
}

int orion_wbfm_chain_seek(orion_block* b, uint64_t index) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    if (orion::wbfm_chain_seek(b->impl.get(), index) == -4) return fail(ORION_E_TYPE, "not a WBFM chain");
    return ORION_OK;
  });
}

int orion_block_process(orion_block* b, const void* in, size_t n_in, void* out, size_t out_cap,
                        orion_work_report* wr) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((!in && n_in) || (!out && out_cap)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::WorkReport w = b->impl->process_host(in, n_in, out, out_cap);
    if (wr) { wr->in_read = w.in_read; wr->out_written = w.out_written; }
    return ORION_OK;
  });
}
int orion_block_process_device(orion_block* b, const void* in, size_t n_in, void* out, size_t out_cap,
                               void* stream, orion_work_report* wr) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((!in && n_in) || (!out && out_cap)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::Block& blk = *b->impl;
    const size_t nch = static_cast<size_t>(blk.channels());
    const size_t ib = nch * n_in * orion::dt_size(blk.in_type()), ob = nch * out_cap * orion::dt_size(blk.out_type());
    const char *ip = static_cast<const char*>(in), *op = static_cast<const char*>(out);
    if (ib && ob && ip < op + ob && op < ip + ib && !blk.alias_ok())
      return fail(ORION_E_ARG, "input and output device ranges overlap (not supported by this block)");
    b->impl->check_device_errors();  // a wait that timed out in an earlier call of this handle
    const orion::WorkReport w = b->impl->process_device(in, n_in, out, out_cap, static_cast<hipStream_t>(stream));
    if (wr) { wr->in_read = w.in_read; wr->out_written = w.out_written; }
    return ORION_OK;
  });
}
int orion_batch_process(orion_block* b, const void* in, size_t n_ch, size_t n_per_ch, void* out, size_t out_cap,
                        void* stream, orion_work_report* wr) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if (n_ch != static_cast<size_t>(b->impl->channels()))
    return fail(ORION_E_ARG, "n_ch differs from the handle's channel count (build it with a *_batch_new constructor)");
  return orion_block_process_device(b, in, n_per_ch, out, out_cap, stream, wr);
}
int orion_block_configure(orion_block* b, int option, long long value) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    const int rc = b->impl->configure(option, value);
    if (rc == -4) return fail(ORION_E_TYPE, "option not supported by this block");
    if (rc != 0) return fail(ORION_E_ARG, "bad option value");
    return ORION_OK;
  });
}
int orion_block_status(orion_block* b) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    b->impl->check_device_errors();
    return ORION_OK;
  });
}
void orion_debug_set_spin_limit(uint32_t polls) { orion::set_spin_limit(polls); }
uint32_t orion_debug_spin_limit(void) { return orion::spin_limit(); }
int orion_block_reset(orion_block* b) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    b->impl->reset();
    return ORION_OK;
  });
}
void orion_block_free(orion_block* b) { delete b; }
int orion_block_in_type(const orion_block* b) { return b ? static_cast<int>(b->impl->in_type()) : ORION_E_NULL; }
int orion_block_out_type(const orion_block* b) { return b ? static_cast<int>(b->impl->out_type()) : ORION_E_NULL; }
size_t orion_block_out_len(const orion_block* b, size_t n) { return b ? b->impl->out_len(n) : 0; }
size_t orion_block_channels(const orion_block* b) { return b ? static_cast<size_t>(b->impl->channels()) : 0; }
const char* orion_block_name(const orion_block* b) { return b ? b->impl->name() : ""; }
int orion_block_taps(const orion_block* b, int which, float* out, size_t cap, size_t* n) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  const auto t = b->impl->taps(which);
  if (n) *n = t.size();
  if (out) std::memcpy(out, t.data(), std::min(cap, t.size()) * sizeof(float));
  return ORION_OK;
}

size_t orion_fir_lowpass_design(float fs, float pass_hz, float trans_hz, float* taps, size_t cap) {
  const auto t = orion::fir_lowpass_taps(fs, pass_hz, trans_hz);
  if (taps) std::memcpy(taps, t.data(), std::min(cap, t.size()) * sizeof(float));
  return t.size();
}
size_t orion_kaiser_lowpass_taps(size_t num_taps, float cutoff_norm, float stopband_db, float* taps, size_t cap) {
  const auto t = orion::kaiser_lowpass_taps(num_taps, cutoff_norm, stopband_db);
  if (taps) std::memcpy(taps, t.data(), std::min(cap, t.size()) * sizeof(float));
  return t.size();
}
float orion_kaiser_transition_norm(size_t num_taps, float stopband_db) {
  return orion::kaiser_transition_norm(num_taps, stopband_db);
}
size_t orion_kaiser_num_taps(float transition_norm, float stopband_db) {
  return orion::kaiser_num_taps(transition_norm, stopband_db);
}
static orion::TxLowpassSpec tx_spec(const orion_tx_lowpass* t) { return {t->cutoff_norm, t->num_taps, t->stopband_db}; }
orion_tx_lowpass orion_tx_lowpass_for_null_band(size_t n_fft, size_t occupied_half, size_t num_taps, float stopband_db) {
  const auto s = orion::tx_lowpass_for_null_band(n_fft, occupied_half, num_taps, stopband_db);
  return {s.cutoff_norm, s.num_taps, s.stopband_db};
}
size_t orion_tx_lowpass_taps_for_null_band(size_t n_fft, size_t occupied_half, float stopband_db) {
  return orion::tx_lowpass_taps_for_null_band(n_fft, occupied_half, stopband_db);
}
size_t orion_tx_lowpass_group_delay(const orion_tx_lowpass* t) { return t ? orion::tx_lowpass_group_delay(tx_spec(t)) : 0; }
float orion_tx_lowpass_transition_norm(const orion_tx_lowpass* t) {
  return t ? orion::tx_lowpass_transition_norm(tx_spec(t)) : 0.0f;
}
int orion_tx_lowpass_transition_fits(const orion_tx_lowpass* t, size_t n_fft, size_t occupied_half) {
  return t && orion::tx_lowpass_transition_fits(tx_spec(t), n_fft, occupied_half) ? 1 : 0;
}
float orion_tx_lowpass_stopband_edge_norm(const orion_tx_lowpass* t) {
  return t ? orion::tx_lowpass_stopband_edge_norm(tx_spec(t)) : 0.0f;
}
int orion_tx_lowpass_fits_guard(const orion_tx_lowpass* t, size_t cp_len, size_t roll_off, size_t backoff) {
  return t && orion::tx_lowpass_fits_guard(tx_spec(t), cp_len, roll_off, backoff) ? 1 : 0;
}
orion_block* orion_tx_lowpass_filter(const orion_tx_lowpass* t) {
  if (!t) { g_err = "null spec"; return nullptr; }
  return make([&] { return orion::make_fir_lowpass_iq(orion::kaiser_lowpass_taps(t->num_taps, t->cutoff_norm, t->stopband_db)); });
}
void orion_lp_cascade_design(float fs, float fc, float out5[5]) {
  const auto c = orion::lp_cascade_design(fs, fc);
  out5[0] = c.b0; out5[1] = c.b1; out5[2] = c.b2; out5[3] = c.a1; out5[4] = c.a2;
}

/* ---- FT8 / FT4 sync (sync_blocks.hpp) ---- */
orion_sync* orion_sync_new(void) {
  try {
    return new orion_sync;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_sync_free(orion_sync* h) { delete h; }
int orion_sync_set_rows_per_lane(orion_sync* h, int rows) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    h->impl.set_rows_per_lane(rows);
    return ORION_OK;
  });
}
int orion_waterfall_compute(orion_sync* h, const void* iq, float fs, float base_hz, float tone_spacing_hz,
                            size_t samples_per_sym, size_t num_syms, size_t num_tones, size_t time_offset,
                            size_t nch, size_t n_per_ch, int mode, float* mag) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || (!mag && num_syms && num_tones)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.waterfall_host(iq, fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones, time_offset, nch,
                           n_per_ch, mode, mag);
    return ORION_OK;
  });
}
int orion_waterfall_compute_device(orion_sync* h, const void* iq, float fs, float base_hz, float tone_spacing_hz,
                                   size_t samples_per_sym, size_t num_syms, size_t num_tones, size_t time_offset,
                                   size_t nch, size_t n_per_ch, int mode, float* mag, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || (!mag && num_syms && num_tones)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.waterfall(iq, fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones, time_offset, nch,
                      n_per_ch, mode, mag, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_costas_find_candidates_device(orion_sync* h, const float* wf, size_t nch, size_t num_syms,
                                        size_t num_tones, int pattern, int t_min, int t_max, size_t max_cand,
                                        orion_candidate* cand, uint32_t* count, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!wf && num_syms && num_tones) || !count || (!cand && max_cand)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.find_candidates(wf, nch, num_syms, num_tones, pattern, t_min, t_max, max_cand,
                            reinterpret_cast<orion::SyncCandidate*>(cand), count, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_sync_llr_device(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern,
                          const orion_candidate* cand, const uint32_t* count, size_t max_cand, float* llr,
                          void* stream) {
  if ((!wf && num_syms && num_tones) || !count || !cand || !llr) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::sync_llr(wf, nch, num_syms, num_tones, pattern, reinterpret_cast<const orion::SyncCandidate*>(cand), count,
                    max_cand, llr, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
namespace {
int sync_device(int pattern, orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr,
                void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || (max_cand && (!cand || !llr))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.sync(pattern, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand,
                 reinterpret_cast<orion::SyncCandidate*>(cand), count, llr, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int sync_host(int pattern, orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
              float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || (max_cand && (!cand || !llr))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.sync_host(pattern, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand,
                      reinterpret_cast<orion::SyncCandidate*>(cand), count, llr);
    return ORION_OK;
  });
}
}  // namespace
int orion_ft8_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                   int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr) {
  return sync_host(ORION_COSTAS_FT8, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, cand, count, llr);
}
int orion_ft8_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                          float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand,
                          uint32_t* count, float* llr, void* stream) {
  return sync_device(ORION_COSTAS_FT8, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, cand, count,
                     llr, stream);
}
int orion_ft4_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                   int t_min, int t_max, size_t max_cand, orion_candidate* cand, uint32_t* count, float* llr) {
  return sync_host(ORION_COSTAS_FT4, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, cand, count, llr);
}
int orion_ft4_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                          float max_hz, int t_min, int t_max, size_t max_cand, orion_candidate* cand,
                          uint32_t* count, float* llr, void* stream) {
  return sync_device(ORION_COSTAS_FT4, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, cand, count,
                     llr, stream);
}
int orion_sync_geometry(int pattern, float base_hz, float max_hz, int t_min, int t_max, size_t geom[5]) {
  if (!geom) return fail(ORION_E_NULL, "null argument");
  return guarded([&] {
    const orion::SyncGeometry g = orion::sync_geometry(pattern, base_hz, max_hz, t_min, t_max);
    geom[0] = g.num_bins;
    geom[1] = g.wf_syms;
    geom[2] = g.wf_sample_start;
    geom[3] = static_cast<size_t>(g.sym_offset_adj);
    geom[4] = static_cast<size_t>(g.wf_t_max);
    return ORION_OK;
  });
}

/* ---- FT8 / FT4 channel codec (ldpc.hpp, k_ldpc.hip) ---- */
int orion_ldpc_decode(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                      size_t max_iter, orion_ldpc_result* results, uint8_t* plain) {
  if (n && (!llr || !results)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc_decode_host(llr, n, count, max_cand, protocol, rule, max_iter, results, plain);
    return ORION_OK;
  });
}
int orion_ldpc_decode_device(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                             size_t max_iter, orion_ldpc_result* results, uint8_t* plain, void* stream) {
  if (n && (!llr || !results)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc_decode(llr, n, count, max_cand, protocol, rule, max_iter, results, plain,
                       static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
namespace {
int decode_device(int pattern, orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                  float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                  uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || !pick || (max_cand && (!cand || !llr || !results)))
    return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.decode(pattern, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter,
                   reinterpret_cast<orion::SyncCandidate*>(cand), count, llr, results,
                   reinterpret_cast<orion::DecodePick*>(pick), static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int decode_host(int pattern, orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || !pick || (max_cand && (!cand || !results))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.decode_host(pattern, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter,
                        reinterpret_cast<orion::SyncCandidate*>(cand), count, llr, results,
                        reinterpret_cast<orion::DecodePick*>(pick));
    return ORION_OK;
  });
}
}  // namespace
int orion_ft8_decode(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                     uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick) {
  return decode_host(ORION_COSTAS_FT8, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter,
                     cand, count, llr, results, pick);
}
int orion_ft8_decode_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter,
                            orion_candidate* cand, uint32_t* count, float* llr, orion_ldpc_result* results,
                            orion_decode_pick* pick, void* stream) {
  return decode_device(ORION_COSTAS_FT8, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule,
                       max_iter, cand, count, llr, results, pick, stream);
}
int orion_ft4_decode(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, orion_candidate* cand,
                     uint32_t* count, float* llr, orion_ldpc_result* results, orion_decode_pick* pick) {
  return decode_host(ORION_COSTAS_FT4, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter,
                     cand, count, llr, results, pick);
}
int orion_ft4_decode_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, int t_min, int t_max, size_t max_cand, int rule, size_t max_iter,
                            orion_candidate* cand, uint32_t* count, float* llr, orion_ldpc_result* results,
                            orion_decode_pick* pick, void* stream) {
  return decode_device(ORION_COSTAS_FT4, h, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule,
                       max_iter, cand, count, llr, results, pick, stream);
}
int orion_ft8_encode(const uint8_t payload[10], uint8_t tones[58], const uint8_t* a91_xor) {
  if (!payload || !tones) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc::encode_tones(orion::ldpc::kFt8, payload, tones, a91_xor);
    return ORION_OK;
  });
}
int orion_ft4_encode(const uint8_t payload[10], uint8_t tones[87], const uint8_t* a91_xor) {
  if (!payload || !tones) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc::encode_tones(orion::ldpc::kFt4, payload, tones, a91_xor);
    return ORION_OK;
  });
}
int orion_ft_frame_to_llr_hard(int protocol, const uint8_t* tones, float llr[174]) {
  if (!tones || !llr) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc::frame_to_llr_hard(protocol, tones, llr);
    return ORION_OK;
  });
}
int orion_ldpc_decode_host(const float llr[174], int protocol, int rule, size_t max_iter, orion_ldpc_result* result,
                           uint8_t* plain) {
  if (!llr || !result) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpc::check_args(protocol, rule, max_iter);
    orion::ldpc::decode_payload(protocol, llr, static_cast<int>(max_iter), rule,
                                reinterpret_cast<orion::ldpc::Result*>(result), plain);
    return ORION_OK;
  });
}
uint16_t orion_ft_crc14(const uint8_t* message, size_t num_bits) {
  if (!message || num_bits > (1u << 20)) return 0;
  return orion::ldpc::crc14(message, static_cast<int>(num_bits));
}
int orion_ldpc_tables(uint8_t* edges, uint16_t* row_start, uint8_t* bit_check, uint8_t* generator) {
  return guarded([&] {
    const orion::ldpc::Tables& t = orion::ldpc::tables();
    if (edges) std::memcpy(edges, orion::ldpc::kEdge, sizeof orion::ldpc::kEdge);
    if (row_start) std::memcpy(row_start, t.row_start, sizeof t.row_start);
    if (bit_check) std::memcpy(bit_check, t.bit_check, sizeof t.bit_check);
    if (generator) std::memcpy(generator, t.generator, sizeof t.generator);
    return ORION_OK;
  });
}

/* ---- FT8 / FT4 modulators, slot synthesis and hard demodulators (ftmod.hpp, k_ftmod.hip) ---- */
orion_ft_mod* orion_ft_mod_new(int protocol, float fs, float base_hz, float rf_hz, float gain) {
  try {
    return new orion_ft_mod(protocol, fs, base_hz, rf_hz, gain);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_ft_mod_free(orion_ft_mod* h) { delete h; }
int orion_ft_mod_modulate(orion_ft_mod* h, const uint8_t* tones, size_t nframes, void* iq) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (nframes && (!tones || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.modulate_host(tones, nframes, iq);
    return ORION_OK;
  });
}
int orion_ft_mod_modulate_device(orion_ft_mod* h, const uint8_t* tones, size_t nframes, void* iq, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (nframes && (!tones || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.modulate(tones, nframes, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ft_mod_host(int protocol, float fs, float base_hz, float rf_hz, float gain, const uint8_t* tones, void* iq) {
  if (!tones || !iq) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ftmod::modulate_host(protocol, fs, base_hz, rf_hz, gain, tones, static_cast<float*>(iq));
    return ORION_OK;
  });
}
int orion_ft_symbol_sequence(int protocol, const uint8_t* tones, uint8_t* syms) {
  if (!tones || !syms) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ftmod::symbol_sequence(protocol, tones, syms);
    return ORION_OK;
  });
}
int orion_ft_mod_tables(int protocol, float fs, float base_hz, const uint8_t* tones, float* w, uint64_t* step,
                        uint64_t* enter) {
  if (!tones && enter) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    float ww[2 * orion::ftmod::kMaxTones];
    uint64_t q[orion::ftmod::kMaxTones];
    const orion::ftmod::Proto& m = orion::ftmod::proto(protocol);
    orion::ftmod::tone_steps(protocol, fs, base_hz, ww, q);
    if (w) std::memcpy(w, ww, 2 * m.tones * sizeof(float));
    if (step) std::memcpy(step, q, m.tones * sizeof(uint64_t));
    if (enter) {
      uint8_t syms[orion::ftmod::kMaxSyms];
      orion::ftmod::symbol_sequence(protocol, tones, syms);
      orion::ftmod::enter_phases(protocol, syms, q, enter);
    }
    return ORION_OK;
  });
}
int orion_ft_synth(int protocol, float fs, const orion_ft_signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                   size_t n_per_ch, int accumulate, void* iq) {
  if ((nsig && (!signals || !tones)) || (nch && n_per_ch && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ft_synth_host(protocol, fs, reinterpret_cast<const orion::ftmod::Signal*>(signals), tones, nsig, nch, n_per_ch,
                         accumulate != 0, iq);
    return ORION_OK;
  });
}
int orion_ft_synth_device(int protocol, float fs, const orion_ft_signal* signals, const uint8_t* tones, size_t nsig,
                          size_t nch, size_t n_per_ch, int accumulate, void* iq, void* stream) {
  if ((nsig && (!signals || !tones)) || (nch && n_per_ch && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ft_synth(protocol, fs, reinterpret_cast<const orion::ftmod::Signal*>(signals), tones, nsig, nch, n_per_ch,
                    accumulate != 0, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ft_demod(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                   uint8_t* tones, float* energies) {
  if (nframes && (!iq || !tones)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ft_demod_host(protocol, fs, base_hz, iq, nframes, n_per_frame, tones, energies);
    return ORION_OK;
  });
}
int orion_ft_demod_device(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                          uint8_t* tones, float* energies, void* stream) {
  if (nframes && (!iq || !tones)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ft_demod(protocol, fs, base_hz, iq, nframes, n_per_frame, tones, energies, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ft_demod_host(int protocol, float fs, float base_hz, const void* iq, uint8_t* tones, float* energies) {
  if (!iq || !tones) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ftmod::demodulate_host(protocol, fs, base_hz, static_cast<const float*>(iq), tones, energies);
    return ORION_OK;
  });
}

/* ---- PSK31 channel code (psk31.hpp, k_psk31.hip) ---- */
int orion_psk31_tables(uint16_t* varicode_bits, uint8_t* varicode_len, float* dqpsk_exp) {
  return guarded([&] {
    const orion::psk31::Codeword* t = orion::psk31::varicode_table();
    for (int i = 0; i < 128; ++i) {
      if (varicode_bits) varicode_bits[i] = t[i].bits;
      if (varicode_len) varicode_len[i] = t[i].len;
    }
    if (dqpsk_exp) std::memcpy(dqpsk_exp, orion::psk31::kDqpskExp, sizeof orion::psk31::kDqpskExp);
    return ORION_OK;
  });
}
int orion_varicode_encode(uint8_t byte, uint16_t* bits, uint8_t* len) {
  if (!bits || !len) return fail(ORION_E_NULL, "null buffer");
  const orion::psk31::Codeword c = orion::psk31::varicode_encode(byte);
  *bits = c.bits;
  *len = c.len;
  return ORION_OK;
}
int orion_varicode_decode(uint16_t bits, uint8_t len) { return orion::psk31::varicode_decode(bits, len); }
orion_varicode_encoder* orion_varicode_encoder_new(void) {
  try {
    return new orion_varicode_encoder;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_varicode_encoder_free(orion_varicode_encoder* e) { delete e; }
int orion_varicode_encoder_push_preamble(orion_varicode_encoder* e, size_t n_bits) {
  if (!e) return fail(ORION_E_NULL, "null handle");
  if (n_bits > (1u << 30)) return fail(ORION_E_ARG, "varicode: more than 2^30 bits in one call");
  return guarded([&] {
    e->impl.push_preamble(n_bits);
    return ORION_OK;
  });
}
int orion_varicode_encoder_push_byte(orion_varicode_encoder* e, uint8_t byte) {
  if (!e) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    e->impl.push_byte(byte);
    return ORION_OK;
  });
}
int orion_varicode_encoder_push_postamble(orion_varicode_encoder* e, size_t n_bits) {
  if (!e) return fail(ORION_E_NULL, "null handle");
  if (n_bits > (1u << 30)) return fail(ORION_E_ARG, "varicode: more than 2^30 bits in one call");
  return guarded([&] {
    e->impl.push_postamble(n_bits);
    return ORION_OK;
  });
}
size_t orion_varicode_encoder_pending(const orion_varicode_encoder* e) { return e ? e->impl.pending() : 0; }
int orion_varicode_encoder_drain(orion_varicode_encoder* e, uint8_t* bits, size_t cap, size_t* n_bits) {
  if (!e) return fail(ORION_E_NULL, "null handle");
  if (!n_bits || (!bits && e->impl.pending())) return fail(ORION_E_NULL, "null buffer");
  if (cap < e->impl.pending()) return fail(ORION_E_ARG, "varicode: capacity below the pending bits");
  return guarded([&] {
    const std::vector<uint8_t> v = e->impl.drain_bits();
    if (!v.empty()) std::memcpy(bits, v.data(), v.size());
    *n_bits = v.size();
    return ORION_OK;
  });
}
orion_varicode_decoder* orion_varicode_decoder_new(void) {
  try {
    return new orion_varicode_decoder;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_varicode_decoder_free(orion_varicode_decoder* d) { delete d; }
int orion_varicode_decoder_push_bits(orion_varicode_decoder* d, const uint8_t* bits, size_t n) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  if (n && !bits) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    for (size_t i = 0; i < n; ++i) d->impl.push_bit(bits[i]);
    return ORION_OK;
  });
}
size_t orion_varicode_decoder_pending(const orion_varicode_decoder* d) { return d ? d->impl.pending() : 0; }
int orion_varicode_decoder_pop_bytes(orion_varicode_decoder* d, uint8_t* bytes, size_t cap, size_t* n_bytes) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  if (!n_bytes || (!bytes && d->impl.pending())) return fail(ORION_E_NULL, "null buffer");
  if (cap < d->impl.pending()) return fail(ORION_E_ARG, "varicode: capacity below the pending characters");
  size_t k = 0;
  for (int c; (c = d->impl.pop_char()) >= 0;) bytes[k++] = static_cast<uint8_t>(c);
  *n_bytes = k;
  return ORION_OK;
}
int orion_conv_encode(const uint8_t* bits, size_t n, uint8_t* coded) {
  if (n && (!bits || !coded)) return fail(ORION_E_NULL, "null buffer");
  orion::psk31::conv_encode(bits, n, coded);
  return ORION_OK;
}
int orion_psk31_viterbi(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits) {
  if (nstreams && n_syms && (!soft || !bits)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31_viterbi_host(soft, nstreams, n_syms, bits);
    return ORION_OK;
  });
}
int orion_psk31_viterbi_device(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits, void* work,
                               size_t work_bytes, void* stream) {
  if (nstreams && n_syms && (!soft || !bits || !work)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31_viterbi(soft, nstreams, n_syms, bits, work, work_bytes, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_psk31_viterbi_work_bytes(size_t nstreams, size_t n_syms) {
  if (nstreams > 0x7fffffffull - 3 || n_syms > 0x7fffffffull) return 0;
  return orion::psk31::viterbi_work_bytes(nstreams, n_syms);
}
int orion_psk31_viterbi_host(const float* soft, size_t n_syms, uint8_t* bits) {
  if (n_syms && (!soft || !bits)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31::viterbi_decode(soft, n_syms, bits);
    return ORION_OK;
  });
}
int orion_psk31_viterbi_hard_host(const uint8_t* coded, size_t n_syms, uint8_t* bits) {
  if (n_syms && (!coded || !bits)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31::viterbi_decode_hard(coded, n_syms, bits);
    return ORION_OK;
  });
}
orion_psk31_streaming_viterbi* orion_psk31_streaming_viterbi_new(void) {
  try {
    return new orion_psk31_streaming_viterbi;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_psk31_streaming_viterbi_free(orion_psk31_streaming_viterbi* v) { delete v; }
int orion_psk31_streaming_viterbi_feed(orion_psk31_streaming_viterbi* v, const float* soft, size_t n_syms,
                                       uint8_t* bits, size_t* n_bits) {
  if (!v) return fail(ORION_E_NULL, "null handle");
  if (!n_bits || (n_syms && (!soft || !bits))) return fail(ORION_E_NULL, "null buffer");
  size_t k = 0;
  for (size_t i = 0; i < n_syms; ++i) {
    const int b = v->impl.feed_symbol(soft[2 * i], soft[2 * i + 1]);
    if (b >= 0) bits[k++] = static_cast<uint8_t>(b);
  }
  *n_bits = k;
  return ORION_OK;
}
int orion_psk31_streaming_viterbi_flush(orion_psk31_streaming_viterbi* v, uint8_t* bits, size_t* n_bits) {
  if (!v) return fail(ORION_E_NULL, "null handle");
  if (!n_bits || !bits) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<uint8_t> out = v->impl.flush();
    if (!out.empty()) std::memcpy(bits, out.data(), out.size());
    *n_bits = out.size();
    return ORION_OK;
  });
}

/* ---- PSK31 modulators and demodulators (psk31.hpp, k_psk31.hip) ---- */
size_t orion_psk31_sps(float fs) { return orion::psk31::psk31_sps(fs); }
int orion_psk31_text_bits(const uint8_t* text, size_t n, size_t preamble_bits, size_t postamble_bits, uint8_t* bits,
                          size_t cap, size_t* n_bits) {
  if (!n_bits || (n && !text)) return fail(ORION_E_NULL, "null buffer");
  if (n > (1u << 24) || preamble_bits > (1u << 30) || postamble_bits > (1u << 30))
    return fail(ORION_E_ARG, "psk31 text: more than 2^24 bytes or 2^30 preamble / postamble bits");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::psk31::text_bits(text, n, preamble_bits, postamble_bits);
    *n_bits = v.size();
    if (cap < v.size()) return fail(ORION_E_ARG, "psk31 text: capacity below the bit count");
    if (!v.empty()) {
      if (!bits) return fail(ORION_E_NULL, "null buffer");
      std::memcpy(bits, v.data(), v.size());
    }
    return ORION_OK;
  });
}
orion_psk31_mod* orion_psk31_mod_new(int mode, float fs, float rf_hz, float gain) {
  try {
    return new orion_psk31_mod(mode, fs, rf_hz, gain);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_psk31_mod_free(orion_psk31_mod* m) { delete m; }
int orion_psk31_mod_set_gain(orion_psk31_mod* m, float gain) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  m->impl.set_gain(gain);
  return ORION_OK;
}
int orion_psk31_mod_reset(orion_psk31_mod* m) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  m->impl.reset();
  return ORION_OK;
}
int orion_psk31_mod_modulate_bits(orion_psk31_mod* m, const uint8_t* bits, size_t n, void* iq) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  if (n && (!bits || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    m->impl.modulate_bits(bits, n, static_cast<float*>(iq));
    return ORION_OK;
  });
}
int orion_psk31_mod_modulate_bits_device(orion_psk31_mod* m, const uint8_t* bits, size_t n, void* iq, void* stream) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  if (n && (!bits || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    m->dev.modulate(bits, n, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_psk31_mod_modulate_batch(orion_psk31_mod* m, const uint8_t* bits, size_t nstreams, size_t n, void* iq) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  if (nstreams && n && (!bits || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    m->dev.modulate_batch_host(bits, nstreams, n, iq);
    return ORION_OK;
  });
}
int orion_psk31_mod_modulate_batch_device(orion_psk31_mod* m, const uint8_t* bits, size_t nstreams, size_t n, void* iq,
                                          void* stream) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  if (nstreams && n && (!bits || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    m->dev.modulate_batch(bits, nstreams, n, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_psk31_synth(float fs, const orion_psk31_signal* signals, const uint8_t* bits, size_t nsig, size_t nch,
                      size_t n_per_ch, int accumulate, void* iq) {
  if ((nsig && !signals) || (nch && n_per_ch && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31_synth_host(fs, reinterpret_cast<const orion::psk31::Signal*>(signals), bits, nsig, nch, n_per_ch,
                            accumulate != 0, iq);
    return ORION_OK;
  });
}
int orion_psk31_synth_device(float fs, const orion_psk31_signal* signals, const uint8_t* bits, size_t nsig, size_t nch,
                             size_t n_per_ch, int accumulate, void* iq, void* stream) {
  if ((nsig && !signals) || (nch && n_per_ch && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::psk31_synth(fs, reinterpret_cast<const orion::psk31::Signal*>(signals), bits, nsig, nch, n_per_ch,
                       accumulate != 0, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
uint64_t orion_psk31_rotator_q64(float freq_hz, float fs) { return orion::psk31::rotator_step_q64(freq_hz, fs); }
int orion_psk31_mod_process(orion_psk31_mod* m, const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap,
                            orion_work_report* report) {
  if (!m) return fail(ORION_E_NULL, "null handle");
  if (!report || (n_bits && !bits) || (out_cap && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    m->impl.process(bits, n_bits, static_cast<float*>(iq), out_cap, &report->in_read, &report->out_written);
    return ORION_OK;
  });
}
orion_psk31_demod* orion_psk31_demod_new(int mode, float fs, float rf_hz, float gain, size_t offset) {
  try {
    return new orion_psk31_demod(mode, fs, rf_hz, gain, offset);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_psk31_demod_free(orion_psk31_demod* d) { delete d; }
int orion_psk31_demod_set_gain(orion_psk31_demod* d, float gain) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  d->impl.set_gain(gain);
  return ORION_OK;
}
int orion_psk31_demod_reset(orion_psk31_demod* d) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  d->impl.reset();
  return ORION_OK;
}
int orion_psk31_demod_process(orion_psk31_demod* d, const void* iq, size_t n, float* soft, size_t out_cap,
                              orion_work_report* report) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  if (!report || (n && !iq) || (out_cap && !soft)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    d->impl.process(static_cast<const float*>(iq), n, soft, out_cap, &report->in_read, &report->out_written);
    return ORION_OK;
  });
}
int orion_bpsk31_decide(const float* soft, size_t n, uint8_t* bits) {
  if (n && (!soft || !bits)) return fail(ORION_E_NULL, "null buffer");
  orion::psk31::bpsk31_decide(soft, n, bits);
  return ORION_OK;
}
int orion_psk31_find_carriers_host(const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                                   size_t min_carrier_syms, float peak_margin_db, size_t max_cand,
                                   orion_candidate* cand, uint32_t* count) {
  if (!cand || !count || (nch && num_syms && num_bins && !wf)) return fail(ORION_E_NULL, "null buffer");
  if (max_cand == 0) return fail(ORION_E_ARG, "max_cand == 0");
  if (max_cand > (1u << 16)) return fail(ORION_E_ARG, "max_cand above 65536");
  if (nch > 65535 || num_syms > 0x7fffffffull || num_bins > 0x7fffffffull ||
      static_cast<unsigned long long>(nch) * num_syms * num_bins > 0x7fffffffull)
    return fail(ORION_E_ARG, "psk31 carrier search: nch <= 65535 and a waterfall below 2^31 cells");
  return guarded([&] {
    for (size_t ch = 0; ch < nch; ++ch) {
      const std::vector<orion::psk31::Carrier> v = orion::psk31::find_carriers(
          wf + ch * num_syms * num_bins, num_syms, num_bins, min_carrier_syms, peak_margin_db, max_cand);
      count[ch] = static_cast<uint32_t>(v.size());
      for (size_t k = 0; k < max_cand; ++k) {
        orion_candidate& c = cand[ch * max_cand + k];
        c = orion_candidate{0, 0u, 0.0f};
        if (k < v.size()) c = orion_candidate{v[k].time_sym, v[k].freq_bin, v[k].score};
      }
    }
    return ORION_OK;
  });
}
int orion_psk31_find_carriers(orion_sync* h, const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                              size_t min_carrier_syms, float peak_margin_db, size_t max_cand, orion_candidate* cand,
                              uint32_t* count) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!cand || !count || (nch && num_syms && num_bins && !wf)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->psk.find_carriers_host(wf, nch, num_syms, num_bins, min_carrier_syms, peak_margin_db, max_cand,
                              reinterpret_cast<orion::SyncCandidate*>(cand), count);
    return ORION_OK;
  });
}
int orion_psk31_find_carriers_device(orion_sync* h, const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                                     size_t min_carrier_syms, float peak_margin_db, size_t max_cand,
                                     orion_candidate* cand, uint32_t* count, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!cand || !count || (nch && num_syms && num_bins && !wf)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->psk.find_carriers(wf, nch, num_syms, num_bins, min_carrier_syms, peak_margin_db, max_cand,
                         reinterpret_cast<orion::SyncCandidate*>(cand), count, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_psk31_sync(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand,
                     orion_candidate* cand, uint32_t* count, float* soft, orion_psk31_report* reports) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || !reports || (max_cand && (!cand || !soft))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->psk.sync_host(h->impl, iq, nch, n_per_ch, fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand,
                     reinterpret_cast<orion::SyncCandidate*>(cand), count, soft, reinterpret_cast<uint64_t*>(reports));
    return ORION_OK;
  });
}
int orion_psk31_sync_device(orion_sync* h, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz,
                            float max_hz, size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand,
                            orion_candidate* cand, uint32_t* count, float* soft, orion_psk31_report* reports,
                            void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((!iq && n_per_ch) || !count || !reports || (max_cand && (!cand || !soft))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->psk.sync(h->impl, iq, nch, n_per_ch, fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand,
                reinterpret_cast<orion::SyncCandidate*>(cand), count, soft, reinterpret_cast<uint64_t*>(reports),
                static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_psk31_sync_num_bins(float base_hz, float max_hz) {
  try {
    return orion::psk31::sync_num_bins(base_hz, max_hz);
  } catch (const std::exception& e) {
    g_err = e.what();
    return 0;
  }
}
orion_psk31_demod_bank* orion_psk31_demod_bank_new(float fs, const orion_psk31_stream* streams, size_t nstreams,
                                                   size_t nch) {
  if (!streams) {
    g_err = "null buffer";
    return nullptr;
  }
  try {
    return new orion_psk31_demod_bank(fs, reinterpret_cast<const orion::psk31::Stream*>(streams), nstreams, nch);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_psk31_demod_bank_free(orion_psk31_demod_bank* b) { delete b; }
int orion_psk31_demod_bank_process(orion_psk31_demod_bank* b, const void* iq, size_t nch, size_t n, float* soft,
                                   size_t out_stride, uint8_t* bits, orion_psk31_report* reports) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((n && !iq) || !reports || (out_stride && !soft)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    b->impl.process_host(iq, nch, n, soft, out_stride, bits, reinterpret_cast<uint64_t*>(reports));
    return ORION_OK;
  });
}
int orion_psk31_demod_bank_process_device(orion_psk31_demod_bank* b, const void* iq, size_t nch, size_t n, float* soft,
                                          size_t out_stride, uint8_t* bits, orion_psk31_report* reports, void* stream) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  if ((n && !iq) || !reports || (out_stride && !soft)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    b->impl.process(iq, nch, n, soft, out_stride, bits, reinterpret_cast<uint64_t*>(reports),
                    static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_psk31_demod_bank_set_gain(orion_psk31_demod_bank* b, size_t index, float gain) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    b->impl.set_gain(index, gain);
    return ORION_OK;
  });
}
int orion_psk31_demod_bank_reset(orion_psk31_demod_bank* b) {
  if (!b) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    b->impl.reset();
    return ORION_OK;
  });
}

// ---- the OFDM symbol layer --------------------------------------------------------------
orion_ofdm_config* orion_ofdm_config_new(size_t n_fft, size_t cp_len, const int32_t* data_carriers, size_t n_data,
                                         const int32_t* pilot_idx, const float* pilot_val, size_t n_pilots, float fs,
                                         float rf_hz, float gain, int constellation) {
  if ((n_data && !data_carriers) || (n_pilots && (!pilot_idx || !pilot_val))) {
    fail(ORION_E_NULL, "null buffer");
    return nullptr;
  }
  try {
    auto c = new orion_ofdm_config;
    c->impl.plan.n_fft = n_fft;
    c->impl.plan.cp_len = cp_len;
    c->impl.plan.data.assign(data_carriers, data_carriers + n_data);
    c->impl.plan.pilot_idx.assign(pilot_idx, pilot_idx + n_pilots);
    c->impl.plan.pilot_val.assign(pilot_val, pilot_val + 2 * n_pilots);
    c->impl.fs = fs;
    c->impl.rf_hz = rf_hz;
    c->impl.gain = gain;
    c->impl.constellation = constellation;
    return c;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_ofdm_config_free(orion_ofdm_config* c) { delete c; }
int orion_ofdm_config_contiguous_data(orion_ofdm_config* c, size_t edge_guard, int include_dc) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  if (c->impl.plan.n_fft > (size_t{1} << 24)) return fail(ORION_E_ARG, "n_fft above 2^24");
  return guarded([&] {
    orion::ofdm::plan_contiguous_data(c->impl.plan, edge_guard, include_dc != 0);
    return ORION_OK;
  });
}
int orion_ofdm_config_set_rx_window_backoff(orion_ofdm_config* c, size_t backoff) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  c->impl.rx_window_backoff = backoff;
  return ORION_OK;
}
int orion_ofdm_config_set_symbol_window(orion_ofdm_config* c, size_t roll_off) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  c->impl.plan.roll_off = roll_off;
  return ORION_OK;
}
int orion_ofdm_config_validate(const orion_ofdm_config* c, long long edge_guard, int32_t* bad_index) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    return edge_guard >= 0
               ? orion::ofdm::plan_validate_edge_guard(c->impl.plan, static_cast<size_t>(edge_guard), bad_index)
               : orion::ofdm::plan_validate(c->impl.plan, bad_index);
  });
}
int orion_ofdm_config_info(const orion_ofdm_config* c, size_t* info) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  if (!info) return fail(ORION_E_NULL, "null buffer");
  const orion::ofdm::Config& k = c->impl;
  info[0] = k.plan.n_fft;
  info[1] = k.plan.cp_len;
  info[2] = k.plan.data.size();
  info[3] = k.plan.pilot_idx.size();
  info[4] = k.bits_per_ofdm_symbol();
  info[5] = k.samples_per_ofdm_symbol();
  info[6] = orion::ofdm::plan_occupied_half_carriers(k.plan);
  info[7] = k.plan.roll_off;
  return ORION_OK;
}
int orion_ofdm_config_data_carriers(const orion_ofdm_config* c, int32_t* out, size_t cap) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  const auto& d = c->impl.plan.data;
  if (cap < d.size()) return fail(ORION_E_ARG, "cap below the data-carrier count");
  if (!d.empty() && !out) return fail(ORION_E_NULL, "null buffer");
  std::copy(d.begin(), d.end(), out);
  return ORION_OK;
}
int orion_ofdm_config_occupied_bins(const orion_ofdm_config* c, uint32_t* out, size_t cap, size_t* n) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  if (!n) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<size_t> b = orion::ofdm::plan_occupied_bins(c->impl.plan);
    if (cap < b.size()) return fail(ORION_E_ARG, "cap below the occupied-bin count");
    if (!b.empty() && !out) return fail(ORION_E_NULL, "null buffer");
    for (size_t i = 0; i < b.size(); ++i) out[i] = static_cast<uint32_t>(b[i]);
    *n = b.size();
    return ORION_OK;
  });
}
int orion_ofdm_config_grid(const orion_ofdm_config* c, uint32_t* data_bins, uint32_t* pilot_bins) {
  if (!c) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    const orion::ofdm::Grid g = orion::ofdm::grid_from_plan(c->impl.plan);
    if ((!g.data_bins.empty() && !data_bins) || (!g.pilot_bins.empty() && !pilot_bins))
      return fail(ORION_E_NULL, "null buffer");
    std::copy(g.data_bins.begin(), g.data_bins.end(), data_bins);
    std::copy(g.pilot_bins.begin(), g.pilot_bins.end(), pilot_bins);
    return ORION_OK;
  });
}
size_t orion_ofdm_max_pilot_safe_backoff(size_t n_fft, size_t pilot_spacing) {
  return orion::ofdm::max_pilot_safe_backoff(n_fft, pilot_spacing);
}
int orion_ofdm_tables(int constellation, float* axis, float* thresholds, size_t n_fft, float* training, float* twiddles,
                      size_t symbol_len, size_t roll_off, float* ramp) {
  return guarded([&] {
    const size_t bps = orion::ofdm::bits_per_symbol(constellation);
    if ((axis || thresholds) && bps == 0) return fail(ORION_E_ARG, "unknown constellation");
    if (axis) {
      std::fill(axis, axis + 16, 0.0f);
      if (bps >= 4) orion::ofdm::axis_table(bps, axis);
    }
    if (thresholds) {
      std::fill(thresholds, thresholds + 15, 0.0f);
      if (bps >= 4) orion::ofdm::threshold_table(bps, thresholds);
    }
    if ((training || twiddles) && n_fft > (size_t{1} << 24)) return fail(ORION_E_ARG, "n_fft above 2^24");
    if (training) orion::ofdm::training_pattern(n_fft, training);
    if (twiddles) {
      const std::vector<float> tw = orion::ofdm::fft_twiddles(n_fft);
      std::copy(tw.begin(), tw.end(), twiddles);
    }
    if (ramp) {
      if (roll_off > (size_t{1} << 30)) return fail(ORION_E_ARG, "roll_off above 2^30");
      const std::vector<float> r = orion::ofdm::window_ramp(symbol_len, roll_off);
      std::copy(r.begin(), r.end(), ramp);
    }
    return ORION_OK;
  });
}
int orion_ofdm_map_host(int constellation, const uint8_t* bits, size_t n_syms, void* syms) {
  if (n_syms && (!bits || !syms)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (orion::ofdm::bits_per_symbol(constellation) == 0) return fail(ORION_E_ARG, "unknown constellation");
    orion::ofdm::map_bits(constellation, bits, n_syms, static_cast<float*>(syms));
    return ORION_OK;
  });
}
int orion_ofdm_decide_host(int constellation, const void* syms, size_t n_syms, uint8_t* bits) {
  if (n_syms && (!bits || !syms)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (orion::ofdm::bits_per_symbol(constellation) == 0) return fail(ORION_E_ARG, "unknown constellation");
    orion::ofdm::decide(constellation, static_cast<const float*>(syms), n_syms, bits);
    return ORION_OK;
  });
}
int orion_ofdm_llr_host(int constellation, const void* syms, size_t n_syms, float* llr) {
  if (n_syms && (!llr || !syms)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (orion::ofdm::bits_per_symbol(constellation) == 0) return fail(ORION_E_ARG, "unknown constellation");
    orion::ofdm::soft_llr(constellation, static_cast<const float*>(syms), n_syms, llr);
    return ORION_OK;
  });
}
int orion_fft_host(size_t n_fft, int inverse, const void* in, size_t n_sym, void* out) {
  if (n_sym && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::ofdm::Fft f(n_fft, inverse != 0);
    size_t r, w;
    for (size_t s = 0; s < n_sym; ++s)
      f.process(static_cast<const float*>(in) + 2 * s * n_fft, n_fft, static_cast<float*>(out) + 2 * s * n_fft, n_fft,
                &r, &w);
    return ORION_OK;
  });
}
int orion_ofdm_window_host(size_t symbol_len, size_t roll_off, void* iq, size_t n_sym) {
  if (n_sym && symbol_len && !iq) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<float> r = orion::ofdm::window_ramp(symbol_len, std::min<size_t>(roll_off, symbol_len));
    for (size_t s = 0; s < n_sym; ++s) orion::ofdm::window_apply(static_cast<float*>(iq) + 2 * s * symbol_len, symbol_len, r);
    return ORION_OK;
  });
}
int orion_ofdm_rotator_host(float freq_hz, float fs, size_t n, void* out) {
  if (n && !out) return fail(ORION_E_NULL, "null buffer");
  orion::ofdm::Rotator r(freq_hz, fs);
  float* o = static_cast<float*>(out);
  for (size_t i = 0; i < n; ++i) r.next(o + 2 * i, o + 2 * i + 1);
  return ORION_OK;
}
int orion_ofdm_evm_db_host(int constellation, const void* soft, size_t n_soft, const uint8_t* bits, size_t n_bits,
                           size_t num_symbols, float* evm_db, int* valid) {
  if (!evm_db || !valid || (n_soft && !soft) || (n_bits && !bits)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    *valid = orion::ofdm::evm_db(constellation, static_cast<const float*>(soft), n_soft, bits, n_bits, num_symbols, evm_db)
                 ? 1
                 : 0;
    return ORION_OK;
  });
}
int orion_ofdm_equalizer_weight_host(const void* h, size_t n, void* w) {
  if (n && (!h || !w)) return fail(ORION_E_NULL, "null buffer");
  const float* hp = static_cast<const float*>(h);
  float* wp = static_cast<float*>(w);
  for (size_t i = 0; i < n; ++i) orion::ofdm::equalizer_weight(hp[2 * i], hp[2 * i + 1], wp + 2 * i, wp + 2 * i + 1);
  return ORION_OK;
}
int orion_ofdm_interpolate_host(const uint32_t* pilot_bins, const void* ratios, size_t n_pilots, const uint32_t* bins,
                                size_t n_bins, void* out) {
  if (n_pilots == 0) return fail(ORION_E_ARG, "interpolate_at needs at least one pilot");
  if (!pilot_bins || !ratios || (n_bins && (!bins || !out))) return fail(ORION_E_NULL, "null buffer");
  for (size_t i = 0; i + 1 < n_pilots; ++i)
    if (pilot_bins[i] >= pilot_bins[i + 1]) return fail(ORION_E_ARG, "pilot bins not strictly ascending");
  float* o = static_cast<float*>(out);
  for (size_t i = 0; i < n_bins; ++i)
    orion::ofdm::interpolate_at(pilot_bins, static_cast<const float*>(ratios), n_pilots, bins[i], o + 2 * i, o + 2 * i + 1);
  return ORION_OK;
}

static orion_fft* fft_new(size_t n_fft, bool inverse) {
  try {
    return new orion_fft(n_fft, inverse);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
orion_fft* orion_fft_new(size_t n_fft) { return fft_new(n_fft, false); }
orion_fft* orion_ifft_new(size_t n_fft) { return fft_new(n_fft, true); }
void orion_fft_free(orion_fft* f) { delete f; }
int orion_fft_process(orion_fft* f, const void* in, size_t n_in, void* out, size_t out_cap, orion_work_report* report) {
  if (!f) return fail(ORION_E_NULL, "null handle");
  if (!report || (n_in && !in) || (out_cap && !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::WorkReport w = f->impl.process_host(in, n_in, out, out_cap);
    report->in_read = w.in_read;
    report->out_written = w.out_written;
    return ORION_OK;
  });
}
int orion_fft_batch(orion_fft* f, const void* in, size_t in_stride, void* out, size_t out_stride, size_t batch,
                    void* stream) {
  if (!f) return fail(ORION_E_NULL, "null handle");
  if (batch && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    f->impl.batch(in, in_stride, out, out_stride, batch, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

static orion_ofdm* ofdm_new(int kind, const orion_ofdm_config* c, int eq) {
  if (!c) {
    fail(ORION_E_NULL, "null configuration");
    return nullptr;
  }
  try {
    return new orion_ofdm(kind, c->impl, eq);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
orion_ofdm* orion_ofdm_mod_new(const orion_ofdm_config* c) { return ofdm_new(kOfdmMod, c, ORION_OFDM_EQ_NONE); }
orion_ofdm* orion_ofdm_demod_new(const orion_ofdm_config* c, int equalizer) { return ofdm_new(kOfdmDemod, c, equalizer); }
orion_ofdm* orion_ofdm_decider_new(const orion_ofdm_config* c) { return ofdm_new(kOfdmDecider, c, ORION_OFDM_EQ_NONE); }
orion_ofdm* orion_ofdm_soft_demod_new(const orion_ofdm_config* c) {
  return ofdm_new(kOfdmSoftDemod, c, ORION_OFDM_EQ_NONE);
}
orion_ofdm* orion_ofdm_equalizer_new(const orion_ofdm_config* c, int method) {
  if (method == ORION_OFDM_EQ_NONE) {
    fail(ORION_E_ARG, "an equalizer needs a method");
    return nullptr;
  }
  return ofdm_new(kOfdmEqualizer, c, method);
}
void orion_ofdm_free(orion_ofdm* h) { delete h; }
int orion_ofdm_set_gain(orion_ofdm* h, float gain) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind == kOfdmMod)
    h->impl.set_mod_gain(gain);
  else if (h->kind == kOfdmDemod)
    h->impl.set_demod_gain(gain);
  else
    return fail(ORION_E_TYPE, "not a modulator or demodulator");
  return ORION_OK;
}
int orion_ofdm_reset(orion_ofdm* h) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  return guarded([&] {
    h->impl.reset();
    return ORION_OK;
  });
}
int orion_ofdm_estimate_channel(orion_ofdm* h, const void* received_freq, size_t n) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (n && !received_freq) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.estimate_channel(static_cast<const float*>(received_freq), n);
    return ORION_OK;
  });
}
int orion_ofdm_process(orion_ofdm* h, const void* in, size_t n_in, void* out, size_t out_cap,
                       orion_work_report* report) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!report || (n_in && !in) || (out_cap && !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::WorkReport w;
    switch (h->kind) {
      case kOfdmMod: w = h->impl.mod_host(static_cast<const uint8_t*>(in), n_in, out, out_cap); break;
      case kOfdmDemod: w = h->impl.demod_host(in, n_in, out, out_cap); break;
      case kOfdmDecider: w = h->impl.decide_host(in, n_in, static_cast<uint8_t*>(out), out_cap); break;
      case kOfdmSoftDemod: w = h->impl.soft_demod_host(in, n_in, static_cast<float*>(out), out_cap); break;
      default: w = h->impl.equalize_host(in, n_in, out, out_cap); break;
    }
    report->in_read = w.in_read;
    report->out_written = w.out_written;
    return ORION_OK;
  });
}
int orion_ofdm_mod_device(orion_ofdm* h, const uint8_t* bits, size_t n_channels, size_t n_symbols, void* iq,
                          void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmMod) return fail(ORION_E_TYPE, "not a modulator");
  if (n_channels && n_symbols && (!bits || !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.modulate(bits, n_channels, n_symbols, iq, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_demod_device(orion_ofdm* h, const void* iq, size_t n_channels, size_t n_symbols, void* soft,
                            uint8_t* bits, float* llr, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmDemod) return fail(ORION_E_TYPE, "not a demodulator");
  if (n_channels && n_symbols && (!iq || !soft)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.demodulate(iq, n_channels, n_symbols, soft, bits, llr, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
static int ofdm_count(size_t a, size_t b, size_t c, size_t* out) {
  if (a > (size_t{1} << 30) || b > (size_t{1} << 30) || a * b > (size_t{1} << 30) || c > (size_t{1} << 24)) return -1;
  *out = a * b * c;
  return 0;
}
int orion_ofdm_decider_device(orion_ofdm* h, const void* soft, size_t n_channels, size_t n_symbols, uint8_t* bits,
                              void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmDecider) return fail(ORION_E_TYPE, "not a decider");
  if (n_channels && n_symbols && (!soft || !bits)) return fail(ORION_E_NULL, "null buffer");
  size_t n;
  if (ofdm_count(n_channels, n_symbols, h->impl.num_data(), &n)) return fail(ORION_E_ARG, "more than 2^30 symbols");
  return guarded([&] {
    h->impl.decide(soft, n, bits, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_soft_demod_device(orion_ofdm* h, const void* soft, size_t n_channels, size_t n_symbols, float* llr,
                                 void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmSoftDemod) return fail(ORION_E_TYPE, "not a soft demodulator");
  if (n_channels && n_symbols && (!soft || !llr)) return fail(ORION_E_NULL, "null buffer");
  size_t n;
  if (ofdm_count(n_channels, n_symbols, h->impl.num_data(), &n)) return fail(ORION_E_ARG, "more than 2^30 symbols");
  return guarded([&] {
    h->impl.soft_demod(soft, n, llr, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_equalizer_device(orion_ofdm* h, const void* in, size_t n_channels, size_t n_symbols, void* out,
                                void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmEqualizer) return fail(ORION_E_TYPE, "not an equalizer");
  if (n_channels && n_symbols && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  size_t n;
  if (ofdm_count(n_channels, n_symbols, 1, &n)) return fail(ORION_E_ARG, "more than 2^30 symbols");
  return guarded([&] {
    h->impl.equalize(in, n, out, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_mod_host(orion_ofdm* h, const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap,
                        orion_work_report* report) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!report || (n_bits && !bits) || (out_cap && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.mod().process(bits, n_bits, static_cast<float*>(iq), out_cap, &report->in_read, &report->out_written);
    return ORION_OK;
  });
}
int orion_ofdm_demod_host(orion_ofdm* h, const void* iq, size_t n, void* soft, size_t out_cap,
                          orion_work_report* report) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!report || (n && !iq) || (out_cap && !soft)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.demod().process(static_cast<const float*>(iq), n, static_cast<float*>(soft), out_cap, h->impl.equalizer(),
                            &report->in_read, &report->out_written);
    return ORION_OK;
  });
}
int orion_ofdm_equalize_host(orion_ofdm* h, const void* in, size_t n, void* out, size_t out_cap,
                             orion_work_report* report) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (!h->impl.equalizer()) return fail(ORION_E_TYPE, "this handle has no equalizer");
  if (!report || (n && !in) || (out_cap && !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const size_t nf = h->impl.equalizer()->n_fft(), k = std::min(n / nf, out_cap / nf);
    size_t r, w;
    for (size_t s = 0; s < k; ++s)
      h->impl.equalizer()->process(static_cast<const float*>(in) + 2 * s * nf, nf, static_cast<float*>(out) + 2 * s * nf,
                                   nf, &r, &w);
    report->in_read = report->out_written = k * nf;
    return ORION_OK;
  });
}
int orion_ofdm_set_pilot_bins_host(orion_ofdm* h, const uint32_t* pilot_bins, const void* pilot_val, size_t n_pilots,
                                   const uint32_t* data_bins, size_t n_data) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if ((n_pilots && (!pilot_bins || !pilot_val)) || (n_data && !data_bins)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.set_pilot_bins(pilot_bins, static_cast<const float*>(pilot_val), n_pilots, data_bins, n_data);
    return ORION_OK;
  });
}

/* ---- the inner code (fec.hpp, k_fec.hip) ---- */
size_t orion_fec_punctured_coded_len(int code, size_t info_bits, int rate) {
  try {
    return info_bits ? orion::fec::punctured_coded_len(code, info_bits, rate) : 0;
  } catch (const std::exception& e) {
    fail(ORION_E_ARG, e.what());
    return 0;
  }
}
size_t orion_fec_encoded_len(int code, size_t info_bits, int rate, size_t rows, size_t cols) {
  try {
    return orion::fec_encoded_len(code, info_bits, rate, rows, cols);
  } catch (const std::exception& e) {
    fail(ORION_E_ARG, e.what());
    return 0;
  }
}
int orion_fec_conv_encode(int code, int rate, const uint8_t* info, size_t info_bits, uint8_t* coded) {
  if (!info || !coded) return fail(ORION_E_NULL, "null buffer");
  if (info_bits == 0) return fail(ORION_E_ARG, "fec: info_bits == 0");
  return guarded([&] {
    orion::fec::conv_encode_punctured(code, info, info_bits, rate, coded);
    return ORION_OK;
  });
}
int orion_fec_viterbi_host(int code, int rate, const float* llr, size_t n_llr, size_t info_bits, size_t rows,
                           size_t cols, uint8_t* bits) {
  if ((n_llr && !llr) || !bits) return fail(ORION_E_NULL, "null buffer");
  if (info_bits == 0) return fail(ORION_E_ARG, "fec: info_bits == 0");
  if ((rows == 0) != (cols == 0)) return fail(ORION_E_ARG, "fec: interleaver rows, cols both zero (none) or both nonzero");
  if (n_llr > orion::fec::kMaxLlr) return fail(ORION_E_ARG, "fec viterbi: n_llr above 2^31 - 1");
  return guarded([&] {
    if (rows) {
      const std::vector<float> d = orion::fec::BlockInterleaver(rows, cols).deinterleave_llrs(llr, n_llr);
      orion::fec::viterbi_decode_soft(code, d.data(), n_llr, info_bits, rate, bits);
    } else {
      orion::fec::viterbi_decode_soft(code, llr, n_llr, info_bits, rate, bits);
    }
    return ORION_OK;
  });
}
int orion_fec_viterbi(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                      size_t rows, size_t cols, uint8_t* bits) {
  if (nstreams && ((n_llr && !llr) || !bits)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::fec_viterbi_host(code, rate, llr, nstreams, n_llr, info_bits, rows, cols, bits);
    return ORION_OK;
  });
}
int orion_fec_viterbi_device(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                             size_t rows, size_t cols, uint8_t* bits, void* work, size_t work_bytes, void* stream) {
  if (nstreams && ((n_llr && !llr) || !bits || !work)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::fec_viterbi(code, rate, llr, nstreams, n_llr, info_bits, rows, cols, bits, work, work_bytes,
                       static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_fec_viterbi_work_bytes(int code, size_t nstreams, size_t info_bits) {
  if (info_bits == 0 || info_bits > orion::fec::kMaxInfoBits || nstreams > orion::fec::kMaxStreams) return 0;
  try {
    return orion::fec::viterbi_work_bytes(orion::fec::code_spec(code).reg_bits, nstreams, info_bits);
  } catch (const std::exception& e) {
    fail(ORION_E_ARG, e.what());
    return 0;
  }
}
int orion_fec_conv_encode_batch(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits,
                                size_t rows, size_t cols, uint8_t* coded) {
  if (nstreams && (!info || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::fec_encode_batch_host(code, rate, info, nstreams, info_bits, rows, cols, coded);
    return ORION_OK;
  });
}
int orion_fec_conv_encode_batch_device(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits,
                                       size_t rows, size_t cols, uint8_t* coded, void* stream) {
  if (nstreams && (!info || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::fec_encode_batch(code, rate, info, nstreams, info_bits, rows, cols, coded, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_fec_interleave_u8(size_t rows, size_t cols, const uint8_t* in, uint8_t* out) {
  return fec_block(rows, cols, in, out, false);
}
int orion_fec_interleave_f32(size_t rows, size_t cols, const float* in, float* out) {
  return fec_block(rows, cols, in, out, false);
}
int orion_fec_deinterleave_u8(size_t rows, size_t cols, const uint8_t* in, uint8_t* out) {
  return fec_block(rows, cols, in, out, true);
}
int orion_fec_deinterleave_f32(size_t rows, size_t cols, const float* in, float* out) {
  return fec_block(rows, cols, in, out, true);
}
size_t orion_fec_interleaved_len(size_t rows, size_t cols, size_t n) {
  try {
    if (n > (size_t(1) << 40)) throw std::invalid_argument("interleaver: n above 2^40");
    return orion::fec::BlockInterleaver(rows, cols).interleaved_len(n);
  } catch (const std::exception& e) {
    fail(ORION_E_ARG, e.what());
    return 0;
  }
}
int orion_fec_interleave_bits(size_t rows, size_t cols, const uint8_t* bits, size_t n, uint8_t* out) {
  if (n && (!bits || !out)) return fail(ORION_E_NULL, "null buffer");
  if (n > (size_t(1) << 40)) return fail(ORION_E_ARG, "interleaver: n above 2^40");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::fec::BlockInterleaver(rows, cols).interleave_bits(bits, n);
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_fec_deinterleave_llrs(size_t rows, size_t cols, const float* llr, size_t n, float* out) {
  if (n && (!llr || !out)) return fail(ORION_E_NULL, "null buffer");
  if (n > (size_t(1) << 40)) return fail(ORION_E_ARG, "interleaver: n above 2^40");
  return guarded([&] {
    const std::vector<float> v = orion::fec::BlockInterleaver(rows, cols).deinterleave_llrs(llr, n);
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(float));
    return ORION_OK;
  });
}

/* ---- the outer code (rs.hpp, k_rs.hip) ---- */
int orion_rs_gf_tables(uint8_t* exp, uint8_t* log) {
  if (!exp || !log) return fail(ORION_E_NULL, "null buffer");
  const orion::rs::GfTables& t = orion::rs::Gf256::shared().tables();
  std::memcpy(exp, t.exp, sizeof t.exp);
  std::memcpy(log, t.log, sizeof t.log);
  return ORION_OK;
}
int orion_rs_gf_mul(unsigned a, unsigned b) {
  if (a > 255 || b > 255) return fail(ORION_E_ARG, "gf: an element is 0..255");
  return orion::rs::Gf256::shared().mul(static_cast<uint8_t>(a), static_cast<uint8_t>(b));
}
int orion_rs_gf_div(unsigned a, unsigned b) {
  if (a > 255 || b > 255) return fail(ORION_E_ARG, "gf: an element is 0..255");
  return guarded([&] { return int(orion::rs::Gf256::shared().div(static_cast<uint8_t>(a), static_cast<uint8_t>(b))); });
}
int orion_rs_gf_inv(unsigned a) {
  if (a > 255) return fail(ORION_E_ARG, "gf: an element is 0..255");
  return guarded([&] { return int(orion::rs::Gf256::shared().inv(static_cast<uint8_t>(a))); });
}
int orion_rs_gf_pow(unsigned a, size_t n) {
  if (a > 255) return fail(ORION_E_ARG, "gf: an element is 0..255");
  return orion::rs::Gf256::shared().pow(static_cast<uint8_t>(a), n);
}
int orion_rs_gf_exp_of(size_t i) { return orion::rs::Gf256::shared().exp_of(i); }
int orion_rs_generator(size_t n, size_t n_parity, uint8_t* out) {
  if (!out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::rs::ReedSolomon code(n, n_parity);
    std::memcpy(out, code.generator().data(), code.generator().size());
    return ORION_OK;
  });
}
int orion_rs_encode(size_t n, size_t n_parity, const uint8_t* msgs, size_t nwords, uint8_t* cws) {
  if (nwords && (!msgs || !cws)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "rs: nwords above 2^32");
  return guarded([&] {
    const orion::rs::ReedSolomon code(n, n_parity);
    if (n_parity == 0) throw std::invalid_argument("rs encode: a code without parity symbols has no shift register");
    for (size_t w = 0; w < nwords; ++w) code.encode(msgs + w * code.k(), cws + w * n);
    return ORION_OK;
  });
}
int orion_rs_decode_counted(size_t n, size_t n_parity, const uint8_t* words, size_t nwords, uint8_t* msgs,
                            int32_t* status) {
  if (nwords && (!words || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "rs: nwords above 2^32");
  return guarded([&] {
    const orion::rs::ReedSolomon code(n, n_parity);
    for (size_t w = 0; w < nwords; ++w) status[w] = code.decode_counted(words + w * n, msgs + w * code.k());
    return ORION_OK;
  });
}
orion_rs_forney* orion_rs_forney_new(size_t branches, size_t depth, int inverse) {
  return make_handle([&]() -> orion_rs_forney* {
    if (inverse) return new orion_rs_forney{orion::rs::ConvDeinterleaver(branches, depth)};
    return new orion_rs_forney{orion::rs::ConvInterleaver(branches, depth)};
  });
}
void orion_rs_forney_free(orion_rs_forney* f) { delete f; }
int orion_rs_forney_feed(orion_rs_forney* f, const uint8_t* in, size_t n, uint8_t* out) {
  if (!f || (n && (!in || !out))) return fail(ORION_E_NULL, "null handle or buffer");
  f->impl.feed(in, n, out);
  return ORION_OK;
}
int orion_rs_forney_flush(orion_rs_forney* f, uint8_t* out) {
  if (!f || (f->impl.roundtrip_delay() && !out)) return fail(ORION_E_NULL, "null handle or buffer");
  return guarded([&] {
    const std::vector<uint8_t> v = f->impl.flush();
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_rs_forney_reset(orion_rs_forney* f) {
  if (!f) return fail(ORION_E_NULL, "null handle");
  f->impl.reset();
  return ORION_OK;
}
size_t orion_rs_forney_delay(size_t branches, size_t depth) {
  return size_or_zero([&] { return orion::rs::conv_roundtrip_delay(branches, depth); });
}
size_t orion_rs_forney_frame_len(size_t branches, size_t depth, size_t n) {
  return size_or_zero([&] { return orion::rs::forney_frame_len(branches, depth, n); });
}
int orion_rs_forney_frame_interleave(size_t branches, size_t depth, const uint8_t* bytes, size_t n, uint8_t* out) {
  if ((n && !bytes) || !out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::rs::forney_frame_interleave(branches, depth, bytes, n);
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_rs_forney_frame_deinterleave(size_t branches, size_t depth, const uint8_t* bytes, size_t total,
                                       uint8_t* out) {
  if (total && (!bytes || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::rs::forney_frame_deinterleave(branches, depth, bytes, total);
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_rs_pn_scramble(uint32_t taps, uint32_t width, uint32_t seed, uint8_t* data, size_t n) {
  if (n && !data) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs::PnScrambler(taps, width, seed).scramble(data, n);
    return ORION_OK;
  });
}
orion_rs_pn_stream* orion_rs_pn_stream_new(uint32_t taps, uint32_t width, uint32_t seed) {
  return make_handle([&] { return new orion_rs_pn_stream{orion::rs::PnScramblerStream(taps, width, seed)}; });
}
void orion_rs_pn_stream_free(orion_rs_pn_stream* s) { delete s; }
int orion_rs_pn_stream_feed(orion_rs_pn_stream* s, uint8_t* data, size_t n) {
  if (!s || (n && !data)) return fail(ORION_E_NULL, "null handle or buffer");
  s->impl.feed_in_place(data, n);
  return ORION_OK;
}
int orion_rs_pn_stream_reset(orion_rs_pn_stream* s) {
  if (!s) return fail(ORION_E_NULL, "null handle");
  s->impl.reset();
  return ORION_OK;
}
orion_rs_dispersal* orion_rs_dispersal_new(void) {
  return make_handle([&] { return new orion_rs_dispersal{}; });
}
void orion_rs_dispersal_free(orion_rs_dispersal* d) { delete d; }
int orion_rs_dispersal_feed(orion_rs_dispersal* d, uint8_t* data, size_t n) {
  if (!d || (n && !data)) return fail(ORION_E_NULL, "null handle or buffer");
  d->impl.feed_in_place(data, n);
  return ORION_OK;
}
int orion_rs_dispersal_advance_byte(orion_rs_dispersal* d) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  d->impl.advance_byte();
  return ORION_OK;
}
int orion_rs_dispersal_reset(orion_rs_dispersal* d) {
  if (!d) return fail(ORION_E_NULL, "null handle");
  d->impl.reset();
  return ORION_OK;
}
int orion_rs_ts_energy_disperse(uint8_t* packets, size_t n) {
  if (n && !packets) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs::ts_energy_disperse(packets, n);
    return ORION_OK;
  });
}
int orion_rs_ts_dispersal_mask(uint8_t* out) {
  if (!out) return fail(ORION_E_NULL, "null buffer");
  const orion::rs::TsDispersalMask& mask = orion::rs::ts_dispersal_mask();
  std::memcpy(out, mask.m, sizeof mask.m);
  return ORION_OK;
}
size_t orion_rs_ts_packetized_len(size_t n) {
  if (n > (size_t(1) << 40)) {
    fail(ORION_E_ARG, "ts: n above 2^40");
    return 0;
  }
  return std::max<size_t>((n + orion::rs::kTsPayloadLen - 1) / orion::rs::kTsPayloadLen, 1) * orion::rs::kTsPacketLen;
}
int orion_rs_ts_packetize(const uint8_t* payload, size_t n, uint8_t* out) {
  if ((n && !payload) || !out) return fail(ORION_E_NULL, "null buffer");
  if (n > (size_t(1) << 40)) return fail(ORION_E_ARG, "ts: n above 2^40");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::rs::ts_packetize(payload, n);
    std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_rs_ts_depacketize(const uint8_t* packets, size_t n, uint8_t* out) {
  if (n && (!packets || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::rs::ts_depacketize(packets, n);
    std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
int orion_rs_ts_null_packet(uint8_t* out) {
  if (!out) return fail(ORION_E_NULL, "null buffer");
  orion::rs::ts_null_packet(out);
  return ORION_OK;
}
int orion_rs_ts_stuff_null_packets(const uint8_t* ts, size_t n, size_t target_packets, uint8_t* out) {
  if ((n && !ts) || ((n || target_packets) && !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    std::vector<uint8_t> v(ts, ts + n);
    orion::rs::ts_stuff_null_packets(v, target_packets);
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return ORION_OK;
  });
}
size_t orion_rs_decode_stream_len(size_t n, size_t n_parity, size_t ncw, int bits, size_t branches, size_t depth) {
  return size_or_zero([&] { return orion::rs_decode_stream_len(n, n_parity, ncw, rs_fusion(bits, branches, depth, 0)); });
}
int orion_rs_decode_batch(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, int bits,
                          size_t branches, size_t depth, int derandomize, uint8_t* msgs, int32_t* status) {
  if (nstreams && (!in || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs_decode_batch_host(n, n_parity, in, nstreams, ncw, rs_fusion(bits, branches, depth, derandomize), msgs,
                                status);
    return ORION_OK;
  });
}
int orion_rs_decode_batch_device(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, int bits,
                                 size_t branches, size_t depth, int derandomize, uint8_t* msgs, int32_t* status,
                                 void* stream) {
  if (nstreams && (!in || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs_decode_batch(n, n_parity, in, nstreams, ncw, rs_fusion(bits, branches, depth, derandomize), msgs, status,
                           static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_rs_encode_batch(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw, int disperse,
                          uint8_t* cws) {
  if (nstreams && (!msgs || !cws)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs_encode_batch_host(n, n_parity, msgs, nstreams, ncw, rs_fusion(0, 0, 0, disperse), cws);
    return ORION_OK;
  });
}
int orion_rs_encode_batch_device(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw,
                                 int disperse, uint8_t* cws, void* stream) {
  if (nstreams && (!msgs || !cws)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::rs_encode_batch(n, n_parity, msgs, nstreams, ncw, rs_fusion(0, 0, 0, disperse), cws,
                           static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_rs_forney_interleave_len(size_t branches, size_t depth, size_t len, int bits) {
  return size_or_zero([&] { return orion::forney_interleave_stream_len(branches, depth, len, bits != 0); });
}
int orion_rs_forney_interleave_batch(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len,
                                     int bits, uint8_t* out) {
  if (nstreams && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::forney_interleave_batch_host(branches, depth, in, nstreams, len, bits != 0, out);
    return ORION_OK;
  });
}
int orion_rs_forney_interleave_batch_device(size_t branches, size_t depth, const uint8_t* in, size_t nstreams,
                                            size_t len, int bits, uint8_t* out, void* stream) {
  if (nstreams && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::forney_interleave_batch(branches, depth, in, nstreams, len, bits != 0, out,
                                   static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

/* ---- the frame chain's codes (ldpc_family.hpp, bch.hpp, k_ldpc_family.hip, k_bch.hip) ---- */
int orion_ldpcf_dims(int code, uint32_t* out) {
  if (!out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::ldpcf::Ldpc& c = orion::ldpcf::Ldpc::get(code);
    const size_t v[6] = {c.n(), c.k(), c.m(), c.n_edges(), c.max_check_degree(), c.relaxed_picks()};
    for (int i = 0; i < 6; ++i) out[i] = static_cast<uint32_t>(v[i]);
    return ORION_OK;
  });
}
int orion_ldpcf_graph(int code, uint32_t* check_start, uint32_t* check_bits, uint32_t* bit_start,
                      uint32_t* bit_checks, uint32_t* bit_edges) {
  if (!check_start || !check_bits || !bit_start || !bit_checks || !bit_edges) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::ldpcf::Ldpc& c = orion::ldpcf::Ldpc::get(code);
    std::copy(c.check_start().begin(), c.check_start().end(), check_start);
    std::copy(c.check_bits().begin(), c.check_bits().end(), check_bits);
    std::copy(c.bit_start().begin(), c.bit_start().end(), bit_start);
    std::copy(c.bit_checks().begin(), c.bit_checks().end(), bit_checks);
    std::copy(c.bit_edges().begin(), c.bit_edges().end(), bit_edges);
    return ORION_OK;
  });
}
int orion_ldpcf_encode(int code, const uint8_t* msgs, size_t nwords, uint8_t* cws) {
  if (nwords && (!msgs || !cws)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "ldpc family: nwords above 2^32");
  return guarded([&] {
    const orion::ldpcf::Ldpc& c = orion::ldpcf::Ldpc::get(code);
    for (size_t w = 0; w < nwords; ++w) c.encode(msgs + w * c.k(), cws + w * c.n());
    return ORION_OK;
  });
}
int orion_ldpcf_syndrome_weight(int code, const uint8_t* hard, size_t nwords, int32_t* unsat) {
  if (nwords && (!hard || !unsat)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "ldpc family: nwords above 2^32");
  return guarded([&] {
    const orion::ldpcf::Ldpc& c = orion::ldpcf::Ldpc::get(code);
    for (size_t w = 0; w < nwords; ++w) unsat[w] = static_cast<int32_t>(c.syndrome_weight(hard + w * c.n()));
    return ORION_OK;
  });
}
int orion_ldpcf_decode_soft(int code, const float* llr, size_t nwords, size_t max_iter, int rule, float scale,
                            uint8_t* bits, int32_t* unsat, int32_t* iterations) {
  if (nwords && (!llr || !bits || !unsat || !iterations)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "ldpc family: nwords above 2^32");
  return guarded([&] {
    const orion::ldpcf::Ldpc& c = orion::ldpcf::Ldpc::get(code);
    orion::ldpcf::check_rule(rule);
    if (max_iter > orion::kLdpcfMaxIter) throw std::invalid_argument("ldpc family decode: max_iter above 2^30");
    for (size_t w = 0; w < nwords; ++w) {
      const orion::ldpcf::DecodeResult r = c.decode_soft(llr + w * c.n(), max_iter, rule, scale, bits + w * c.k());
      unsat[w] = static_cast<int32_t>(r.unsat);
      iterations[w] = static_cast<int32_t>(r.iterations);
    }
    return ORION_OK;
  });
}
size_t orion_ldpcf_decode_blocks(int code, size_t n_llr, size_t rows, size_t cols) {
  return size_or_zero([&] { return orion::ldpcf_decode_blocks(code, n_llr, rows, cols); });
}
int orion_ldpcf_decode_batch(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                             size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat,
                             int32_t* iterations) {
  if (nstreams && (!llr || !bits || !unsat || !iterations)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpcf_decode_batch_host(code, llr, nstreams, n_llr, rows, cols, max_iter, rule, scale, bits, unsat,
                                   iterations);
    return ORION_OK;
  });
}
int orion_ldpcf_decode_batch_device(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows,
                                    size_t cols, size_t max_iter, int rule, float scale, uint8_t* bits,
                                    int32_t* unsat, int32_t* iterations, void* stream) {
  if (nstreams && (!llr || !bits || !unsat || !iterations)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpcf_decode_batch(code, llr, nstreams, n_llr, rows, cols, max_iter, rule, scale, bits, unsat, iterations,
                              static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_ldpcf_encoded_len(int code, size_t nbits, size_t rows, size_t cols) {
  return size_or_zero([&] { return orion::ldpcf_encoded_len(code, nbits, rows, cols); });
}
int orion_ldpcf_encode_batch(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                             uint8_t* coded) {
  if (nstreams && (!bits || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpcf_encode_batch_host(code, bits, nstreams, nbits, rows, cols, coded);
    return ORION_OK;
  });
}
int orion_ldpcf_encode_batch_device(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows,
                                    size_t cols, uint8_t* coded, void* stream) {
  if (nstreams && (!bits || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::ldpcf_encode_batch(code, bits, nstreams, nbits, rows, cols, coded, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
size_t orion_bch_parity_bits(size_t t) {
  return size_or_zero([&] { return orion::bch::Bch(255, t).parity_bits(); });
}
int orion_bch_generator(size_t n, size_t t, uint8_t* out) {
  if (!out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::bch::Bch code(n, t);
    std::memcpy(out, code.generator().data(), code.generator().size());
    return ORION_OK;
  });
}
int orion_bch_encode(size_t n, size_t t, const uint8_t* msgs, size_t nwords, uint8_t* cws) {
  if (nwords && (!msgs || !cws)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "bch: nwords above 2^32");
  return guarded([&] {
    const orion::bch::Bch code(n, t);
    for (size_t w = 0; w < nwords; ++w) code.encode(msgs + w * code.k(), cws + w * n);
    return ORION_OK;
  });
}
int orion_bch_decode(size_t n, size_t t, const uint8_t* words, size_t nwords, uint8_t* msgs, int32_t* status,
                     int32_t* locator_len) {
  if (nwords && (!words || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  if (nwords > kRsMaxHostWords) return fail(ORION_E_ARG, "bch: nwords above 2^32");
  return guarded([&] {
    const orion::bch::Bch code(n, t);
    for (size_t w = 0; w < nwords; ++w) {
      size_t len = 0;
      status[w] = code.decode(words + w * n, msgs + w * code.k(), &len);
      if (locator_len) locator_len[w] = static_cast<int32_t>(len);
    }
    return ORION_OK;
  });
}
int orion_bch_decode_batch(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                           int32_t* status) {
  if (nstreams && (!in || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::bch_decode_batch_host(t, info_bits, in, nstreams, nb, msgs, status);
    return ORION_OK;
  });
}
int orion_bch_decode_batch_device(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb,
                                  uint8_t* msgs, int32_t* status, void* stream) {
  if (nstreams && (!in || !msgs || !status)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::bch_decode_batch(t, info_bits, in, nstreams, nb, msgs, status, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_bch_encode_batch(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                           uint8_t* coded) {
  if (nstreams && (!bits || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::bch_encode_batch_host(t, info_bits, bits, nstreams, nbits, coded);
    return ORION_OK;
  });
}
int orion_bch_encode_batch_device(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                                  uint8_t* coded, void* stream) {
  if (nstreams && (!bits || !coded)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::bch_encode_batch(t, info_bits, bits, nstreams, nbits, coded, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

}  // extern "C"

/* ---- the frame layer's coding chain (frame.hpp, k_frame.hip) ---- */
namespace {
static_assert(sizeof(long long) == sizeof(int64_t) && ORION_FRAME_CRC32 == orion::frame::kCrc32 &&
                  ORION_FRAME_OUTER_RS == orion::frame::kOuterRs && ORION_FRAME_INNER_CONV == orion::frame::kInnerConv &&
                  ORION_FRAME_IL_FORNEY == orion::frame::kIlForney && ORION_FRAME_SCR_DVBT == orion::frame::kScrDvbT &&
                  ORION_FRAME_SCR_AFTER_INNER == orion::frame::kAfterInnerFec &&
                  ORION_FRAME_HEADER_FIELD_BYTES == orion::frame::kHeaderFieldBytes &&
                  ORION_RX_MALFORMED_HEADER == orion::frame::kRxMalformedHeader &&
                  ORION_RX_FEC_UNCORRECTABLE == orion::frame::kRxFecUncorrectable,
              "the header's frame constants are frame.hpp's");
orion::frame::Scheme scheme_of(const orion_frame_scheme* s) {
  if (!s) throw std::invalid_argument("frame: null scheme");
  orion::frame::Scheme o;
  o.crc = s->crc;
  o.outer = s->outer;
  o.outer_a = s->outer_a;
  o.outer_b = s->outer_b;
  o.inner = s->inner;
  o.inner_a = s->inner_a;
  o.inner_b = s->inner_b;
  o.outer_il = s->outer_il;
  o.outer_il_a = s->outer_il_a;
  o.outer_il_b = s->outer_il_b;
  o.inner_il = s->inner_il;
  o.inner_il_a = s->inner_il_a;
  o.inner_il_b = s->inner_il_b;
  o.scrambler = s->scrambler;
  o.scr_poly = s->scr_poly;
  o.scr_width = s->scr_width;
  o.scr_per_frame = s->scr_per_frame;
  o.scr_seed = s->scr_seed;
  o.scrambler_pos = s->scrambler_pos;
  orion::frame::check_scheme(o);
  return o;
}
const long long* ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
long long* ll(int64_t* p) { return reinterpret_cast<long long*>(p); }
}  // namespace

extern "C" {

uint32_t orion_frame_crc16(const uint8_t* data, size_t n) { return data || !n ? orion::frame::crc16(data, n) : 0; }
uint32_t orion_frame_crc32(const uint8_t* data, size_t n) { return data || !n ? orion::frame::crc32(data, n) : 0; }
int orion_frame_append_crc(int crc, const uint8_t* data, size_t n, uint8_t* out) {
  if ((n && !data) || !out) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<uint8_t> v = orion::frame::append_crc(crc, data, n);
    std::copy(v.begin(), v.end(), out);
    return ORION_OK;
  });
}
int orion_frame_check_crc(int crc, const uint8_t* data, size_t n, int32_t* ok) {
  if ((n && !data) || !ok) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    *ok = orion::frame::check_crc(crc, data, n) ? 1 : 0;
    return ORION_OK;
  });
}
int orion_frame_pack_header(const uint32_t* fields, uint8_t* out14) {
  if (!fields || !out14) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame::pack_header_fields({fields[0], fields[1], fields[2], fields[3], fields[4]}, out14);
    return ORION_OK;
  });
}
int orion_frame_unpack_header(const uint8_t* in14, uint32_t* fields) {
  if (!fields || !in14) return fail(ORION_E_NULL, "null buffer");
  const orion::frame::HeaderFields f = orion::frame::unpack_header_fields(in14);
  const uint32_t v[5] = {f.mcs_index, f.payload_len, f.sequence_num, f.flags, f.scrambler_seed};
  std::copy(v, v + 5, fields);
  return ORION_OK;
}
uint32_t orion_frame_reduce_seed(uint32_t width, uint32_t raw) { return orion::frame::reduce_seed(width, raw); }
int orion_frame_scramble_bytes(const orion_frame_scheme* s, uint32_t per_frame_seed, uint8_t* bytes, size_t n) {
  if (n && !bytes) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame::scramble_bytes(scheme_of(s), per_frame_seed, bytes, n);
    return ORION_OK;
  });
}
int orion_frame_scramble_bits(const orion_frame_scheme* s, uint32_t per_frame_seed, uint8_t* bits, size_t n) {
  if (n && !bits) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame::scramble_bits(scheme_of(s), per_frame_seed, bits, n);
    return ORION_OK;
  });
}
int orion_frame_apply_pn_to_llrs(const orion_frame_scheme* s, uint32_t per_frame_seed, float* llr, size_t n) {
  if (n && !llr) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame::apply_pn_to_llrs(scheme_of(s), per_frame_seed, llr, n);
    return ORION_OK;
  });
}
int orion_frame_block_plan(const orion_frame_scheme* s, size_t info_bytes, size_t* plan) {
  if (!plan) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::frame::BlockPlan p = orion::frame::block_plan(info_bytes, scheme_of(s));
    const size_t v[6] = {p.info_bytes,    p.framed_bytes,     p.outer_coded_bits,
                         p.outer_il_bits, p.inner_coded_bits, p.coded_bits};
    std::copy(v, v + 6, plan);
    return ORION_OK;
  });
}
int orion_frame_encode_chain(const orion_frame_scheme* s, const uint8_t* bytes, size_t n, uint32_t per_frame_seed,
                             uint8_t* coded, uint8_t* outer_il_bits) {
  if ((n && !bytes) || !coded) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::frame::EncodedStages st = orion::frame::encode_chain_stages(bytes, n, scheme_of(s), per_frame_seed);
    std::copy(st.coded.begin(), st.coded.end(), coded);
    if (outer_il_bits) std::copy(st.outer_il_bits.begin(), st.outer_il_bits.end(), outer_il_bits);
    return ORION_OK;
  });
}
int orion_frame_decode_chain(const orion_frame_scheme* s, const float* llr, size_t n_llr, size_t info_bytes,
                             uint32_t per_frame_seed, int ldpc_rule, float ldpc_scale, uint8_t* bytes,
                             int32_t* outcome, uint8_t* inner_out_bits, size_t inner_cap, size_t* inner_out_len) {
  if ((n_llr && !llr) || (info_bytes && !bytes) || !outcome) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::frame::Scheme sch = scheme_of(s);
    const orion::frame::BlockPlan plan = orion::frame::block_plan(info_bytes, sch);
    const orion::frame::ChainOutcome o =
        orion::frame::decode_chain(llr, n_llr, plan, sch, per_frame_seed, ldpc_rule, ldpc_scale);
    std::fill(outcome, outcome + 8, 0);
    outcome[0] = o.error;
    if (inner_out_len) *inner_out_len = o.inner_out_bits.size();
    if (o.error) return ORION_OK;
    if (inner_out_bits) {
      if (o.inner_out_bits.size() > inner_cap) throw std::invalid_argument("frame decode: inner_out_bits too small");
      std::copy(o.inner_out_bits.begin(), o.inner_out_bits.end(), inner_out_bits);
    }
    std::copy(o.bytes.begin(), o.bytes.end(), bytes);
    outcome[1] = o.inner_ok;
    outcome[2] = o.outer_ok;
    outcome[3] = o.crc_ok;
    outcome[4] = o.crc_present;
    outcome[5] = o.outer_present;
    outcome[6] = static_cast<int32_t>(o.outer_corrected_bytes);
    outcome[7] = o.is_valid();
    return ORION_OK;
  });
}
int orion_frame_pack_batch(const orion_frame_scheme* s, const uint8_t* payload, const int64_t* fields,
                           const int64_t* seeds, size_t nframes, size_t info_len, int out_bytes, uint8_t* out) {
  if (nframes && ((!payload && !fields && info_len) || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_pack_batch_host(scheme_of(s), payload, ll(fields), ll(seeds), nframes, info_len, out_bytes != 0, out);
    return ORION_OK;
  });
}
int orion_frame_pack_batch_device(const orion_frame_scheme* s, const uint8_t* payload, const int64_t* fields,
                                  const int64_t* seeds, size_t nframes, size_t info_len, int out_bytes, uint8_t* out,
                                  void* stream) {
  if (nframes && ((!payload && !fields && info_len) || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_pack_batch(scheme_of(s), payload, ll(fields), ll(seeds), nframes, info_len, out_bytes != 0, out,
                            static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_frame_unpack_batch(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, int in_bytes,
                             const int64_t* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                             size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                             int32_t* corrected, int64_t* fields) {
  if (nframes && (!in || (!payload && info_len) || !flags || !corrected)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_unpack_batch_host(scheme_of(s), in, in_stride, in_bytes != 0, ll(seeds), unsat, n_inner, status,
                                   n_outer, nframes, info_len, payload, flags, corrected, ll(fields));
    return ORION_OK;
  });
}
int orion_frame_unpack_batch_device(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, int in_bytes,
                                    const int64_t* seeds, const int32_t* unsat, size_t n_inner,
                                    const int32_t* status, size_t n_outer, size_t nframes, size_t info_len,
                                    uint8_t* payload, uint8_t* flags, int32_t* corrected, int64_t* fields,
                                    void* stream) {
  if (nframes && (!in || (!payload && info_len) || !flags || !corrected)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_unpack_batch(scheme_of(s), in, in_stride, in_bytes != 0, ll(seeds), unsat, n_inner, status, n_outer,
                              nframes, info_len, payload, flags, corrected, ll(fields),
                              static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_frame_coded_bits_batch(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride, size_t nbits,
                                 const int64_t* seeds, size_t nframes, size_t out_len, uint8_t* out) {
  if (nframes && ((!in && nbits) || (!out && out_len))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_coded_bits_batch_host(scheme_of(s), in, in_stride, nbits, ll(seeds), nframes, out_len, out);
    return ORION_OK;
  });
}
int orion_frame_coded_bits_batch_device(const orion_frame_scheme* s, const uint8_t* in, size_t in_stride,
                                        size_t nbits, const int64_t* seeds, size_t nframes, size_t out_len,
                                        uint8_t* out, void* stream) {
  if (nframes && ((!in && nbits) || (!out && out_len))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_coded_bits_batch(scheme_of(s), in, in_stride, nbits, ll(seeds), nframes, out_len, out,
                                  static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_frame_llr_prepare_batch(const orion_frame_scheme* s, const float* in, size_t in_stride, size_t n,
                                  const int64_t* seeds, size_t nframes, float* out) {
  if (nframes && n && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_llr_prepare_batch_host(scheme_of(s), in, in_stride, n, ll(seeds), nframes, out);
    return ORION_OK;
  });
}
int orion_frame_llr_prepare_batch_device(const orion_frame_scheme* s, const float* in, size_t in_stride, size_t n,
                                         const int64_t* seeds, size_t nframes, float* out, void* stream) {
  if (nframes && n && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_llr_prepare_batch(scheme_of(s), in, in_stride, n, ll(seeds), nframes, out,
                                   static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_frame_assemble_batch_device(const void* lead, size_t lead_len, const void* hdr, size_t hdr_len,
                                      const void* pay, size_t pay_len, size_t nframes, size_t sps, size_t win_start,
                                      const float* ramp, size_t ramp_len, void* out, void* stream) {
  if (nframes && ((lead_len && !lead) || (hdr_len && !hdr) || (pay_len && !pay) || !out))
    return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_assemble_batch(static_cast<const float*>(lead), lead_len, static_cast<const float*>(hdr), hdr_len,
                                static_cast<const float*>(pay), pay_len, nframes, sps, win_start, ramp, ramp_len,
                                static_cast<float*>(out), static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_frame_bytes_to_bits_batch(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out) {
  if (nframes && nbytes && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_bytes_to_bits_batch_host(in, nframes, nbytes, out);
    return ORION_OK;
  });
}
int orion_frame_bytes_to_bits_batch_device(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out,
                                           void* stream) {
  if (nframes && nbytes && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::frame_bytes_to_bits_batch(in, nframes, nbytes, out, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

// ---- OFDM burst acquisition (acquire.hpp) ----
static orion::acquire::Preamble preamble_of(const orion_ofdm_preamble* p) {
  orion::acquire::Preamble q;
  q.num_repeats = p->num_repeats;
  q.repeat_len = p->repeat_len;
  q.training = p->training != 0;
  q.tn_fft = q.training ? p->training_n_fft : 0;
  q.tcp = q.training ? p->training_cp_len : 0;
  return q;
}
size_t orion_ofdm_sync_offsets(size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                               size_t search_end) {
  if (!pre) return 0;
  const orion::acquire::Preamble q = preamble_of(pre);
  if (!orion::acquire::search_ok(n, fs, q, search_start, search_end)) return 0;
  return orion::acquire::search_end(n, q, search_end) - search_start;
}
int orion_ofdm_sync_host(const void* iq, size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                         size_t search_end, orion_ofdm_sync_result* results, size_t cap, size_t* count, float* r_peak) {
  if (!pre || !count || (n && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const std::vector<orion::acquire::SyncResult> r =
        orion::acquire::ofdm_sync(static_cast<const float*>(iq), n, fs, preamble_of(pre), search_start, search_end, r_peak);
    if (r.size() > cap || (r.size() && !results)) return fail(ORION_E_ARG, "ofdm_sync: results holds fewer than the offsets");
    if (!r.empty()) std::memcpy(results, r.data(), r.size() * sizeof(orion_ofdm_sync_result));
    *count = r.size();
    return ORION_OK;
  });
}
int orion_ofdm_sc_metric_host(const void* iq, size_t n, float fs, const orion_ofdm_preamble* pre, size_t search_start,
                              size_t search_end, void* p, float* r) {
  if (!pre || (n && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::acquire::Preamble q = preamble_of(pre);
    if (!orion::acquire::search_ok(n, fs, q, search_start, search_end)) return ORION_OK;
    if (!p || !r) return fail(ORION_E_NULL, "null buffer");
    orion::acquire::sc_metric(static_cast<const float*>(iq), q, search_start, orion::acquire::search_end(n, q, search_end),
                              static_cast<float*>(p), r);
    return ORION_OK;
  });
}
int orion_ofdm_earliest_accepted(const orion_ofdm_sync_result* results, size_t n, float score_threshold,
                                 size_t cluster_len, int64_t* index) {
  if (!index || (n && !results)) return fail(ORION_E_NULL, "null buffer");
  *index = orion::acquire::earliest_accepted(reinterpret_cast<const orion::acquire::SyncResult*>(results), n,
                                             score_threshold, cluster_len);
  return ORION_OK;
}
int orion_ofdm_integer_cfo_host(const void* iq, size_t n, float fs, size_t training_n_fft, size_t training_cp_len,
                                size_t training_start, float fractional_cfo_hz, int32_t* bins, float* corr2) {
  if (!bins || (n && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    *bins = orion::acquire::estimate_integer_cfo_bins(static_cast<const float*>(iq), n, fs, training_n_fft, training_cp_len,
                                                      training_start, fractional_cfo_hz, corr2);
    return ORION_OK;
  });
}
int orion_ofdm_rotate_block_host(float freq_hz, float fs, const void* in, size_t n, void* out) {
  if (n && (!in || !out)) return fail(ORION_E_NULL, "null buffer");
  orion::acquire::rotate_block(freq_hz, fs, static_cast<const float*>(in), n, static_cast<float*>(out));
  return ORION_OK;
}
int orion_ofdm_cpe_host(int constellation, void* syms, size_t n_sym, size_t n_data) {
  if (n_sym && n_data && !syms) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (orion::ofdm::bits_per_symbol(constellation) == 0) return fail(ORION_E_ARG, "unknown constellation");
    orion::acquire::remove_common_phase_error(constellation, static_cast<float*>(syms), n_sym, n_data);
    return ORION_OK;
  });
}
int orion_ofdm_soft_demap_equalized_host(const orion_ofdm_config* cfg, int constellation, const void* iq, size_t n_sym,
                                         const void* training_freq, void* syms, float* llr) {
  if (!cfg) return fail(ORION_E_NULL, "null configuration");
  if (!training_freq || (n_sym && (!iq || !syms))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    if (orion::ofdm::bits_per_symbol(constellation) == 0) return fail(ORION_E_ARG, "unknown constellation");
    orion::ofdm::Config c = cfg->impl;
    c.constellation = constellation;
    orion::acquire::soft_demap_equalized(c, static_cast<const float*>(iq), n_sym, static_cast<const float*>(training_freq),
                                         static_cast<float*>(syms), llr);
    return ORION_OK;
  });
}
orion_ofdm_acquire* orion_ofdm_acquire_new(const orion_ofdm_preamble* pre) {
  if (!pre) {
    fail(ORION_E_NULL, "null preamble");
    return nullptr;
  }
  try {
    return new orion_ofdm_acquire(preamble_of(pre));
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void orion_ofdm_acquire_free(orion_ofdm_acquire* a) { delete a; }
int orion_ofdm_sync_batch_device(orion_ofdm_acquire* a, const void* iq, size_t ncap, size_t n, float fs,
                                 size_t search_start, size_t search_end, float score_threshold,
                                 const orion_ofdm_sync_out* out, void* stream) {
  if (!a) return fail(ORION_E_NULL, "null handle");
  if (!out || (ncap && !iq)) return fail(ORION_E_NULL, "null buffer");
  const void* const* f = reinterpret_cast<const void* const*>(out);
  for (size_t k = 0; k < sizeof(orion_ofdm_sync_out) / sizeof(void*); ++k)
    if (ncap && !f[k]) return fail(ORION_E_NULL, "null output");
  return guarded([&] {
    orion::SyncOut o;
    std::memcpy(&o, out, sizeof(o));
    a->impl.sync_batch(iq, ncap, n, fs, search_start, search_end, score_threshold, o, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_acquire_correct_device(orion_ofdm_acquire* a, const void* iq, size_t ncap, size_t n, float fs, size_t n_fft,
                                      const orion_ofdm_sync_out* sync, void* rows, int32_t* avail, float* total_cfo,
                                      void* stream) {
  if (!a) return fail(ORION_E_NULL, "null handle");
  if (!sync || (ncap && n && (!iq || !rows || !avail || !total_cfo || !sync->accepted_start || !sync->accepted_cfo_hz ||
                              !sync->accepted_bins)))
    return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::SyncOut o;
    std::memcpy(&o, sync, sizeof(o));
    a->impl.correct(iq, ncap, n, fs, n_fft, o, rows, avail, total_cfo, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_acquire_weights_device(orion_ofdm_acquire* a, const void* rows, size_t ncap, size_t n, size_t window,
                                      void* weights, void* stream) {
  if (!a) return fail(ORION_E_NULL, "null handle");
  if (ncap && (!rows || !weights)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    a->impl.weights(rows, ncap, n, window, weights, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_ofdm_equalize_track_device(orion_ofdm* h, const void* raw, const void* weights, size_t frames, size_t n_symbols,
                                     void* syms, float* llr, void* stream) {
  if (!h) return fail(ORION_E_NULL, "null handle");
  if (h->kind != kOfdmDemod) return fail(ORION_E_TYPE, "not a demodulator");
  if (frames && n_symbols && (!raw || !weights || !syms)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    h->impl.equalize_track(raw, weights, frames, n_symbols, syms, llr, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

// ---- the DVB-T 2K frame (dvbt.hpp, dvbt_blocks.hpp) ----
static_assert(ORION_DVBT_N_FFT == orion::dvbt::kNFft && ORION_DVBT_DATA_CARRIERS == orion::dvbt::kData &&
                  ORION_DVBT_TPS_CARRIERS == orion::dvbt::kTps && ORION_DVBT_CONTINUAL_PILOTS == orion::dvbt::kContinual &&
                  ORION_DVBT_TPS_SYMBOLS == orion::dvbt::kTpsSymbols && ORION_DVBT_MAX_REF_PILOTS == orion::dvbt::kMaxRefPilots &&
                  ORION_DVBT_MAX_RX_WINDOW_BACKOFF == orion::dvbt::kMaxRxWindowBackoff &&
                  sizeof(orion_dvbt_gi_out) == sizeof(orion::GiOut),
              "the header's DVB-T constants are dvbt.hpp's");
static bool dvbt_v_ok(size_t v) { return v == 2 || v == 4 || v == 6; }
int orion_dvbt_constants(uint32_t* continual, uint32_t* tps, uint32_t* continual_bins, uint32_t* tps_bins, uint8_t* wk) {
  return guarded([&] {
    const orion::dvbt::Tables& t = orion::dvbt::tables();
    for (size_t i = 0; i < orion::dvbt::kContinual; ++i) {
      if (continual) continual[i] = orion::dvbt::kContinualPilots2k[i];
      if (continual_bins) continual_bins[i] = t.continual_bins[i];
    }
    for (size_t i = 0; i < orion::dvbt::kTps; ++i) {
      if (tps) tps[i] = orion::dvbt::kTpsCarriers2k[i];
      if (tps_bins) tps_bins[i] = t.tps_bins[i];
    }
    if (wk) {
      const std::vector<uint8_t> w = orion::dvbt::wk_prbs(orion::dvbt::kActive);
      std::memcpy(wk, w.data(), w.size());
    }
    return ORION_OK;
  });
}
float orion_dvbt_boosted_pilot_value(uint8_t wk) { return orion::dvbt::boosted_pilot_value(wk); }
int orion_dvbt_phase(int phase, uint32_t* data_bins, uint32_t* pilot_bins, float* pilot_vals, size_t* n_pilots,
                     uint32_t* ref_bins, float* ref_vals, size_t* n_ref, int32_t* role) {
  if (phase < 0 || phase > 3) return fail(ORION_E_ARG, "dvbt: phase is 0..3");
  return guarded([&] {
    const orion::dvbt::Phase& p = orion::dvbt::tables().phase[phase];
    if (data_bins) std::copy(p.data_bins.begin(), p.data_bins.end(), data_bins);
    if (pilot_bins) std::copy(p.pilot_bins.begin(), p.pilot_bins.end(), pilot_bins);
    if (pilot_vals) std::copy(p.pilot_val.begin(), p.pilot_val.end(), pilot_vals);
    if (n_pilots) *n_pilots = p.pilot_bins.size();
    if (ref_bins) std::copy(p.ref_bins.begin(), p.ref_bins.end(), ref_bins);
    if (ref_vals) std::copy(p.ref_val.begin(), p.ref_val.end(), ref_vals);
    if (n_ref) *n_ref = p.ref_bins.size();
    if (role) std::copy(p.role.begin(), p.role.end(), role);
    return ORION_OK;
  });
}
int orion_dvbt_map_host(const uint8_t* bits, size_t n, size_t v, void* syms) {
  if (!dvbt_v_ok(v)) return fail(ORION_E_ARG, "dvbt: v is 2, 4 or 6");
  if (n && (!bits || !syms)) return fail(ORION_E_NULL, "null buffer");
  float* s = static_cast<float*>(syms);
  for (size_t i = 0; i < n; ++i) orion::dvbt::map_symbol(bits + i * v, v, s + 2 * i, s + 2 * i + 1);
  return ORION_OK;
}
int orion_dvbt_demap_host(const void* syms, size_t n, size_t v, uint8_t* bits) {
  if (!dvbt_v_ok(v)) return fail(ORION_E_ARG, "dvbt: v is 2, 4 or 6");
  if (n && (!bits || !syms)) return fail(ORION_E_NULL, "null buffer");
  const float* s = static_cast<const float*>(syms);
  for (size_t i = 0; i < n; ++i) orion::dvbt::demap_symbol(s[2 * i], s[2 * i + 1], v, bits + i * v);
  return ORION_OK;
}
int orion_dvbt_llr_host(const void* syms, size_t n, size_t v, float* llr) {
  if (!dvbt_v_ok(v)) return fail(ORION_E_ARG, "dvbt: v is 2, 4 or 6");
  if (n && (!llr || !syms)) return fail(ORION_E_NULL, "null buffer");
  const float* s = static_cast<const float*>(syms);
  for (size_t i = 0; i < n; ++i) orion::dvbt::soft_llr(s[2 * i], s[2 * i + 1], v, llr + i * v);
  return ORION_OK;
}
int orion_dvbt_tps_bch_encode(const uint8_t* info, uint8_t* codeword) {
  if (!info || !codeword) return fail(ORION_E_NULL, "null buffer");
  orion::dvbt::tps_bch_encode(info, codeword);
  return ORION_OK;
}
int orion_dvbt_tps_bch_decode(const uint8_t* codeword, uint8_t* info, int* ok) {
  if (!info || !codeword || !ok) return fail(ORION_E_NULL, "null buffer");
  *ok = orion::dvbt::tps_bch_decode(codeword, info) ? 1 : 0;
  return ORION_OK;
}
int orion_dvbt_tps_pack(const int32_t* fields, uint8_t* bits) {
  if (!fields || !bits) return fail(ORION_E_NULL, "null buffer");
  if (fields[0] < 0 || fields[0] > 3 || fields[1] < ORION_OFDM_QPSK || fields[1] > ORION_OFDM_QAM64 || fields[2] < 0 ||
      fields[2] > 4 || fields[3] < 0 || fields[3] > 3 || fields[4] < 0 || fields[4] > 255)
    return fail(ORION_E_ARG, "dvbt: a TPS field out of range");
  orion::dvbt::TpsWord w;
  w.frame_number = fields[0];
  w.constellation = fields[1];
  w.code_rate = fields[2];
  w.guard = fields[3];
  w.cell_id = fields[4];
  orion::dvbt::tps_pack(w, bits);
  return ORION_OK;
}
int orion_dvbt_tps_unpack(const uint8_t* bits, int32_t* fields, int* ok) {
  if (!fields || !bits || !ok) return fail(ORION_E_NULL, "null buffer");
  orion::dvbt::TpsWord w;
  *ok = orion::dvbt::tps_unpack(bits, &w) ? 1 : 0;
  const int32_t f[5] = {w.frame_number, w.constellation, w.code_rate, w.guard, w.cell_id};
  for (int i = 0; i < 5; ++i) fields[i] = *ok ? f[i] : 0;
  return ORION_OK;
}
int orion_dvbt_tps_encode_host(const uint8_t* bits, size_t n_symbols, void* cells) {
  if (!bits || (n_symbols && !cells)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    const orion::dvbt::Tables& t = orion::dvbt::tables();
    std::vector<float> signs(n_symbols);
    orion::dvbt::tps_symbol_signs(bits, n_symbols, signs.data());
    float* c = static_cast<float*>(cells);
    for (size_t l = 0; l < n_symbols; ++l)
      for (size_t j = 0; j < orion::dvbt::kTps; ++j) {
        c[2 * (l * orion::dvbt::kTps + j)] = signs[l] * t.tps_sign[j];
        c[2 * (l * orion::dvbt::kTps + j) + 1] = 0.0f;
      }
    return ORION_OK;
  });
}
int orion_dvbt_tps_decide_host(const void* cells, size_t n_symbols, uint8_t* bits, size_t* n_bits) {
  if (!bits || !n_bits || (n_symbols && !cells)) return fail(ORION_E_NULL, "null buffer");
  *n_bits = orion::dvbt::tps_decide(static_cast<const float*>(cells), n_symbols, bits);
  return ORION_OK;
}
int orion_dvbt_gi_sync_host(const void* iq, size_t n, size_t n_fft, size_t cp_len, float fs, size_t search_len, float rho,
                            size_t max_symbols, float origin_score_ratio, int64_t* start, float* out, int* found,
                            float* metric) {
  if (!start || !out || !found || (n && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt::GiConfig cfg;
    cfg.rho = rho;
    cfg.max_symbols = max_symbols;
    cfg.origin_score_ratio = origin_score_ratio;
    orion::dvbt::GiResult r;
    *found = orion::dvbt::gi_sync(static_cast<const float*>(iq), n, n_fft, cp_len, fs, search_len, cfg, &r, metric) ? 1 : 0;
    *start = *found ? static_cast<int64_t>(r.start) : 0;
    const float o[5] = {r.cfo_hz, r.score, r.gamma_re, r.gamma_im, r.phi};
    for (int i = 0; i < 5; ++i) out[i] = *found ? o[i] : 0.0f;
    return ORION_OK;
  });
}
int orion_dvbt_integer_cfo_host(const void* freq, size_t n_freq, size_t n_fft, int max_bins, int32_t* bins,
                                float* confidence, int* found) {
  if (!bins || !found || (n_freq && !freq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    *bins = 0;
    *found = orion::dvbt::integer_cfo(static_cast<const float*>(freq), n_freq, n_fft, max_bins, bins, confidence) ? 1 : 0;
    return ORION_OK;
  });
}
int orion_dvbt_mod_symbols_host(const uint8_t* bits, size_t n_bits, size_t v, size_t cp_len, const uint8_t* tps,
                                size_t n_symbols, size_t roll_off, void* iq) {
  if (!tps || (n_bits && !bits) || (n_symbols && !iq)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt::mod_symbols(bits, n_bits, v, cp_len, tps, n_symbols, roll_off, static_cast<float*>(iq));
    return ORION_OK;
  });
}
int orion_dvbt_demod_symbols_host(const void* iq, size_t n_symbols, size_t cp_len, size_t backoff, size_t v, float* llr,
                                  void* cells, void* syms) {
  if (n_symbols && (!iq || !llr || !cells)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt::demod_symbols(static_cast<const float*>(iq), n_symbols, cp_len, backoff, v, llr, static_cast<float*>(cells),
                               static_cast<float*>(syms));
    return ORION_OK;
  });
}
int orion_dvbt_mod_symbols_device(const uint8_t* bits, size_t frames, size_t row_bits, const int32_t* nbits,
                                  const uint32_t* tps, size_t v, size_t cp_len, size_t n_symbols, size_t roll_off,
                                  void* iq, void* stream) {
  if (frames && n_symbols && (!tps || !iq || (row_bits && !bits))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt_mod_symbols(bits, frames, row_bits, nbits, tps, v, cp_len, n_symbols, roll_off, iq,
                            static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_dvbt_gi_sync_batch_device(const void* iq, size_t ncap, size_t n, size_t n_fft, size_t cp_len, float fs,
                                    size_t search_len, float rho, size_t max_symbols, float origin_score_ratio,
                                    const orion_dvbt_gi_out* out, void* stream) {
  if (!out || (ncap && n && !iq)) return fail(ORION_E_NULL, "null buffer");
  const void* const* f = reinterpret_cast<const void* const*>(out);
  for (size_t k = 0; k < sizeof(orion_dvbt_gi_out) / sizeof(void*); ++k)
    if (ncap && !f[k]) return fail(ORION_E_NULL, "null output");
  return guarded([&] {
    orion::GiOut o;
    std::memcpy(&o, out, sizeof(o));
    orion::dvbt::GiConfig cfg;
    cfg.rho = rho;
    cfg.max_symbols = max_symbols;
    cfg.origin_score_ratio = origin_score_ratio;
    orion::dvbt_gi_sync_batch(iq, ncap, n, n_fft, cp_len, fs, search_len, cfg, o, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_dvbt_demod_symbols_device(const void* iq, size_t ncap, size_t n, const int32_t* start, const int32_t* found,
                                    size_t n_symbols, size_t cp_len, size_t backoff, size_t v, float* llr, void* cells,
                                    void* syms, void* stream) {
  if (ncap && n_symbols && (!iq || !start || !found || !llr || !cells)) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt_demod_symbols(iq, ncap, n, start, found, n_symbols, cp_len, backoff, v, llr, cells, syms,
                              static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}
int orion_dvbt_tps_decode_device(const void* cells, size_t frames, size_t n_symbols, int32_t* fields, int32_t* status,
                                 void* stream) {
  if (frames && (!fields || !status || (n_symbols && !cells))) return fail(ORION_E_NULL, "null buffer");
  return guarded([&] {
    orion::dvbt_tps_decode(cells, frames, n_symbols, fields, status, static_cast<hipStream_t>(stream));
    return ORION_OK;
  });
}

}  // extern "C"
