// dvbt_blocks.hpp — the DVB-T 2K frame on the device over k_dvbt.hip (host side): the fused
// per-symbol modulator and demodulator, the guard-interval acquisition and the TPS decoder,
// each batched over frames or captures, stateless across launches. The scalar code they are
// held to is dvbt.hpp. Device pointers throughout, asynchronous on the caller's stream.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blocks.hpp"
#include "dvbt.hpp"
#include "hip_common.hpp"

namespace orion {

constexpr int kDvbtThreads = 256;  // lanes of one (frame, symbol) workgroup: T = 256 share a 2048-point symbol
constexpr int kGiThreads = 256;    // candidate offsets of one k_gi_metric workgroup
constexpr int kDvbtRefMax = static_cast<int>(dvbt::kMaxRefPilots);

// What the kernels read (device pointers); one copy per device, uploaded by the first call.
struct DvbtDev {
  const f2* tw;               // [1024] ofdm::fft_twiddles(2048)
  const int32_t* role;        // [4][2048] dvbt::Phase::role
  const uint32_t* data_bins;  // [4][1512]
  const uint32_t* ref_bins;   // [4][kDvbtRefMax] sorted by bin
  const float* ref_val;       // [4][kDvbtRefMax]
  const uint16_t* bracket;    // [4][1512][2] the reference pilots interpolate_at picks per data index
  const uint32_t* tps_bins;   // [17]
  const float* tps_sign;      // [17]
  const uint8_t* gf_exp;      // [254] GF(2^7)
  const uint8_t* gf_log;      // [128]
  int n_ref[4];
};
const DvbtDev& dvbt_dev(hipStream_t s);
// SymbolWindow's ramp for (2048 + cp, roll_off) on this device; null for roll_off == 0.
const float* dvbt_ramp(size_t cp, size_t roll_off, int* len, hipStream_t s);

// Per-capture outputs of the acquisition (device pointers, [ncap] each) and the per-offset sums
// ([ncap][search_len]) that k_gi_select reads back.
struct GiOut {
  int32_t* start;
  int32_t* found;
  float* score;
  float* cfo_hz;
  f2* gamma;
  float* phi;
  float* metric;
  f2* gamma_all;
  float* phi_all;
};

// k_dvbt_mod: bits [frames][row_bits] u8 (nbits [frames] int32, or null: every row holds
// row_bits), tps [frames][3] u32 (bit l of the 68-bit word is s_l) -> iq [frames][n_symbols (2048 + cp)].
void dvbt_mod_symbols(const uint8_t* bits, size_t frames, size_t row_bits, const int32_t* nbits, const uint32_t* tps,
                      size_t v, size_t cp, size_t n_symbols, size_t roll_off, void* iq, hipStream_t s);
// k_gi_metric + k_gi_select: iq [ncap][n].
void dvbt_gi_sync_batch(const void* iq, size_t ncap, size_t n, size_t n_fft, size_t cp, float fs, size_t search_len,
                        const dvbt::GiConfig& cfg, const GiOut& out, hipStream_t s);
// k_dvbt_demod: iq [ncap][n] from start[c] (skipped, outputs untouched, unless found[c] and the
// frame fits) -> llr [ncap][n_symbols][1512 v], cells [ncap][n_symbols][17], syms (may be null)
// [ncap][n_symbols][1512].
void dvbt_demod_symbols(const void* iq, size_t ncap, size_t n, const int32_t* start, const int32_t* found, size_t n_symbols,
                        size_t cp, size_t backoff, size_t v, float* llr, void* cells, void* syms, hipStream_t s);
// k_tps_decode: cells [frames][n_symbols][17] -> fields [frames][5] int32 (frame_number,
// constellation, code_rate, guard, cell_id) and status [frames] (0 decoded, 1 not).
void dvbt_tps_decode(const void* cells, size_t frames, size_t n_symbols, int32_t* fields, int32_t* status, hipStream_t s);

// k_dvbt.hip
void launch_dvbt_mod(const uint8_t* bits, long long row_bits, const int32_t* nbits, const uint32_t* tps, int frames,
                     int n_symbols, int v, float scale, int cp, int roll, const float* ramp, f2* iq, const DvbtDev& d,
                     hipStream_t s);
void launch_gi_sync(const f2* iq, int ncap, long long n, int n_fft, int cp, float fs, int search_len, int max_syms,
                    float rho, float ratio, const GiOut& out, hipStream_t s);
void launch_dvbt_demod(const f2* iq, int ncap, long long n, const int32_t* start, const int32_t* found, int n_symbols,
                       int cp, int win, int v, float scale, float* llr, f2* cells, f2* syms, const DvbtDev& d,
                       hipStream_t s);
void launch_tps_decode(const f2* cells, int frames, int n_symbols, int32_t* fields, int32_t* status, const DvbtDev& d,
                       hipStream_t s);

}  // namespace orion
