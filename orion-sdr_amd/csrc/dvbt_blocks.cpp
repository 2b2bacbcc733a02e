// dvbt_blocks.cpp — the DVB-T device entries' host glue (dvbt_blocks.hpp): the tables built
// from dvbt.cpp once per device, argument checks and the launches of k_dvbt.hip.
#include "dvbt_blocks.hpp"

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "ofdm.hpp"

namespace orion {

namespace {
struct DvbtTables {
  DevTable tw, role, data_bins, ref_bins, ref_val, bracket, tps_bins, tps_sign, gf_exp, gf_log;
  DvbtDev d{};
};
void init_tables(DvbtTables& t, int) {
  const dvbt::Tables& h = dvbt::tables();
  std::vector<int32_t> role;
  std::vector<uint32_t> dbin, rbin(dvbt::kPhases * kDvbtRefMax, 0u);
  std::vector<float> rval(dvbt::kPhases * kDvbtRefMax, 1.0f);
  std::vector<uint16_t> br;
  for (size_t p = 0; p < dvbt::kPhases; ++p) {
    const dvbt::Phase& ph = h.phase[p];
    role.insert(role.end(), ph.role.begin(), ph.role.end());
    dbin.insert(dbin.end(), ph.data_bins.begin(), ph.data_bins.end());
    std::copy(ph.ref_bins.begin(), ph.ref_bins.end(), rbin.begin() + p * kDvbtRefMax);
    std::copy(ph.ref_val.begin(), ph.ref_val.end(), rval.begin() + p * kDvbtRefMax);
    for (size_t c = 0; c < dvbt::kData; ++c) {
      br.push_back(ph.br_lo[c]);
      br.push_back(ph.br_hi[c]);
    }
    t.d.n_ref[p] = static_cast<int>(ph.ref_bins.size());
  }
  std::vector<uint8_t> gexp(254), glog(128, 0);
  uint32_t x = 1;
  for (size_t i = 0; i < 127; ++i) {  // GF(2^7), x^7 + x^3 + 1
    gexp[i] = gexp[i + 127] = static_cast<uint8_t>(x);
    glog[x] = static_cast<uint8_t>(i);
    x <<= 1;
    if (x & 0x80) x ^= 0x89;
  }
  t.tw.set(ofdm::fft_twiddles(dvbt::kNFft), nullptr);
  t.role.set(role, nullptr);
  t.data_bins.set(dbin, nullptr);
  t.ref_bins.set(rbin, nullptr);
  t.ref_val.set(rval, nullptr);
  t.bracket.set(br, nullptr);
  t.tps_bins.set(h.tps_bins.data(), sizeof(h.tps_bins), nullptr);
  t.tps_sign.set(h.tps_sign.data(), sizeof(h.tps_sign), nullptr);
  t.gf_exp.set(gexp, nullptr);
  t.gf_log.set(glog, nullptr);
  t.d.tw = t.tw.as<f2>();
  t.d.role = t.role.as<int32_t>();
  t.d.data_bins = t.data_bins.as<uint32_t>();
  t.d.ref_bins = t.ref_bins.as<uint32_t>();
  t.d.ref_val = t.ref_val.as<float>();
  t.d.bracket = t.bracket.as<uint16_t>();
  t.d.tps_bins = t.tps_bins.as<uint32_t>();
  t.d.tps_sign = t.tps_sign.as<float>();
  t.d.gf_exp = t.gf_exp.as<uint8_t>();
  t.d.gf_log = t.gf_log.as<uint8_t>();
}

struct RampTable {
  DevTable t;
  int len = 0;
};
void init_ramp(RampTable& r, int key) {
  const size_t cp = static_cast<size_t>(key) >> 12, roll = static_cast<size_t>(key) & 0xfff;
  const std::vector<float> ramp = ofdm::window_ramp(dvbt::kNFft + cp, roll);
  r.len = static_cast<int>(ramp.size());
  r.t.set(ramp, nullptr);
}

float check_v(size_t v) {
  if (v != 2 && v != 4 && v != 6) throw std::invalid_argument("dvbt: bits per carrier is 2, 4 or 6");
  return ofdm::axis_scale(v);
}
void check_cp(size_t cp) {
  if (cp != 64 && cp != 128 && cp != 256 && cp != 512) throw std::invalid_argument("dvbt: cp_len is 64, 128, 256 or 512");
}
int as_int(size_t v, const char* what) {
  if (v > 0x7fffffffu) throw std::invalid_argument(std::string("dvbt: ") + what + " does not fit one launch");
  return static_cast<int>(v);
}
}  // namespace

const DvbtDev& dvbt_dev(hipStream_t) { return per_device<DvbtTables>(0, init_tables).d; }

const float* dvbt_ramp(size_t cp, size_t roll_off, int* len, hipStream_t) {
  *len = 0;
  if (roll_off == 0) return nullptr;
  if (roll_off > 0xfff) throw std::invalid_argument("dvbt: roll_off above 4095");
  RampTable& r = per_device<RampTable>(static_cast<int>((cp << 12) | roll_off), init_ramp);
  *len = r.len;
  return r.t.as<float>();
}

void dvbt_mod_symbols(const uint8_t* bits, size_t frames, size_t row_bits, const int32_t* nbits, const uint32_t* tps,
                      size_t v, size_t cp, size_t n_symbols, size_t roll_off, void* iq, hipStream_t s) {
  const float scale = check_v(v);
  check_cp(cp);
  if (frames == 0 || n_symbols == 0) return;
  if (frames > 65535) throw std::invalid_argument("dvbt: at most 65535 frames in one call");
  as_int(row_bits, "a row of coded bits");
  int roll = 0;
  const float* ramp = dvbt_ramp(cp, roll_off, &roll, s);
  launch_dvbt_mod(bits, static_cast<long long>(row_bits), nbits, tps, static_cast<int>(frames), as_int(n_symbols, "n_symbols"),
                  static_cast<int>(v), scale, static_cast<int>(cp), roll, ramp, static_cast<f2*>(iq), dvbt_dev(s), s);
}

void dvbt_gi_sync_batch(const void* iq, size_t ncap, size_t n, size_t n_fft, size_t cp, float fs, size_t search_len,
                        const dvbt::GiConfig& cfg, const GiOut& out, hipStream_t s) {
  if (ncap == 0) return;
  if (ncap > 65535) throw std::invalid_argument("dvbt: at most 65535 captures in one call");
  if (n > 0x7fffffffu || n_fft > (1u << 24) || cp > (1u << 24) || search_len > 0x7fffffffu)
    throw std::invalid_argument("dvbt: a capture of at most 2^31 - 1 samples");
  const float ratio = cfg.origin_score_ratio > 0.0f ? std::min(std::max(cfg.origin_score_ratio, 0.0f), 1.0f) : -1.0f;
  launch_gi_sync(static_cast<const f2*>(iq), static_cast<int>(ncap), static_cast<long long>(n), static_cast<int>(n_fft),
                 static_cast<int>(cp), fs, static_cast<int>(search_len),
                 static_cast<int>(std::min<size_t>(std::max<size_t>(cfg.max_symbols, 1), 1u << 20)), cfg.rho, ratio, out, s);
}

void dvbt_demod_symbols(const void* iq, size_t ncap, size_t n, const int32_t* start, const int32_t* found, size_t n_symbols,
                        size_t cp, size_t backoff, size_t v, float* llr, void* cells, void* syms, hipStream_t s) {
  const float scale = check_v(v);
  check_cp(cp);
  if (ncap == 0 || n_symbols == 0) return;
  if (ncap > 65535) throw std::invalid_argument("dvbt: at most 65535 captures in one call");
  if (n > 0x7fffffffu) throw std::invalid_argument("dvbt: a capture of at most 2^31 - 1 samples");
  launch_dvbt_demod(static_cast<const f2*>(iq), static_cast<int>(ncap), static_cast<long long>(n), start, found,
                    as_int(n_symbols, "n_symbols"), static_cast<int>(cp), static_cast<int>(cp - std::min(backoff, cp)),
                    static_cast<int>(v), scale, llr, static_cast<f2*>(cells), static_cast<f2*>(syms), dvbt_dev(s), s);
}

void dvbt_tps_decode(const void* cells, size_t frames, size_t n_symbols, int32_t* fields, int32_t* status, hipStream_t s) {
  if (frames == 0) return;
  launch_tps_decode(static_cast<const f2*>(cells), as_int(frames, "frames"), as_int(n_symbols, "n_symbols"), fields, status,
                    dvbt_dev(s), s);
}

}  // namespace orion
