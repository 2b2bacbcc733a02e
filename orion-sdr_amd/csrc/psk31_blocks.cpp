// psk31_blocks.cpp — host side of the PSK31 kernels (psk31_blocks.hpp).
#include "psk31_blocks.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace orion {

namespace {
constexpr size_t kMaxCh = 65535;  // channels ride a 32-bit record field; the limit of the sync entries
}  // namespace

// ---- the batched Viterbi decode ----
void psk31_viterbi(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits, void* work, size_t work_bytes,
                   hipStream_t s) {
  if (nstreams > 0x7fffffffull - 3 || n_syms > 0x7fffffffull)
    throw std::invalid_argument("psk31 viterbi: nstreams <= 2^31 - 4 and n_syms <= 2^31 - 1");
  if (nstreams == 0 || n_syms == 0) return;
  if (!work || work_bytes < psk31::viterbi_work_bytes(nstreams, n_syms))
    throw std::invalid_argument("psk31 viterbi: work below orion_psk31_viterbi_work_bytes(nstreams, n_syms)");
  if (reinterpret_cast<uintptr_t>(work) % 4 || reinterpret_cast<uintptr_t>(soft) % 4)
    throw std::invalid_argument("psk31 viterbi: soft / work not 4-byte aligned");
  launch_psk31_viterbi(soft, static_cast<long long>(nstreams), static_cast<long long>(n_syms), bits,
                       static_cast<uint32_t*>(work), s);
}

void psk31_viterbi_host(const float* soft, size_t nstreams, size_t n_syms, uint8_t* bits) {
  if (nstreams > 0x7fffffffull - 3 || n_syms > 0x7fffffffull)
    throw std::invalid_argument("psk31 viterbi: nstreams <= 2^31 - 4 and n_syms <= 2^31 - 1");
  if (nstreams == 0 || n_syms == 0) return;
  const size_t sb = nstreams * n_syms * 2 * sizeof(float), bb = nstreams * n_syms;
  const size_t wb = psk31::viterbi_work_bytes(nstreams, n_syms);
  StagedIn d_soft(soft, sb, 0);
  DevBuf d_bits(bb + 16), d_work(wb);
  psk31_viterbi(d_soft.as<float>(), nstreams, n_syms, d_bits.as<uint8_t>(), d_work.as<void>(), wb, nullptr);
  stage_out(bits, d_bits, bb);
  ORION_HIP(hipDeviceSynchronize());
}

// ---- the demodulator bank ----
Psk31DemodBank::Psk31DemodBank(float fs, const psk31::Stream* streams, size_t nstreams, size_t nch) : nch_(nch) {
  if (nch < 1 || nch > kMaxCh) throw std::invalid_argument("psk31 bank: 1 <= nch <= 65535");
  if (nstreams < 1 || nstreams > (1u << 24)) throw std::invalid_argument("psk31 bank: 1 <= nstreams <= 2^24");
  std::vector<size_t> order(nstreams);
  for (size_t k = 0; k < nstreams; ++k) {
    if (streams[k].channel >= nch) throw std::invalid_argument("psk31 bank: a stream's channel >= nch");
    if (streams[k].out_cap > (1u << 30)) throw std::invalid_argument("psk31 bank: out_cap above 2^30");
    order[k] = k;
  }
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return streams[a].channel != streams[b].channel ? streams[a].channel < streams[b].channel
                                                    : streams[a].start < streams[b].start;
  });
  rec_.resize(nstreams);
  st0_.resize(nstreams);
  // the window, its square sum and the initial state are the host demodulator's own (one
  // stream's constructor: they do not depend on the stream); the first count does
  const psk31::Demod proto(psk31::kBpsk, fs, 0.0f, 1.0f, 0);
  sps_ = proto.sps();
  hann_ = proto.hann();
  hann_sq_sum_ = proto.hann_sq_sum();
  for (size_t j = 0; j < nstreams; ++j) {
    const psk31::Stream& t = streams[order[j]];
    if (t.mode != static_cast<uint32_t>(psk31::kBpsk) && t.mode != static_cast<uint32_t>(psk31::kQpsk))
      throw std::invalid_argument("psk31: unknown mode (ORION_PSK31_BPSK / ORION_PSK31_QPSK)");
    psk31::BankRecord& r = rec_[j];
    r.start = t.start;
    r.mode = t.mode;
    r.channel = t.channel;
    r.slot = static_cast<uint32_t>(order[j]);
    r.out_cap = t.out_cap;
    r.rot = t.rf_hz != 0.0f ? 1u : 0u;
    r.w_re = 1.0f;
    r.w_im = 0.0f;
    if (r.rot) psk31::rotator_step(-t.rf_hz, fs, &r.w_re, &r.w_im);
    r.scale = t.gain / hann_sq_sum_;
    st0_[j] = proto.state();
    st0_[j].count = psk31::demod_start_count(sps_, t.offset);
    max_cap_ = std::max(max_cap_, static_cast<size_t>(t.out_cap));
  }
}

void Psk31DemodBank::set_gain(size_t slot, float gain) {
  for (psk31::BankRecord& r : rec_)
    if (r.slot == slot) {
      r.scale = gain / hann_sq_sum_;
      rec_dirty_ = true;
      return;
    }
  throw std::invalid_argument("psk31 bank: no such stream");
}

void Psk31DemodBank::reset() {
  base_ = 0;
  fresh_ = true;
}

void Psk31DemodBank::process(const void* iq, size_t nch, size_t n, float* soft, size_t out_stride, uint8_t* bits,
                             uint64_t* reports, hipStream_t s) {
  if (nch != nch_) throw std::invalid_argument("psk31 bank: nch is not the bank's");
  if (out_stride < max_cap_) throw std::invalid_argument("psk31 bank: out_stride below the largest out_cap");
  if (n > (1ull << 40) || out_stride > (1ull << 31))
    throw std::invalid_argument("psk31 bank: n above 2^40 or out_stride above 2^31");
  const auto misaligned = [](const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
  if (misaligned(iq, 8) || misaligned(reports, 8) || misaligned(soft, 4))
    throw std::invalid_argument("psk31 bank: iq / reports not 8-byte aligned, or soft not 4-byte aligned");
  if (fresh_) d_st_.set(st0_, s);  // after a reset this waits for the launches that carry the old states
  if (fresh_ || rec_dirty_) d_rec_.set(rec_, s);
  if (d_hann_.empty()) d_hann_.set(hann_, s);
  fresh_ = rec_dirty_ = false;
  launch_psk31_demod(static_cast<const f2*>(iq), static_cast<long long>(n), base_, d_rec_.as<psk31::BankRecord>(),
                     d_st_.as<psk31::DemodState>(), static_cast<int>(rec_.size()), d_hann_.as<float>(),
                     static_cast<uint32_t>(sps_), soft, static_cast<long long>(out_stride), bits,
                     reinterpret_cast<unsigned long long*>(reports), s);
  base_ += n;
}

void Psk31DemodBank::process_host(const void* iq, size_t nch, size_t n, float* soft, size_t out_stride, uint8_t* bits,
                                  uint64_t* reports) {
  if (nch != nch_) throw std::invalid_argument("psk31 bank: nch is not the bank's");
  if (out_stride < max_cap_) throw std::invalid_argument("psk31 bank: out_stride below the largest out_cap");
  const size_t ns = rec_.size(), ib = nch * n * 8, sb = ns * out_stride * sizeof(float), bb = bits ? ns * out_stride : 0;
  const size_t rb = ns * 2 * sizeof(uint64_t);
  stage_in(h_iq_, iq, ib);
  h_soft_.resize(sb + 16);
  h_bits_.resize(bb + 16);
  h_rep_.resize(rb);
  if (sb) ORION_HIP(hipMemset(h_soft_.as<void>(), 0, sb));
  if (bb) ORION_HIP(hipMemset(h_bits_.as<void>(), 0, bb));
  process(h_iq_.as<void>(), nch, n, h_soft_.as<float>(), out_stride, bits ? h_bits_.as<uint8_t>() : nullptr,
          h_rep_.as<uint64_t>(), nullptr);
  stage_out(soft, h_soft_, sb);
  stage_out(bits, h_bits_, bb);
  stage_out(reports, h_rep_, rb);
  ORION_HIP(hipDeviceSynchronize());
}

// ---- the modulator ----
void Psk31ModDev::run(const std::vector<float>& ph, size_t nstreams, size_t n, void* iq_dev, hipStream_t s) {
  const size_t sps = host_.sps(), per = n * sps;
  if (nstreams > 0x7fffffffull || per > (1ull << 40)) throw std::invalid_argument("psk31 mod: batch too large");
  if (reinterpret_cast<uintptr_t>(iq_dev) % 8) throw std::invalid_argument("psk31 mod: iq not 8-byte aligned");
  if (nstreams == 0 || n == 0) return;
  if (hann_.empty()) hann_.set(host_.hann().data(), sps * sizeof(float), s);
  if (host_.rf_hz() != 0.0f && rot_n_ < per) {  // a fresh Rotator per call: any call's phasors are a prefix
    std::vector<float> z(2 * per);
    psk31::rotator_table(host_.rf_hz(), host_.fs(), per, z.data());
    rot_.set(z, s);
    rot_n_ = per;
  }
  std::memcpy(ph_.begin(ph.size() * sizeof(float)), ph.data(), ph.size() * sizeof(float));
  launch_psk31_mod(reinterpret_cast<const f2*>(ph_.push(s)), hann_.as<float>(),
                   host_.rf_hz() != 0.0f ? rot_.as<f2>() : nullptr, static_cast<int>(nstreams),
                   static_cast<long long>(n), static_cast<uint32_t>(sps), host_.gain(), static_cast<f2*>(iq_dev), s);
  ph_.done(s);
}

void Psk31ModDev::modulate(const uint8_t* bits, size_t n, void* iq_dev, hipStream_t s) {
  std::vector<float> ph(2 * (n + 1));
  host_.symbol_phasors(bits, n, ph.data());
  run(ph, 1, n, iq_dev, s);
}

void Psk31ModDev::modulate_batch(const uint8_t* bits, size_t nstreams, size_t n, void* iq_dev, hipStream_t s) {
  if (nstreams > (1u << 24) || n > (1ull << 32)) throw std::invalid_argument("psk31 mod: nstreams <= 2^24, n <= 2^32");
  std::vector<float> ph(2 * (n + 1) * nstreams);
  for (size_t k = 0; k < nstreams; ++k) {
    psk31::Mod fresh(host_.mode(), host_.fs(), host_.rf_hz(), host_.gain());
    fresh.symbol_phasors(bits + k * n, n, ph.data() + 2 * (n + 1) * k);
  }
  run(ph, nstreams, n, iq_dev, s);
}

void Psk31ModDev::modulate_batch_host(const uint8_t* bits, size_t nstreams, size_t n, void* iq) {
  const size_t ob = nstreams * n * host_.sps() * 8;
  if (ob == 0) return;
  h_out_.resize(ob);
  modulate_batch(bits, nstreams, n, h_out_.as<void>(), nullptr);
  stage_out(iq, h_out_, ob);
  ORION_HIP(hipDeviceSynchronize());
}

// ---- band synthesis ----
namespace {
std::mutex g_synth_mu;
struct Psk31SynthDev {  // one per device (blocks.hpp per_device)
  PlanUpload plan;  // records | rows | phasors, each at a 16-byte offset
  DevTable hann;    // the window for hann_fs
  float hann_fs = 0.0f;
};
size_t up16(size_t b) { return (b + 15) / 16 * 16; }
}  // namespace

void psk31_synth(float fs, const psk31::Signal* signals, const uint8_t* bits, size_t nsig, size_t nch, size_t n,
                 bool accumulate, void* iq_dev, hipStream_t s) {
  if (nch < 1 || nch > kMaxCh) throw std::invalid_argument("psk31 synth: 1 <= nch <= 65535");
  if (nsig > (1u << 24) || n > (1ull << 40)) throw std::invalid_argument("psk31 synth: nsig <= 2^24, n <= 2^40");
  if (reinterpret_cast<uintptr_t>(iq_dev) % 8) throw std::invalid_argument("psk31 synth: iq not 8-byte aligned");
  const psk31::Mod proto(psk31::kBpsk, fs, 0.0f, 1.0f);  // checks fs; the window
  const size_t sps = proto.sps();
  std::vector<size_t> order(nsig), first(nsig);
  size_t total_bits = 0;
  for (size_t k = 0; k < nsig; ++k) {
    if (signals[k].channel >= nch) throw std::invalid_argument("psk31 synth: a signal's channel >= nch");
    if (signals[k].n_bits > (1ull << 32)) throw std::invalid_argument("psk31 synth: n_bits above 2^32");
    order[k] = k;
    first[k] = total_bits;
    total_bits += signals[k].n_bits;
  }
  if (total_bits > (1ull << 34)) throw std::invalid_argument("psk31 synth: more than 2^34 bits");
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return signals[a].channel < signals[b].channel; });
  std::vector<psk31::SynthRecord> rec(nsig);
  std::vector<uint32_t> rows(nch + 1, 0);
  std::vector<float> ph(2 * (total_bits + nsig));
  size_t at = 0;
  for (size_t j = 0; j < nsig; ++j) {
    const psk31::Signal& g = signals[order[j]];
    psk31::Mod fresh(static_cast<int>(g.mode), fs, g.rf_hz, g.gain);
    fresh.symbol_phasors(bits + first[order[j]], g.n_bits, ph.data() + 2 * at);
    rec[j] = {g.offset, static_cast<int64_t>(g.n_bits * sps), at, psk31::rotator_step_q64(g.rf_hz, fs), g.gain,
              g.rf_hz != 0.0f ? 1u : 0u};
    // an offset this far out never meets the channel; keep the kernel's i - offset inside int64
    if (g.offset < -(1LL << 62) || g.offset > (1LL << 62)) rec[j].len = 0;
    at += g.n_bits + 1;
    rows[g.channel + 1] += 1;
  }
  for (size_t ch = 0; ch < nch; ++ch) rows[ch + 1] += rows[ch];
  const size_t rec_b = nsig * sizeof(psk31::SynthRecord), rows_b = rows.size() * sizeof(uint32_t);
  const size_t rows_at = up16(rec_b), ph_at = rows_at + up16(rows_b);
  std::lock_guard<std::mutex> lock(g_synth_mu);
  Psk31SynthDev& d = per_device<Psk31SynthDev>();
  char* h = d.plan.begin(ph_at + ph.size() * sizeof(float));
  if (rec_b) std::memcpy(h, rec.data(), rec_b);
  std::memcpy(h + rows_at, rows.data(), rows_b);
  if (!ph.empty()) std::memcpy(h + ph_at, ph.data(), ph.size() * sizeof(float));
  if (d.hann_fs != fs || d.hann.empty()) {
    d.hann.set(proto.hann().data(), sps * sizeof(float), s);
    d.hann_fs = fs;
  }
  const char* dev = d.plan.push(s);
  launch_psk31_synth(reinterpret_cast<const psk31::SynthRecord*>(dev), reinterpret_cast<const uint32_t*>(dev + rows_at),
                     reinterpret_cast<const f2*>(dev + ph_at), d.hann.as<float>(), static_cast<uint32_t>(sps),
                     static_cast<int>(nch), static_cast<long long>(n), accumulate, static_cast<f2*>(iq_dev), s);
  d.plan.done(s);
}

void psk31_synth_host(float fs, const psk31::Signal* signals, const uint8_t* bits, size_t nsig, size_t nch, size_t n,
                      bool accumulate, void* iq) {
  const size_t ob = nch * n * 8;
  DevBuf d_out;
  stage_in(d_out, accumulate ? iq : nullptr, ob);
  psk31_synth(fs, signals, bits, nsig, nch, n, accumulate, d_out.as<void>(), nullptr);
  stage_out(iq, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

// ---- psk31_sync on the device ----
namespace {
constexpr size_t kMaxCand = 1u << 16;
void check_search(size_t nch, size_t num_syms, size_t num_bins, size_t max_cand) {
  if (max_cand == 0) throw std::invalid_argument("max_cand == 0");  // as the FT entries
  if (max_cand > kMaxCand) throw std::invalid_argument("max_cand above 65536");
  if (nch < 1 || nch > kMaxCh) throw std::invalid_argument("psk31 sync: 1 <= nch <= 65535");
  if (num_syms > 0x7fffffffull || num_bins > (1u << 24) || nch * num_syms * num_bins > 0x7fffffffull)
    throw std::invalid_argument("psk31 sync: waterfall above 2^31 - 1 cells");
  if (nch * num_bins * max_cand > (1ull << 26) || num_bins * max_cand > (1ull << 22))
    throw std::invalid_argument("psk31 sync: nch * num_bins * max_cand <= 2^26 and num_bins * max_cand <= 2^22");
}
// The stride of sync's per-slot outputs, once nch, max_cand and n_bits are in range. The host
// entry sizes its staging from it, so there it runs before any device call.
size_t check_stride(size_t slots, size_t n_bits) {
  if (slots * (n_bits + 2) > (1ull << 32))
    throw std::invalid_argument("psk31 sync: nch * max_cand * (n_bits + 2) above 2^32");
  return n_bits + 2;
}
}  // namespace

void Psk31Sync::find_carriers(const float* wf, size_t nch, size_t num_syms, size_t num_bins, size_t min_carrier_syms,
                              float peak_margin_db, size_t max_cand, SyncCandidate* cand, uint32_t* count,
                              hipStream_t s) {
  check_search(nch, num_syms, num_bins, max_cand);
  const float ln_margin = peak_margin_db * 0.693147180559945309417f / 3.0f;  // psk31_sync.rs:82
  const size_t min_run = min_carrier_syms > 1 ? min_carrier_syms : 1;
  med_.resize((nch * num_bins + 1) * sizeof(float));
  floor_.resize(nch * sizeof(float));
  runs_.resize((nch * num_bins * max_cand + 1) * sizeof(SyncCandidate));
  nruns_.resize((nch * num_bins + 1) * sizeof(uint32_t));
  head_.resize((nch * num_bins + 1) * sizeof(uint32_t));
  launch_psk31_carriers(wf, static_cast<int>(nch), static_cast<int>(num_syms), static_cast<int>(num_bins),
                        static_cast<int>(min_run > 0x7fffffffull ? 0x7fffffffull : min_run), ln_margin,
                        static_cast<int>(max_cand), med_.as<float>(), floor_.as<float>(), runs_.as<SyncCandidate>(),
                        nruns_.as<uint32_t>(), head_.as<uint32_t>(), cand, count, s);
}

void Psk31Sync::sync(Sync& eng, const void* iq, size_t nch, size_t n, float fs, float base_hz, float max_hz,
                     size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand, SyncCandidate* cand,
                     uint32_t* count, float* soft, uint64_t* reports, hipStream_t s) {
  if (n_bits > (1u << 30) - 2) throw std::invalid_argument("psk31 sync: n_bits above 2^30 - 2");
  if (reinterpret_cast<uintptr_t>(iq) % 8 || reinterpret_cast<uintptr_t>(reports) % 8)
    throw std::invalid_argument("psk31 sync: iq / reports not 8-byte aligned");
  const size_t num_bins = psk31::sync_num_bins(base_hz, max_hz);
  const size_t sps = psk31::psk31_sps(fs);
  const size_t num_syms = sps ? n / sps : 0;
  check_search(nch, num_syms, num_bins, max_cand);
  const size_t slots = nch * max_cand, stride = check_stride(slots, n_bits);
  ORION_HIP(hipMemsetAsync(soft, 0, slots * stride * sizeof(float), s));
  ORION_HIP(hipMemsetAsync(reports, 0, slots * 2 * sizeof(uint64_t), s));
  if (num_syms == 0) {  // psk31_sync.rs:60-68: no candidates
    ORION_HIP(hipMemsetAsync(cand, 0, slots * sizeof(SyncCandidate), s));
    ORION_HIP(hipMemsetAsync(count, 0, nch * sizeof(uint32_t), s));
    return;
  }
  if (fs != hann_fs_ || hann_.empty()) {
    const psk31::Demod proto(psk31::kBpsk, fs, 0.0f, 1.0f, 0);
    hann_.set(proto.hann(), s);
    hann_sq_sum_ = proto.hann_sq_sum();
    hann_fs_ = fs;
    st_bins_ = 0;
  }
  if (num_bins != st_bins_ || fs != st_fs_ || base_hz != st_base_) {
    // each bin's carrier as record_candidate computes it, and Bpsk31Demod::new's Rotator step
    std::vector<float> w(3 * num_bins);
    for (size_t b = 0; b < num_bins; ++b) {
      const float carrier = base_hz + static_cast<float>(b) * 31.25f;
      w[3 * b] = 1.0f;
      w[3 * b + 1] = 0.0f;
      w[3 * b + 2] = carrier != 0.0f ? 1.0f : 0.0f;
      if (carrier != 0.0f) psk31::rotator_step(-carrier, fs, &w[3 * b], &w[3 * b + 1]);
    }
    steps_.set(w, s);
    st_bins_ = num_bins;
    st_fs_ = fs;
    st_base_ = base_hz;
  }
  wf_.resize(nch * num_syms * num_bins * sizeof(float));
  rec_.resize(slots * sizeof(psk31::BankRecord));
  st_.resize(slots * sizeof(psk31::DemodState));
  eng.waterfall(iq, fs, base_hz, 31.25f, sps, num_syms, num_bins, 0, nch, n, kWfLog, wf_.as<float>(), s);
  find_carriers(wf_.as<float>(), nch, num_syms, num_bins, min_carrier_syms, peak_margin_db, max_cand, cand, count, s);
  launch_psk31_cand_records(cand, count, static_cast<int>(nch), static_cast<int>(max_cand), steps_.as<float>(),
                            static_cast<uint32_t>(sps), static_cast<uint32_t>(stride), 1.0f / hann_sq_sum_,
                            rec_.as<psk31::BankRecord>(), st_.as<psk31::DemodState>(), s);
  launch_psk31_demod(static_cast<const f2*>(iq), static_cast<long long>(n), 0ull, rec_.as<psk31::BankRecord>(),
                     st_.as<psk31::DemodState>(), static_cast<int>(slots), hann_.as<float>(), static_cast<uint32_t>(sps),
                     soft, static_cast<long long>(stride), nullptr, reinterpret_cast<unsigned long long*>(reports), s);
}

void Psk31Sync::find_carriers_host(const float* wf, size_t nch, size_t num_syms, size_t num_bins,
                                   size_t min_carrier_syms, float peak_margin_db, size_t max_cand, SyncCandidate* cand,
                                   uint32_t* count) {
  check_search(nch, num_syms, num_bins, max_cand);
  const size_t nb = nch * sizeof(uint32_t), n_off = cand_count_offset(nch, max_cand);
  stage_in(h_in_, wf, nch * num_syms * num_bins * sizeof(float));
  h_cand_.resize(n_off + nb + 16);
  find_carriers(h_in_.as<float>(), nch, num_syms, num_bins, min_carrier_syms, peak_margin_db, max_cand,
                h_cand_.as<SyncCandidate>(), reinterpret_cast<uint32_t*>(h_cand_.as<char>() + n_off), nullptr);
  stage_out(cand, h_cand_, nch * max_cand * sizeof(SyncCandidate));
  stage_out(count, h_cand_, nb, n_off);
  ORION_HIP(hipDeviceSynchronize());
}

void Psk31Sync::sync_host(Sync& eng, const void* iq, size_t nch, size_t n, float fs, float base_hz, float max_hz,
                          size_t min_carrier_syms, float peak_margin_db, size_t n_bits, size_t max_cand,
                          SyncCandidate* cand, uint32_t* count, float* soft, uint64_t* reports) {
  if (max_cand == 0) throw std::invalid_argument("max_cand == 0");
  if (max_cand > kMaxCand || nch < 1 || nch > kMaxCh || n_bits > (1u << 30) - 2)
    throw std::invalid_argument("psk31 sync: 1 <= nch <= 65535, max_cand <= 65536, n_bits <= 2^30 - 2");
  const size_t slots = nch * max_cand, stride = check_stride(slots, n_bits);
  const size_t sb = slots * stride * sizeof(float), rb = slots * 2 * sizeof(uint64_t);
  const size_t nb = nch * sizeof(uint32_t), n_off = cand_count_offset(nch, max_cand);
  stage_in(h_in_, iq, nch * n * 8);
  h_cand_.resize(n_off + nb + 16);
  h_soft_.resize(sb);
  h_rep_.resize(rb);
  sync(eng, h_in_.as<void>(), nch, n, fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand,
       h_cand_.as<SyncCandidate>(), reinterpret_cast<uint32_t*>(h_cand_.as<char>() + n_off), h_soft_.as<float>(),
       h_rep_.as<uint64_t>(), nullptr);
  stage_out(cand, h_cand_, slots * sizeof(SyncCandidate));
  stage_out(count, h_cand_, nb, n_off);
  stage_out(soft, h_soft_, sb);
  stage_out(reports, h_rep_, rb);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
