// sync_blocks.cpp — host side of the FT8 / FT4 sync front end (sync_blocks.hpp).
#include "sync_blocks.hpp"

#include <cmath>
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "ldpc.hpp"

namespace orion {

namespace {
// modulate/ft8.rs:9-18, sync/ft8_sync.rs:44-45; modulate/ft4.rs:9-24, sync/ft4_sync.rs:44-47
struct Mode {
  float spacing;
  int sps, tones, total;
  CostasPattern pat;
};
const Mode kFt8 = {6.25f, 1920, 8, 79,
                   {3, 7, 8, {0, 36, 72, 0}, {{3, 1, 4, 0, 6, 5, 2}, {3, 1, 4, 0, 6, 5, 2}, {3, 1, 4, 0, 6, 5, 2}, {}}}};
const Mode kFt4 = {20.833334f, 576, 4, 105,
                   {4, 4, 4, {1, 34, 67, 100}, {{0, 1, 3, 2}, {1, 0, 2, 3}, {2, 3, 1, 0}, {3, 2, 0, 1}}}};
const Mode& mode_of(int pattern) {
  if (pattern == kCostasFt8) return kFt8;
  if (pattern == kCostasFt4) return kFt4;
  throw std::invalid_argument("unknown Costas pattern (ORION_COSTAS_FT8 / ORION_COSTAS_FT4)");
}
// Grid limits of the kernels (k_sync.hip): symbol-row groups and channels ride grid
// dimensions y / z, cell indices are 32-bit.
constexpr size_t kMaxSyms = 65535, kMaxTones = 1u << 20, kMaxCh = 65535, kMaxCand = 1u << 16;
void check_grid(size_t nch, size_t num_syms, size_t num_tones) {
  if (nch < 1 || nch > kMaxCh) throw std::invalid_argument("sync: 1 <= nch <= 65535");
  if (num_syms > kMaxSyms || num_tones > kMaxTones) throw std::invalid_argument("sync: num_syms <= 65535, num_tones <= 2^20");
  if (nch * num_syms * num_tones > 0x7fffffffull) throw std::invalid_argument("sync: waterfall above 2^31 - 1 cells");
}
// What a search is sized from; the host entries check it before any device call.
void check_slots(size_t nch, size_t max_cand) {
  // costas.rs:159: the reference reads heap[0] of an empty Vec when max_candidates == 0
  if (max_cand == 0) throw std::invalid_argument("max_cand == 0");
  if (max_cand > kMaxCand) throw std::invalid_argument("max_cand above 65536");
  if (nch < 1 || nch > kMaxCh) throw std::invalid_argument("sync: 1 <= nch <= 65535");
}
}  // namespace

std::vector<float> waterfall_steps(float fs, float base_hz, float tone_spacing_hz, size_t num_tones) {
  constexpr float kTau = 6.28318530717958647692f;
  std::vector<float> w(2 * num_tones);
  for (size_t k = 0; k < num_tones; ++k) {
    const float f = base_hz + static_cast<float>(k) * tone_spacing_hz;
    const float phi = -kTau * f / fs;
    w[2 * k] = std::cos(phi);
    w[2 * k + 1] = std::sin(phi);
  }
  return w;
}

SyncGeometry sync_geometry(int pattern, float base_hz, float max_hz, int t_min, int t_max) {
  const Mode& m = mode_of(pattern);
  const float d = max_hz - base_hz;
  const float freq_range = d > 0.0f ? d : 0.0f;  // f32::max(0.0): a NaN gives 0
  const float bins = std::ceil(freq_range / m.spacing);
  if (!(bins < static_cast<float>(kMaxTones))) throw std::invalid_argument("sync: frequency range above 2^20 bins");
  const long long syms = static_cast<long long>(t_max) + m.total - t_min;
  if (syms > static_cast<long long>(kMaxSyms)) throw std::invalid_argument("sync: more than 65535 waterfall rows");
  SyncGeometry g;
  g.num_bins = static_cast<size_t>(bins) + m.tones + 1;
  g.wf_syms = static_cast<size_t>(syms > 1 ? syms : 1);
  g.wf_sample_start = t_min >= 0 ? static_cast<size_t>(t_min) * m.sps : 0;
  g.sym_offset_adj = t_min < 0 ? -t_min : 0;
  const int over = static_cast<int>(g.wf_syms) - m.total;
  g.wf_t_max = over > 0 ? over : 0;
  return g;
}

void Sync::set_rows_per_lane(int s) {
  if (s != 0 && s != 1 && s != 2 && s != 4 && s != 8) throw std::invalid_argument("rows per lane: 0 (auto), 1, 2, 4 or 8");
  rows_ = s;
}

// Measured (tools/sync_bench.py): sharing the phasor chain among rows pays
// only once the launch still has about 32 waves per SIMD; below that one row per lane,
// which spreads a call over the most waves, is fastest. 8 rows per lane never won.
int Sync::rows_for(size_t num_syms, size_t num_tones, size_t nch) const {
  if (rows_) return rows_;
  const long long want = 32LL * 4 * device_cus();
  for (int s = 4; s > 1; s /= 2)
    if (static_cast<long long>((num_tones + 63) / 64) * ((num_syms + s - 1) / s) * nch >= want) return s;
  return 1;
}

void Sync::waterfall(const void* iq, float fs, float base_hz, float tone_spacing_hz, size_t samples_per_sym,
                     size_t num_syms, size_t num_tones, size_t time_offset, size_t nch, size_t n_per_ch, int mode,
                     float* mag, hipStream_t s) {
  if (mode != kWfLog && mode != kWfEnergy) throw std::invalid_argument("waterfall mode: ORION_WF_LOG / ORION_WF_ENERGY");
  check_grid(nch, num_syms, num_tones);
  if (samples_per_sym > 0x7fffffffu) throw std::invalid_argument("waterfall: samples_per_sym above 2^31 - 1");
  if (n_per_ch > (1ull << 40) || time_offset > (1ull << 40)) throw std::invalid_argument("waterfall: length above 2^40");
  if (num_syms == 0 || num_tones == 0) return;
  if (num_tones != st_tones_ || fs != st_fs_ || base_hz != st_base_ || tone_spacing_hz != st_spacing_ ||
      steps_.empty()) {
    steps_.set(waterfall_steps(fs, base_hz, tone_spacing_hz, num_tones), s);
    st_tones_ = num_tones;
    st_fs_ = fs;
    st_base_ = base_hz;
    st_spacing_ = tone_spacing_hz;
  }
  launch_waterfall(static_cast<const f2*>(iq), steps_.as<f2>(), mag, static_cast<int>(nch),
                   static_cast<long long>(n_per_ch), static_cast<int>(samples_per_sym), static_cast<int>(num_syms),
                   static_cast<int>(num_tones), static_cast<long long>(time_offset), mode,
                   rows_for(num_syms, num_tones, nch), s);
}

void Sync::find_candidates(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern, int t_min,
                           int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, hipStream_t s) {
  const Mode& m = mode_of(pattern);
  check_slots(nch, max_cand);
  check_grid(nch, num_syms, num_tones);
  size_t cells = 0;
  if (num_tones > static_cast<size_t>(m.tones) && t_max >= t_min) {
    const unsigned long long nt = static_cast<unsigned long long>(static_cast<long long>(t_max) - t_min + 1);
    const unsigned long long per = nt * (num_tones - m.tones + 1);
    if (per > 0x7fffffffull || per * nch > (1ull << 33)) throw std::invalid_argument("costas search: too many cells");
    cells = static_cast<size_t>(per) * nch;
  }
  score_.resize(cells * sizeof(float));
  launch_costas_search(wf, score_.as<float>(), static_cast<int>(nch), static_cast<int>(num_syms),
                       static_cast<int>(num_tones), m.pat, t_min, t_max, static_cast<int>(max_cand), cand, count, s);
}

void sync_llr(const float* wf, size_t nch, size_t num_syms, size_t num_tones, int pattern, const SyncCandidate* cand,
              const uint32_t* count, size_t max_cand, float* llr, hipStream_t s) {
  mode_of(pattern);
  if (max_cand == 0 || max_cand > kMaxCand) throw std::invalid_argument("1 <= max_cand <= 65536");
  check_grid(nch, num_syms, num_tones);
  launch_sync_llr(wf, static_cast<int>(nch), static_cast<int>(num_syms), static_cast<int>(num_tones),
                  pattern == kCostasFt4, cand, count, static_cast<int>(max_cand), llr, nullptr, 0, s);
}

void Sync::sync(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                int t_min, int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, float* llr,
                hipStream_t s) {
  const Mode& m = mode_of(pattern);
  if (max_cand == 0) throw std::invalid_argument("max_cand == 0");
  const SyncGeometry g = sync_geometry(pattern, base_hz, max_hz, t_min, t_max);
  check_grid(nch, g.wf_syms, g.num_bins);
  wf_.resize(nch * g.wf_syms * g.num_bins * sizeof(float));
  waterfall(iq, fs, base_hz, m.spacing, m.sps, g.wf_syms, g.num_bins, g.wf_sample_start, nch, n_per_ch, kWfLog,
            wf_.as<float>(), s);
  // ft8_sync.rs:130-143: the search runs over waterfall rows 0 ..= wf_t_max
  find_candidates(wf_.as<float>(), nch, g.wf_syms, g.num_bins, pattern, 0, g.wf_t_max, max_cand, cand, count, s);
  launch_sync_llr(wf_.as<float>(), static_cast<int>(nch), static_cast<int>(g.wf_syms), static_cast<int>(g.num_bins),
                  pattern == kCostasFt4, cand, count, static_cast<int>(max_cand), llr, cand, g.sym_offset_adj, s);
}

void ldpc_decode(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                 size_t max_iter, void* results, uint8_t* plain, hipStream_t s) {
  ldpc::check_args(protocol, rule, max_iter);
  if (n > 0x7fffffffull) throw std::invalid_argument("ldpc decode: more than 2^31 - 1 codewords");
  if (count && (max_cand == 0 || max_cand > kMaxCand || n % max_cand != 0))
    throw std::invalid_argument("ldpc decode: with count, n = nch * max_cand and 1 <= max_cand <= 65536");
  if (reinterpret_cast<uintptr_t>(results) % 4) throw std::invalid_argument("ldpc decode: results not 4-byte aligned");
  launch_ldpc_decode(llr, static_cast<long long>(n), count, static_cast<int>(count ? max_cand : 1),
                     protocol == ldpc::kFt4, rule, static_cast<int>(max_iter), results, plain, s);
}

void ldpc_decode_host(const float* llr, size_t n, const uint32_t* count, size_t max_cand, int protocol, int rule,
                      size_t max_iter, void* results, uint8_t* plain) {
  ldpc::check_args(protocol, rule, max_iter);
  if (count && (max_cand == 0 || n % max_cand != 0))
    throw std::invalid_argument("ldpc decode: with count, n = nch * max_cand and max_cand >= 1");
  if (n == 0) return;
  const size_t lb = n * ldpc::kN * sizeof(float), rb = n * sizeof(ldpc::Result), pb = plain ? n * ldpc::kN : 0;
  const size_t nb = count ? n / max_cand * sizeof(uint32_t) : 0;
  StagedIn d_llr(llr, lb, 0), d_count(count, nb);
  DevBuf d_res(rb), d_plain(pb + 16);
  ldpc_decode(d_llr.as<float>(), n, d_count.opt<uint32_t>(), max_cand, protocol, rule, max_iter, d_res.as<void>(),
              plain ? d_plain.as<uint8_t>() : nullptr, nullptr);
  stage_out(results, d_res, rb);
  stage_out(plain, d_plain, pb);
  ORION_HIP(hipDeviceSynchronize());
}

void Sync::decode(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                  int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, SyncCandidate* cand, uint32_t* count,
                  float* llr, void* results, DecodePick* pick, hipStream_t s) {
  const Mode& m = mode_of(pattern);
  ldpc::check_args(pattern, rule, max_iter);
  sync(pattern, iq, nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, cand, count, llr, s);
  ldpc_decode(llr, nch * max_cand, count, max_cand, pattern, rule, max_iter, results, nullptr, s);
  launch_decode_pick(cand, count, results, static_cast<int>(nch), static_cast<int>(max_cand), base_hz, m.spacing, pick,
                     s);
}

void Sync::decode_host(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                       int t_min, int t_max, size_t max_cand, int rule, size_t max_iter, SyncCandidate* cand,
                       uint32_t* count, float* llr, void* results, DecodePick* pick) {
  check_slots(nch, max_cand);
  ldpc::check_args(pattern, rule, max_iter);
  const size_t lb = nch * max_cand * kSyncLlr * sizeof(float);
  const size_t cb = nch * max_cand * sizeof(SyncCandidate), nb = nch * sizeof(uint32_t);
  const size_t rb = nch * max_cand * sizeof(ldpc::Result), kb = nch * sizeof(DecodePick);
  const size_t n_off = cand_count_offset(nch, max_cand), k_off = (rb + 15) / 16 * 16;  // pick sits behind results
  stage_in(h_iq_, iq, nch * n_per_ch * 8);
  h_cand_.resize(n_off + nb + 16);
  h_out_.resize(lb + 16);
  h_res_.resize(k_off + kb + 16);
  decode(pattern, h_iq_.as<void>(), nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter,
         h_cand_.as<SyncCandidate>(), reinterpret_cast<uint32_t*>(h_cand_.as<char>() + n_off), h_out_.as<float>(),
         h_res_.as<void>(), reinterpret_cast<DecodePick*>(h_res_.as<char>() + k_off), nullptr);
  stage_out(cand, h_cand_, cb);
  stage_out(count, h_cand_, nb, n_off);
  stage_out(llr, h_out_, lb);
  stage_out(results, h_res_, rb);
  stage_out(pick, h_res_, kb, k_off);
  ORION_HIP(hipDeviceSynchronize());
}

// ---- FT8 / FT4 modulators, slot synthesis and hard demodulators --------------------------
namespace {
void check_synth(int protocol, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch, size_t n) {
  ftmod::check_signals(protocol, signals, tones, nsig, nch);
  if (n > (1ull << 36)) throw std::invalid_argument("synth: more than 2^36 samples per channel");
}
}  // namespace

FtSynth::~FtSynth() {
  if (done_) (void)hipEventDestroy(done_);
  if (pin_) (void)hipHostFree(pin_);
}

void FtSynth::run(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                  size_t n, bool accumulate, void* iq, const f2* rot, hipStream_t s) {
  check_synth(protocol, signals, tones, nsig, nch, n);
  if (nch == 0 || n == 0) return;
  const size_t rb = nsig * sizeof(ftmod::SynthRecord), bytes = rb + (nch + 1) * sizeof(uint32_t);
  // the previous launch's copy out of the pinned plan and its reads of the device plan
  if (!done_) ORION_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
  else ORION_HIP(hipEventSynchronize(done_));
  if (bytes > pin_n_) {
    if (pin_) ORION_HIP(hipHostFree(pin_));
    pin_ = nullptr;
    pin_n_ = 0;
    ORION_HIP(hipHostMalloc(&pin_, bytes + bytes / 2, hipHostMallocDefault));
    pin_n_ = bytes + bytes / 2;
  }
  tab_.resize(bytes);
  char* h = static_cast<char*>(pin_);
  ftmod::synth_plan_into(protocol, fs, signals, tones, nsig, nch, reinterpret_cast<ftmod::SynthRecord*>(h),
                         reinterpret_cast<uint32_t*>(h + rb));
  ORION_HIP(hipMemcpyAsync(tab_.as<void>(), pin_, bytes, hipMemcpyHostToDevice, s));
  launch_ft_synth(protocol == ftmod::kFt4, tab_.as<FtSynthRecord>(), reinterpret_cast<const uint32_t*>(tab_.as<char>() + rb),
                  static_cast<f2*>(iq), static_cast<int>(nch), static_cast<long long>(n), accumulate, rot, s);
  ORION_HIP(hipEventRecord(done_, s));
}

FtMod::FtMod(int protocol, float fs, float base_hz, float rf_hz, float gain)
    : protocol_(protocol), fs_(fs), base_hz_(base_hz), rf_hz_(rf_hz), gain_(gain) {
  ftmod::proto(protocol);  // throws for an unknown protocol
}

void FtMod::modulate(const uint8_t* tones, size_t nframes, void* iq_dev, hipStream_t s) {
  if (nframes > 0x7fffffffull) throw std::invalid_argument("modulate: more than 2^31 - 1 frames");
  sig_.resize(nframes);
  for (size_t f = 0; f < nframes; ++f) sig_[f] = ftmod::Signal{static_cast<uint32_t>(f), 0u, 0, base_hz_, gain_};
  if (rf_hz_ != 0.0f && rot_.empty()) {  // the first device call: construction touches no device
    std::vector<float> p(2 * frame_len());
    ftmod::rotator_table(rf_hz_, fs_, frame_len(), p.data());
    rot_.set(p, s);
  }
  synth_.run(protocol_, fs_, sig_.data(), tones, nframes, nframes, frame_len(), false, iq_dev,
             rf_hz_ != 0.0f ? rot_.as<f2>() : nullptr, s);
}

void FtMod::modulate_host(const uint8_t* tones, size_t nframes, void* iq) {
  const size_t ob = nframes * frame_len() * 8;
  h_out_.resize(ob + 16);
  modulate(tones, nframes, h_out_.as<void>(), nullptr);
  stage_out(iq, h_out_, ob);
  ORION_HIP(hipDeviceSynchronize());
}

namespace {
std::mutex g_synth_mu;
}  // namespace

void ft_synth(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
              size_t n, bool accumulate, void* iq_dev, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_synth_mu);
  per_device<FtSynth>().run(protocol, fs, signals, tones, nsig, nch, n, accumulate, iq_dev, nullptr, s);
}

void ft_synth_host(int protocol, float fs, const ftmod::Signal* signals, const uint8_t* tones, size_t nsig, size_t nch,
                   size_t n, bool accumulate, void* iq) {
  check_synth(protocol, signals, tones, nsig, nch, n);  // before any device call
  const size_t ob = nch * n * 8;
  DevBuf d;
  stage_in(d, accumulate ? iq : nullptr, ob);
  ft_synth(protocol, fs, signals, tones, nsig, nch, n, accumulate, d.as<void>(), nullptr);
  stage_out(iq, d, ob);
  ORION_HIP(hipDeviceSynchronize());
}

namespace {
const ftmod::Proto& check_demod(int protocol, size_t nframes, size_t n_per_frame) {
  const ftmod::Proto& m = ftmod::proto(protocol);
  if (n_per_frame < static_cast<size_t>(m.frame_len()))
    throw std::invalid_argument("demodulate: fewer samples per frame than a frame (FT8: 151680, FT4: 60480)");
  if (nframes > kMaxCh || n_per_frame > (1ull << 40))
    throw std::invalid_argument("demodulate: nframes <= 65535, n_per_frame <= 2^40");
  return m;
}
}  // namespace

void ft_demod(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame, uint8_t* tones,
              float* energies, hipStream_t s) {
  check_demod(protocol, nframes, n_per_frame);
  float w[2 * ftmod::kMaxTones];
  ftmod::demod_steps(protocol, fs, base_hz, w);
  launch_ft_demod(protocol == ftmod::kFt4, static_cast<const f2*>(iq), static_cast<int>(nframes),
                  static_cast<long long>(n_per_frame), w, tones, energies, s);
}

void ft_demod_host(int protocol, float fs, float base_hz, const void* iq, size_t nframes, size_t n_per_frame,
                   uint8_t* tones, float* energies) {
  const ftmod::Proto& m = check_demod(protocol, nframes, n_per_frame);  // before any device call
  if (nframes == 0) return;
  const size_t ib = nframes * n_per_frame * 8, tb = nframes * m.data, eb = energies ? nframes * m.total * m.tones * 4 : 0;
  StagedIn d_iq(iq, ib, 0);
  DevBuf d_t(tb + 16), d_e(eb + 16);
  ft_demod(protocol, fs, base_hz, d_iq.as<void>(), nframes, n_per_frame, d_t.as<uint8_t>(),
           energies ? d_e.as<float>() : nullptr, nullptr);
  stage_out(tones, d_t, tb);
  stage_out(energies, d_e, eb);
  ORION_HIP(hipDeviceSynchronize());
}

void Sync::waterfall_host(const void* iq, float fs, float base_hz, float tone_spacing_hz, size_t samples_per_sym,
                          size_t num_syms, size_t num_tones, size_t time_offset, size_t nch, size_t n_per_ch,
                          int mode, float* mag) {
  check_grid(nch, num_syms, num_tones);
  const size_t ob = nch * num_syms * num_tones * sizeof(float);
  stage_in(h_iq_, iq, nch * n_per_ch * 8);
  h_out_.resize(ob + 16);
  waterfall(h_iq_.as<void>(), fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones, time_offset, nch,
            n_per_ch, mode, h_out_.as<float>(), nullptr);
  stage_out(mag, h_out_, ob);
  ORION_HIP(hipDeviceSynchronize());
}

void Sync::sync_host(int pattern, const void* iq, size_t nch, size_t n_per_ch, float fs, float base_hz, float max_hz,
                     int t_min, int t_max, size_t max_cand, SyncCandidate* cand, uint32_t* count, float* llr) {
  check_slots(nch, max_cand);
  const size_t cb = nch * max_cand * sizeof(SyncCandidate), nb = nch * sizeof(uint32_t);
  const size_t lb = nch * max_cand * kSyncLlr * sizeof(float), n_off = cand_count_offset(nch, max_cand);
  stage_in(h_iq_, iq, nch * n_per_ch * 8);
  h_cand_.resize(n_off + nb + 16);
  h_out_.resize(lb + 16);
  sync(pattern, h_iq_.as<void>(), nch, n_per_ch, fs, base_hz, max_hz, t_min, t_max, max_cand,
       h_cand_.as<SyncCandidate>(), reinterpret_cast<uint32_t*>(h_cand_.as<char>() + n_off), h_out_.as<float>(), nullptr);
  stage_out(cand, h_cand_, cb);
  stage_out(count, h_cand_, nb, n_off);
  stage_out(llr, h_out_, lb);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
