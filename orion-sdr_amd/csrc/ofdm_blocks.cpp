// ofdm_blocks.cpp — FftDev and OfdmEngine (ofdm_blocks.hpp): table upload, launches, and
// the host-memory forms of the Block contract.
#include "ofdm_blocks.hpp"

#include <cmath>
#include <limits>
#include <stdexcept>

namespace orion {

namespace {
int log2_of(size_t n) {
  int b = 0;
  while ((size_t{1} << b) < n) ++b;
  return b;
}
void check_ptr8(const void* p) {
  if (reinterpret_cast<uintptr_t>(p) % 8) throw std::invalid_argument("ofdm: cf32 buffer not 8-byte aligned");
}
constexpr size_t kMaxSymbols = size_t{1} << 30;
}  // namespace

// ---- FftDev -----------------------------------------------------------------------------
void FftDev::batch(const void* in, size_t in_stride, void* out, size_t out_stride, size_t batch, hipStream_t s) {
  const size_t n = host_.n();
  if (batch == 0) return;
  if (in_stride < n || out_stride < n) throw std::invalid_argument("fft: a symbol stride below n_fft");
  if (batch > kMaxSymbols) throw std::invalid_argument("fft: more than 2^30 symbols in one call");
  check_ptr8(in);
  check_ptr8(out);
  if (tw_.empty()) tw_.set(host_.twiddles(), s);
  launch_fft(static_cast<const f2*>(in), static_cast<long long>(in_stride), static_cast<f2*>(out),
             static_cast<long long>(out_stride), static_cast<long long>(batch), static_cast<int>(n), log2_of(n),
             tw_.as<f2>(), host_.inverse(), s);
}

WorkReport FftDev::process_host(const void* in, size_t n_in, void* out, size_t out_cap) {
  const size_t n = host_.n();
  if (n_in < n || out_cap < n) return {};
  stage_in(h_in_, in, n * 8, 0);
  h_out_.resize(n * 8);
  batch(h_in_.as<void>(), n, h_out_.as<void>(), n, 1, nullptr);
  stage_out(out, h_out_, n * 8);
  ORION_HIP(hipDeviceSynchronize());
  return {n, n};
}

// ---- OfdmEngine -------------------------------------------------------------------------
OfdmEngine::OfdmEngine(const ofdm::Config& c, int eq) : mod_(c), demod_(c) {
  if (eq != ofdm::kEqNone) eq_.reset(new ofdm::Equalizer(c, eq));
}

void OfdmEngine::reset() {
  mod_.reset();
  if (osc_) osc_->reset();
}

const OfdmDev& OfdmEngine::dev(hipStream_t s) {
  const ofdm::Config& c = mod_.config();
  const ofdm::Grid& g = mod_.grid();
  const size_t n = c.plan.n_fft;
  if (!up_) {
    const ofdm::Equalizer identity(c, ofdm::kEqTrainingSymbolHold);
    const ofdm::Equalizer& e = eq_ ? *eq_ : identity;
    std::vector<int32_t> map(n, -1), emap(n, 0);
    for (size_t k = 0; k < g.data_bins.size(); ++k) map[g.data_bins[k]] = static_cast<int32_t>(k);
    for (size_t p = 0; p < g.pilot_bins.size(); ++p) map[g.pilot_bins[p]] = -2 - static_cast<int32_t>(p);
    for (uint32_t b : e.data_bins()) emap[b] = 1;
    for (size_t p = 0; p < e.pilot_bins().size(); ++p) emap[e.pilot_bins()[p]] = 2 + static_cast<int32_t>(p);
    std::vector<float> axis(16, 0.0f), thr(15, 0.0f);
    const size_t bps = ofdm::bits_per_symbol(c.constellation);
    if (bps >= 4) {
      ofdm::axis_table(bps, axis.data());
      ofdm::threshold_table(bps, thr.data());
    }
    tw_.set(mod_.ifft().twiddles(), s);
    map_.set(map, s);
    pval_.set(g.pilot_val, s);
    dbin_.set(g.data_bins, s);
    spbin_.set(e.pilot_bins(), s);
    spval_.set(e.pilot_val(), s);
    emap_.set(emap, s);
    weight_.set(e.weight(), s);
    hold_.set(e.estimate(), s);
    ramp_.set(mod_.ramp(), s);
    axis_.set(axis, s);
    thr_.set(thr, s);
    d_.n = static_cast<int>(n);
    d_.log2n = log2_of(n);
    d_.cp = static_cast<int>(c.plan.cp_len);
    d_.T = ofdm_threads_per_symbol(n);
    d_.order = c.constellation;
    d_.bps = static_cast<int>(bps);
    d_.nd = static_cast<int>(g.data_bins.size());
    d_.np = static_cast<int>(e.pilot_bins().size());
    d_.roll = static_cast<int>(mod_.ramp().size());
    d_.tw = tw_.as<f2>();
    d_.map = map_.as<int32_t>();
    d_.pilot_val = pval_.as<f2>();
    d_.data_bins = dbin_.as<uint32_t>();
    d_.spbin = spbin_.as<uint32_t>();
    d_.spval = spval_.as<f2>();
    d_.emap = emap_.as<int32_t>();
    d_.weight = weight_.as<f2>();
    d_.hold = hold_.as<f2>();
    d_.ramp = ramp_.as<float>();
    d_.axis = axis_.as<float>();
    d_.thr = thr_.as<float>();
    up_ = true;
    weight_dirty_ = false;
  }
  if (weight_dirty_ && eq_) {
    weight_.set(eq_->weight(), s);
    weight_dirty_ = false;
  }
  return d_;
}

void OfdmEngine::equalize_track(const void* raw, const void* weights, size_t frames, size_t nsym, void* syms, float* llr,
                                hipStream_t s) {
  if (frames == 0 || nsym == 0) return;
  if (frames > kMaxSymbols || nsym > (size_t{1} << 20) || frames * nsym > kMaxSymbols)
    throw std::invalid_argument("ofdm: more than 2^30 symbols in one call");
  if (nsym * num_data() >= (size_t{1} << 31)) throw std::invalid_argument("ofdm: a frame of 2^31 soft symbols or more");
  check_ptr8(raw);
  check_ptr8(weights);
  check_ptr8(syms);
  const OfdmDev& d = dev(s);
  launch_frame_eq_cpe(static_cast<const f2*>(raw), static_cast<const f2*>(weights), static_cast<long long>(frames),
                      static_cast<int>(nsym), d, static_cast<f2*>(syms), s);
  if (llr)
    launch_ofdm_llr(static_cast<const f2*>(syms), static_cast<long long>(frames * nsym * d.nd), d.order, d.axis, llr, s);
}

void OfdmEngine::estimate_channel(const float* received, size_t n) {
  if (!eq_) throw std::invalid_argument("ofdm: this handle has no equalizer");
  eq_->estimate_from_training_symbol(received, n);
  weight_dirty_ = true;
}

void OfdmEngine::set_pilot_bins(const uint32_t* bins, const float* vals, size_t n, const uint32_t* data_bins,
                                size_t n_data) {
  if (!eq_) throw std::invalid_argument("ofdm: this handle has no equalizer");
  eq_->set_pilot_bins(bins, vals, n, data_bins, n_data);
  up_ = false;
}

void OfdmEngine::modulate(const uint8_t* bits, size_t nch, size_t nsym, void* iq, hipStream_t s) {
  if (nch == 0 || nsym == 0) return;
  if (nch > kMaxSymbols || nsym > kMaxSymbols || nch * nsym > kMaxSymbols)
    throw std::invalid_argument("ofdm mod: more than 2^30 symbols in one call");
  check_ptr8(iq);
  const ofdm::Config& c = mod_.config();
  const OfdmDev& d = dev(s);
  const bool rf = c.rf_hz != 0.0f;
  launch_ofdm_mod(bits, static_cast<f2*>(iq), static_cast<long long>(nch * nsym), d, c.gain, !rf, s);
  if (rf) {
    if (!osc_) osc_.reset(new RefOsc(c.rf_hz, c.fs));
    const uint64_t per = static_cast<uint64_t>(nsym) * c.samples_per_ofdm_symbol();
    const OscDev o = osc_->dev(per, s);
    launch_ofdm_rf(static_cast<f2*>(iq), static_cast<long long>(per), static_cast<long long>(nch), osc_->count(), o,
                   c.gain, s);
    osc_->advance(per);
  }
}

void OfdmEngine::demodulate(const void* iq, size_t nch, size_t nsym, void* soft, uint8_t* bits, float* llr,
                            hipStream_t s) {
  if (nch == 0 || nsym == 0) return;
  if (nch > kMaxSymbols || nsym > kMaxSymbols || nch * nsym > kMaxSymbols)
    throw std::invalid_argument("ofdm demod: more than 2^30 symbols in one call");
  check_ptr8(iq);
  check_ptr8(soft);
  const OfdmDev& d = dev(s);
  const float g = demod_.gain();
  const bool scale = std::fabs(g - 1.0f) > std::numeric_limits<float>::epsilon();
  launch_ofdm_demod(static_cast<const f2*>(iq), static_cast<f2*>(soft), bits, llr, static_cast<long long>(nch * nsym),
                    d, static_cast<int>(demod_.window_start()), g, scale, eq_method(), s);
}

void OfdmEngine::decide(const void* soft, size_t n, uint8_t* bits, hipStream_t s) {
  if (n == 0) return;
  if (n > (size_t{1} << 40)) throw std::invalid_argument("ofdm decider: more than 2^40 symbols in one call");
  check_ptr8(soft);
  const OfdmDev& d = dev(s);
  launch_ofdm_decide(static_cast<const f2*>(soft), static_cast<long long>(n), d.order, d.thr, bits, s);
}

void OfdmEngine::soft_demod(const void* soft, size_t n, float* llr, hipStream_t s) {
  if (n == 0) return;
  if (n > (size_t{1} << 40)) throw std::invalid_argument("ofdm soft demod: more than 2^40 symbols in one call");
  check_ptr8(soft);
  const OfdmDev& d = dev(s);
  launch_ofdm_llr(static_cast<const f2*>(soft), static_cast<long long>(n), d.order, d.axis, llr, s);
}

void OfdmEngine::equalize(const void* in, size_t nsym, void* out, hipStream_t s) {
  if (!eq_) throw std::invalid_argument("ofdm: this handle has no equalizer");
  if (nsym == 0) return;
  if (nsym > kMaxSymbols) throw std::invalid_argument("ofdm equalizer: more than 2^30 symbols in one call");
  check_ptr8(in);
  check_ptr8(out);
  if (in == out) throw std::invalid_argument("ofdm equalizer: in place is not supported");
  const OfdmDev& d = dev(s);
  launch_ofdm_equalize(static_cast<const f2*>(in), static_cast<f2*>(out), static_cast<long long>(nsym), d,
                       eq_->method(), s);
}

// ---- host memory --------------------------------------------------------------------------
WorkReport OfdmEngine::mod_host(const uint8_t* bits, size_t n_bits, void* iq, size_t out_cap) {
  const size_t bps = config().bits_per_ofdm_symbol(), len = config().samples_per_ofdm_symbol();
  const size_t k = std::min(n_bits / bps, out_cap / len);
  if (k == 0) return {};
  stage_in(h_in_, bits, k * bps, 0);
  h_out_.resize(k * len * 8);
  modulate(h_in_.as<uint8_t>(), 1, k, h_out_.as<void>(), nullptr);
  stage_out(iq, h_out_, k * len * 8);
  ORION_HIP(hipDeviceSynchronize());
  return {k * bps, k * len};
}

WorkReport OfdmEngine::demod_host(const void* iq, size_t n, void* soft, size_t out_cap) {
  const size_t len = config().samples_per_ofdm_symbol(), nd = num_data();
  const size_t k = std::min(n / len, out_cap / nd);
  if (k == 0) return {};
  stage_in(h_in_, iq, k * len * 8, 0);
  h_out_.resize(k * nd * 8);
  demodulate(h_in_.as<void>(), 1, k, h_out_.as<void>(), nullptr, nullptr, nullptr);
  stage_out(soft, h_out_, k * nd * 8);
  ORION_HIP(hipDeviceSynchronize());
  return {k * len, k * nd};
}

WorkReport OfdmEngine::decide_host(const void* soft, size_t n, uint8_t* bits, size_t out_cap) {
  const size_t nd = num_data(), bps = config().bits_per_ofdm_symbol();
  const size_t k = std::min(n / nd, out_cap / bps);
  if (k == 0) return {};
  stage_in(h_in_, soft, k * nd * 8, 0);
  h_out_.resize(k * bps);
  decide(h_in_.as<void>(), k * nd, h_out_.as<uint8_t>(), nullptr);
  stage_out(bits, h_out_, k * bps);
  ORION_HIP(hipDeviceSynchronize());
  return {k * nd, k * bps};
}

WorkReport OfdmEngine::soft_demod_host(const void* soft, size_t n, float* llr, size_t out_cap) {
  const size_t nd = num_data(), bps = config().bits_per_ofdm_symbol();
  const size_t k = std::min(n / nd, out_cap / bps);
  if (k == 0) return {};
  stage_in(h_in_, soft, k * nd * 8, 0);
  h_out_.resize(k * bps * 4);
  soft_demod(h_in_.as<void>(), k * nd, h_out_.as<float>(), nullptr);
  stage_out(llr, h_out_, k * bps * 4);
  ORION_HIP(hipDeviceSynchronize());
  return {k * nd, k * bps};
}

WorkReport OfdmEngine::equalize_host(const void* in, size_t n, void* out, size_t out_cap) {
  const size_t nf = config().plan.n_fft;
  const size_t k = std::min(n / nf, out_cap / nf);
  if (k == 0) return {};
  stage_in(h_in_, in, k * nf * 8, 0);
  h_out_.resize(k * nf * 8);
  equalize(h_in_.as<void>(), k, h_out_.as<void>(), nullptr);
  stage_out(out, h_out_, k * nf * 8);
  ORION_HIP(hipDeviceSynchronize());
  return {k * nf, k * nf};
}

}  // namespace orion
