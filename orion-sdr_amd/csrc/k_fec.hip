// k_fec.hip — the inner code on the device: the batched soft-input Viterbi decode of the
// punctured, zero-tail-terminated rate 1/2 convolutional code (fec/conv.rs:304-398,
// viterbi_decode_soft_with; K = 5 and DVB-T's K = 7), and the batched encoder
// (conv.rs:234-263) with the block interleaver of the frame chain on either side.
//
// The Viterbi decode is trellis_wave.hpp's engine (one lane per state: K = 7 is one stream per
// wave64 workgroup, K = 5 four; the exactness argument is there), maximising. What is this
// kernel's: the branch metric is one of the four correlations l0 + l1, l0 - l1, -l0 + l1,
// -l0 - l1 of the step's LLR pair (uniform over the stream; negation is exact,
// -ffp-contract=off), a per-lane constant choice for each of the lane's two branches. The LLRs
// are fetched cooperatively: a group is W / 2 steps (W lanes per stream), lane i of the
// stream loads mother position 2 t0 + i of the group, one group ahead of the metric chain
// (the addresses do not depend on it), and a step broadcasts its pair with two shuffles.
// That fetch fuses the depuncturing and the deinterleaving: the punctured index of a mother
// position is full periods times kept-per-period plus a prefix count inside the period; a
// deleted position, and an index at or past the coded length or n_llr, reads as 0.0; the
// index goes through the inverse block permutation in[b R C + c R + r] where its block lies
// wholly inside n_llr, and is itself in a short last chunk (deinterleave_llrs,
// demodulate/ofdm_frame.rs). The traceback starts from state 0 (the zero tail) and writes
// the first info_bits bits of the n_steps <= 2^24 + 6.
#include <algorithm>

#include "code_dev.hpp"
#include "fec_blocks.hpp"
#include "trellis_wave.hpp"

namespace orion {

namespace {
// what a launch's streams share; every field is wave-uniform
struct FecGeom {
  uint32_t n_steps, info_bits, n_llr;
  uint32_t coded_len;  // punctured_coded_len
  uint32_t lim;        // decode: min(coded_len, n_llr); encode: the output length of a stream
  uint32_t period, kept, keep;
  uint32_t rows, cols, block;  // block = rows * cols, 0: no interleaver
  uint32_t g0, g1;
};

// The LLR of mother position 2 (full * period + col) + j of a stream: 0.0 unless the bit was
// kept and its punctured index lies inside lim.
__device__ __forceinline__ float fec_fetch(const float* __restrict__ L, const FecGeom& g, uint32_t full, uint32_t col,
                                           uint32_t j) {
  const uint32_t pos = 2u * col + j;
  if (!(g.keep >> pos & 1u)) return 0.0f;
  const uint32_t p = full * g.kept + static_cast<uint32_t>(__popc(g.keep & ((1u << pos) - 1u)));
  if (p >= g.lim) return 0.0f;
  uint32_t src = p;
  if (g.block) {  // uniform
    const uint32_t b0 = p / g.block * g.block;
    if (b0 + g.block <= g.n_llr) src = b0 + block_il_offset(p - b0, g.rows, g.cols);  // a full block
  }
  return L[src];
}
}  // namespace

template <int RB>
__global__ __launch_bounds__(64) void k_conv_viterbi(const float* __restrict__ llr, long long nstreams, FecGeom g,
                                                     uint8_t* __restrict__ bits, void* __restrict__ work) {
  using trellis::parity;
  constexpr int W = 1 << RB, H = W / 2;  // lanes per stream; steps per fetch group
  const trellis::Wave<RB> tw(nstreams);
  const uint32_t st = static_cast<uint32_t>(tw.st);
  const float* L = llr + tw.row * static_cast<long long>(g.n_llr);

  // the coded pair (c0 << 1 | c1) of the branches from this state's two predecessors
  const uint32_t w0 = tw.inbit << RB | static_cast<uint32_t>(tw.p0);
  const uint32_t sym0 = parity(w0 & g.g0) << 1 | parity(w0 & g.g1);
  const uint32_t sym1 = parity((w0 + 1u) & g.g0) << 1 | parity((w0 + 1u) & g.g1);

  // this lane's mother position in the group, as (full periods, column, generator); a group on, the
  // step count grows by H
  const uint32_t j = st & 1u;
  uint32_t full = (st >> 1) / g.period;
  uint32_t col = (st >> 1) - full * g.period;
  const uint32_t dfull = static_cast<uint32_t>(H) / g.period, dcol = static_cast<uint32_t>(H) - dfull * g.period;

  float pm = st == 0 ? 0.0f : trellis::Maximise::start();
  float cur = fec_fetch(L, g, full, col, j);
  for (uint32_t t0 = 0; t0 < g.n_steps; t0 += H) {
    full += dfull;
    col += dcol;
    if (col >= g.period) {
      col -= g.period;
      ++full;
    }
    // past the last step every index is at or past coded_len: no load
    const float nxt = fec_fetch(L, g, full, col, j);
#pragma unroll
    for (int k = 0; k < H; ++k) {
      if (t0 + k < g.n_steps) {  // uniform over the wave
        const float l0 = __shfl(cur, 2 * k, W), l1 = __shfl(cur, 2 * k + 1, W);
        const float n0 = -l0;
        const float c0 = l0 + l1, c1 = l0 - l1, c2 = n0 + l1, c3 = n0 - l1;  // conv.rs:363
        const float ca = sym0 & 2u ? (sym0 & 1u ? c3 : c2) : (sym0 & 1u ? c1 : c0);
        const float cb = sym1 & 2u ? (sym1 & 1u ? c3 : c2) : (sym1 & 1u ? c1 : c0);
        tw.store(work, static_cast<long long>(t0 + k), tw.template acs<trellis::Maximise>(pm, ca, cb));
      }
    }
    cur = nxt;
  }
  // conv.rs:385-397
  tw.traceback(work, g.n_steps, 0u, bits + tw.stream * static_cast<long long>(g.info_bits), g.info_bits);
}

// One thread per output bit of a stream's interleave_bits(conv_encode_punctured(info)): the
// output index goes back through the block permutation (out[c rows + r] = in[r cols + c];
// past coded_len: the padding, 0), the punctured index back to its mother position (full
// periods and the rem-th kept bit of the period), and the coded bit is the parity of the K-bit
// window of the information bits that ends at that step (zero before the start and in the tail).
template <int RB>
__global__ __launch_bounds__(256) void k_conv_encode(const uint8_t* __restrict__ info, long long nstreams, FecGeom g,
                                                     uint8_t* __restrict__ out) {
  const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= nstreams * static_cast<long long>(g.lim)) return;
  const long long stream = idx / g.lim;
  const uint32_t o = static_cast<uint32_t>(idx - stream * g.lim);
  uint32_t p = o;
  if (g.block) {
    const uint32_t b0 = o / g.block * g.block;
    p = b0 + block_il_offset(o - b0, g.cols, g.rows);  // the inverse map
  }
  uint8_t v = 0;
  if (p < g.coded_len) {
    const uint32_t full = p / g.kept, rem = p - full * g.kept;
    uint32_t m = g.keep;
    for (uint32_t i = 0; i < rem; ++i) m &= m - 1u;  // rem < kept <= 8
    const uint32_t pos = static_cast<uint32_t>(__ffs(static_cast<int>(m))) - 1u;
    const long long t = static_cast<long long>(full) * g.period + (pos >> 1);
    const uint8_t* I = info + stream * static_cast<long long>(g.info_bits);
    uint32_t window = 0;
#pragma unroll
    for (int i = 0; i <= RB; ++i) {  // window bit RB is the step's input, bit 0 the oldest register bit
      const long long ti = t - RB + i;
      if (ti >= 0 && ti < static_cast<long long>(g.info_bits)) window |= static_cast<uint32_t>(I[ti] & 1u) << i;
    }
    v = static_cast<uint8_t>(trellis::parity(window & (pos & 1u ? g.g1 : g.g0)));
  }
  out[idx] = v;
}

// ---- host side ---------------------------------------------------------------------------
namespace {
FecGeom fec_geom(int code, int rate, size_t nstreams, size_t info_bits, size_t rows, size_t cols) {
  const fec::CodeSpec c = fec::code_spec(code);
  const fec::RateSpec r = fec::rate_spec(rate);
  if (info_bits == 0 || info_bits > fec::kMaxInfoBits) throw std::invalid_argument("fec: 1 <= info_bits <= 2^24");
  if (nstreams > fec::kMaxStreams) throw std::invalid_argument("fec: nstreams above 2^24");
  if ((rows == 0) != (cols == 0)) throw std::invalid_argument("fec: interleaver rows, cols both zero (none) or both nonzero");
  if (rows) fec::BlockInterleaver check(rows, cols);  // rows * cols <= 2^24
  FecGeom g{};
  g.n_steps = static_cast<uint32_t>(info_bits) + static_cast<uint32_t>(c.reg_bits);
  g.info_bits = static_cast<uint32_t>(info_bits);
  g.coded_len = static_cast<uint32_t>(fec::punctured_coded_len(code, info_bits, rate));
  g.period = static_cast<uint32_t>(r.period);
  g.kept = static_cast<uint32_t>(r.kept);
  g.keep = r.keep;
  g.rows = static_cast<uint32_t>(rows);
  g.cols = static_cast<uint32_t>(cols);
  g.block = static_cast<uint32_t>(rows * cols);
  g.g0 = c.g0;
  g.g1 = c.g1;
  return g;
}
}  // namespace

void fec_viterbi(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits, size_t rows,
                 size_t cols, uint8_t* bits, void* work, size_t work_bytes, hipStream_t s) {
  FecGeom g = fec_geom(code, rate, nstreams, info_bits, rows, cols);
  if (n_llr > fec::kMaxLlr) throw std::invalid_argument("fec viterbi: n_llr above 2^31 - 1");
  if (nstreams == 0) return;
  const int rb = fec::code_spec(code).reg_bits;
  if (!work || work_bytes < fec::viterbi_work_bytes(rb, nstreams, info_bits))
    throw std::invalid_argument("fec viterbi: work below orion_fec_viterbi_work_bytes(code, nstreams, info_bits)");
  if (reinterpret_cast<uintptr_t>(work) % 8 || reinterpret_cast<uintptr_t>(llr) % 4)
    throw std::invalid_argument("fec viterbi: work not 8-byte aligned, or llr not 4-byte aligned");
  g.n_llr = static_cast<uint32_t>(n_llr);
  g.lim = std::min(g.coded_len, g.n_llr);
  const long long ns = static_cast<long long>(nstreams);
  if (rb == 4)
    k_conv_viterbi<4><<<static_cast<unsigned>((nstreams + 3) / 4), 64, 0, s>>>(llr, ns, g, bits, work);
  else
    k_conv_viterbi<6><<<static_cast<unsigned>(nstreams), 64, 0, s>>>(llr, ns, g, bits, work);
  ORION_LAUNCH_CHECK();
}

void fec_viterbi_host(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                      size_t rows, size_t cols, uint8_t* bits) {
  fec_geom(code, rate, nstreams, info_bits, rows, cols);
  if (n_llr > fec::kMaxLlr) throw std::invalid_argument("fec viterbi: n_llr above 2^31 - 1");
  if (nstreams == 0) return;
  const size_t lb = nstreams * n_llr * sizeof(float), bb = nstreams * info_bits;
  const size_t wb = fec::viterbi_work_bytes(fec::code_spec(code).reg_bits, nstreams, info_bits);
  StagedIn d_llr(llr, lb);
  DevBuf d_bits(bb + 16), d_work(wb);
  fec_viterbi(code, rate, d_llr.as<float>(), nstreams, n_llr, info_bits, rows, cols, d_bits.as<uint8_t>(),
              d_work.as<void>(), wb, nullptr);
  stage_out(bits, d_bits, bb);
  ORION_HIP(hipDeviceSynchronize());
}

size_t fec_encoded_len(int code, size_t info_bits, int rate, size_t rows, size_t cols) {
  const FecGeom g = fec_geom(code, rate, 0, info_bits, rows, cols);
  return g.block ? (static_cast<size_t>(g.coded_len) + g.block - 1) / g.block * g.block : g.coded_len;
}

void fec_encode_batch(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits, size_t rows,
                      size_t cols, uint8_t* coded, hipStream_t s) {
  FecGeom g = fec_geom(code, rate, nstreams, info_bits, rows, cols);
  if (nstreams == 0) return;
  const size_t out_len = fec_encoded_len(code, info_bits, rate, rows, cols);
  const size_t total = nstreams * out_len;
  if (total > (size_t(1) << 38)) throw std::invalid_argument("fec encode: more than 2^38 output bits in a launch");
  g.lim = static_cast<uint32_t>(out_len);
  const unsigned blocks = static_cast<unsigned>((total + 255) / 256);
  const long long ns = static_cast<long long>(nstreams);
  if (fec::code_spec(code).reg_bits == 4)
    k_conv_encode<4><<<blocks, 256, 0, s>>>(info, ns, g, coded);
  else
    k_conv_encode<6><<<blocks, 256, 0, s>>>(info, ns, g, coded);
  ORION_LAUNCH_CHECK();
}

void fec_encode_batch_host(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits, size_t rows,
                           size_t cols, uint8_t* coded) {
  const size_t out_len = fec_encoded_len(code, info_bits, rate, rows, cols);
  if (nstreams > fec::kMaxStreams) throw std::invalid_argument("fec: nstreams above 2^24");
  if (nstreams == 0) return;
  const size_t ib = nstreams * info_bits, ob = nstreams * out_len;
  StagedIn d_info(info, ib);
  DevBuf d_out(ob + 16);
  fec_encode_batch(code, rate, d_info.as<uint8_t>(), nstreams, info_bits, rows, cols, d_out.as<uint8_t>(), nullptr);
  stage_out(coded, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
