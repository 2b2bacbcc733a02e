// k_fec.hip — the inner code on the device: the batched soft-input Viterbi decode of the
// punctured, zero-tail-terminated rate 1/2 convolutional code (fec/conv.rs:304-398,
// viterbi_decode_soft_with; K = 5 and DVB-T's K = 7), and the batched encoder
// (conv.rs:234-263) with the block interleaver of the frame chain on either side.
//
// The Viterbi decode. One lane per trellis state: K = 7 has 64 states, one stream per wave64
// workgroup; K = 5 has 16, four streams per wave. State ns is reached from the two states
// (ns << 1) & mask and that + 1 with input bit ns >> (K - 2) (next_state, conv.rs:150-152), so
// a step is two lane shuffles of the path metric, the four correlations of the step's LLR
// pair (uniform over the stream), a per-lane constant choice of the correlation of each of
// the lane's two branches, and the compare-select. The LLRs are fetched cooperatively: a
// group is W / 2 steps (W lanes per stream), lane i of the stream loads mother position
// 2 t0 + i of the group, one group ahead of the metric chain (the addresses do not depend
// on it), and a step broadcasts its pair with two more shuffles. That fetch fuses the
// depuncturing and the deinterleaving: the punctured index of a mother position is full
// periods times kept-per-period plus a prefix count inside the period; a deleted position,
// and an index at or past the coded length or n_llr, reads as 0.0; the index goes through
// the inverse block permutation in[b R C + c R + r] where its block lies wholly inside
// n_llr, and is itself in a short last chunk (deinterleave_llrs, demodulate/ofdm_frame.rs).
// Each step leaves two ballots per stream in the scratch array (fec.hpp viterbi_work_bytes):
// the higher predecessor won, and a predecessor was taken at all. Lane 0 of the stream then
// runs the traceback from state 0 over those words, reading eight ahead of the chain of states.
//
// Bit-exactness with the host decoder (fec.cpp) and the reference: the start metric is
// f32::MIN / 2 with state 0 at 0; a predecessor whose metric is <= that value is skipped;
// the candidate is pm + corr, one rounding, with corr one of l0 + l1, l0 - l1, -l0 + l1,
// -l0 - l1 (-ffp-contract=off); the reference visits states ascending and replaces a
// survivor on strict > only, which for one next state is: the lower predecessor first, against
// f32::MIN / 2, then the higher one against the result; a survivor entry that nobody wrote
// reads as state 0, as the reference's zeroed table does (what NaN input, or metrics at
// -inf, lead to: the comparisons are the reference's own, so such input gives the host's
// bits too). Every loop is bounded by n_steps.
#include <algorithm>

#include "code_dev.hpp"
#include "fec_blocks.hpp"

namespace orion {

namespace {
constexpr int kTraceAhead = 8;  // survivor words fetched ahead of the traceback's chain of states

// what a launch's streams share; every field is wave-uniform
struct FecGeom {
  uint32_t n_steps, info_bits, n_llr;
  uint32_t coded_len;  // punctured_coded_len
  uint32_t lim;        // decode: min(coded_len, n_llr); encode: the output length of a stream
  uint32_t period, kept, keep;
  uint32_t rows, cols, block;  // block = rows * cols, 0: no interleaver
  uint32_t g0, g1;
};

__device__ __forceinline__ uint32_t fec_parity(uint32_t x) { return static_cast<uint32_t>(__popc(x)) & 1u; }

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
                                                     uint8_t* __restrict__ bits, void* __restrict__ work_v) {
  constexpr int W = 1 << RB;   // states: lanes per stream
  constexpr int SPW = 64 / W;  // streams per wave
  constexpr int H = W / 2;     // steps per fetch group
  const float kNegInf = -3.4028234663852886e38f / 2.0f;  // f32::MIN / 2, conv.rs:343
  const int lane = threadIdx.x;
  const int st = lane & (W - 1), gshift = lane & (64 - W);
  const long long nsr = (nstreams + SPW - 1) / SPW * SPW;
  const long long stream = static_cast<long long>(blockIdx.x) * SPW + (lane >> RB);
  const bool live = stream < nstreams;
  // a group past the last stream runs the last stream's arithmetic (the shuffles and ballots
  // are wave-wide) and stores nothing
  const float* L = llr + (live ? stream : nstreams - 1) * static_cast<long long>(g.n_llr);
  uint32_t* work32 = static_cast<uint32_t*>(work_v);
  uint64_t* work64 = static_cast<uint64_t*>(work_v);

  // this state's two predecessors and the coded pair (c0 << 1 | c1) of their branches
  const int p0 = (st << 1) & (W - 1);
  const uint32_t inbit = static_cast<uint32_t>(st) >> (RB - 1);
  const uint32_t w0 = inbit << RB | static_cast<uint32_t>(p0);
  const uint32_t sym0 = fec_parity(w0 & g.g0) << 1 | fec_parity(w0 & g.g1);
  const uint32_t sym1 = fec_parity((w0 + 1u) & g.g0) << 1 | fec_parity((w0 + 1u) & g.g1);

  // this lane's mother position in the group, as (full periods, column, generator); a group on, the
  // step count grows by H
  const uint32_t j = static_cast<uint32_t>(st) & 1u;
  uint32_t full = (static_cast<uint32_t>(st) >> 1) / g.period;
  uint32_t col = (static_cast<uint32_t>(st) >> 1) - full * g.period;
  const uint32_t dfull = static_cast<uint32_t>(H) / g.period, dcol = static_cast<uint32_t>(H) - dfull * g.period;

  float pm = st == 0 ? 0.0f : kNegInf;
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
        const float pm0 = __shfl(pm, p0, W), pm1 = __shfl(pm, p0 + 1, W);
        float v = kNegInf;
        bool taken = false, upper = false;
        if (!(pm0 <= kNegInf)) {
          const float cand = pm0 + ca;
          if (cand > v) {
            v = cand;
            taken = true;
          }
        }
        if (!(pm1 <= kNegInf)) {
          const float cand = pm1 + cb;
          if (cand > v) {
            v = cand;
            taken = true;
            upper = true;
          }
        }
        pm = v;
        const uint64_t mu = __ballot(upper), mt = __ballot(taken);
        if (live && st == 0) {
          const long long at = static_cast<long long>(t0 + k) * nsr + stream;
          if constexpr (RB == 4) {
            work32[at] = static_cast<uint32_t>((mu >> gshift) & 0xFFFFu) |
                         static_cast<uint32_t>((mt >> gshift) & 0xFFFFu) << 16;
          } else {
            work64[2 * at] = mu;
            work64[2 * at + 1] = mt;
          }
        }
      }
    }
    cur = nxt;
  }
  if (!live || st != 0) return;

  // conv.rs:385-397: from state 0; the same lane wrote these words, so its own program
  // order suffices
  uint8_t* B = bits + stream * static_cast<long long>(g.info_bits);
  uint32_t state = 0;
  for (long long t1 = g.n_steps; t1 > 0; t1 -= kTraceAhead) {
    uint64_t wu[kTraceAhead], wt[kTraceAhead];
#pragma unroll
    for (int k = 0; k < kTraceAhead; ++k) {
      const long long t = t1 - 1 - k;
      wu[k] = 0;
      wt[k] = 0;
      if (t >= 0) {
        const long long at = t * nsr + stream;
        if constexpr (RB == 4) {
          const uint32_t w = work32[at];
          wu[k] = w & 0xFFFFu;
          wt[k] = w >> 16;
        } else {
          wu[k] = work64[2 * at];
          wt[k] = work64[2 * at + 1];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kTraceAhead; ++k) {
      const long long t = t1 - 1 - k;
      if (t >= 0) {
        if (t < static_cast<long long>(g.info_bits)) B[t] = static_cast<uint8_t>(state >> (RB - 1) & 1u);
        state = (wt[k] >> state) & 1u ? ((state << 1) & (W - 1)) | static_cast<uint32_t>((wu[k] >> state) & 1u) : 0u;
      }
    }
  }
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
    v = static_cast<uint8_t>(fec_parity(window & (pos & 1u ? g.g1 : g.g0)));
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
