// k_ldpc_family.hip — the inner LDPC family on the device: the batched belief-propagation
// decode of fec/ldpc_codes.rs:366-540 (decode_soft_with, all three check rules) and the batched
// staircase encoder (ldpc_codes.rs:304-328), for the three constructed codes.
//
// The decode. One wave64 workgroup per codeword. A codeword's state is one f32 per edge of the
// Tanner graph in LDS (6 KB at most) and one byte per edge for the hard decision of the edge's
// bit. Every edge belongs to one check and one bit, so the one array serves both directions: the
// check phase reads a check's bit -> check messages and writes the check -> bit messages into
// the same slots, the variable phase reads a bit's up to three check -> bit messages and
// writes the new bit -> check messages back. Lanes run over checks in the check phase (M / 64 =
// 2 to 4 checks per lane, a check's edges are consecutive slots) and over bits in the variable
// phase (N / 64 = 8 or 9 bits per lane); a lane keeps its bits' LLRs and the descriptors of
// its bits and checks in registers, loaded once from the code's table (uploaded once per code
// and device by the host side below). The variable phase takes the decision and writes the new
// messages in one pass: the messages of an iteration that ends the decode are never read. The
// syndrome runs with lanes over checks on the edge bytes and the unsatisfied count is a sum of
// ballots, so the early exit is wave-uniform and every barrier is reached by all lanes. The
// LLR fetch goes through the inverse block permutation of deinterleave_llrs.
//
// Bit-exactness with the host decoder (ldpc_family.cpp) and the reference: tanh_half is taken
// once per edge, the leave-one-out product starts at 1.0 and runs in index order (a slot past
// the check's degree holds 1.0, and x * 1.0 is x), the decision sum is ((llr + e0) + e1) + e2
// and the update sum llr + ((e0 + e1) + e2), every * and + is its own rounding
// (-ffp-contract=off, no FMA here), / is the IEEE divide, and the comparisons are the
// reference's own (NaN and +-inf behave as on the host). Every loop over degrees is bounded
// by a constant of the code.
#include <algorithm>
#include <vector>

#include "code_dev.hpp"
#include "fec.hpp"
#include "ldpc_family_blocks.hpp"

namespace orion {

namespace {
// what a launch's words share; every field is wave-uniform
struct LdpcfGeom {
  uint32_t nblocks;  // codewords per stream
  uint32_t stream_len;  // decode: LLRs of a stream; encode: information bits of a stream
  uint32_t out_len;     // encode: elements of a coded stream
  uint32_t rows, cols, block;  // block = rows * cols, 0: no interleaver
  int32_t max_iter;
  float scale;
};

// The code's table, u32 words: per bit b words 2 b, 2 b + 1 = e0 | e1 << 16, e2 | degree << 16
// (the bit's edges in ascending check order); per check c word 2 N + c = first edge | degree <<
// 16; per message bit i word 2 N + M + i = its three rows, a byte each.
template <int N, int K>
struct Tab {
  static constexpr int M = N - K, kChecks = 2 * N, kRows = 2 * N + M, kWords = 2 * N + M + K;
  static constexpr int kEdges = 3 * K + 2 * M - 1;
};

// unsatisfied checks; lanes over checks, on the hard decisions the edges carry
template <int NC, int MAXDEG>
__device__ __forceinline__ int lf_syndrome(const uint32_t (&ck)[NC], const uint8_t* s_hb) {
  int unsat = 0;
#pragma unroll
  for (int r = 0; r < NC; ++r) {
    const uint32_t st = ck[r] & 0xFFFFu, deg = ck[r] >> 16;
    uint32_t x = 0;
#pragma unroll
    for (int j = 0; j < MAXDEG; ++j)
      if (j < static_cast<int>(deg)) x ^= s_hb[st + j];
    unsat += __popcll(__ballot(x & 1u));
  }
  return unsat;
}
}  // namespace

template <int N, int K, int MAXDEG, bool SP>
__global__ __launch_bounds__(64) void k_ldpcf_decode(const float* __restrict__ llr, LdpcfGeom g,
                                                     const uint32_t* __restrict__ tab, uint8_t* __restrict__ bits,
                                                     int32_t* __restrict__ unsat_out,
                                                     int32_t* __restrict__ iters_out) {
  using T = Tab<N, K>;
  constexpr int NB = N / 64, NC = T::M / 64;
  static_assert(N % 64 == 0 && T::M % 64 == 0, "whole bits and checks per lane");
  __shared__ float s_msg[T::kEdges + 1];
  __shared__ uint8_t s_hb[T::kEdges + 1];
  const uint32_t lane = threadIdx.x;
  const uint32_t w = blockIdx.x;
  const uint32_t stream = w / g.nblocks, blk = w - stream * g.nblocks;
  const float* L = llr + static_cast<uint64_t>(stream) * g.stream_len;

  // this lane's bits and checks
  uint32_t bd0[NB], bd1[NB], ck[NC];
  float lv[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const uint32_t b = lane + 64u * q;
    bd0[q] = tab[2u * b];
    bd1[q] = tab[2u * b + 1u];
    const uint32_t p = blk * N + b;
    uint32_t src = p;
    if (g.block) {  // uniform; every block is whole
      const uint32_t b0 = p / g.block * g.block;
      src = b0 + block_il_offset(p - b0, g.rows, g.cols);
    }
    lv[q] = L[src];
  }
#pragma unroll
  for (int r = 0; r < NC; ++r) ck[r] = tab[T::kChecks + lane + 64u * r];

  // the initial decision (llr <= 0) and the first messages, the LLRs themselves
  uint32_t hard = 0;
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const uint32_t e0 = bd0[q] & 0xFFFFu, e1 = bd0[q] >> 16, e2 = bd1[q] & 0xFFFFu, deg = bd1[q] >> 16;
    const uint32_t h = lv[q] <= 0.0f ? 1u : 0u;
    hard |= h << q;
    s_msg[e0] = lv[q];
    s_hb[e0] = static_cast<uint8_t>(h);
    if (deg > 1) {
      s_msg[e1] = lv[q];
      s_hb[e1] = static_cast<uint8_t>(h);
    }
    if (deg > 2) {
      s_msg[e2] = lv[q];
      s_hb[e2] = static_cast<uint8_t>(h);
    }
  }
  lds_barrier();
  int min_unsat = lf_syndrome<NC, MAXDEG>(ck, s_hb);
  uint32_t best = hard;
  int iterations = 0;

  if (min_unsat != 0) {  // uniform
    for (int it = 0; it < g.max_iter; ++it) {
      iterations = it + 1;
      // check phase: bit -> check messages become check -> bit messages in place
#pragma unroll
      for (int r = 0; r < NC; ++r) {
        const uint32_t st = ck[r] & 0xFFFFu;
        const int deg = static_cast<int>(ck[r] >> 16);
        if (SP) {
          float th[MAXDEG];
#pragma unroll
          for (int j = 0; j < MAXDEG; ++j) th[j] = j < deg ? fast_tanh(s_msg[st + j] / 2.0f) : 1.0f;
#pragma unroll
          for (int i1 = 0; i1 < MAXDEG; ++i1) {
            float prod = 1.0f;
#pragma unroll
            for (int i2 = 0; i2 < MAXDEG; ++i2)
              if (i2 != i1) prod *= th[i2];
            if (prod < -1.0f) prod = -1.0f;  // f32::clamp: NaN passes
            if (prod > 1.0f) prod = 1.0f;
            if (i1 < deg) s_msg[st + i1] = 2.0f * fast_atanh(prod);
          }
        } else {
          float v[MAXDEG];
          float min1 = __builtin_inff(), min2 = __builtin_inff(), sign_parity = 1.0f;
          int argmin = 0;
#pragma unroll
          for (int j = 0; j < MAXDEG; ++j) {
            v[j] = j < deg ? s_msg[st + j] : 0.0f;
            if (j < deg) {
              if (v[j] < 0.0f) sign_parity = -sign_parity;
              const float a = __builtin_fabsf(v[j]);
              if (a < min1) {
                min2 = min1;
                min1 = a;
                argmin = j;
              } else if (a < min2) {
                min2 = a;
              }
            }
          }
#pragma unroll
          for (int i1 = 0; i1 < MAXDEG; ++i1) {
            const float s_other = v[i1] < 0.0f ? -sign_parity : sign_parity;
            const float mag = i1 == argmin ? min2 : min1;
            if (i1 < deg) s_msg[st + i1] = (g.scale * s_other) * mag;
          }
        }
      }
      lds_barrier();

      // variable phase: the decision, and the next bit -> check messages in place
      hard = 0;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const uint32_t e0 = bd0[q] & 0xFFFFu, e1 = bd0[q] >> 16, e2 = bd1[q] & 0xFFFFu, deg = bd1[q] >> 16;
        const float x0 = s_msg[e0];
        const float x1 = deg > 1 ? s_msg[e1] : 0.0f;
        const float x2 = deg > 2 ? s_msg[e2] : 0.0f;
        float l = lv[q] + x0, sum = x0;
        if (deg > 1) {
          l += x1;
          sum += x1;
        }
        if (deg > 2) {
          l += x2;
          sum += x2;
        }
        const float total = lv[q] + sum;
        const uint32_t h = l <= 0.0f ? 1u : 0u;
        hard |= h << q;
        s_msg[e0] = total - x0;
        s_hb[e0] = static_cast<uint8_t>(h);
        if (deg > 1) {
          s_msg[e1] = total - x1;
          s_hb[e1] = static_cast<uint8_t>(h);
        }
        if (deg > 2) {
          s_msg[e2] = total - x2;
          s_hb[e2] = static_cast<uint8_t>(h);
        }
      }
      lds_barrier();
      const int unsat = lf_syndrome<NC, MAXDEG>(ck, s_hb);
      if (unsat < min_unsat) {  // uniform
        min_unsat = unsat;
        best = hard;
        if (unsat == 0) break;
      }
    }
  }

  uint8_t* B = bits + static_cast<uint64_t>(w) * K;
#pragma unroll
  for (int q = 0; q < K / 64; ++q) B[lane + 64u * q] = static_cast<uint8_t>((best >> q) & 1u);
  if (lane == 0) {
    unsat_out[w] = min_unsat;
    iters_out[w] = iterations;
  }
}

// One wave64 workgroup per codeword. Lanes over message bits copy the message and XOR bit 0
// of each into the bit's three rows of the packed row sums in LDS (M / 32 words); the
// staircase p_i = s_i ^ p_(i-1) is the inclusive prefix XOR over the M row sums: a prefix
// inside each word by shifts, then the parity of the words below by a scan over the lanes
// that hold them. A message element at or past the stream's end reads as 0; an output
// element goes through the block permutation out[c rows + r] = in[r cols + c].
template <int N, int K>
__global__ __launch_bounds__(64) void k_ldpcf_encode(const uint8_t* __restrict__ in, LdpcfGeom g,
                                                     const uint32_t* __restrict__ tab, uint8_t* __restrict__ out) {
  using T = Tab<N, K>;
  constexpr int NW = T::M / 32;
  __shared__ uint32_t s_w[NW];
  const uint32_t lane = threadIdx.x;
  const uint32_t w = blockIdx.x;
  const uint32_t stream = w / g.nblocks, blk = w - stream * g.nblocks;
  const uint8_t* I = in + static_cast<uint64_t>(stream) * g.stream_len;
  uint8_t* O = out + static_cast<uint64_t>(stream) * g.out_len;
  auto dst = [&](uint32_t p) {
    if (!g.block) return p;
    const uint32_t b0 = p / g.block * g.block;
    return b0 + block_il_offset(p - b0, g.rows, g.cols);
  };
  if (lane < NW) s_w[lane] = 0u;
  lds_barrier();
#pragma unroll
  for (int q = 0; q < K / 64; ++q) {
    const uint32_t i = lane + 64u * q, src = blk * K + i;
    const uint32_t v = src < g.stream_len ? I[src] : 0u;
    O[dst(blk * N + i)] = static_cast<uint8_t>(v);
    if (v & 1u) {
      const uint32_t rows = tab[T::kRows + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint32_t r = (rows >> (8 * j)) & 255u;
        atomicXor(&s_w[r >> 5], 1u << (r & 31u));
      }
    }
  }
  lds_barrier();
  uint32_t x = lane < NW ? s_w[lane] : 0u;
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  const uint32_t par = x >> 31;  // the parity of this lane's whole word
  uint32_t carry = 0;
#pragma unroll
  for (int d = 0; d < NW - 1; ++d) {
    const uint32_t pd = __shfl(par, d, 64);
    if (static_cast<uint32_t>(d) < lane) carry ^= pd;
  }
  if (carry) x = ~x;
  lds_barrier();
  if (lane < NW) s_w[lane] = x;
  lds_barrier();
#pragma unroll
  for (int q = 0; q < T::M / 64; ++q) {
    const uint32_t i = lane + 64u * q;
    O[dst(blk * N + K + i)] = static_cast<uint8_t>((s_w[i >> 5] >> (i & 31u)) & 1u);
  }
}

// ---- host side ---------------------------------------------------------------------------
namespace {
constexpr int kMaxDeg[ldpcf::kNumCodes] = {5, 8, 11};  // the codes' largest check degrees

std::vector<uint32_t> make_table(const ldpcf::Ldpc& c) {
  const size_t n = c.n(), m = c.m(), k = c.k();
  if (c.n_edges() != 3 * k + 2 * m - 1 || c.max_check_degree() > static_cast<size_t>(kMaxDeg[c.code()]) || m > 256)
    throw std::logic_error("ldpc family: the constructed graph does not fit the kernel's constants");
  std::vector<uint32_t> t(2 * n + m + k, 0);
  for (size_t b = 0; b < n; ++b) {
    const uint32_t j0 = c.bit_start()[b], deg = c.bit_start()[b + 1] - j0;
    if (deg < 1 || deg > 3) throw std::logic_error("ldpc family: a bit has 1 to 3 checks");
    uint32_t e[3] = {0, 0, 0};
    for (uint32_t j = 0; j < deg; ++j) e[j] = c.bit_edges()[j0 + j];
    t[2 * b] = e[0] | e[1] << 16;
    t[2 * b + 1] = e[2] | deg << 16;
    if (b < k) {
      if (deg != 3) throw std::logic_error("ldpc family: a message bit has three checks");
      t[2 * n + m + b] = c.bit_checks()[j0] | c.bit_checks()[j0 + 1] << 8 | c.bit_checks()[j0 + 2] << 16;
    }
  }
  for (size_t r = 0; r < m; ++r) t[2 * n + r] = c.check_start()[r] | (c.check_start()[r + 1] - c.check_start()[r]) << 16;
  return t;
}

// the code's table on the current device: built and uploaded on first use, then kept
struct CodeTable {
  DevTable t;
};
const uint32_t* device_table(int code) {
  return per_device<CodeTable>(code, [](CodeTable& c, int code) { c.t.set(make_table(ldpcf::Ldpc::get(code)), nullptr); })
      .t.as<uint32_t>();
}

LdpcfGeom ldpcf_geom(size_t nstreams, size_t nblocks, size_t rows, size_t cols) {
  if (nstreams > kLdpcfMaxStreams) throw std::invalid_argument("ldpc family: nstreams above 2^24");
  if (nblocks < 1 || nblocks > kLdpcfMaxBlocks)
    throw std::invalid_argument("ldpc family: 1 to 2^20 codewords per stream");
  if (nstreams * nblocks > kLdpcfMaxWords) throw std::invalid_argument("ldpc family: more than 2^30 codewords in a launch");
  if ((rows == 0) != (cols == 0))
    throw std::invalid_argument("ldpc family: interleaver rows, cols both zero (none) or both nonzero");
  if (rows) fec::BlockInterleaver check(rows, cols);  // rows * cols <= 2^24
  LdpcfGeom g{};
  g.nblocks = static_cast<uint32_t>(nblocks);
  g.rows = static_cast<uint32_t>(rows);
  g.cols = static_cast<uint32_t>(cols);
  g.block = static_cast<uint32_t>(rows * cols);
  return g;
}

template <int N, int K, int MAXDEG>
void launch_decode(bool sp, size_t total, hipStream_t s, const float* llr, const LdpcfGeom& g, const uint32_t* tab,
                   uint8_t* bits, int32_t* unsat, int32_t* iterations) {
  if (sp)
    k_ldpcf_decode<N, K, MAXDEG, true><<<static_cast<unsigned>(total), 64, 0, s>>>(llr, g, tab, bits, unsat, iterations);
  else
    k_ldpcf_decode<N, K, MAXDEG, false><<<static_cast<unsigned>(total), 64, 0, s>>>(llr, g, tab, bits, unsat, iterations);
}
}  // namespace

size_t ldpcf_decode_blocks(int code, size_t n_llr, size_t rows, size_t cols) {
  const ldpcf::Ldpc& c = ldpcf::Ldpc::get(code);
  if (n_llr > (size_t(1) << 31) - 1) throw std::invalid_argument("ldpc family decode: n_llr above 2^31 - 1");
  if (n_llr < c.n()) throw std::invalid_argument("ldpc family decode: a stream is at least one codeword of N LLRs");
  ldpcf_geom(0, 1, rows, cols);
  if (rows && n_llr % (rows * cols))
    throw std::invalid_argument("ldpc family decode: with an interleaver n_llr is whole blocks of rows * cols");
  const size_t nblocks = n_llr / c.n();
  ldpcf_geom(0, nblocks, rows, cols);
  return nblocks;
}

namespace {
// The argument checks of the device entry, which the host entry runs before any device call: the
// codewords per stream.
size_t check_decode(int code, size_t nstreams, size_t n_llr, size_t rows, size_t cols, size_t max_iter, int rule) {
  const size_t nblocks = ldpcf_decode_blocks(code, n_llr, rows, cols);
  ldpcf::check_rule(rule);
  if (max_iter > kLdpcfMaxIter) throw std::invalid_argument("ldpc family decode: max_iter above 2^30");
  ldpcf_geom(nstreams, nblocks, rows, cols);
  return nblocks;
}
}  // namespace

void ldpcf_decode_batch(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                        size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat, int32_t* iterations,
                        hipStream_t s) {
  const size_t nblocks = check_decode(code, nstreams, n_llr, rows, cols, max_iter, rule);
  LdpcfGeom g = ldpcf_geom(nstreams, nblocks, rows, cols);
  if (nstreams == 0) return;
  if (reinterpret_cast<uintptr_t>(llr) % 4 || reinterpret_cast<uintptr_t>(unsat) % 4 ||
      reinterpret_cast<uintptr_t>(iterations) % 4)
    throw std::invalid_argument("ldpc family decode: llr, unsat or iterations not 4-byte aligned");
  g.stream_len = static_cast<uint32_t>(n_llr);
  g.max_iter = static_cast<int32_t>(max_iter);
  g.scale = rule == ldpcf::kRuleScaledMinSum ? scale : 1.0f;
  const uint32_t* tab = device_table(code);
  const size_t total = nstreams * nblocks;
  const bool sp = rule == ldpcf::kRuleSumProduct;
  if (code == ldpcf::kN512R12)
    launch_decode<512, 256, kMaxDeg[0]>(sp, total, s, llr, g, tab, bits, unsat, iterations);
  else if (code == ldpcf::kN576R23)
    launch_decode<576, 384, kMaxDeg[1]>(sp, total, s, llr, g, tab, bits, unsat, iterations);
  else
    launch_decode<512, 384, kMaxDeg[2]>(sp, total, s, llr, g, tab, bits, unsat, iterations);
  ORION_LAUNCH_CHECK();
}

void ldpcf_decode_batch_host(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                             size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat,
                             int32_t* iterations) {
  const size_t nblocks = check_decode(code, nstreams, n_llr, rows, cols, max_iter, rule);
  if (nstreams == 0) return;
  const size_t lb = nstreams * n_llr * sizeof(float), bb = nstreams * nblocks * ldpcf::Ldpc::get(code).k(),
               sb = nstreams * nblocks * sizeof(int32_t);
  StagedIn d_llr(llr, lb);
  DevBuf d_bits(bb + 16), d_unsat(sb), d_iters(sb);
  ldpcf_decode_batch(code, d_llr.as<float>(), nstreams, n_llr, rows, cols, max_iter, rule, scale, d_bits.as<uint8_t>(),
                     d_unsat.as<int32_t>(), d_iters.as<int32_t>(), nullptr);
  stage_out(bits, d_bits, bb);
  stage_out(unsat, d_unsat, sb);
  stage_out(iterations, d_iters, sb);
  ORION_HIP(hipDeviceSynchronize());
}

size_t ldpcf_encoded_len(int code, size_t nbits, size_t rows, size_t cols) {
  const ldpcf::Ldpc& c = ldpcf::Ldpc::get(code);
  if (nbits < 1 || nbits > (size_t(1) << 30)) throw std::invalid_argument("ldpc family encode: 1 <= nbits <= 2^30");
  const size_t nblocks = (nbits + c.k() - 1) / c.k();
  const LdpcfGeom g = ldpcf_geom(0, nblocks, rows, cols);
  const size_t coded = nblocks * c.n();
  return g.block ? (coded + g.block - 1) / g.block * g.block : coded;
}

namespace {
// As check_decode, for an encode: its geometry.
LdpcfGeom check_encode(int code, size_t nstreams, size_t nbits, size_t rows, size_t cols) {
  const size_t out_len = ldpcf_encoded_len(code, nbits, rows, cols), k = ldpcf::Ldpc::get(code).k();
  LdpcfGeom g = ldpcf_geom(nstreams, (nbits + k - 1) / k, rows, cols);
  g.stream_len = static_cast<uint32_t>(nbits);
  g.out_len = static_cast<uint32_t>(out_len);
  return g;
}
}  // namespace

void ldpcf_encode_batch(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                        uint8_t* coded, hipStream_t s) {
  const LdpcfGeom g = check_encode(code, nstreams, nbits, rows, cols);
  if (nstreams == 0) return;
  const size_t nblocks = g.nblocks, out_len = g.out_len;
  const uint32_t* tab = device_table(code);
  // the last block's padding is written by nobody else
  if (out_len != nblocks * ldpcf::Ldpc::get(code).n()) ORION_HIP(hipMemsetAsync(coded, 0, nstreams * out_len, s));
  const unsigned total = static_cast<unsigned>(nstreams * nblocks);
  if (code == ldpcf::kN512R12)
    k_ldpcf_encode<512, 256><<<total, 64, 0, s>>>(bits, g, tab, coded);
  else if (code == ldpcf::kN576R23)
    k_ldpcf_encode<576, 384><<<total, 64, 0, s>>>(bits, g, tab, coded);
  else
    k_ldpcf_encode<512, 384><<<total, 64, 0, s>>>(bits, g, tab, coded);
  ORION_LAUNCH_CHECK();
}

void ldpcf_encode_batch_host(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                             uint8_t* coded) {
  const LdpcfGeom g = check_encode(code, nstreams, nbits, rows, cols);
  if (nstreams == 0) return;
  const size_t ib = nstreams * nbits, ob = nstreams * g.out_len;
  StagedIn d_in(bits, ib);
  DevBuf d_out(ob + 16);
  ldpcf_encode_batch(code, d_in.as<uint8_t>(), nstreams, nbits, rows, cols, d_out.as<uint8_t>(), nullptr);
  stage_out(coded, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
