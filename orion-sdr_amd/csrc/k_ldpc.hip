// k_ldpc.hip — batched LDPC(174,91) belief-propagation decode + CRC-14 of FT8 / FT4
// candidates (codec/ldpc.rs:673-757, codec/ft8.rs:91-130, codec/ft4.rs:91-127).
//
// One wave64 workgroup per codeword. The reference's m[check][bit] / e[check][bit] arrays
// are touched at the 522 edges of the Tanner graph only, so a codeword's whole state is
// its 174 LLRs (in registers), 522 values t = fast_tanh(-m / 2) and 522 check -> bit
// messages e (4.2 KB of LDS). Lanes run over edges in the check update (9 edges per lane) and over bits in the
// variable updates (3 bits per lane); each lane keeps the descriptors of its edges, bits
// and checks in registers. The hard decision of the 174 bits is three ballots, the
// syndrome two ballots over the 83 checks, so the early exit and the errors == 0 break
// are uniform and every barrier is reached by all lanes.
//
// Bit-exactness with the host decoder (ldpc.cpp) and the reference: the product over a
// check's other entries runs left to right in table order, the sums in ascending check
// order, every * and + is its own rounding (-ffp-contract=off, no FMA here), / is the
// IEEE divide, and the comparisons are the reference's own (NaN and +-inf behave as on
// the host).
#include "code_dev.hpp"
#include "kernels.hpp"
#include "ldpc.hpp"

namespace orion {

namespace {
__device__ const ldpc::Packed kTab = ldpc::make_packed();

// The hard decisions of a codeword: bit i is bit (i & 63) of w[i >> 6]; wave-uniform.
struct Word {
  uint64_t w[3];
};
__device__ __forceinline__ uint32_t word_bit(const Word& h, uint32_t i) {
  const uint64_t w = i < 64 ? h.w[0] : (i < 128 ? h.w[1] : h.w[2]);
  return static_cast<uint32_t>(w >> (i & 63)) & 1u;
}

// ldpc.rs:625-637: unsatisfied checks; lanes over checks (ck: checks lane and lane + 64).
__device__ __forceinline__ int syndrome(const uint64_t ck[2], const Word& h) {
  int errors = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int nr = static_cast<int>(ck[c] >> 56);  // 0 for a lane without a check
    uint32_t x = 0;
#pragma unroll
    for (int ii = 0; ii < 7; ++ii)
      if (ii < nr) x ^= word_bit(h, static_cast<uint32_t>(ck[c] >> (8 * ii)) & 255u);
    errors += __popcll(__ballot(x != 0));
  }
  return errors;
}

// crc.rs:37-54 over the first num_bits bits of message.
__device__ __forceinline__ uint32_t crc14(const uint8_t* message, int num_bits) {
  uint32_t rem = 0;
  int idx_byte = 0;
  for (int idx_bit = 0; idx_bit < num_bits; ++idx_bit) {
    if (idx_bit % 8 == 0) rem ^= static_cast<uint32_t>(message[idx_byte++]) << 6;
    rem = (rem & 0x2000u) ? ((rem << 1) ^ ldpc::kCrcPoly) : (rem << 1);
    rem &= 0xFFFFu;
  }
  return rem & 0x3FFFu;
}
}  // namespace

// llr [n][174]; res [n] records of 16 bytes; plain [n][174] u8 or null. count (optional):
// codeword w is candidate w % max_cand of channel w / max_cand, and slots at or past
// count[channel] give an all-zero record (and plain) without being decoded.
__global__ __launch_bounds__(64) void k_ldpc_decode(const float* __restrict__ llr, const uint32_t* __restrict__ count,
                                                    int max_cand, int ft4, int rule, int max_iter,
                                                    uint32_t* __restrict__ res, uint8_t* __restrict__ plain) {
  __shared__ float s_t[ldpc::kEdges + 6];  // a check's 7th slot is never read past its entries; padded anyway
  __shared__ float s_e[ldpc::kEdges];
  const int lane = threadIdx.x;
  const long long w = blockIdx.x;
  uint32_t* R = res + w * 4;
  uint8_t* P = plain ? plain + w * ldpc::kN : nullptr;

  if (count && static_cast<uint32_t>(w % max_cand) >= count[w / max_cand]) {
    if (lane < 4) R[lane] = 0u;
    if (P)
      for (int i = lane; i < ldpc::kN; i += 64) P[i] = 0;
    return;
  }

  // this lane's edges, bits and checks
  uint32_t ed[9], bt[3];
  uint64_t ck[2];
  float lv[3];
#pragma unroll
  for (int p = 0; p < 9; ++p) ed[p] = lane + 64 * p < ldpc::kEdges ? kTab.edge[lane + 64 * p] : 0u;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int i = lane + 64 * q;
    bt[q] = i < ldpc::kN ? kTab.bit[i] : 0u;
    lv[q] = i < ldpc::kN ? llr[w * ldpc::kN + i] : 1.0f;  // a lane without a bit votes 0
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) ck[c] = lane + 64 * c < ldpc::kM ? kTab.check[lane + 64 * c] : 0ull;

  // ldpc.rs:679-685: the initial decision, returned at once when it is valid
  Word best;
#pragma unroll
  for (int q = 0; q < 3; ++q) best.w[q] = __ballot(lv[q] <= 0.0f);
  int min_errors = syndrome(ck, best);
  int iterations = 0;

  if (min_errors != 0 && max_iter > 0) {
    // ldpc.rs:692-694: m starts as the LLRs
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (lane + 64 * q < ldpc::kN) {
        const float t = fast_tanh(-lv[q] / 2.0f);
        s_t[bt[q] & 1023u] = t;
        s_t[(bt[q] >> 10) & 1023u] = t;
        s_t[(bt[q] >> 20) & 1023u] = t;
      }
    }
    for (int iter = 0; iter < max_iter; ++iter) {
      ++iterations;
      __syncthreads();
      // check update, ldpc.rs:703-718: e = -2 atanh(prod of the other entries' tanh(-m / 2))
#pragma unroll
      for (int p = 0; p < 9; ++p) {
        const int k = lane + 64 * p;
        if (k < ldpc::kEdges) {
          const int rs = ed[p] & 1023u, pos = (ed[p] >> 10) & 7u, nr = (ed[p] >> 13) & 7u;
          float a = 1.0f;
#pragma unroll
          for (int ii = 0; ii < 7; ++ii)
            if (ii < nr && ii != pos) a *= s_t[rs + ii];
          const float factor = (rule == ldpc::kRuleSumProduct && nr == 7) ? 2.0f : -2.0f;
          s_e[k] = factor * fast_atanh(a);
        }
      }
      __syncthreads();
      // variable decision, ldpc.rs:721-727, and the three bit -> check sums, ldpc.rs:740-751
      Word cur;
      float m0[3], m1[3], m2[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        bool one = false;
        m0[q] = m1[q] = m2[q] = 0.0f;
        if (lane + 64 * q < ldpc::kN) {
          const float e0 = s_e[bt[q] & 1023u], e1 = s_e[(bt[q] >> 10) & 1023u], e2 = s_e[(bt[q] >> 20) & 1023u];
          float l = lv[q];
          l += e0;
          l += e1;
          l += e2;
          one = l <= 0.0f;
          m0[q] = (lv[q] + e1) + e2;
          m1[q] = (lv[q] + e0) + e2;
          m2[q] = (lv[q] + e0) + e1;
        }
        cur.w[q] = __ballot(one);
      }
      const int errors = syndrome(ck, cur);
      if (errors < min_errors) {
        min_errors = errors;
        best = cur;
        if (errors == 0) break;
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (lane + 64 * q < ldpc::kN) {
          s_t[bt[q] & 1023u] = fast_tanh(-m0[q] / 2.0f);
          s_t[(bt[q] >> 10) & 1023u] = fast_tanh(-m1[q] / 2.0f);
          s_t[(bt[q] >> 20) & 1023u] = fast_tanh(-m2[q] / 2.0f);
        }
      }
    }
  }

  if (P)
    for (int i = lane; i < ldpc::kN; i += 64) P[i] = static_cast<uint8_t>(word_bit(best, i));

  // ft8.rs:98-129 / ft4.rs:98-127: a91, the CRC over the zeroed 82 bits, the payload
  uint32_t status = ldpc::kParityFailed;
  uint8_t pay[12] = {};
  if (min_errors == 0) {
    uint8_t a91[ldpc::kKBytes];
    for (int b = 0; b < ldpc::kKBytes; ++b) {
      uint32_t v = 0;
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * b + j;
        v = v << 1 | (i < ldpc::kK ? word_bit(best, i) : 0u);
      }
      a91[b] = static_cast<uint8_t>(v);
    }
    const uint32_t extracted = (a91[9] & 0x07u) << 11 | static_cast<uint32_t>(a91[10]) << 3 | a91[11] >> 5;
    uint8_t buf[ldpc::kKBytes];
    for (int b = 0; b < ldpc::kKBytes; ++b) buf[b] = a91[b];
    buf[9] &= 0xF8;
    buf[10] = 0;
    buf[11] = 0;
    if (extracted == crc14(buf, 82)) {
      status = ldpc::kDecoded;
      for (int b = 0; b < 10; ++b) pay[b] = ft4 ? a91[b] ^ ldpc::kFt4Xor[b] : a91[b];
      pay[9] &= 0xF8;
    } else {
      status = ldpc::kCrcMismatch;
    }
  }
  if (lane == 0) {
    R[0] = pay[0] | pay[1] << 8 | pay[2] << 16 | static_cast<uint32_t>(pay[3]) << 24;
    R[1] = pay[4] | pay[5] << 8 | pay[6] << 16 | static_cast<uint32_t>(pay[7]) << 24;
    R[2] = pay[8] | pay[9] << 8 | status << 16 | static_cast<uint32_t>(iterations) << 24;
    R[3] = static_cast<uint32_t>(min_errors);
  }
}

void launch_ldpc_decode(const float* llr_dev, long long n, const uint32_t* count_dev, int max_cand, bool ft4, int rule,
                        int max_iter, void* res_dev, uint8_t* plain_dev, hipStream_t s) {
  if (n < 1) return;
  if (n > 0x7fffffffLL) throw std::invalid_argument("ldpc decode: more than 2^31 - 1 codewords");
  k_ldpc_decode<<<static_cast<unsigned>(n), 64, 0, s>>>(llr_dev, count_dev, max_cand < 1 ? 1 : max_cand, ft4 ? 1 : 0, rule,
                                                        max_iter, static_cast<uint32_t*>(res_dev), plain_dev);
  ORION_LAUNCH_CHECK();
}

// One lane per channel: the first candidate whose record says decoded (ft8.rs:302-320
// stops there), its carrier base_hz + freq_bin * spacing (two roundings) and its score.
__global__ __launch_bounds__(64) void k_decode_pick(const SyncCandidate* __restrict__ cand,
                                                    const uint32_t* __restrict__ count, const uint32_t* __restrict__ res,
                                                    int nch, int max_cand, float base_hz, float spacing,
                                                    DecodePick* __restrict__ pick) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= nch) return;
  const uint32_t n = count[ch] < static_cast<uint32_t>(max_cand) ? count[ch] : static_cast<uint32_t>(max_cand);
  DecodePick p = {-1, 0.0f, 0.0f, 0u};
  for (uint32_t c = 0; c < n; ++c) {
    const long long slot = static_cast<long long>(ch) * max_cand + c;
    if (((res[slot * 4 + 2] >> 16) & 255u) == static_cast<uint32_t>(ldpc::kDecoded)) {
      p.first_ok = static_cast<int32_t>(c);
      p.carrier_hz = base_hz + static_cast<float>(cand[slot].freq_bin) * spacing;
      p.snr_db = cand[slot].score;
      break;
    }
  }
  pick[ch] = p;
}

void launch_decode_pick(const SyncCandidate* cand_dev, const uint32_t* count_dev, const void* res_dev, int nch,
                        int max_cand, float base_hz, float spacing, DecodePick* pick_dev, hipStream_t s) {
  if (nch < 1) return;
  k_decode_pick<<<div_up(nch, 64), 64, 0, s>>>(cand_dev, count_dev, static_cast<const uint32_t*>(res_dev), nch, max_cand,
                                               base_hz, spacing, pick_dev);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
