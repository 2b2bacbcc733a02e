// gf256_wave.hpp — the GF(2^8) algebra of one wave64 that holds one word of at most 256
// elements, four per lane: lane l has positions l, l + 64, l + 128, l + 192. What the
// Reed-Solomon and the BCH decoder (k_rs.hip, k_bch.hip) share; what differs between them (the
// start exponents, which elements count, what a root does) is the caller's.
//
// The exp[512] | log[256] tables (rs.hpp make_gf_tables, constexpr, the host's own) are
// __constant__ data that a workgroup copies into 192 words of its LDS. The field is exact, so
// the order of a sum does not matter. Every loop is bounded by an argument that is wave-uniform.
#pragma once
#include "hip_common.hpp"
#include "rs.hpp"

namespace orion {
namespace gf256 {

constexpr int kTableWords = 192;

static __constant__ __attribute__((aligned(16))) rs::GfTables d_tables = rs::make_gf_tables();

// The tables into s_tab[kTableWords]: exp at byte 0, log at byte 512. The caller's workgroup
// barrier follows.
__device__ __forceinline__ void load_tables(uint32_t* s_tab, uint32_t tid) {
  if (tid < kTableWords) s_tab[tid] = reinterpret_cast<const uint32_t*>(&d_tables)[tid];
}

__device__ __forceinline__ uint32_t mul(const uint8_t* ex, const uint8_t* lg, uint32_t a, uint32_t b) {
  const uint32_t v = ex[lg[a] + lg[b]];
  return a != 0 && b != 0 ? v : 0u;
}

// Position p has code degree 254 - p whatever the word's length is.
__device__ __forceinline__ uint32_t degree(uint32_t p) { return p < 255u ? 254u - p : 0u; }

// ns <= 4 NW syndromes of the word, four to a word of sw, the same in every lane: byte k % 4 of
// sw[k / 4] is the XOR over the positions p with valid[] set of exp[(start + k degree(p)) mod
// 255]. The lane steps the exponent by the degree per syndrome and never multiplies. Each word
// goes to seen(word) as it is reduced: a caller that folds the words there (their OR, the count
// of nonzero bytes) does not keep all of sw live for it.
template <int NW, class Seen>
__device__ __forceinline__ void syndromes(const uint8_t* ex, uint32_t lane, const uint32_t start[4],
                                          const bool valid[4], uint32_t ns, uint32_t (&sw)[NW], Seen&& seen) {
  uint32_t e[4], d[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    e[a] = start[a];
    d[a] = degree(lane + 64u * a);
  }
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    uint32_t word = 0;
    if (4u * w < ns) {  // uniform
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (4u * w + jj < ns) {
          uint32_t byte = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            if (valid[a]) byte ^= ex[e[a]];
            e[a] += d[a];
            if (e[a] >= 255u) e[a] -= 255u;
          }
          word |= byte << (8 * jj);
        }
      }
      word = wave_xor(word);
      seen(word);
    }
    sw[w] = word;
  }
}

// Berlekamp-Massey over the ns syndromes syn[0 .. ns - 1] (reed_solomon.rs:286-318,
// bch.rs:318-356): locator coefficient i and the auxiliary polynomial's in lane i, an entry
// past a polynomial's end is 0. The discrepancy is a wave XOR reduction of sigma_i syn[it - i],
// the x^m shift a lane shuffle, the auxiliary polynomial is rescaled by 1 / delta. Returns this
// lane's sigma_i; the degree stays <= ns <= 63.
__device__ __forceinline__ uint32_t berlekamp_massey(const uint8_t* ex, const uint8_t* lg, const uint8_t* syn,
                                                     uint32_t lane, uint32_t ns) {
  uint32_t sigma = lane == 0 ? 1u : 0u, bpoly = sigma;
  uint32_t L = 0, m = 1;
  for (uint32_t it = 0; it < ns; ++it) {
    uint32_t term = 0;
    if (lane >= 1 && lane <= L) term = mul(ex, lg, sigma, syn[it - lane]);  // L <= it
    const uint32_t delta = wave_xor(term) ^ syn[it];
    if (delta == 0) {
      ++m;
    } else {
      uint32_t sh = __shfl_up(bpoly, m, 64);
      if (lane < m) sh = 0;
      const uint32_t next = sigma ^ mul(ex, lg, delta, sh);
      if (2u * L <= it) {
        L = it + 1u - L;
        bpoly = mul(ex, lg, sigma, ex[255u - lg[delta]]);
        m = 1;
      } else {
        ++m;
      }
      sigma = next;
    }
  }
  return sigma;
}

// Chien: sigma(2^-i) = sum over d <= max_deg of exp[(log sig[d] + d (255 - i)) mod 255], sig
// the locator in LDS. Degree i < 255 is a root where this is 0.
__device__ __forceinline__ uint32_t chien(const uint8_t* ex, const uint8_t* lg, const uint8_t* sig, uint32_t i,
                                          uint32_t max_deg) {
  const uint32_t step = (255u - i % 255u) % 255u;
  uint32_t e = 0, val = 0;
  for (uint32_t d = 0; d <= max_deg; ++d) {
    const uint32_t c = sig[d];
    if (c != 0) val ^= ex[lg[c] + e];
    e += step;
    if (e >= 255u) e -= 255u;
  }
  return val;
}

}  // namespace gf256
}  // namespace orion
