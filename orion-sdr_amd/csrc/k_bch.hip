// k_bch.hip — the outer BCH code on the device: the batched decode of fec/bch.rs:131-207
// (syndromes, Berlekamp-Massey, Chien, the residual check) and the batched LFSR encoder
// (bch.rs:105-125), for the code of any t <= 31 shortened to any n.
//
// The decode. One wave64 per word, kBchWaves words per workgroup; the GF(2^8) exp/log tables
// and the wave algebra on them are gf256_wave.hpp's; the tables sit in LDS, as do the word, its
// syndromes and the locator of each wave. Lane l holds elements l, l + 64, l + 128, l + 192 of the word; an element is set when
// it is nonzero. Position p has code degree 254 - p whatever n is, so syndrome j of a set
// element is exp[j (254 - p) mod 255]: the lane steps that exponent by 254 - p per syndrome
// and never multiplies; four syndromes are packed in a word and XOR-reduced across the wave.
// All-zero syndromes end the word there (wave-uniform). Berlekamp-Massey keeps locator entry
// i and the auxiliary polynomial's in lane i: the reference's vectors never outgrow 2 t + 1 <=
// 63 entries, an entry past a vector's end reads as 0, which is what its i < sigma.len() guard
// and its resizes amount to; the discrepancy is a wave XOR reduction of sigma_i S_(n-i), the x^m
// shift a lane shuffle, the auxiliary polynomial is rescaled by 1 / delta. Chien: lane l
// evaluates sigma at 2^-d for the degrees d = l, l + 64, l + 128, l + 192 < 255; a root at or
// above 255 - n flips bit 0 of its element in LDS and is counted by a ballot, one below (never
// transmitted) is neither applied nor counted. The syndrome pass over the flipped word gives
// the residual: the number of nonzero syndromes. The store writes the k message elements, of
// the flipped word or, for a failed one, of the received word, and the status.
//
// The field is exact, so the order of a sum does not matter: every value here is the host's
// (bch.cpp), and so are the decisions. Every loop is bounded by a launch constant.
#include <algorithm>

#include "bch_blocks.hpp"
#include "gf256_wave.hpp"

namespace orion {

namespace {
constexpr int kBchWaves = 4;  // words per workgroup

// what a launch's words share; every field is wave-uniform
struct BchGeom {
  uint32_t n, k, t, ncw;
  uint64_t stream_len;  // elements of one input stream
};

// The 2 t syndromes of the word whose elements lane, lane + 64, .. this lane holds in r, four
// to a word of sw (S_j in byte (j - 1) % 4 of sw[(j - 1) / 4]), the same in every lane: S_1
// comes first, so a set element starts at its degree. Returns how many are nonzero.
__device__ __forceinline__ uint32_t bch_syndromes(const uint8_t* ex, const uint32_t r[4], uint32_t lane,
                                                  const BchGeom& g, uint32_t (&sw)[16]) {
  uint32_t start[4];
  bool nz[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    nz[a] = lane + 64u * a < g.n && r[a] != 0;
    start[a] = gf256::degree(lane + 64u * a);
  }
  uint32_t count = 0;
  gf256::syndromes(ex, lane, start, nz, 2u * g.t, sw, [&](uint32_t word) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) count += (word >> (8 * jj)) & 255u ? 1u : 0u;
  });
  return count;
}
}  // namespace

__global__ __launch_bounds__(64 * kBchWaves) void k_bch_decode(const uint8_t* __restrict__ in, long long total_cw,
                                                              BchGeom g, uint8_t* __restrict__ msgs,
                                                              int32_t* __restrict__ status) {
  __shared__ uint32_t s_tab[gf256::kTableWords];  // exp[512] | log[256]
  __shared__ uint8_t s_word[kBchWaves][256];
  __shared__ uint32_t s_syn[kBchWaves][16];
  __shared__ uint8_t s_sig[kBchWaves][64];
  const uint32_t tid = threadIdx.x;
  gf256::load_tables(s_tab, tid);
  __syncthreads();  // the only workgroup barrier: a wave without a word leaves after it
  const uint8_t* ex = reinterpret_cast<const uint8_t*>(s_tab);
  const uint8_t* lg = ex + 512;

  const uint32_t wave = tid >> 6, lane = tid & 63u;
  const long long gcw = static_cast<long long>(blockIdx.x) * kBchWaves + wave;
  if (gcw >= total_cw) return;
  const long long stream = gcw / g.ncw;
  const uint32_t cw = static_cast<uint32_t>(gcw - stream * g.ncw);
  const uint8_t* base = in + static_cast<uint64_t>(stream) * g.stream_len + static_cast<uint64_t>(cw) * g.n;
  uint8_t* word = s_word[wave];
  uint8_t* sig = s_sig[wave];
  const uint8_t* syn = reinterpret_cast<const uint8_t*>(s_syn[wave]);  // S_j is syn[j - 1]

  uint32_t r[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t p = lane + 64u * a;
    r[a] = p < g.n ? base[p] : 0u;
    word[p] = static_cast<uint8_t>(r[a]);
  }

  uint32_t sw[16];
  int32_t result = 0;
  if (bch_syndromes(ex, r, lane, g, sw) != 0) {  // uniform
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < 16; ++w) s_syn[wave][w] = sw[w];
    }
    wave_lds_fence();

    sig[lane] = static_cast<uint8_t>(gf256::berlekamp_massey(ex, lg, syn, lane, 2u * g.t));  // sigma_i in lane i
    wave_lds_fence();

    // Chien, bch.rs:171-195: a transmitted root flips its element and is counted
    uint32_t n_found = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const uint32_t d = lane + 64u * a;
      const bool applied = d < 255u && gf256::chien(ex, lg, sig, d, 2u * g.t) == 0 && d >= 255u - g.n;
      if (applied) word[254u - d] ^= 1u;
      n_found += static_cast<uint32_t>(__popcll(__ballot(applied)));
    }
    wave_lds_fence();

    uint32_t r2[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) r2[a] = word[lane + 64u * a];
    const uint32_t residual = bch_syndromes(ex, r2, lane, g, sw);
    if (residual != 0 || n_found > g.t) {
      result = -static_cast<int32_t>(max(residual, n_found));
    } else {
      result = static_cast<int32_t>(n_found);
#pragma unroll
      for (int a = 0; a < 4; ++a) r[a] = r2[a];
    }
  }

  uint8_t* M = msgs + static_cast<uint64_t>(gcw) * g.k;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t p = lane + 64u * a;
    if (p < g.k) M[p] = static_cast<uint8_t>(r[a]);
  }
  if (lane == 0) status[gcw] = result;
}

// what the encoder's words share
struct BchEncGeom {
  uint32_t n, k, pb, ncw;
  uint64_t nbits;    // information elements of one input stream
  uint8_t gc[256];   // generator coefficient i + 1 (highest degree first): what cell i adds of the feedback
};

// One wave64 per word. The shift register of bch.rs:105-125 has up to 248 cells: lane l holds
// cells l, l + 64, l + 128, l + 192 as bits 0..3 of one register. A step broadcasts cell 0,
// moves every cell down one (a shuffle from the next lane; lane 63 takes lane 0's next bit)
// and adds the feedback where the generator has a coefficient. The message is loaded, and
// copied to the output, 64 elements at a time; an element at or past the stream's end is 0.
__global__ __launch_bounds__(64 * kBchWaves) void k_bch_encode(const uint8_t* __restrict__ in, long long total_cw,
                                                              BchEncGeom g, uint8_t* __restrict__ out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const long long gcw = static_cast<long long>(blockIdx.x) * kBchWaves + (tid >> 6);
  if (gcw >= total_cw) return;  // whole waves only
  const long long stream = gcw / g.ncw;
  const uint64_t cw = static_cast<uint64_t>(gcw - stream * g.ncw);
  const uint8_t* I = in + static_cast<uint64_t>(stream) * g.nbits;
  uint8_t* C = out + static_cast<uint64_t>(gcw) * g.n;
  uint32_t gmask = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t c = lane + 64u * a;
    if (c < g.pb && g.gc[c]) gmask |= 1u << a;
  }
  uint32_t reg = 0;
  for (uint32_t p0 = 0; p0 < g.k; p0 += 64) {
    uint32_t mine = 0;
    if (p0 + lane < g.k) {
      const uint64_t src = cw * g.k + p0 + lane;
      if (src < g.nbits) mine = I[src];
      C[p0 + lane] = static_cast<uint8_t>(mine);
    }
    const uint32_t steps = min(64u, g.k - p0);
    for (uint32_t j = 0; j < steps; ++j) {
      const uint32_t r0 = __shfl(reg, 0, 64);
      const uint32_t fb = (__shfl(mine, static_cast<int>(j), 64) ^ r0) & 1u;
      uint32_t next = __shfl_down(reg, 1, 64);
      if (lane == 63) next = r0 >> 1;
      reg = next ^ (fb ? gmask : 0u);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t c = lane + 64u * a;
    if (c < g.pb) C[g.k + c] = static_cast<uint8_t>((reg >> a) & 1u);
  }
}

// ---- host side ---------------------------------------------------------------------------
bch::Bch bch_device_code(size_t t, size_t info_bits) {
  if (t < 1 || t > kBchMaxT) throw std::invalid_argument("bch: 1 <= t <= 31 on the device");
  return bch::Bch::for_info_bits(t, info_bits);
}

namespace {
void bch_counts(size_t nstreams, size_t ncw) {
  if (ncw < 1 || ncw > kBchMaxCw) throw std::invalid_argument("bch: a stream is 1 to 2^24 words");
  if (nstreams > kBchMaxStreams || nstreams * ncw > kBchMaxWords)
    throw std::invalid_argument("bch: nstreams above 2^24 or more than 2^30 words in a launch");
}
}  // namespace

void bch_decode_batch(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                      int32_t* status, hipStream_t s) {
  const bch::Bch code = bch_device_code(t, info_bits);
  const size_t ncw = nb / code.n();
  bch_counts(nstreams, ncw);
  if (nstreams == 0) return;
  if (reinterpret_cast<uintptr_t>(status) % 4) throw std::invalid_argument("bch decode: status not 4-byte aligned");
  BchGeom g{};
  g.n = static_cast<uint32_t>(code.n());
  g.k = static_cast<uint32_t>(code.k());
  g.t = static_cast<uint32_t>(t);
  g.ncw = static_cast<uint32_t>(ncw);
  g.stream_len = nb;
  const size_t total = nstreams * ncw;
  k_bch_decode<<<static_cast<unsigned>((total + kBchWaves - 1) / kBchWaves), 64 * kBchWaves, 0, s>>>(
      in, static_cast<long long>(total), g, msgs, status);
  ORION_LAUNCH_CHECK();
}

void bch_decode_batch_host(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                           int32_t* status) {
  const bch::Bch code = bch_device_code(t, info_bits);
  const size_t ncw = nb / code.n();
  bch_counts(nstreams, ncw);
  if (nstreams == 0) return;
  const size_t ib = nstreams * nb, mb = nstreams * ncw * code.k(), sb = nstreams * ncw * sizeof(int32_t);
  StagedIn d_in(in, ib);
  DevBuf d_msgs(mb + 16), d_status(sb);
  bch_decode_batch(t, info_bits, d_in.as<uint8_t>(), nstreams, nb, d_msgs.as<uint8_t>(), d_status.as<int32_t>(),
                   nullptr);
  stage_out(msgs, d_msgs, mb);
  stage_out(status, d_status, sb);
  ORION_HIP(hipDeviceSynchronize());
}

void bch_encode_batch(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits, uint8_t* coded,
                      hipStream_t s) {
  const bch::Bch code = bch_device_code(t, info_bits);
  if (nbits < 1 || nbits > (size_t(1) << 32)) throw std::invalid_argument("bch encode: 1 <= nbits <= 2^32");
  const size_t ncw = (nbits + code.k() - 1) / code.k();
  bch_counts(nstreams, ncw);
  if (nstreams == 0) return;
  BchEncGeom g{};
  g.n = static_cast<uint32_t>(code.n());
  g.k = static_cast<uint32_t>(code.k());
  g.pb = static_cast<uint32_t>(code.parity_bits());
  g.ncw = static_cast<uint32_t>(ncw);
  g.nbits = nbits;
  for (size_t i = 0; i < code.parity_bits(); ++i) g.gc[i] = code.generator()[i + 1];
  const size_t total = nstreams * ncw;
  k_bch_encode<<<static_cast<unsigned>((total + kBchWaves - 1) / kBchWaves), 64 * kBchWaves, 0, s>>>(
      bits, static_cast<long long>(total), g, coded);
  ORION_LAUNCH_CHECK();
}

void bch_encode_batch_host(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                           uint8_t* coded) {
  const bch::Bch code = bch_device_code(t, info_bits);
  if (nbits < 1 || nbits > (size_t(1) << 32)) throw std::invalid_argument("bch encode: 1 <= nbits <= 2^32");
  const size_t ncw = (nbits + code.k() - 1) / code.k();
  bch_counts(nstreams, ncw);
  if (nstreams == 0) return;
  const size_t ib = nstreams * nbits, ob = nstreams * ncw * code.n();
  StagedIn d_in(bits, ib);
  DevBuf d_out(ob + 16);
  bch_encode_batch(t, info_bits, d_in.as<uint8_t>(), nstreams, nbits, d_out.as<uint8_t>(), nullptr);
  stage_out(coded, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
