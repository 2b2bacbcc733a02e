// k_rs.hip — the outer code on the device: the batched Reed-Solomon decode of
// fec/reed_solomon.rs:141-233 (decode_counted: syndromes, Berlekamp-Massey, Chien, Forney, the
// residual check), the batched systematic encoder (reed_solomon.rs:90-110) and the frame-mode
// Forney interleaver (fec/interleaver.rs:122-305, modulate/ofdm_frame.rs:464-478).
//
// The decode. One wave64 per codeword, kRsWaves codewords per workgroup; the GF(2^8) exp/log
// tables and the wave algebra on them are gf256_wave.hpp's; the tables sit in LDS, as do the
// word, its syndromes, the locator and the evaluator of each wave. Lane l holds bytes l, l + 64, l + 128, l + 192 of the word. The
// fetch of a byte fuses the bit packing (eight bytes of one bit each, MSB first; one 8-byte
// load where the stream is 8-byte aligned) and the frame-mode Forney deinterleaver (payload
// byte q is stream byte D + q - (I - 1 - q mod I) M I, always inside the stream). Position p
// has code degree 254 - p whatever n is, so syndrome j of a byte b is exp[(log b + j (254 -
// p)) mod 255]: the lane steps that exponent by 254 - p per syndrome and never multiplies;
// four syndromes are packed in a word and XOR-reduced across the wave. All-zero syndromes end
// the word there (wave-uniform). Berlekamp-Massey keeps locator coefficient i and the
// auxiliary polynomial's in lane i (the degree stays <= 2 t <= 32 even for words that will be
// rejected): the discrepancy is a wave XOR reduction of sigma_i S_{n-i}, the x^m shift a lane
// shuffle. Chien: lane l evaluates sigma at 2^-i for the degrees i = l, l + 64, l + 128, l +
// 192 < 255, ballots count the roots. Forney: lane k builds evaluator coefficient k, a lane
// holding a root computes its magnitude and XORs it into the word in LDS (roots on degrees
// below 255 - n, never transmitted, count as roots and are not applied). The syndrome pass
// over the corrected word is the residual check. The store writes the message, of the
// corrected word or, for an uncorrectable one, of the received word, optionally XORed with the
// energy-dispersal sequence (rs.hpp make_ts_dispersal_mask).
//
// The field is exact, so the order of a sum does not matter: every value here is the host's
// (rs.cpp), and so are the decisions. Every loop is bounded by a launch constant.
#include <algorithm>

#include "gf256_wave.hpp"
#include "rs_blocks.hpp"

namespace orion {

namespace {
constexpr int kRsWaves = 4;  // codewords per workgroup of the decoder
constexpr int kEncLanes = 32;  // lanes per codeword of the encoder: one per parity cell

__constant__ __attribute__((aligned(16))) rs::TsDispersalMask d_mask = rs::make_ts_dispersal_mask();

// what a launch's words share; every field is wave-uniform
struct RsGeom {
  uint32_t n, np, k, t, ncw;
  uint32_t il_i, il_mi, il_d;  // branches (0: none), depth * branches, the round-trip delay
  uint32_t bits, aligned8, disperse;
  uint64_t stream_len;  // elements of one input stream
};

// payload byte q of a stream
__device__ __forceinline__ uint32_t rs_fetch(const uint8_t* __restrict__ base, const RsGeom& g, uint32_t q) {
  uint32_t src = q;
  if (g.il_i) src = q + g.il_d - (g.il_i - 1u - q % g.il_i) * g.il_mi;
  if (!g.bits) return base[src];
  const uint8_t* B = base + 8ull * src;
  uint32_t v = 0;
  if (g.aligned8) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(B);
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (static_cast<uint32_t>(w >> (8 * b)) & 1u) << (7 - b);
  } else {
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (B[b] & 1u) << (7 - b);
  }
  return v;
}

// The np syndromes of the word whose bytes lane, lane + 64, .. this lane holds in r, four to
// a word of sw (S_j in byte j % 4 of sw[j / 4]), the same in every lane: a byte b at position p
// starts at exponent log b. Returns their OR.
__device__ __forceinline__ uint32_t rs_syndromes(const uint8_t* ex, const uint8_t* lg, const uint32_t r[4],
                                                 uint32_t lane, const RsGeom& g, uint32_t (&sw)[8]) {
  uint32_t start[4];
  bool nz[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    nz[a] = lane + 64u * a < g.n && r[a] != 0;
    start[a] = lg[r[a]];
  }
  uint32_t any = 0;
  gf256::syndromes(ex, lane, start, nz, g.np, sw, [&](uint32_t word) { any |= word; });
  return any;
}
}  // namespace

__global__ __launch_bounds__(64 * kRsWaves) void k_rs_decode(const uint8_t* __restrict__ in, long long total_cw,
                                                            RsGeom g, uint8_t* __restrict__ msgs,
                                                            int32_t* __restrict__ status) {
  __shared__ uint32_t s_tab[gf256::kTableWords];  // exp[512] | log[256]
  __shared__ uint8_t s_word[kRsWaves][256];
  __shared__ uint32_t s_syn[kRsWaves][8];
  __shared__ uint8_t s_sig[kRsWaves][64];
  __shared__ uint8_t s_omg[kRsWaves][32];
  const uint32_t tid = threadIdx.x;
  gf256::load_tables(s_tab, tid);
  __syncthreads();  // the only workgroup barrier: a wave without a word leaves after it
  const uint8_t* ex = reinterpret_cast<const uint8_t*>(s_tab);
  const uint8_t* lg = ex + 512;

  const uint32_t wave = tid >> 6, lane = tid & 63u;
  const long long gcw = static_cast<long long>(blockIdx.x) * kRsWaves + wave;
  if (gcw >= total_cw) return;
  const long long stream = gcw / g.ncw;
  const uint32_t cw = static_cast<uint32_t>(gcw - stream * g.ncw);
  const uint8_t* base = in + static_cast<uint64_t>(stream) * g.stream_len;
  uint8_t* word = s_word[wave];
  uint8_t* sig = s_sig[wave];
  uint8_t* omg = s_omg[wave];
  const uint8_t* syn = reinterpret_cast<const uint8_t*>(s_syn[wave]);

  uint32_t r[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t p = lane + 64u * a;
    r[a] = p < g.n ? rs_fetch(base, g, cw * g.n + p) : 0u;
    word[p] = static_cast<uint8_t>(r[a]);
  }

  uint32_t sw[8];
  int32_t result = 0;
  if (rs_syndromes(ex, lg, r, lane, g, sw) != 0) {  // uniform
    result = -1;
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < 8; ++w) s_syn[wave][w] = sw[w];
    }
    wave_lds_fence();

    const uint32_t sigma = gf256::berlekamp_massey(ex, lg, syn, lane, 2u * g.t);  // sigma_i in lane i
    const uint64_t nzmask = __ballot(sigma != 0);  // bit 0 is set: sigma_0 = 1
    const uint32_t sigma_deg = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(nzmask)));
    sig[lane] = static_cast<uint8_t>(sigma);
    wave_lds_fence();

    // Chien, reed_solomon.rs:173-185: the roots are recorded for Forney
    uint32_t nroots = 0;
    bool root[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const uint32_t i = lane + 64u * a;
      root[a] = i < 255u && gf256::chien(ex, lg, sig, i, 2u * g.t) == 0;
      nroots += static_cast<uint32_t>(__popcll(__ballot(root[a])));
    }

    if (nroots == sigma_deg && sigma_deg <= g.t) {  // uniform
      // omega = S sigma mod x^np (reed_solomon.rs:335-348): coefficient k in lane k
      if (lane < 32) {
        uint32_t o = 0;
        for (uint32_t j = 0; j < g.np; ++j)
          if (j <= lane && lane < g.np) o ^= gf256::mul(ex, lg, syn[lane - j], sig[j]);
        omg[lane] = static_cast<uint8_t>(o);
      }
      wave_lds_fence();
      // Forney, reed_solomon.rs:209-226: e = X omega(1/X) / sigma'(1/X), X = 2^i
      bool bad = false;
      uint32_t napplied = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const uint32_t i = lane + 64u * a;
        bool applied = false;
        if (root[a]) {
          const uint32_t step = (255u - i) % 255u;  // log of 1/X
          uint32_t e = 0, ov = 0, dv = 0;           // e = (d step) mod 255
          for (uint32_t d = 0; d < g.np; ++d) {
            const uint32_t c = omg[d];
            if (c != 0) ov ^= ex[lg[c] + e];
            e += step;
            if (e >= 255u) e -= 255u;
          }
          e = 0;
          for (uint32_t d = 1; d <= 2u * g.t; d += 2) {  // sigma' coefficient d - 1 is sigma_d, d odd
            const uint32_t c = sig[d];
            if (c != 0) dv ^= ex[lg[c] + e];
            e += 2u * step;
            if (e >= 255u) e -= 255u;
            if (e >= 255u) e -= 255u;
          }
          if (dv == 0) {
            bad = true;
          } else if (ov != 0) {  // magnitude = X ov / dv, nonzero
            const uint32_t quot = ex[lg[ov] + 255u - lg[dv]];
            const uint32_t mag = ex[i + lg[quot]];  // i <= 254
            if (i >= 255u - g.n) {
              word[254u - i] ^= static_cast<uint8_t>(mag);
              applied = true;
            }
          }
        }
        napplied += static_cast<uint32_t>(__popcll(__ballot(applied)));
      }
      wave_lds_fence();
      if (__ballot(bad) == 0) {
        uint32_t r2[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) r2[a] = word[lane + 64u * a];
        if (rs_syndromes(ex, lg, r2, lane, g, sw) == 0) {
          result = static_cast<int32_t>(napplied);
#pragma unroll
          for (int a = 0; a < 4; ++a) r[a] = r2[a];
        }
      }
    }
  }

  uint8_t* M = msgs + static_cast<uint64_t>(gcw) * g.k;
  const uint8_t* mask = d_mask.m + (cw % 8u) * 188u;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t p = lane + 64u * a;
    if (p < g.k) M[p] = static_cast<uint8_t>(r[a] ^ (g.disperse ? mask[p] : 0u));
  }
  if (lane == 0) status[gcw] = result;
}

// what the encoder's words share
struct RsEncGeom {
  uint32_t n, np, k, ncw, disperse;
  uint8_t gcoef[32];  // generator coefficient np - 1 - i: what cell i adds of the feedback
};

// kEncLanes lanes per codeword: lane i holds cell i of the shift register of
// reed_solomon.rs:90-110. A step broadcasts cell 0, shifts the cells down a lane and adds the
// feedback times the lane's generator coefficient. The message is loaded, and copied to the
// output, 32 bytes at a time.
__global__ __launch_bounds__(256) void k_rs_encode(const uint8_t* __restrict__ msgs, long long total_cw, RsEncGeom g,
                                                   uint8_t* __restrict__ cws) {
  __shared__ uint32_t s_tab[gf256::kTableWords];
  const uint32_t tid = threadIdx.x;
  gf256::load_tables(s_tab, tid);
  __syncthreads();
  const uint8_t* ex = reinterpret_cast<const uint8_t*>(s_tab);
  const uint8_t* lg = ex + 512;
  const uint32_t li = tid & (kEncLanes - 1);
  const long long nslots = (total_cw + 1) / 2 * 2;  // both halves of a wave run the same loops
  long long gcw = static_cast<long long>(blockIdx.x) * (256 / kEncLanes) + tid / kEncLanes;
  if (gcw >= nslots) return;  // whole waves only
  const bool live = gcw < total_cw;
  if (!live) gcw = total_cw - 1;
  const uint32_t cw = static_cast<uint32_t>(gcw % g.ncw);
  const uint8_t* Min = msgs + static_cast<uint64_t>(gcw) * g.k;
  uint8_t* C = cws + static_cast<uint64_t>(gcw) * g.n;
  const uint8_t* mask = d_mask.m + (cw % 8u) * 188u;
  const uint32_t gc = li < g.np ? g.gcoef[li] : 0u;
  uint32_t reg = 0;
  for (uint32_t p0 = 0; p0 < g.k; p0 += kEncLanes) {
    uint32_t mine = 0;
    if (p0 + li < g.k) {
      mine = Min[p0 + li] ^ (g.disperse ? mask[p0 + li] : 0u);
      if (live) C[p0 + li] = static_cast<uint8_t>(mine);
    }
    const uint32_t steps = min(static_cast<uint32_t>(kEncLanes), g.k - p0);
    for (uint32_t j = 0; j < steps; ++j) {
      const uint32_t fb = __shfl(mine, static_cast<int>(j), kEncLanes) ^ __shfl(reg, 0, kEncLanes);
      uint32_t next = __shfl_down(reg, 1, kEncLanes);
      if (li + 1u >= g.np) next = 0;
      reg = next ^ gf256::mul(ex, lg, fb, gc);
    }
  }
  if (live && li < g.np) C[g.k + li] = static_cast<uint8_t>(reg);
}

// what the interleaver's streams share
struct ForneyGeom {
  uint32_t len, padded, out_bytes;  // input bytes, rounded up to branches, padded + delay
  uint32_t il_i, il_mi, bits;
  uint64_t out_len;  // elements of one output stream
};

// One thread per output element of a stream's forney_frame_interleave: out[i] = in[i - (i mod
// I) M I], zero where that index is negative or at or past the input (the padding and the
// flush); with bits, element e is bit 7 - e % 8 of byte e / 8.
__global__ __launch_bounds__(256) void k_forney_interleave(const uint8_t* __restrict__ in, long long total,
                                                           ForneyGeom g, uint8_t* __restrict__ out) {
  const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long stream = idx / static_cast<long long>(g.out_len);
  const uint64_t e = static_cast<uint64_t>(idx) - static_cast<uint64_t>(stream) * g.out_len;
  const uint32_t i = static_cast<uint32_t>(g.bits ? e >> 3 : e);
  const uint64_t back = static_cast<uint64_t>(i % g.il_i) * g.il_mi;
  uint32_t v = 0;
  if (i >= back && i - back < g.len) v = in[static_cast<uint64_t>(stream) * g.len + (i - back)];
  if (g.bits) v = (v >> (7u - static_cast<uint32_t>(e & 7u))) & 1u;
  out[idx] = static_cast<uint8_t>(v);
}

// ---- host side ---------------------------------------------------------------------------
namespace {
struct RsCheck {
  size_t k, delay;
};
RsCheck rs_check(size_t n, size_t n_parity, size_t nstreams, size_t ncw, const RsFusion& f) {
  const rs::ReedSolomon code(n, n_parity);  // the reference's argument check
  if (n_parity < 1 || n_parity > kRsMaxParity) throw std::invalid_argument("rs: 1 <= n_parity <= 32 on the device");
  if (ncw < 1 || ncw > kRsMaxCw) throw std::invalid_argument("rs: 1 <= ncw <= 2^20");
  if (nstreams > kRsMaxStreams || nstreams * ncw > kRsMaxWords)
    throw std::invalid_argument("rs: nstreams above 2^24 or nstreams * ncw above 2^30");
  if ((f.branches == 0) != (f.depth == 0))
    throw std::invalid_argument("rs: interleaver branches, depth both zero (none) or both nonzero");
  RsCheck c{code.k(), 0};
  if (f.branches) {
    c.delay = rs::conv_roundtrip_delay(f.branches, f.depth);
    if (ncw * n % f.branches)
      throw std::invalid_argument("rs: with a deinterleaver ncw * n must be a multiple of its branches");
  }
  if (f.disperse && code.k() != rs::kTsPacketLen)
    throw std::invalid_argument("rs: energy dispersal needs k = 188, one transport-stream packet per word");
  return c;
}
}  // namespace

size_t rs_decode_stream_len(size_t n, size_t n_parity, size_t ncw, const RsFusion& f) {
  const RsCheck c = rs_check(n, n_parity, 0, ncw, f);
  return (ncw * n + c.delay) * (f.bits ? 8 : 1);
}

void rs_decode_batch(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, const RsFusion& f,
                     uint8_t* msgs, int32_t* status, hipStream_t s) {
  const RsCheck c = rs_check(n, n_parity, nstreams, ncw, f);
  if (nstreams == 0) return;
  if (reinterpret_cast<uintptr_t>(status) % 4) throw std::invalid_argument("rs decode: status not 4-byte aligned");
  RsGeom g{};
  g.n = static_cast<uint32_t>(n);
  g.np = static_cast<uint32_t>(n_parity);
  g.k = static_cast<uint32_t>(c.k);
  g.t = g.np / 2;
  g.ncw = static_cast<uint32_t>(ncw);
  g.il_i = static_cast<uint32_t>(f.branches);
  g.il_mi = static_cast<uint32_t>(f.depth * f.branches);
  g.il_d = static_cast<uint32_t>(c.delay);
  g.bits = f.bits;
  g.disperse = f.disperse;
  g.stream_len = (ncw * n + c.delay) * (f.bits ? 8 : 1);
  g.aligned8 = f.bits && reinterpret_cast<uintptr_t>(in) % 8 == 0;  // stream_len is a multiple of 8
  const size_t total = nstreams * ncw;
  k_rs_decode<<<static_cast<unsigned>((total + kRsWaves - 1) / kRsWaves), 64 * kRsWaves, 0, s>>>(
      in, static_cast<long long>(total), g, msgs, status);
  ORION_LAUNCH_CHECK();
}

void rs_decode_batch_host(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw,
                          const RsFusion& f, uint8_t* msgs, int32_t* status) {
  const RsCheck c = rs_check(n, n_parity, nstreams, ncw, f);
  if (nstreams == 0) return;
  const size_t ib = nstreams * (ncw * n + c.delay) * (f.bits ? 8 : 1), mb = nstreams * ncw * c.k,
               sb = nstreams * ncw * sizeof(int32_t);
  StagedIn d_in(in, ib);
  DevBuf d_msgs(mb + 16), d_status(sb);
  rs_decode_batch(n, n_parity, d_in.as<uint8_t>(), nstreams, ncw, f, d_msgs.as<uint8_t>(), d_status.as<int32_t>(),
                  nullptr);
  stage_out(msgs, d_msgs, mb);
  stage_out(status, d_status, sb);
  ORION_HIP(hipDeviceSynchronize());
}

void rs_encode_batch(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw, const RsFusion& f,
                     uint8_t* cws, hipStream_t s) {
  if (f.bits || f.branches || f.depth) throw std::invalid_argument("rs encode: only the dispersal can be fused");
  const RsCheck c = rs_check(n, n_parity, nstreams, ncw, f);
  if (nstreams == 0) return;
  const rs::ReedSolomon code(n, n_parity);
  RsEncGeom g{};
  g.n = static_cast<uint32_t>(n);
  g.np = static_cast<uint32_t>(n_parity);
  g.k = static_cast<uint32_t>(c.k);
  g.ncw = static_cast<uint32_t>(ncw);
  g.disperse = f.disperse;
  for (size_t i = 0; i < n_parity; ++i) g.gcoef[i] = code.generator()[n_parity - 1 - i];
  const size_t total = nstreams * ncw, per_block = 256 / kEncLanes;
  k_rs_encode<<<static_cast<unsigned>((total + per_block - 1) / per_block), 256, 0, s>>>(
      msgs, static_cast<long long>(total), g, cws);
  ORION_LAUNCH_CHECK();
}

void rs_encode_batch_host(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw,
                          const RsFusion& f, uint8_t* cws) {
  if (f.bits || f.branches || f.depth) throw std::invalid_argument("rs encode: only the dispersal can be fused");
  const RsCheck c = rs_check(n, n_parity, nstreams, ncw, f);
  if (nstreams == 0) return;
  const size_t mb = nstreams * ncw * c.k, cb = nstreams * ncw * n;
  StagedIn d_msgs(msgs, mb);
  DevBuf d_cws(cb + 16);
  rs_encode_batch(n, n_parity, d_msgs.as<uint8_t>(), nstreams, ncw, f, d_cws.as<uint8_t>(), nullptr);
  stage_out(cws, d_cws, cb);
  ORION_HIP(hipDeviceSynchronize());
}

namespace {
ForneyGeom forney_geom(size_t branches, size_t depth, size_t nstreams, size_t len, bool bits) {
  const size_t d = rs::conv_roundtrip_delay(branches, depth);
  if (len < 1 || len > (size_t(1) << 27)) throw std::invalid_argument("forney interleave: 1 <= len <= 2^27");
  if (nstreams > kRsMaxStreams) throw std::invalid_argument("forney interleave: nstreams above 2^24");
  ForneyGeom g{};
  g.len = static_cast<uint32_t>(len);
  g.padded = static_cast<uint32_t>((len + branches - 1) / branches * branches);
  g.out_bytes = g.padded + static_cast<uint32_t>(d);
  g.il_i = static_cast<uint32_t>(branches);
  g.il_mi = static_cast<uint32_t>(depth * branches);
  g.bits = bits;
  g.out_len = static_cast<uint64_t>(g.out_bytes) * (bits ? 8 : 1);
  if (nstreams * g.out_len > (uint64_t(1) << 38))
    throw std::invalid_argument("forney interleave: more than 2^38 output elements in a launch");
  return g;
}
}  // namespace

size_t forney_interleave_stream_len(size_t branches, size_t depth, size_t len, bool bits) {
  return forney_geom(branches, depth, 0, len, bits).out_len;
}

void forney_interleave_batch(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len, bool bits,
                             uint8_t* out, hipStream_t s) {
  const ForneyGeom g = forney_geom(branches, depth, nstreams, len, bits);
  if (nstreams == 0) return;
  const uint64_t total = nstreams * g.out_len;
  k_forney_interleave<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(in, static_cast<long long>(total), g,
                                                                                 out);
  ORION_LAUNCH_CHECK();
}

void forney_interleave_batch_host(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len,
                                  bool bits, uint8_t* out) {
  const ForneyGeom g = forney_geom(branches, depth, nstreams, len, bits);
  if (nstreams == 0) return;
  const size_t ib = nstreams * len, ob = nstreams * g.out_len;
  StagedIn d_in(in, ib);
  DevBuf d_out(ob + 16);
  forney_interleave_batch(branches, depth, d_in.as<uint8_t>(), nstreams, len, bits, d_out.as<uint8_t>(), nullptr);
  stage_out(out, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
