// k_frame.hip — the glue of the COFDM frame chain on the device: what lies between the batched
// codes (frame_blocks.hpp), held to frame.hpp byte for byte.
//
// Pack and unpack. One wave64 per frame, kFrameWaves frames per workgroup. The framed block is
// info bytes | CRC. The info bytes are cut into nact <= 64 contiguous chunks, lane 0 the first
// head bytes (1..chunk; 0 only for an empty block), lane l >= 1 the chunk bytes from head +
// (l - 1) chunk: the ragged chunk leads, so what follows lane l is (nact - 1 - l) whole chunks.
//   CRC. Each lane runs the byte recurrence over its chunk, lane 0 from the CRC's initial value,
// the others from zero. The register is linear over GF(2) in (state, data), so the frame's CRC
// is the XOR over lanes of each lane's register advanced through the bytes that follow it, as
// zero data: lane l applies B^(nact - 1 - l), B = (one zero byte)^chunk, from the six maps
// B^(2^s) the host prepares; then a wave XOR reduction and the final XOR.
//   Whitener. The additive LFSR (and DVB-T's dispersal PRBS, the same register with taps 3 and
// width 15, its output the feedback bit, MSB first) is linear in its state: lane l >= 1 starts
// from T^(8 head) then (T^(8 chunk))^(l - 1) of the frame's seed, again from prepared powers,
// and steps it eight times per byte along its chunk. The last active lane ends at step 8 info_len
// and carries on over the CRC bytes.
//   No lane walks a frame alone, nothing is staged in LDS, and there is no barrier.
//
// Coded bits and LLR rows. One wave per frame; lane l takes the groups of eight elements l, l
// + 64, ..: its register starts at (T^8)^l of the seed and jumps by (T^8)^64 per round. Element
// i of a row meets PN step 8 (i / 8) + 7 - i % 8 (packed MSB first, whitened LSB first).
//
// Every value is exact (GF(2)), so the order of a sum does not matter. Every loop is bounded by
// a launch constant; every index is checked against the row it addresses by the host wrapper.
#include <algorithm>
#include <vector>

#include "frame_blocks.hpp"
#include "hip_common.hpp"
#include "rs.hpp"

namespace orion {

namespace {
constexpr int kFrameWaves = 4;  // frames per workgroup

// the whitening register; every field is wave-uniform
struct PnGeom {
  uint32_t kind;  // frame::kScrNone / kScrAdditive / kScrDvbT
  uint32_t taps, top, mask, fixed_seed;
};

// pack / unpack
struct FrameGeom {
  uint32_t info_len, clen, crc, chunk, nact, head, hdr, packed;  // packed: the far side is bytes, not bits
  uint32_t n_inner, n_outer, outer_present;
  uint64_t stride;  // elements of one row of the far side
  PnGeom pn;
  uint32_t crc_adv[6][32];   // B^(2^s)
  uint32_t pn_head[32];      // T^(8 head)
  uint32_t pn_chunk[6][32];  // (T^(8 chunk))^(2^s)
};

// coded bits / LLR rows
struct RowGeom {
  uint32_t n, out_len;
  uint64_t in_stride;
  PnGeom pn;
  uint32_t q[7][32];  // (T^8)^(2^s)
};

__device__ __forceinline__ uint32_t gf2_apply(const uint32_t (&col)[32], uint32_t v) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) r ^= (0u - ((v >> i) & 1u)) & col[i];
  return r;
}

__device__ __forceinline__ uint32_t pn_seed(const PnGeom& p, const long long* seeds, long long f) {
  if (p.kind == frame::kScrDvbT) return rs::kDvbTPrbsInit;
  const uint32_t raw = seeds ? static_cast<uint32_t>(seeds[f]) : p.fixed_seed;
  const uint32_t m = raw & p.mask;
  return m == 0 ? 1u : m;
}

// The eight PN bits the next byte is XORed with; the register moves on eight steps.
__device__ __forceinline__ uint32_t pn_byte(const PnGeom& p, uint32_t& reg) {
  uint32_t pn = 0;
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const uint32_t fb = static_cast<uint32_t>(__popc(reg & p.taps)) & 1u;
    pn = p.kind == frame::kScrDvbT ? pn << 1 | fb : pn | (reg & 1u) << bit;
    reg = ((reg >> 1) | (fb << p.top)) & p.mask;
  }
  return pn;
}

__device__ __forceinline__ uint32_t crc_update(uint32_t kind, uint32_t crc, uint32_t byte) {
  if (kind == frame::kCrc16) {
    crc ^= byte << 8;
#pragma unroll
    for (int b = 0; b < 8; ++b) crc = (crc & 0x8000u ? (crc << 1) ^ 0x1021u : crc << 1) & 0xFFFFu;
  } else {
    crc ^= byte;
#pragma unroll
    for (int b = 0; b < 8; ++b) crc = crc & 1u ? (crc >> 1) ^ 0xEDB88320u : crc >> 1;
  }
  return crc;
}

// what a lane of pack / unpack starts from
struct LaneStart {
  uint32_t start, len, reg, crc;
  bool last;  // the last active lane: it takes the CRC bytes
};
__device__ __forceinline__ LaneStart lane_start(const FrameGeom& g, uint32_t lane, uint32_t seed) {
  LaneStart L;
  const bool active = lane < g.nact;
  L.start = lane == 0 ? 0u : g.head + (lane - 1u) * g.chunk;
  L.len = !active ? 0u : lane == 0 ? g.head : g.chunk;
  L.last = lane + 1u == g.nact;
  L.crc = lane == 0 && g.crc != frame::kCrcNone ? (g.crc == frame::kCrc16 ? 0xFFFFu : 0xFFFFFFFFu) : 0u;
  uint32_t reg = seed;
  if (g.pn.kind != frame::kScrNone) {  // uniform
    const uint32_t moved = gf2_apply(g.pn_head, reg);
    reg = lane >= 1 ? moved : reg;
    const uint32_t e = lane >= 1 ? lane - 1u : 0u;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const uint32_t t = gf2_apply(g.pn_chunk[s], reg);
      reg = (e >> s) & 1u ? t : reg;
    }
  }
  L.reg = reg;
  return L;
}

// the frame's CRC from every lane's register, the same in every lane
__device__ __forceinline__ uint32_t crc_combine(const FrameGeom& g, uint32_t lane, uint32_t crc) {
  const uint32_t e = lane < g.nact ? g.nact - 1u - lane : 0u;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const uint32_t t = gf2_apply(g.crc_adv[s], crc);
    crc = (e >> s) & 1u ? t : crc;
  }
  crc = wave_xor(lane < g.nact ? crc : 0u);
  return g.crc == frame::kCrc32 ? ~crc : crc;
}

__device__ __forceinline__ uint32_t header_byte(const long long* F, uint32_t p) {
  if (p == 0) return static_cast<uint32_t>(F[0]) & 255u;
  if (p < 5) return (static_cast<uint32_t>(F[1]) >> (8u * (4u - p))) & 255u;
  if (p < 9) return (static_cast<uint32_t>(F[2]) >> (8u * (8u - p))) & 255u;
  if (p == 9) return static_cast<uint32_t>(F[3]) & 255u;
  return (static_cast<uint32_t>(F[4]) >> (8u * (13u - p))) & 255u;
}
}  // namespace

__global__ __launch_bounds__(64 * kFrameWaves) void k_frame_pack(const uint8_t* __restrict__ payload,
                                                                const long long* __restrict__ fields,
                                                                const long long* __restrict__ seeds,
                                                                long long nframes, FrameGeom g,
                                                                uint8_t* __restrict__ out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const long long f = static_cast<long long>(blockIdx.x) * kFrameWaves + (tid >> 6);
  if (f >= nframes) return;  // whole waves only
  const uint8_t* P = g.hdr ? nullptr : payload + static_cast<uint64_t>(f) * g.info_len;
  const long long* F = g.hdr ? fields + static_cast<uint64_t>(f) * 5u : nullptr;
  uint8_t* O = out + static_cast<uint64_t>(f) * g.stride;
  LaneStart L = lane_start(g, lane, pn_seed(g.pn, seeds, f));

  auto emit = [&](uint32_t p, uint32_t v) {
    if (g.packed) {
      O[p] = static_cast<uint8_t>(v);
    } else {
#pragma unroll
      for (int b = 0; b < 8; ++b) O[8u * p + b] = static_cast<uint8_t>((v >> (7 - b)) & 1u);
    }
  };
  for (uint32_t j = 0; j < g.chunk; ++j) {
    if (j < L.len) {
      const uint32_t p = L.start + j;
      const uint32_t v = g.hdr ? header_byte(F, p) : P[p];
      if (g.crc != frame::kCrcNone) L.crc = crc_update(g.crc, L.crc, v);
      emit(p, g.pn.kind != frame::kScrNone ? v ^ pn_byte(g.pn, L.reg) : v);
    }
  }
  if (g.clen == 0) return;  // uniform
  const uint32_t crc = crc_combine(g, lane, L.crc);
  if (L.last) {
    for (uint32_t i = 0; i < g.clen; ++i) {
      const uint32_t v = (crc >> (8u * (g.clen - 1u - i))) & 255u;
      emit(g.info_len + i, g.pn.kind != frame::kScrNone ? v ^ pn_byte(g.pn, L.reg) : v);
    }
  }
}

__global__ __launch_bounds__(64 * kFrameWaves) void k_frame_unpack(
    const uint8_t* __restrict__ in, const long long* __restrict__ seeds, const int32_t* __restrict__ unsat,
    const int32_t* __restrict__ status, long long nframes, FrameGeom g, uint8_t* __restrict__ payload,
    uint8_t* __restrict__ flags, int32_t* __restrict__ corrected, long long* __restrict__ fields) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const long long f = static_cast<long long>(blockIdx.x) * kFrameWaves + (tid >> 6);
  if (f >= nframes) return;  // whole waves only
  const uint8_t* I = in + static_cast<uint64_t>(f) * g.stride;
  uint8_t* P = payload + static_cast<uint64_t>(f) * g.info_len;
  LaneStart L = lane_start(g, lane, pn_seed(g.pn, seeds, f));

  auto fetch = [&](uint32_t p) {
    if (g.packed) return static_cast<uint32_t>(I[p]);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v = v << 1 | (I[8u * p + b] & 1u);
    return v;
  };
  uint32_t mine = 0;  // header: byte l of the fields is lane l's
  for (uint32_t j = 0; j < g.chunk; ++j) {
    if (j < L.len) {
      const uint32_t p = L.start + j;
      uint32_t v = fetch(p);
      if (g.pn.kind != frame::kScrNone) v ^= pn_byte(g.pn, L.reg);
      if (g.crc != frame::kCrcNone) L.crc = crc_update(g.crc, L.crc, v);
      P[p] = static_cast<uint8_t>(v);
      mine = v;
    }
  }
  uint32_t ok = 1;
  if (g.clen != 0) {  // uniform
    const uint32_t crc = crc_combine(g, lane, L.crc);
    uint32_t rx = 0;
    if (L.last) {
      for (uint32_t i = 0; i < g.clen; ++i) {
        uint32_t v = fetch(g.info_len + i);
        if (g.pn.kind != frame::kScrNone) v ^= pn_byte(g.pn, L.reg);
        rx = rx << 8 | v;
      }
    }
    ok = __shfl(rx == crc ? 1u : 0u, static_cast<int>(g.nact - 1u), 64);
  }

  bool bad_in = false, bad_out = false;
  uint32_t fixed = 0;
  if (unsat)
    for (uint32_t i = lane; i < g.n_inner; i += 64) bad_in |= unsat[static_cast<uint64_t>(f) * g.n_inner + i] != 0;
  if (status)
    for (uint32_t i = lane; i < g.n_outer; i += 64) {
      const int32_t st = status[static_cast<uint64_t>(f) * g.n_outer + i];
      bad_out |= st < 0;
      fixed += st > 0 ? static_cast<uint32_t>(st) : 0u;
    }
  const uint32_t inner_ok = __ballot(bad_in) == 0 ? 1u : 0u, outer_ok = __ballot(bad_out) == 0 ? 1u : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) fixed += __shfl_xor(fixed, off, 64);

  uint32_t fb[frame::kHeaderFieldBytes] = {};
  if (g.hdr) {  // uniform
#pragma unroll
    for (int i = 0; i < static_cast<int>(frame::kHeaderFieldBytes); ++i) fb[i] = __shfl(mine, i, 64);
  }
  if (lane == 0) {
    uint8_t* fl = flags + static_cast<uint64_t>(f) * 4u;
    fl[0] = static_cast<uint8_t>(inner_ok);
    fl[1] = static_cast<uint8_t>(outer_ok);
    fl[2] = static_cast<uint8_t>(ok);
    fl[3] = static_cast<uint8_t>(g.clen != 0 ? ok : g.outer_present ? outer_ok : inner_ok);
    corrected[f] = static_cast<int32_t>(fixed);
    if (g.hdr) {
      long long* F = fields + static_cast<uint64_t>(f) * 5u;
      F[0] = fb[0];
      F[1] = static_cast<long long>(fb[1] << 24 | fb[2] << 16 | fb[3] << 8 | fb[4]);
      F[2] = static_cast<long long>(fb[5] << 24 | fb[6] << 16 | fb[7] << 8 | fb[8]);
      F[3] = fb[9];
      F[4] = static_cast<long long>(fb[10] << 24 | fb[11] << 16 | fb[12] << 8 | fb[13]);
    }
  }
}

namespace {
// lane l's register at its first group of eight elements
__device__ __forceinline__ uint32_t row_reg(const RowGeom& g, uint32_t lane, uint32_t seed) {
  uint32_t reg = seed;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const uint32_t t = gf2_apply(g.q[s], reg);
    reg = (lane >> s) & 1u ? t : reg;
  }
  return reg;
}
}  // namespace

__global__ __launch_bounds__(64 * kFrameWaves) void k_frame_coded_bits(const uint8_t* __restrict__ in,
                                                                      const long long* __restrict__ seeds,
                                                                      long long nframes, RowGeom g,
                                                                      uint8_t* __restrict__ out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const long long f = static_cast<long long>(blockIdx.x) * kFrameWaves + (tid >> 6);
  if (f >= nframes) return;
  const uint8_t* I = in + static_cast<uint64_t>(f) * g.in_stride;
  uint8_t* O = out + static_cast<uint64_t>(f) * g.out_len;
  const bool pn_on = g.pn.kind != frame::kScrNone;  // uniform
  uint32_t reg = pn_on ? row_reg(g, lane, pn_seed(g.pn, seeds, f)) : 0u;
  for (uint32_t g0 = 0; 8u * g0 < g.out_len; g0 += 64) {
    const uint32_t base = 8u * (g0 + lane);
    uint32_t pn = 0;
    if (pn_on) {
      uint32_t r = reg;
      pn = pn_byte(g.pn, r);
      reg = gf2_apply(g.q[6], reg);
    }
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const uint32_t i = base + b;
      if (i < g.out_len) {
        uint32_t v = i < g.n ? I[i] : 0u;
        if (pn_on && i < g.n) v = (v & 1u) ^ ((pn >> (7u - b)) & 1u);
        O[i] = static_cast<uint8_t>(v);
      }
    }
  }
}

__global__ __launch_bounds__(64 * kFrameWaves) void k_frame_llr_prepare(const uint32_t* __restrict__ in,
                                                                       const long long* __restrict__ seeds,
                                                                       long long nframes, RowGeom g,
                                                                       uint32_t* __restrict__ out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const long long f = static_cast<long long>(blockIdx.x) * kFrameWaves + (tid >> 6);
  if (f >= nframes) return;
  const uint32_t* I = in + static_cast<uint64_t>(f) * g.in_stride;
  uint32_t* O = out + static_cast<uint64_t>(f) * g.n;
  const bool pn_on = g.pn.kind != frame::kScrNone;  // uniform
  uint32_t reg = pn_on ? row_reg(g, lane, pn_seed(g.pn, seeds, f)) : 0u;
  for (uint32_t g0 = 0; 8u * g0 < g.n; g0 += 64) {
    const uint32_t base = 8u * (g0 + lane);
    uint32_t pn = 0;
    if (pn_on) {
      uint32_t r = reg;
      pn = pn_byte(g.pn, r);
      reg = gf2_apply(g.q[6], reg);
    }
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const uint32_t i = base + b;
      if (i < g.n) O[i] = I[i] ^ (((pn >> (7u - b)) & 1u) << 31);
    }
  }
}

__global__ __launch_bounds__(256) void k_frame_bytes_to_bits(const uint8_t* __restrict__ in, long long total_bits,
                                                            uint8_t* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < total_bits) out[i] = static_cast<uint8_t>((in[i >> 3] >> (7 - (i & 7))) & 1u);
}

// The frame's IQ: the shared lead (S&C repeats and training symbol), then this frame's header
// and payload symbols. One thread per sample. From win_start on the stream is whole symbols of
// sps samples, each tapered on its first and last ramp_len samples: x.re * w and x.im * w, the
// host's two f32 multiplies (SymbolWindow::process); a trailing part shorter than a symbol is
// left alone, as the host's post-pass leaves it.
struct AssembleGeom {
  uint32_t lead_len, hdr_len, pay_len, frame_len, sps, win_start, ramp_len;
};
__global__ __launch_bounds__(256) void k_frame_assemble(const float2* __restrict__ lead, const float2* __restrict__ hdr,
                                                       const float2* __restrict__ pay,
                                                       const float* __restrict__ ramp, long long total,
                                                       AssembleGeom g, float2* __restrict__ out) {
  const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long f = idx / g.frame_len;
  const uint32_t i = static_cast<uint32_t>(idx - f * g.frame_len);
  float2 v;
  if (i < g.lead_len)
    v = lead[i];
  else if (i < g.lead_len + g.hdr_len)
    v = hdr[static_cast<uint64_t>(f) * g.hdr_len + (i - g.lead_len)];
  else
    v = pay[static_cast<uint64_t>(f) * g.pay_len + (i - g.lead_len - g.hdr_len)];
  if (g.ramp_len != 0 && i >= g.win_start) {
    const uint32_t r = i - g.win_start, sym = r / g.sps, pos = r - sym * g.sps;
    if ((sym + 1u) * g.sps <= g.frame_len - g.win_start) {
      if (pos < g.ramp_len) {
        const float w = ramp[pos];
        v.x *= w;
        v.y *= w;
      } else if (pos >= g.sps - g.ramp_len) {
        const float w = ramp[g.sps - 1u - pos];
        v.x *= w;
        v.y *= w;
      }
    }
  }
  out[idx] = v;
}

// ---- host side ---------------------------------------------------------------------------
namespace {
void copy_map(const frame::BitMatrix& m, uint32_t (&dst)[32]) { std::copy(m.col, m.col + 32, dst); }

// the register of the scheme's whitener when it sits at pos, and its one-step map
PnGeom pn_geom(const frame::Scheme& sch, int pos, frame::BitMatrix* step) {
  PnGeom p{};
  *step = frame::bitmatrix_identity();
  if (sch.scrambler == frame::kScrNone || sch.scrambler_pos != pos) return p;
  if (sch.scrambler == frame::kScrDvbT) {
    if (pos != frame::kBeforeOuterFec) return p;  // the dispersal is byte-domain only
    p.kind = frame::kScrDvbT;
    p.taps = 3;
    p.top = 14;
    p.mask = 0x7FFF;
  } else {
    p.kind = frame::kScrAdditive;
    p.taps = sch.scr_poly;
    p.top = sch.scr_width - 1;
    p.mask = sch.scr_width >= 32 ? 0xFFFFFFFFu : (1u << sch.scr_width) - 1u;
    p.fixed_seed = sch.scr_seed;
  }
  *step = frame::lfsr_step_map(p.taps, p.top + 1);
  return p;
}

void frame_counts(size_t nframes, size_t info_len, bool header) {
  if (nframes > kFrameMaxFrames) throw std::invalid_argument("frame: nframes above 2^24");
  if (info_len > kFrameMaxInfo) throw std::invalid_argument("frame: a block is at most 2^16 bytes on the device");
  if (header && info_len != frame::kHeaderFieldBytes)
    throw std::invalid_argument("frame: a header block is its 14 field bytes");
}

FrameGeom frame_geom(const frame::Scheme& sch, size_t info_len, bool header, bool packed, size_t stride) {
  frame::check_scheme(sch);
  FrameGeom g{};
  g.info_len = static_cast<uint32_t>(info_len);
  g.crc = static_cast<uint32_t>(sch.crc);
  g.clen = static_cast<uint32_t>(frame::crc_len(sch.crc));
  g.chunk = std::max<uint32_t>(1, (g.info_len + 63u) / 64u);
  g.nact = std::max<uint32_t>(1, (g.info_len + g.chunk - 1u) / g.chunk);
  g.head = g.info_len - (g.nact - 1u) * g.chunk;
  g.hdr = header;
  g.packed = packed;
  g.stride = stride;
  g.outer_present = sch.outer != frame::kOuterNone;
  frame::BitMatrix step;
  g.pn = pn_geom(sch, frame::kBeforeOuterFec, &step);
  frame::BitMatrix b = frame::bitmatrix_pow(frame::crc_byte_map(sch.crc), g.chunk);
  frame::BitMatrix c = frame::bitmatrix_pow(step, 8ull * g.chunk);
  copy_map(frame::bitmatrix_pow(step, 8ull * g.head), g.pn_head);
  for (int s = 0; s < 6; ++s) {
    copy_map(b, g.crc_adv[s]);
    copy_map(c, g.pn_chunk[s]);
    b = frame::bitmatrix_mul(b, b);
    c = frame::bitmatrix_mul(c, c);
  }
  return g;
}

RowGeom row_geom(const frame::Scheme& sch, size_t in_stride, size_t n, size_t out_len, size_t nframes) {
  frame::check_scheme(sch);
  if (nframes > kFrameMaxFrames) throw std::invalid_argument("frame: nframes above 2^24");
  if (in_stride > kFrameMaxRow || out_len > kFrameMaxRow || n > in_stride || n > out_len)
    throw std::invalid_argument("frame: rows of at most 2^24 elements, the kept count within both rows");
  RowGeom g{};
  g.n = static_cast<uint32_t>(n);
  g.out_len = static_cast<uint32_t>(out_len);
  g.in_stride = in_stride;
  frame::BitMatrix step;
  g.pn = pn_geom(sch, frame::kAfterInnerFec, &step);
  frame::BitMatrix q = frame::bitmatrix_pow(step, 8);
  for (int s = 0; s < 7; ++s) {
    copy_map(q, g.q[s]);
    q = frame::bitmatrix_mul(q, q);
  }
  return g;
}

unsigned frame_grid(size_t nframes) { return static_cast<unsigned>((nframes + kFrameWaves - 1) / kFrameWaves); }
}  // namespace

void frame_pack_batch(const frame::Scheme& sch, const uint8_t* payload, const long long* fields,
                      const long long* seeds, size_t nframes, size_t info_len, bool out_bytes, uint8_t* out,
                      hipStream_t s) {
  const bool header = fields != nullptr;
  frame_counts(nframes, info_len, header);
  const size_t framed = info_len + frame::crc_len(sch.crc);
  const FrameGeom g = frame_geom(sch, info_len, header, out_bytes, out_bytes ? framed : framed * 8);
  if (nframes == 0 || framed == 0) return;
  k_frame_pack<<<frame_grid(nframes), 64 * kFrameWaves, 0, s>>>(payload, fields, seeds,
                                                                static_cast<long long>(nframes), g, out);
  ORION_LAUNCH_CHECK();
}

void frame_unpack_batch(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, bool in_bytes,
                        const long long* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                        size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                        int32_t* corrected, long long* fields, hipStream_t s) {
  const bool header = fields != nullptr;
  frame_counts(nframes, info_len, header);
  const size_t framed = info_len + frame::crc_len(sch.crc);
  if (in_stride > kFrameMaxRow * 8 || in_stride < (in_bytes ? framed : framed * 8))
    throw std::invalid_argument("frame unpack: a row holds at least the framed block, at most 2^27 elements");
  if (n_inner > kFrameMaxRow || n_outer > kFrameMaxRow)
    throw std::invalid_argument("frame unpack: at most 2^24 words per frame");
  FrameGeom g = frame_geom(sch, info_len, header, in_bytes, in_stride);
  g.n_inner = static_cast<uint32_t>(n_inner);
  g.n_outer = static_cast<uint32_t>(n_outer);
  if (nframes == 0) return;
  k_frame_unpack<<<frame_grid(nframes), 64 * kFrameWaves, 0, s>>>(in, seeds, unsat, status,
                                                                  static_cast<long long>(nframes), g, payload, flags,
                                                                  corrected, fields);
  ORION_LAUNCH_CHECK();
}

void frame_coded_bits_batch(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, size_t nbits,
                            const long long* seeds, size_t nframes, size_t out_len, uint8_t* out, hipStream_t s) {
  const RowGeom g = row_geom(sch, in_stride, nbits, out_len, nframes);
  if (nframes == 0 || out_len == 0) return;
  k_frame_coded_bits<<<frame_grid(nframes), 64 * kFrameWaves, 0, s>>>(in, seeds, static_cast<long long>(nframes), g,
                                                                      out);
  ORION_LAUNCH_CHECK();
}

void frame_llr_prepare_batch(const frame::Scheme& sch, const float* in, size_t in_stride, size_t n,
                             const long long* seeds, size_t nframes, float* out, hipStream_t s) {
  const RowGeom g = row_geom(sch, in_stride, n, n, nframes);
  if (nframes == 0 || n == 0) return;
  if (reinterpret_cast<uintptr_t>(in) % 4 || reinterpret_cast<uintptr_t>(out) % 4)
    throw std::invalid_argument("frame llr prepare: rows not 4-byte aligned");
  k_frame_llr_prepare<<<frame_grid(nframes), 64 * kFrameWaves, 0, s>>>(
      reinterpret_cast<const uint32_t*>(in), seeds, static_cast<long long>(nframes), g,
      reinterpret_cast<uint32_t*>(out));
  ORION_LAUNCH_CHECK();
}

void frame_bytes_to_bits_batch(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out, hipStream_t s) {
  if (nframes > kFrameMaxFrames || nbytes > kFrameMaxRow || nframes * nbytes > (size_t(1) << 36))
    throw std::invalid_argument("frame: nframes above 2^24, rows above 2^24 bytes or more than 2^36 bytes");
  const size_t total = nframes * nbytes * 8;
  if (total == 0) return;
  k_frame_bytes_to_bits<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(in, static_cast<long long>(total),
                                                                                   out);
  ORION_LAUNCH_CHECK();
}

void frame_assemble_batch(const float* lead, size_t lead_len, const float* hdr, size_t hdr_len, const float* pay,
                          size_t pay_len, size_t nframes, size_t sps, size_t win_start, const float* ramp,
                          size_t ramp_len, float* out, hipStream_t s) {
  const size_t frame_len = lead_len + hdr_len + pay_len;
  if (nframes > kFrameMaxFrames || frame_len > kFrameMaxRow || nframes * frame_len > (size_t(1) << 36))
    throw std::invalid_argument("frame assemble: nframes above 2^24, frames above 2^24 samples or 2^36 in all");
  if (ramp_len && (sps == 0 || 2 * ramp_len > sps || win_start > frame_len || !ramp))
    throw std::invalid_argument("frame assemble: the ramp is at most half a symbol, the window starts inside the frame");
  if (nframes == 0 || frame_len == 0) return;
  for (const void* p : {static_cast<const void*>(lead), static_cast<const void*>(hdr), static_cast<const void*>(pay),
                        static_cast<const void*>(out)})
    if (reinterpret_cast<uintptr_t>(p) % 8) throw std::invalid_argument("frame assemble: IQ not 8-byte aligned");
  AssembleGeom g{static_cast<uint32_t>(lead_len), static_cast<uint32_t>(hdr_len),   static_cast<uint32_t>(pay_len),
                 static_cast<uint32_t>(frame_len), static_cast<uint32_t>(sps ? sps : 1), static_cast<uint32_t>(win_start),
                 static_cast<uint32_t>(ramp_len)};
  const size_t total = nframes * frame_len;
  k_frame_assemble<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(
      reinterpret_cast<const float2*>(lead), reinterpret_cast<const float2*>(hdr), reinterpret_cast<const float2*>(pay),
      ramp, static_cast<long long>(total), g, reinterpret_cast<float2*>(out));
  ORION_LAUNCH_CHECK();
}

// ---- host-memory variants: copy in, one launch, copy out --------------------------------------
void frame_pack_batch_host(const frame::Scheme& sch, const uint8_t* payload, const long long* fields,
                           const long long* seeds, size_t nframes, size_t info_len, bool out_bytes, uint8_t* out) {
  frame_counts(nframes, info_len, fields != nullptr);
  const size_t framed = info_len + frame::crc_len(sch.crc), ob = nframes * framed * (out_bytes ? 1 : 8);
  if (nframes == 0) return;
  StagedIn d_pay(fields ? nullptr : payload, fields ? 0 : nframes * info_len), d_f(fields, fields ? nframes * 40 : 0),
      d_s(seeds, seeds ? nframes * 8 : 0);
  DevBuf d_out(ob + 16);
  frame_pack_batch(sch, d_pay.as<uint8_t>(), d_f.opt<long long>(), d_s.opt<long long>(), nframes, info_len, out_bytes,
                   d_out.as<uint8_t>(), nullptr);
  stage_out(out, d_out, ob);
  ORION_HIP(hipDeviceSynchronize());
}

void frame_unpack_batch_host(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, bool in_bytes,
                             const long long* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                             size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                             int32_t* corrected, long long* fields) {
  frame_counts(nframes, info_len, fields != nullptr);
  const size_t framed = info_len + frame::crc_len(sch.crc);
  if (in_stride > kFrameMaxRow * 8 || in_stride < (in_bytes ? framed : framed * 8) || n_inner > kFrameMaxRow ||
      n_outer > kFrameMaxRow)
    throw std::invalid_argument("frame unpack: a row holds the framed block and at most 2^27 elements, at most 2^24 words per frame");
  if (nframes == 0) return;
  StagedIn d_in(in, nframes * in_stride), d_s(seeds, seeds ? nframes * 8 : 0),
      d_u(unsat, unsat ? nframes * n_inner * 4 : 0), d_st(status, status ? nframes * n_outer * 4 : 0);
  DevBuf d_pay(nframes * info_len + 16), d_fl(nframes * 4 + 16), d_c(nframes * 4 + 16), d_f(nframes * 40 + 16);
  frame_unpack_batch(sch, d_in.as<uint8_t>(), in_stride, in_bytes, d_s.opt<long long>(), d_u.opt<int32_t>(), n_inner,
                     d_st.opt<int32_t>(), n_outer, nframes, info_len, d_pay.as<uint8_t>(), d_fl.as<uint8_t>(),
                     d_c.as<int32_t>(), fields ? d_f.as<long long>() : nullptr, nullptr);
  stage_out(payload, d_pay, nframes * info_len);
  stage_out(flags, d_fl, nframes * 4);
  stage_out(corrected, d_c, nframes * 4);
  stage_out(fields, d_f, nframes * 40);
  ORION_HIP(hipDeviceSynchronize());
}

void frame_coded_bits_batch_host(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, size_t nbits,
                                 const long long* seeds, size_t nframes, size_t out_len, uint8_t* out) {
  row_geom(sch, in_stride, nbits, out_len, nframes);
  if (nframes == 0) return;
  StagedIn d_in(in, nframes * in_stride), d_s(seeds, seeds ? nframes * 8 : 0);
  DevBuf d_out(nframes * out_len + 16);
  frame_coded_bits_batch(sch, d_in.as<uint8_t>(), in_stride, nbits, d_s.opt<long long>(), nframes, out_len,
                         d_out.as<uint8_t>(), nullptr);
  stage_out(out, d_out, nframes * out_len);
  ORION_HIP(hipDeviceSynchronize());
}

void frame_llr_prepare_batch_host(const frame::Scheme& sch, const float* in, size_t in_stride, size_t n,
                                  const long long* seeds, size_t nframes, float* out) {
  row_geom(sch, in_stride, n, n, nframes);
  if (nframes == 0) return;
  StagedIn d_in(in, nframes * in_stride * 4), d_s(seeds, seeds ? nframes * 8 : 0);
  DevBuf d_out(nframes * n * 4 + 16);
  frame_llr_prepare_batch(sch, d_in.as<float>(), in_stride, n, d_s.opt<long long>(), nframes, d_out.as<float>(),
                          nullptr);
  stage_out(out, d_out, nframes * n * 4);
  ORION_HIP(hipDeviceSynchronize());
}

void frame_bytes_to_bits_batch_host(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out) {
  if (nframes > kFrameMaxFrames || nbytes > kFrameMaxRow || nframes * nbytes > (size_t(1) << 36))
    throw std::invalid_argument("frame: nframes above 2^24, rows above 2^24 bytes or more than 2^36 bytes");
  if (nframes * nbytes == 0) return;
  StagedIn d_in(in, nframes * nbytes);
  DevBuf d_out(nframes * nbytes * 8 + 16);
  frame_bytes_to_bits_batch(d_in.as<uint8_t>(), nframes, nbytes, d_out.as<uint8_t>(), nullptr);
  stage_out(out, d_out, nframes * nbytes * 8);
  ORION_HIP(hipDeviceSynchronize());
}

}  // namespace orion
