// frame.cpp — the coding chain of the COFDM frame layer on the host (frame.hpp).
#include "frame.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "bch.hpp"
#include "fec.hpp"
#include "ldpc_family.hpp"
#include "rs.hpp"

namespace orion {
namespace frame {

namespace {
size_t round_up(size_t n, size_t block) { return block == 0 ? n : (n + block - 1) / block * block; }
size_t div_ceil(size_t n, size_t d) { return (n + d - 1) / d; }

void check_il(int kind, uint32_t a, uint32_t b, const char* what) {
  if (kind == kIlNone) return;
  if (kind == kIlBlock) {
    fec::BlockInterleaver(a, b);
    return;
  }
  if (kind == kIlForney) {
    rs::conv_roundtrip_delay(a, b);
    return;
  }
  throw std::invalid_argument(std::string(what) + ": unknown interleaver kind");
}

// pack_bits_padded: MSB first, the last partial byte zero-padded
std::vector<uint8_t> pack_bits_padded(const uint8_t* bits, size_t n) {
  std::vector<uint8_t> padded(round_up(n, 8), 0), bytes(div_ceil(n, 8));
  std::copy(bits, bits + n, padded.begin());
  rs::bits_to_bytes(padded.data(), bytes.size(), bytes.data());
  return bytes;
}

// interleave_bits, modulate/ofdm_frame.rs:445-480
std::vector<uint8_t> interleave_bits(int kind, uint32_t a, uint32_t b, const std::vector<uint8_t>& bits) {
  if (kind == kIlBlock) return fec::BlockInterleaver(a, b).interleave_bits(bits.data(), bits.size());
  if (kind == kIlForney) {
    const std::vector<uint8_t> bytes = pack_bits_padded(bits.data(), bits.size());
    const std::vector<uint8_t> il = rs::forney_frame_interleave(a, b, bytes.data(), bytes.size());
    std::vector<uint8_t> out(il.size() * 8);
    rs::bytes_to_bits(il.data(), il.size(), out.data());
    return out;
  }
  return bits;
}

// deinterleave_bits, demodulate/ofdm_frame.rs:381-417: a short last block passes through
std::vector<uint8_t> deinterleave_bits(int kind, uint32_t a, uint32_t b, const uint8_t* bits, size_t n) {
  if (kind == kIlBlock) {
    const fec::BlockInterleaver bi(a, b);
    const size_t block = bi.block_len();
    std::vector<uint8_t> out(n);
    size_t at = 0;
    for (; at + block <= n; at += block) bi.deinterleave(bits + at, out.data() + at);
    for (; at < n; ++at) out[at] = bits[at];
    return out;
  }
  if (kind == kIlForney) {
    const size_t total = n / 8;
    std::vector<uint8_t> bytes(total);
    rs::bits_to_bytes(bits, total, bytes.data());
    const std::vector<uint8_t> de = rs::forney_frame_deinterleave(a, b, bytes.data(), total);
    std::vector<uint8_t> out(de.size() * 8);
    rs::bytes_to_bits(de.data(), de.size(), out.data());
    return out;
  }
  return std::vector<uint8_t>(bits, bits + n);
}

// the Additive scrambler's PN bytes (what scramble XORs onto zeros)
std::vector<uint8_t> pn_bytes(const Scheme& s, uint32_t per_frame_seed, size_t n) {
  std::vector<uint8_t> pn(n, 0);
  rs::PnScrambler(s.scr_poly, s.scr_width, scheme_seed(s, per_frame_seed)).scramble(pn.data(), n);
  return pn;
}
}  // namespace

void check_scheme(const Scheme& s) {
  crc_len(s.crc);
  if (s.outer == kOuterBch)
    bch::Bch::for_info_bits(s.outer_a, kBchInfoBits);
  else if (s.outer == kOuterRs)
    rs::ReedSolomon(s.outer_a, s.outer_b);
  else if (s.outer != kOuterNone)
    throw std::invalid_argument("frame: unknown outer FEC");
  if (s.inner == kInnerLdpc)
    ldpcf::Ldpc::get(static_cast<int>(s.inner_a));
  else if (s.inner == kInnerConv) {
    fec::code_spec(static_cast<int>(s.inner_a));
    fec::rate_spec(static_cast<int>(s.inner_b));
  } else if (s.inner != kInnerNone)
    throw std::invalid_argument("frame: unknown inner FEC");
  check_il(s.outer_il, s.outer_il_a, s.outer_il_b, "outer interleaver");
  check_il(s.inner_il, s.inner_il_a, s.inner_il_b, "inner interleaver");
  if (s.scrambler == kScrAdditive)
    rs::PnScramblerStream(s.scr_poly, s.scr_width, reduce_seed(s.scr_width, s.scr_seed));
  else if (s.scrambler != kScrNone && s.scrambler != kScrDvbT)
    throw std::invalid_argument("frame: unknown scrambler kind");
  if (s.scrambler_pos != kBeforeOuterFec && s.scrambler_pos != kAfterInnerFec)
    throw std::invalid_argument("frame: unknown scrambler position");
}

// ---- CRCs ----------------------------------------------------------------------------------
uint16_t crc16(const uint8_t* bytes, size_t n) {
  uint16_t crc = 0xFFFF;
  for (size_t i = 0; i < n; ++i) {
    crc = static_cast<uint16_t>(crc ^ (static_cast<uint16_t>(bytes[i]) << 8));
    for (int b = 0; b < 8; ++b)
      crc = crc & 0x8000 ? static_cast<uint16_t>((crc << 1) ^ 0x1021) : static_cast<uint16_t>(crc << 1);
  }
  return crc;
}

uint32_t crc32(const uint8_t* bytes, size_t n) {
  uint32_t crc = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    crc ^= bytes[i];
    for (int b = 0; b < 8; ++b) crc = crc & 1u ? (crc >> 1) ^ 0xEDB88320u : crc >> 1;
  }
  return crc ^ 0xFFFFFFFFu;
}

size_t crc_len(int crc) {
  if (crc == kCrcNone) return 0;
  if (crc == kCrc16) return 2;
  if (crc == kCrc32) return 4;
  throw std::invalid_argument("frame: unknown CRC kind");
}

std::vector<uint8_t> append_crc(int crc, const uint8_t* data, size_t n) {
  const size_t clen = crc_len(crc);
  std::vector<uint8_t> out(n + clen);
  std::copy(data, data + n, out.begin());
  const uint32_t v = crc == kCrc16 ? crc16(data, n) : crc == kCrc32 ? crc32(data, n) : 0u;
  for (size_t i = 0; i < clen; ++i) out[n + i] = static_cast<uint8_t>(v >> (8 * (clen - 1 - i)));
  return out;
}

bool check_crc(int crc, const uint8_t* data, size_t n) {
  const size_t clen = crc_len(crc);
  if (n < clen) throw std::invalid_argument("frame: data shorter than its CRC field");
  const std::vector<uint8_t> again = append_crc(crc, data, n - clen);
  return std::equal(again.begin() + static_cast<std::ptrdiff_t>(n - clen), again.end(), data + (n - clen));
}

// ---- header fields -------------------------------------------------------------------------
void pack_header_fields(const HeaderFields& f, uint8_t out[kHeaderFieldBytes]) {
  if (f.mcs_index > 255 || f.flags > 255) throw std::invalid_argument("frame header: mcs_index and flags are bytes");
  out[0] = static_cast<uint8_t>(f.mcs_index);
  out[9] = static_cast<uint8_t>(f.flags);
  for (int i = 0; i < 4; ++i) {
    out[1 + i] = static_cast<uint8_t>(f.payload_len >> (24 - 8 * i));
    out[5 + i] = static_cast<uint8_t>(f.sequence_num >> (24 - 8 * i));
    out[10 + i] = static_cast<uint8_t>(f.scrambler_seed >> (24 - 8 * i));
  }
}

HeaderFields unpack_header_fields(const uint8_t in[kHeaderFieldBytes]) {
  auto be = [&](int at) {
    return static_cast<uint32_t>(in[at]) << 24 | static_cast<uint32_t>(in[at + 1]) << 16 |
           static_cast<uint32_t>(in[at + 2]) << 8 | in[at + 3];
  };
  return HeaderFields{in[0], be(1), be(5), in[9], be(10)};
}

// ---- scramblers ----------------------------------------------------------------------------
uint32_t reduce_seed(uint32_t width, uint32_t raw) {
  const uint32_t mask = width >= 32 ? 0xFFFFFFFFu : (1u << width) - 1u;
  const uint32_t m = raw & mask;
  return m == 0 ? 1u : m;
}

uint32_t scheme_seed(const Scheme& s, uint32_t per_frame_seed) {
  return reduce_seed(s.scr_width, s.scr_per_frame ? per_frame_seed : s.scr_seed);
}

void scramble_bytes(const Scheme& s, uint32_t per_frame_seed, uint8_t* bytes, size_t n) {
  if (s.scrambler == kScrDvbT)
    rs::DvbTEnergyDispersal().feed_in_place(bytes, n);
  else if (s.scrambler == kScrAdditive)
    rs::PnScrambler(s.scr_poly, s.scr_width, scheme_seed(s, per_frame_seed)).scramble(bytes, n);
}

void scramble_bits(const Scheme& s, uint32_t per_frame_seed, uint8_t* bits, size_t n) {
  if (s.scrambler != kScrAdditive) return;
  const std::vector<uint8_t> pn = pn_bytes(s, per_frame_seed, div_ceil(n, 8));
  for (size_t i = 0; i < n; ++i) bits[i] = static_cast<uint8_t>((bits[i] & 1u) ^ ((pn[i / 8] >> (7 - i % 8)) & 1u));
}

void apply_pn_to_llrs(const Scheme& s, uint32_t per_frame_seed, float* llr, size_t n) {
  if (s.scrambler != kScrAdditive) return;
  const std::vector<uint8_t> pn = pn_bytes(s, per_frame_seed, div_ceil(n, 8));
  for (size_t i = 0; i < n; ++i) {
    if (!((pn[i / 8] >> (7 - i % 8)) & 1u)) continue;
    uint32_t u;
    std::memcpy(&u, llr + i, 4);
    u ^= 0x80000000u;  // -x: the sign bit and nothing else, NaN included
    std::memcpy(llr + i, &u, 4);
  }
}

// ---- block accounting ----------------------------------------------------------------------
BlockPlan block_plan(size_t info_bytes, const Scheme& s) {
  check_scheme(s);
  if (info_bytes > kMaxInfoBytes) throw std::invalid_argument("frame: a block is at most 2^24 bytes");
  BlockPlan p{};
  p.info_bytes = info_bytes;
  p.framed_bytes = info_bytes + crc_len(s.crc);
  const size_t framed_bits = p.framed_bytes * 8;
  if (s.outer == kOuterBch) {
    const bch::Bch code = bch::Bch::for_info_bits(s.outer_a, kBchInfoBits);
    p.outer_coded_bits = div_ceil(framed_bits, kBchInfoBits) * code.n();
  } else if (s.outer == kOuterRs) {
    const rs::ReedSolomon code(s.outer_a, s.outer_b);
    if (code.k() == 0) throw std::invalid_argument("frame: the Reed-Solomon code carries no message");
    p.outer_coded_bits = div_ceil(p.framed_bytes, code.k()) * code.n() * 8;
  } else {
    p.outer_coded_bits = framed_bits;
  }
  auto after_il = [](int kind, uint32_t a, uint32_t b, size_t bits) {
    if (kind == kIlBlock) return round_up(bits, static_cast<size_t>(a) * b);
    if (kind == kIlForney) return (round_up(div_ceil(bits, 8), a) + rs::conv_roundtrip_delay(a, b)) * 8;
    return bits;
  };
  p.outer_il_bits = after_il(s.outer_il, s.outer_il_a, s.outer_il_b, p.outer_coded_bits);
  if (s.inner == kInnerLdpc) {
    const ldpcf::Ldpc& c = ldpcf::Ldpc::get(static_cast<int>(s.inner_a));
    p.inner_coded_bits = div_ceil(p.outer_il_bits, c.k()) * c.n();
  } else if (s.inner == kInnerConv) {
    p.inner_coded_bits =
        fec::punctured_coded_len(static_cast<int>(s.inner_a), p.outer_il_bits, static_cast<int>(s.inner_b));
  } else {
    p.inner_coded_bits = p.outer_il_bits;
  }
  p.coded_bits = after_il(s.inner_il, s.inner_il_a, s.inner_il_b, p.inner_coded_bits);
  return p;
}

// ---- encode --------------------------------------------------------------------------------
EncodedStages encode_chain_stages(const uint8_t* bytes, size_t n, const Scheme& s, uint32_t per_frame_seed) {
  const BlockPlan plan = block_plan(n, s);
  std::vector<uint8_t> framed = append_crc(s.crc, bytes, n);
  if (s.scrambler_pos == kBeforeOuterFec) scramble_bytes(s, per_frame_seed, framed.data(), framed.size());

  // outer_encode
  std::vector<uint8_t> outer_bits(plan.outer_coded_bits);
  if (s.outer == kOuterBch) {
    std::vector<uint8_t> msg_bits(framed.size() * 8);
    rs::bytes_to_bits(framed.data(), framed.size(), msg_bits.data());
    const bch::Bch code = bch::Bch::for_info_bits(s.outer_a, kBchInfoBits);
    bch::encode_stream(code, msg_bits.data(), msg_bits.size(), outer_bits.data());
  } else if (s.outer == kOuterRs) {
    const rs::ReedSolomon code(s.outer_a, s.outer_b);
    const size_t k = code.k(), nb = div_ceil(framed.size(), k);
    std::vector<uint8_t> block(k), out_bytes(nb * code.n());
    for (size_t w = 0; w < nb; ++w) {
      const size_t len = std::min(k, framed.size() - w * k);
      std::copy(framed.begin() + static_cast<std::ptrdiff_t>(w * k),
                framed.begin() + static_cast<std::ptrdiff_t>(w * k + len), block.begin());
      std::fill(block.begin() + static_cast<std::ptrdiff_t>(len), block.end(), 0);
      code.encode(block.data(), out_bytes.data() + w * code.n());
    }
    rs::bytes_to_bits(out_bytes.data(), out_bytes.size(), outer_bits.data());
  } else {
    rs::bytes_to_bits(framed.data(), framed.size(), outer_bits.data());
  }

  EncodedStages st;
  st.outer_il_bits = interleave_bits(s.outer_il, s.outer_il_a, s.outer_il_b, outer_bits);

  // inner_encode
  std::vector<uint8_t> inner_bits(plan.inner_coded_bits);
  if (s.inner == kInnerLdpc) {
    ldpcf::encode_stream(static_cast<int>(s.inner_a), st.outer_il_bits.data(), st.outer_il_bits.size(),
                         inner_bits.data());
  } else if (s.inner == kInnerConv) {
    fec::conv_encode_punctured(static_cast<int>(s.inner_a), st.outer_il_bits.data(), st.outer_il_bits.size(),
                               static_cast<int>(s.inner_b), inner_bits.data());
  } else {
    inner_bits = st.outer_il_bits;
  }
  st.coded = interleave_bits(s.inner_il, s.inner_il_a, s.inner_il_b, inner_bits);
  if (s.scrambler_pos == kAfterInnerFec) scramble_bits(s, per_frame_seed, st.coded.data(), st.coded.size());
  return st;
}

// ---- decode --------------------------------------------------------------------------------
ChainOutcome decode_chain(const float* coded_llrs, size_t n_llr, const BlockPlan& plan, const Scheme& s,
                          uint32_t per_frame_seed, int ldpc_rule, float ldpc_scale) {
  check_scheme(s);
  if (s.inner == kInnerLdpc) ldpcf::check_rule(ldpc_rule);
  // 1. trim, undo the after-inner scramble
  std::vector<float> llrs(coded_llrs, coded_llrs + std::min(n_llr, plan.coded_bits));
  if (s.scrambler_pos == kAfterInnerFec) apply_pn_to_llrs(s, per_frame_seed, llrs.data(), llrs.size());

  // 2. inner deinterleave and decode (a Forney kind in the LLR domain passes through)
  if (s.inner_il == kIlBlock)
    llrs = fec::BlockInterleaver(s.inner_il_a, s.inner_il_b).deinterleave_llrs(llrs.data(), llrs.size());
  const size_t n_in = std::min(plan.inner_coded_bits, llrs.size());
  ChainOutcome o;
  o.inner_ok = true;
  if (s.inner == kInnerLdpc) {
    const ldpcf::Ldpc& c = ldpcf::Ldpc::get(static_cast<int>(s.inner_a));
    const size_t nb = n_in / c.n();
    if (n_in % c.n()) o.inner_ok = false;  // a short last chunk ends the loop
    o.inner_out_bits.resize(nb * c.k());
    for (size_t w = 0; w < nb; ++w) {
      const ldpcf::DecodeResult r = c.decode_soft(llrs.data() + w * c.n(), ldpcf::kDefaultMaxIter, ldpc_rule,
                                                  ldpc_scale, o.inner_out_bits.data() + w * c.k());
      if (r.unsat != 0) o.inner_ok = false;
    }
  } else if (s.inner == kInnerConv) {
    o.inner_out_bits.resize(plan.outer_il_bits);
    fec::viterbi_decode_soft(static_cast<int>(s.inner_a), llrs.data(), n_in, plan.outer_il_bits,
                             static_cast<int>(s.inner_b), o.inner_out_bits.data());
  } else {
    o.inner_out_bits.resize(n_in);
    for (size_t i = 0; i < n_in; ++i) o.inner_out_bits[i] = llrs[i] <= 0.0f ? 1 : 0;
  }

  // 3. outer deinterleave and decode over what the plan says is there
  const size_t n_il = std::min(plan.outer_il_bits, o.inner_out_bits.size());
  std::vector<uint8_t> outer_de = deinterleave_bits(s.outer_il, s.outer_il_a, s.outer_il_b, o.inner_out_bits.data(), n_il);
  if (outer_de.size() > plan.outer_coded_bits) outer_de.resize(plan.outer_coded_bits);
  std::vector<uint8_t> framed_bits;
  o.outer_ok = true;
  if (s.outer == kOuterBch) {
    const bch::Bch code = bch::Bch::for_info_bits(s.outer_a, kBchInfoBits);
    const size_t nb = outer_de.size() / code.n();
    if (outer_de.size() % code.n()) o.outer_ok = false;
    framed_bits.resize(nb * code.k());
    for (size_t w = 0; w < nb; ++w)
      if (code.decode(outer_de.data() + w * code.n(), framed_bits.data() + w * code.k()) < 0) o.outer_ok = false;
  } else if (s.outer == kOuterRs) {
    if (outer_de.size() % 8) throw std::invalid_argument("frame: bit count must be a whole number of bytes");
    const rs::ReedSolomon code(s.outer_a, s.outer_b);
    std::vector<uint8_t> coded_bytes(outer_de.size() / 8);
    rs::bits_to_bytes(outer_de.data(), coded_bytes.size(), coded_bytes.data());
    const size_t nb = coded_bytes.size() / code.n();
    if (coded_bytes.size() % code.n()) o.outer_ok = false;
    std::vector<uint8_t> msg(nb * code.k());
    o.outer_corrected_bytes = 0;
    for (size_t w = 0; w < nb; ++w) {
      const int fixed = code.decode_counted(coded_bytes.data() + w * code.n(), msg.data() + w * code.k());
      if (fixed < 0)
        o.outer_ok = false;
      else
        o.outer_corrected_bytes += fixed;
    }
    framed_bits.resize(msg.size() * 8);
    rs::bytes_to_bits(msg.data(), msg.size(), framed_bits.data());
  } else {
    framed_bits = outer_de;
  }
  if (framed_bits.size() < plan.framed_bytes * 8) {
    ChainOutcome bad;
    bad.error = kRxMalformedHeader;
    return bad;
  }
  std::vector<uint8_t> framed(plan.framed_bytes);
  rs::bits_to_bytes(framed_bits.data(), framed.size(), framed.data());

  // 4. undo the before-outer scramble, 5. check and strip the CRC
  if (s.scrambler_pos == kBeforeOuterFec) scramble_bytes(s, per_frame_seed, framed.data(), framed.size());
  const size_t clen = crc_len(s.crc);
  if (framed.size() < clen) {
    ChainOutcome bad;
    bad.error = kRxMalformedHeader;
    return bad;
  }
  o.crc_ok = check_crc(s.crc, framed.data(), framed.size());
  o.bytes.assign(framed.begin(), framed.end() - static_cast<std::ptrdiff_t>(clen));
  o.crc_present = s.crc != kCrcNone;
  o.outer_present = s.outer != kOuterNone;
  return o;
}

// ---- GF(2) maps ----------------------------------------------------------------------------
BitMatrix bitmatrix_identity() {
  BitMatrix m{};
  for (int i = 0; i < 32; ++i) m.col[i] = 1u << i;
  return m;
}
uint32_t bitmatrix_apply(const BitMatrix& a, uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i)
    if ((v >> i) & 1u) r ^= a.col[i];
  return r;
}
BitMatrix bitmatrix_mul(const BitMatrix& a, const BitMatrix& b) {
  BitMatrix m{};
  for (int i = 0; i < 32; ++i) m.col[i] = bitmatrix_apply(a, b.col[i]);
  return m;
}
BitMatrix bitmatrix_pow(BitMatrix a, uint64_t e) {
  BitMatrix r = bitmatrix_identity();
  for (; e; e >>= 1) {
    if (e & 1u) r = bitmatrix_mul(a, r);
    a = bitmatrix_mul(a, a);
  }
  return r;
}
BitMatrix crc_byte_map(int crc) {
  BitMatrix m{};
  if (crc == kCrc16) {
    for (int i = 0; i < 16; ++i) {
      uint32_t v = 1u << i;
      for (int b = 0; b < 8; ++b) v = (v & 0x8000u ? (v << 1) ^ 0x1021u : v << 1) & 0xFFFFu;
      m.col[i] = v;
    }
  } else if (crc == kCrc32) {
    for (int i = 0; i < 32; ++i) {
      uint32_t v = 1u << i;
      for (int b = 0; b < 8; ++b) v = v & 1u ? (v >> 1) ^ 0xEDB88320u : v >> 1;
      m.col[i] = v;
    }
  } else {
    crc_len(crc);
  }
  return m;
}
BitMatrix lfsr_step_map(uint32_t taps, uint32_t width) {
  if (width < 2 || width > 32) throw std::invalid_argument("LFSR width must be in 2..=32");
  const uint32_t mask = width == 32 ? 0xFFFFFFFFu : (1u << width) - 1u;
  BitMatrix m{};
  for (uint32_t i = 0; i < width; ++i) {
    const uint32_t v = 1u << i;
    const uint32_t fb = static_cast<uint32_t>(__builtin_popcount(v & taps)) & 1u;
    m.col[i] = ((v >> 1) | (fb << (width - 1))) & mask;
  }
  return m;
}

}  // namespace frame
}  // namespace orion
