// frame.hpp — the coding chain of the COFDM frame layer, host side (no device): the frame CRCs
// (codec/crc.rs:89-130), the bit/byte and header-field helpers, the scrambler drivers, the
// block accounting and the concatenated chain itself, encode_chain / decode_chain
// (modulate/ofdm_frame.rs:204-682, demodulate/ofdm_frame.rs:351-779), over the codes of
// fec.hpp, rs.hpp, bch.hpp and ldpc_family.hpp. k_frame.hip's kernels are held to these
// functions byte for byte.
//
//   payload -> CRC -> [scramble] -> outer FEC -> outer interleave -> inner FEC ->
//              inner interleave -> [scramble] -> coded bits          (reversed on receive)
//
// Bits are uint8, one per byte, MSB first within a byte. Everything here throws
// std::invalid_argument on a bad argument.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orion {
namespace frame {

enum Crc : int { kCrcNone = 0, kCrc16 = 1, kCrc32 = 2 };
enum Outer : int { kOuterNone = 0, kOuterBch = 1, kOuterRs = 2 };
enum Inner : int { kInnerNone = 0, kInnerLdpc = 1, kInnerConv = 2 };
enum Interleaver : int { kIlNone = 0, kIlBlock = 1, kIlForney = 2 };
enum Scrambler : int { kScrNone = 0, kScrAdditive = 1, kScrDvbT = 2 };
enum ScramblerPos : int { kBeforeOuterFec = 0, kAfterInnerFec = 1 };
// RxError (fec/frame.rs:59-77); 0 is "no error"
enum RxError : int {
  kRxOk = 0,
  kRxPreambleTimeout = 1,
  kRxMalformedHeader = 2,
  kRxHeaderCrcMismatch = 3,
  kRxCrcMismatch = 4,
  kRxFecUncorrectable = 5
};

constexpr size_t kHeaderFieldBytes = 14;  // HEADER_FIELD_BYTES
constexpr size_t kBchInfoBits = 120;      // BCH_INFO_BITS
constexpr size_t kMaxInfoBytes = size_t(1) << 24;

// One logical block's coding chain: what encode_chain's arguments after the bytes say.
struct Scheme {
  int crc = kCrc32;
  int outer = kOuterNone;
  uint32_t outer_a = 0, outer_b = 0;  // Bch: t, -; ReedSolomon: n, n_parity
  int inner = kInnerNone;
  uint32_t inner_a = 0, inner_b = 0;  // Ldpc: ldpcf code, -; Convolutional: fec::Code, fec::Rate
  int outer_il = kIlNone;
  uint32_t outer_il_a = 0, outer_il_b = 0;  // Block: rows, cols; Forney: branches, depth
  int inner_il = kIlNone;
  uint32_t inner_il_a = 0, inner_il_b = 0;
  int scrambler = kScrNone;
  uint32_t scr_poly = 0, scr_width = 0;
  int scr_per_frame = 0;   // SeedMode::PerFrameRandom: the seed is the call's per_frame_seed
  uint32_t scr_seed = 0;   // SeedMode::Fixed
  int scrambler_pos = kBeforeOuterFec;
};
void check_scheme(const Scheme& s);

// ---- CRCs ----------------------------------------------------------------------------------
uint16_t crc16(const uint8_t* bytes, size_t n);  // CCITT-FALSE: 0x1021, init 0xFFFF
uint32_t crc32(const uint8_t* bytes, size_t n);  // ISO-HDLC: 0xEDB88320 reflected, init and final 0xFFFFFFFF
size_t crc_len(int crc);                          // 0, 2, 4; throws on an unknown kind
std::vector<uint8_t> append_crc(int crc, const uint8_t* data, size_t n);  // big-endian
// data = payload | crc: true when it checks (vacuously for kCrcNone). Throws when n < crc_len.
bool check_crc(int crc, const uint8_t* data, size_t n);

// ---- header fields: mcs (1) | payload_len (4, BE) | sequence_num (4) | flags (1) | seed (4) --
struct HeaderFields {
  uint32_t mcs_index, payload_len, sequence_num, flags, scrambler_seed;
};
void pack_header_fields(const HeaderFields& f, uint8_t out[kHeaderFieldBytes]);
HeaderFields unpack_header_fields(const uint8_t in[kHeaderFieldBytes]);

// ---- scramblers ----------------------------------------------------------------------------
// build_scrambler's seed: raw reduced to width bits (all 32 when width >= 32), 0 mapped to 1
uint32_t reduce_seed(uint32_t width, uint32_t raw);
// the seed a scheme's Additive scrambler starts a block from
uint32_t scheme_seed(const Scheme& s, uint32_t per_frame_seed);
// scramble_bytes: self-inverse, in place; Additive (LSB first) or DVB-T dispersal (MSB first)
void scramble_bytes(const Scheme& s, uint32_t per_frame_seed, uint8_t* bytes, size_t n);
// scramble_bits (Additive only, otherwise a no-op): packed MSB first, the PN applied LSB first
// within each byte, so bit i meets PN step 8 (i / 8) + 7 - i % 8
void scramble_bits(const Scheme& s, uint32_t per_frame_seed, uint8_t* bits, size_t n);
// apply_pn_to_llrs: the sign bit of llr[i] flipped where scramble_bits would flip bit i
void apply_pn_to_llrs(const Scheme& s, uint32_t per_frame_seed, float* llr, size_t n);

// ---- block accounting ----------------------------------------------------------------------
struct BlockPlan {
  size_t info_bytes, framed_bytes, outer_coded_bits, outer_il_bits, inner_coded_bits, coded_bits;
};
BlockPlan block_plan(size_t info_bytes, const Scheme& s);
inline size_t symbols_for_coded_bits(size_t n_data_carriers, size_t bits_per_carrier, size_t bits) {
  const size_t bps = n_data_carriers * bits_per_carrier;
  return bps ? (bits + bps - 1) / bps : 0;
}

// ---- the chain -----------------------------------------------------------------------------
struct EncodedStages {
  std::vector<uint8_t> outer_il_bits, coded;
};
EncodedStages encode_chain_stages(const uint8_t* bytes, size_t n, const Scheme& s, uint32_t per_frame_seed);
inline std::vector<uint8_t> encode_chain(const uint8_t* bytes, size_t n, const Scheme& s, uint32_t per_frame_seed) {
  return encode_chain_stages(bytes, n, s, per_frame_seed).coded;
}

struct ChainOutcome {
  int error = kRxOk;  // kRxMalformedHeader: too few bits came out of the decoders; nothing else is set
  std::vector<uint8_t> bytes;
  bool inner_ok = false, outer_ok = false, crc_ok = false, crc_present = false, outer_present = false;
  long long outer_corrected_bytes = -1;  // -1: the outer code reports none (every arm but Reed-Solomon)
  std::vector<uint8_t> inner_out_bits;   // untrimmed
  bool is_valid() const { return crc_present ? crc_ok : outer_present ? outer_ok : inner_ok; }
};
// coded_llrs [n_llr], positive meaning bit 0; LDPC runs 50 iterations under ldpc_rule / scale
ChainOutcome decode_chain(const float* coded_llrs, size_t n_llr, const BlockPlan& plan, const Scheme& s,
                          uint32_t per_frame_seed, int ldpc_rule, float ldpc_scale);

// ---- what k_frame.hip's kernels are given: GF(2) maps as 32 columns -------------------------
// column i of a map is the image of bit i; a map is applied by XORing the columns of the set bits.
struct BitMatrix {
  uint32_t col[32];
};
BitMatrix bitmatrix_identity();
BitMatrix bitmatrix_mul(const BitMatrix& a, const BitMatrix& b);  // a after b
BitMatrix bitmatrix_pow(BitMatrix a, uint64_t e);
uint32_t bitmatrix_apply(const BitMatrix& a, uint32_t v);
// the CRC register (crc16 in the low 16 bits) after one zero data byte, as a map of the register
BitMatrix crc_byte_map(int crc);
// the scrambling register after one step: Additive (taps, width) or DVB-T (taps 3, width 15)
BitMatrix lfsr_step_map(uint32_t taps, uint32_t width);

}  // namespace frame
}  // namespace orion
