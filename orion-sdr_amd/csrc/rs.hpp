// rs.hpp — the outer code of the COFDM / DVB-T chain, host side (no device): GF(2^8)
// arithmetic (fec/gf.rs), the Reed-Solomon code with its counted decoder (fec/reed_solomon.rs;
// DVB-T's RS(204,188)), the Forney convolutional byte interleaver as streaming blocks and in
// frame mode (fec/interleaver.rs:122-305; interleave_bits / deinterleave_bits' Convolutional
// arm, modulate/ofdm_frame.rs:464-478, demodulate/ofdm_frame.rs:399-415), the additive PN
// scrambler (fec/scrambler.rs), the DVB-T energy-dispersal PRBS (waveform/dvb_t.rs:30-110) and
// the transport-stream packet layer (waveform/dvb_t_ts.rs). k_rs.hip's kernels are held to
// these functions byte for byte.
//
// Everything here throws std::invalid_argument on a bad argument (where the reference panics
// or returns an error).
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <vector>

namespace orion {
namespace rs {

// ---- GF(2^8), primitive polynomial 0x11D, generator 2 (gf.rs) -------------------------------
// exp[i] = 2^i over 0..511 (the cycle of 255 repeated, so the sum of two logs needs no
// modulo), log[a] for a in 1..=255 (log[0] is 0 and unused).
struct GfTables {
  uint8_t exp[512];
  uint8_t log[256];
};
constexpr GfTables make_gf_tables() {
  GfTables t{};
  uint32_t x = 1;
  for (int i = 0; i < 255; ++i) {
    t.exp[i] = static_cast<uint8_t>(x);
    t.log[x] = static_cast<uint8_t>(i);
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  for (int i = 255; i < 512; ++i) t.exp[i] = t.exp[i - 255];
  return t;
}

class Gf256 {
 public:
  static const Gf256& shared();
  uint8_t add(uint8_t a, uint8_t b) const { return a ^ b; }
  uint8_t mul(uint8_t a, uint8_t b) const { return a == 0 || b == 0 ? 0 : t_.exp[t_.log[a] + t_.log[b]]; }
  uint8_t div(uint8_t a, uint8_t b) const;  // throws on b == 0
  uint8_t inv(uint8_t a) const;             // throws on a == 0
  // a^n, n reduced modulo 255; 0^0 = 1, 0^n = 0
  uint8_t pow(uint8_t a, size_t n) const {
    if (a == 0) return n == 0 ? 1 : 0;
    return t_.exp[(static_cast<size_t>(t_.log[a]) * (n % 255)) % 255];
  }
  uint8_t exp_of(size_t i) const { return t_.exp[i % 255]; }
  uint8_t log_of(uint8_t a) const;  // throws on a == 0
  const GfTables& tables() const { return t_; }

 private:
  Gf256() : t_(make_gf_tables()) {}
  GfTables t_;
};

// ---- Reed-Solomon over GF(2^8), first consecutive root 0 (reed_solomon.rs) ------------------
// n codeword bytes, k = n - n_parity message bytes, index 0 the highest-degree symbol; a
// shortened code (n < 255) has 255 - n implicit leading zeros. t = n_parity / 2 (floor).
class ReedSolomon {
 public:
  ReedSolomon(size_t n, size_t n_parity);  // 1 <= n <= 255, n_parity < n
  static ReedSolomon dvb() { return ReedSolomon(204, 16); }
  size_t n() const { return n_; }
  size_t k() const { return n_ - np_; }
  size_t t() const { return np_ / 2; }
  size_t parity_bytes() const { return np_; }
  // g(x) = prod (x - 2^i), i < n_parity, low degree first: n_parity + 1 coefficients
  const std::vector<uint8_t>& generator() const { return gen_; }
  // message [k] -> codeword [n] = message | parity. n_parity == 0 throws (the reference's
  // shift register has no cell to write).
  void encode(const uint8_t* message, uint8_t* codeword) const;
  // received [n] -> message [k]; returns the number of codeword bytes the correction changed
  // (parity bytes included), or -1 when the word is uncorrectable, and then message is the
  // systematic prefix received[:k] (the fallback of demodulate/ofdm_frame.rs:531-534).
  // reed_solomon.rs:141-233 step for step: the Chien search runs over all 255 degrees; a root
  // on a never-transmitted degree counts as a root and is not applied; a zero magnitude is not
  // counted; the residual syndromes of the corrected word decide.
  int decode_counted(const uint8_t* received, uint8_t* message) const;

 private:
  size_t n_, np_;
  std::vector<uint8_t> gen_;
};

// ---- the Forney convolutional byte interleaver (interleaver.rs:122-305) ---------------------
// I = branches, M = depth, both nonzero and I * I * M <= 2^24. The interleaver's branch j is
// a FIFO of j M bytes, the deinterleaver's of (I - 1 - j) M; feed is 1:1 in length and
// carries the FIFOs and the commutator across calls; flush feeds roundtrip_delay() =
// I (I - 1) M zeros.
constexpr size_t kMaxForney = size_t(1) << 24;
size_t conv_roundtrip_delay(size_t branches, size_t depth);  // checks the dimensions

class ConvInterleaver {
 public:
  ConvInterleaver(size_t branches, size_t depth) : ConvInterleaver(branches, depth, false) {}
  static ConvInterleaver dvb_t() { return ConvInterleaver(12, 17); }
  size_t branches() const { return branches_; }
  size_t depth() const { return depth_; }
  size_t roundtrip_delay() const { return branches_ * (branches_ - 1) * depth_; }
  void reset();
  void feed(const uint8_t* in, size_t n, uint8_t* out);  // in == out is allowed
  std::vector<uint8_t> flush();

 protected:
  ConvInterleaver(size_t branches, size_t depth, bool inverse);

 private:
  size_t delay_of(size_t j) const { return (inverse_ ? branches_ - 1 - j : j) * depth_; }
  size_t branches_, depth_;
  bool inverse_;
  std::vector<std::deque<uint8_t>> fifos_;
  size_t pos_ = 0;  // the commutator, kept modulo branches
};
class ConvDeinterleaver : public ConvInterleaver {
 public:
  ConvDeinterleaver(size_t branches, size_t depth) : ConvInterleaver(branches, depth, true) {}
  static ConvDeinterleaver dvb_t() { return ConvDeinterleaver(12, 17); }
};

// Frame mode, in bytes. Interleave: the payload zero-padded to a multiple of I bytes, fed
// through a fresh interleaver, then the flush: forney_frame_len(n) = round_up(n, I) + D bytes.
// Deinterleave: a stream of total bytes through a fresh deinterleaver, of which bytes
// D .. total are the padded payload (total <= D: nothing).
size_t forney_frame_len(size_t branches, size_t depth, size_t n);
std::vector<uint8_t> forney_frame_interleave(size_t branches, size_t depth, const uint8_t* bytes, size_t n);
std::vector<uint8_t> forney_frame_deinterleave(size_t branches, size_t depth, const uint8_t* bytes, size_t total);
// bytes_to_bits / bits_to_bytes (modulate/ofdm_frame.rs:207-234): MSB first, one bit per byte.
void bytes_to_bits(const uint8_t* bytes, size_t n, uint8_t* bits);
void bits_to_bytes(const uint8_t* bits, size_t n_bytes, uint8_t* bytes);  // reads bit 0 of each

// ---- the additive PN scrambler (scrambler.rs) -----------------------------------------------
// A Fibonacci LFSR of width bits (2..=32): the scrambling bit is bit 0, the feedback the
// parity of reg & taps, inserted at bit width - 1 as the register shifts right. Data bits are
// taken LSB first. seed nonzero; seed and taps fit in width bits.
class PnScramblerStream {
 public:
  PnScramblerStream(uint32_t taps, uint32_t width, uint32_t seed);
  void reset() { reg_ = seed_; }
  void feed_in_place(uint8_t* data, size_t n);
  uint32_t taps() const { return taps_; }
  uint32_t width() const { return width_; }
  uint32_t seed() const { return seed_; }

 private:
  uint32_t taps_, width_, seed_, mask_, reg_;
};
// Restarts from seed on every scramble call (self-inverse).
class PnScrambler {
 public:
  PnScrambler(uint32_t taps, uint32_t width, uint32_t seed) : s_(taps, width, seed) {}
  void scramble(uint8_t* data, size_t n) const {
    PnScramblerStream s = s_;
    s.feed_in_place(data, n);
  }
  PnScramblerStream into_stream() const { return s_; }

 private:
  PnScramblerStream s_;
};

// ---- DVB-T energy dispersal (dvb_t.rs:30-110) -----------------------------------------------
// PRBS 1 + X^14 + X^15 from 0b100101010000000; stage x1 is bit 14, x15 bit 0; the output bit is
// the feedback x14 ^ x15. Data bits are taken MSB first.
constexpr uint16_t kDvbTPrbsInit = 0x4A80;
constexpr uint32_t dvbt_prbs_next(uint16_t& reg) {
  const uint32_t fb = (reg ^ (reg >> 1)) & 1u;
  reg = static_cast<uint16_t>((reg >> 1) | (fb << 14));
  return fb;
}
constexpr uint8_t dvbt_prbs_byte(uint16_t& reg) {  // the next eight output bits, MSB first
  uint32_t b = 0;
  for (int i = 0; i < 8; ++i) b = b << 1 | dvbt_prbs_next(reg);
  return static_cast<uint8_t>(b);
}
class DvbTEnergyDispersal {
 public:
  void reset() { reg_ = kDvbTPrbsInit; }
  void feed_in_place(uint8_t* data, size_t n) {
    for (size_t i = 0; i < n; ++i) data[i] ^= dvbt_prbs_byte(reg_);
  }
  void advance_byte() { dvbt_prbs_byte(reg_); }

 private:
  uint16_t reg_ = kDvbTPrbsInit;
};

// ---- the transport-stream layer (dvb_t_ts.rs) -----------------------------------------------
constexpr size_t kTsPacketLen = 188, kTsPayloadLen = 187, kTsDispersalGroup = 8;
constexpr uint8_t kTsSync = 0x47, kTsSyncInverted = 0xB8;
// In place over n bytes, a whole number of packets (throws otherwise): the PRBS restarts every
// eight packets, the first sync byte of a group is flipped 0x47 <-> 0xB8 and not clocked
// over, the other seven are clocked over and left alone, every payload byte is whitened.
// Self-inverse. Returns the number of packets.
size_t ts_energy_disperse(uint8_t* packets, size_t n);
// What ts_energy_disperse XORs onto a group of eight packets: k_rs.hip's table. Equal to
// ts_energy_disperse over 1504 zero bytes.
struct TsDispersalMask {
  uint8_t m[kTsDispersalGroup * kTsPacketLen];
};
constexpr TsDispersalMask make_ts_dispersal_mask() {
  TsDispersalMask t{};
  uint16_t reg = kDvbTPrbsInit;
  for (size_t i = 0; i < kTsDispersalGroup; ++i) {
    if (i == 0)
      t.m[0] = kTsSync ^ kTsSyncInverted;
    else
      dvbt_prbs_byte(reg);
    for (size_t p = 1; p < kTsPacketLen; ++p) t.m[i * kTsPacketLen + p] = dvbt_prbs_byte(reg);
  }
  return t;
}
const TsDispersalMask& ts_dispersal_mask();  // the table, built once
// max(1, ceil(n / 187)) packets of 0x47 + 187 payload bytes, the last zero-padded.
std::vector<uint8_t> ts_packetize(const uint8_t* payload, size_t n);
// The payloads of whole packets; throws when n is 0 or no multiple of 188 (the reference's None).
std::vector<uint8_t> ts_depacketize(const uint8_t* packets, size_t n);
// 47 1F FF 10 and 184 bytes of 0xFF.
void ts_null_packet(uint8_t out[kTsPacketLen]);
// Appends null packets until ts holds target_packets (ts: whole packets, throws otherwise).
void ts_stuff_null_packets(std::vector<uint8_t>& ts, size_t target_packets);

}  // namespace rs
}  // namespace orion
