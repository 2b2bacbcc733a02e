// fec.hpp — the inner code of the COFDM / DVB-T chain, host side (no device): the punctured,
// zero-tail-terminated rate 1/2 convolutional code of fec/conv.rs (K = 5, G0 = 25, G1 = 23
// octal, PSK31's code; K = 7, G0 = 171, G1 = 133 octal, DVB-T's), its soft-input Viterbi
// decoder in the reference's exact f32 behaviour, and the rectangular block interleaver of
// fec/interleaver.rs:53-120 with the two chain drivers that use it (interleave_bits,
// modulate/ofdm_frame.rs; deinterleave_llrs, demodulate/ofdm_frame.rs). k_fec.hip's kernels
// are held to these functions byte for byte.
//
// Bits are uint8, one per byte (only bit 0 of an input byte is read). LLRs are f32, positive
// meaning bit 0. Everything here throws std::invalid_argument on a bad argument.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "trellis.hpp"

namespace orion {
namespace fec {

enum Code : int { kK5 = 0, kDvbK7 = 1 };
enum Rate : int { kR1_2 = 0, kR2_3 = 1, kR3_4 = 2, kR5_6 = 3, kR7_8 = 4 };

// What a code is: the register width K - 1 (the tail length; 2^(K-1) states) and the two
// generators as masks over the K-bit window (input << (K - 1)) | register (conv.rs:80-94).
struct CodeSpec {
  int reg_bits;
  uint32_t g0, g1;
};
// What a rate is: the puncture matrix of conv.rs:112-120 as one mask over the mother
// positions of a period, bit 2 col + j set where generator j's bit of column col is kept;
// kept = the mask's population count.
struct RateSpec {
  int period, kept;
  uint32_t keep;
};
CodeSpec code_spec(int code);  // throws on an unknown code
RateSpec rate_spec(int rate);  // throws on an unknown rate

// The limits of every entry here and in k_fec.hip (indices stay inside 32 bits).
constexpr size_t kMaxInfoBits = size_t(1) << 24;
constexpr size_t kMaxStreams = size_t(1) << 24;
constexpr size_t kMaxLlr = 0x7fffffffull;
constexpr size_t kMaxBlock = size_t(1) << 24;  // rows * cols

// punctured_coded_len_with, conv.rs:274-288.
size_t punctured_coded_len(int code, size_t info_bits, int rate);
// conv_encode_punctured_with, conv.rs:234-263: info [info_bits] -> out [punctured_coded_len].
void conv_encode_punctured(int code, const uint8_t* info, size_t info_bits, int rate, uint8_t* out);
// viterbi_decode_soft_with, conv.rs:304-398: llr [n_llr] in punctured order -> bits [info_bits].
// Positions the puncturing deleted, and positions at or past n_llr, read as 0.0.
void viterbi_decode_soft(int code, const float* llr, size_t n_llr, size_t info_bits, int rate, uint8_t* bits);

// BlockInterleaver, interleaver.rs:53-120: in[r cols + c] -> out[c rows + r].
class BlockInterleaver {
 public:
  BlockInterleaver(size_t rows, size_t cols);
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
  size_t block_len() const { return rows_ * cols_; }
  // one block, in and out of block_len() elements
  template <class T>
  void interleave(const T* in, T* out) const {
    for (size_t r = 0; r < rows_; ++r)
      for (size_t c = 0; c < cols_; ++c) out[c * rows_ + r] = in[r * cols_ + c];
  }
  template <class T>
  void deinterleave(const T* in, T* out) const {
    for (size_t r = 0; r < rows_; ++r)
      for (size_t c = 0; c < cols_; ++c) out[r * cols_ + c] = in[c * rows_ + r];
  }
  // interleave_bits (Block kind): the last partial block is zero-padded, so the output is
  // interleaved_len(n) elements, a whole number of blocks.
  size_t interleaved_len(size_t n) const { return (n + block_len() - 1) / block_len() * block_len(); }
  std::vector<uint8_t> interleave_bits(const uint8_t* bits, size_t n) const;
  // deinterleave_llrs (Block kind): full blocks are permuted back, a short last chunk passes
  // through as it is. Output of n elements.
  std::vector<float> deinterleave_llrs(const float* llr, size_t n) const;

 private:
  size_t rows_, cols_;
};

// Bytes of device scratch k_conv_viterbi needs (k_fec.hip): the survivor words of the
// info_bits + reg_bits steps (trellis.hpp).
inline size_t viterbi_work_bytes(int reg_bits, size_t nstreams, size_t info_bits) {
  return trellis::work_bytes(reg_bits, nstreams, info_bits + static_cast<size_t>(reg_bits));
}

}  // namespace fec
}  // namespace orion
