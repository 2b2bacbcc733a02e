// fec_blocks.hpp — the inner code on the device (k_fec.hip): the batched soft Viterbi decode
// (the wave engine of trellis_wave.hpp) with depuncturing and block deinterleaving fused into
// its LLR fetch, and the batched encoder with puncturing and block interleaving. The scalar
// code they are held to is fec.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blocks.hpp"
#include "fec.hpp"

namespace orion {

// A stream is one frame; all streams of a call share code, rate, info_bits and interleaver
// (rows, cols; 0, 0: none). 1 <= info_bits <= 2^24, nstreams <= 2^24, n_llr <= 2^31 - 1,
// rows * cols <= 2^24 (std::invalid_argument otherwise). nstreams == 0 does nothing.

// Per stream: bits = viterbi_decode_soft(deinterleave_llrs(llr [n_llr]), info_bits). llr
// [nstreams][n_llr] f32 -> bits [nstreams][info_bits] u8. Device pointers, one launch,
// asynchronous on s; work: the caller's scratch of at least fec::viterbi_work_bytes bytes
// (8-byte aligned), which the call may overwrite wholly.
void fec_viterbi(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits, size_t rows,
                 size_t cols, uint8_t* bits, void* work, size_t work_bytes, hipStream_t s);
// Host slices: synchronous, the scratch is allocated for the call.
void fec_viterbi_host(int code, int rate, const float* llr, size_t nstreams, size_t n_llr, size_t info_bits,
                      size_t rows, size_t cols, uint8_t* bits);

// The length of a stream's encoder output: punctured_coded_len, rounded up to whole blocks
// when there is an interleaver (interleave_bits zero-pads the last one).
size_t fec_encoded_len(int code, size_t info_bits, int rate, size_t rows, size_t cols);
// Per stream: coded = interleave_bits(conv_encode_punctured(info [info_bits])). info
// [nstreams][info_bits] u8 -> coded [nstreams][fec_encoded_len] u8. Device pointers, one
// launch, asynchronous on s.
void fec_encode_batch(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits, size_t rows,
                      size_t cols, uint8_t* coded, hipStream_t s);
void fec_encode_batch_host(int code, int rate, const uint8_t* info, size_t nstreams, size_t info_bits, size_t rows,
                           size_t cols, uint8_t* coded);

}  // namespace orion
