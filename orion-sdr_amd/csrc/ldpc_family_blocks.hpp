// ldpc_family_blocks.hpp — the inner LDPC family on the device (k_ldpc_family.hip): the
// batched belief-propagation decode with the block deinterleaver fused into its LLR fetch,
// and the batched staircase encoder with the block interleaver fused into its store. The
// scalar code they are held to is ldpc_family.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blocks.hpp"
#include "ldpc_family.hpp"

namespace orion {

// Limits (std::invalid_argument otherwise, nothing is launched): nstreams <= 2^24, at most
// 2^20 codewords per stream and 2^30 per launch, rows * cols <= 2^24, max_iter <= 2^30.
// nstreams == 0 does nothing.
constexpr size_t kLdpcfMaxStreams = size_t(1) << 24, kLdpcfMaxBlocks = size_t(1) << 20,
                 kLdpcfMaxWords = size_t(1) << 30, kLdpcfMaxIter = size_t(1) << 30;

// Codewords of a stream of n_llr LLRs: n_llr / N, at least 1. With an interleaver (rows,
// cols both nonzero) n_llr must be whole blocks of rows * cols.
size_t ldpcf_decode_blocks(int code, size_t n_llr, size_t rows, size_t cols);
// llr [nstreams][n_llr] f32, positive meaning bit 0. Codeword LLR j of a stream is element j
// of deinterleave_llrs(stream); elements at or past nblocks * N are not read. Word w goes
// through Ldpc::decode_soft(max_iter, rule, scale): bits [nstreams][nblocks * K] u8, unsat
// and iterations [nstreams][nblocks] i32. Device pointers, one launch, asynchronous on s. The
// code's graph is uploaded on the first call for a device and kept.
void ldpcf_decode_batch(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                        size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat, int32_t* iterations,
                        hipStream_t s);
void ldpcf_decode_batch_host(int code, const float* llr, size_t nstreams, size_t n_llr, size_t rows, size_t cols,
                             size_t max_iter, int rule, float scale, uint8_t* bits, int32_t* unsat,
                             int32_t* iterations);

// Elements of one coded stream: ceil(nbits / K) * N, rounded up to whole interleaver blocks.
size_t ldpcf_encoded_len(int code, size_t nbits, size_t rows, size_t cols);
// bits [nstreams][nbits] u8 -> coded [nstreams][ldpcf_encoded_len]: interleave_bits of
// ldpcf::encode_stream of each stream (the last message and the last block zero-padded).
void ldpcf_encode_batch(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                        uint8_t* coded, hipStream_t s);
void ldpcf_encode_batch_host(int code, const uint8_t* bits, size_t nstreams, size_t nbits, size_t rows, size_t cols,
                             uint8_t* coded);

}  // namespace orion
