// bch_blocks.hpp — the outer BCH code on the device (k_bch.hip): the batched decoder, reading
// the bit tensor the inner decoders write where it lies, and the batched encoder. The scalar
// code they are held to is bch.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bch.hpp"
#include "blocks.hpp"

namespace orion {

// Limits (std::invalid_argument otherwise, nothing is launched): 1 <= t <= 31 (the locator
// vector, at most 2 t + 1 entries, has one lane per entry), nstreams <= 2^24, at most 2^24
// words per stream and 2^30 per launch. nstreams == 0 does nothing.
constexpr size_t kBchMaxT = 31, kBchMaxStreams = size_t(1) << 24, kBchMaxCw = size_t(1) << 24,
                 kBchMaxWords = size_t(1) << 30;

// The code of a device call, Bch::for_info_bits(t, info_bits), t checked first.
bch::Bch bch_device_code(size_t t, size_t info_bits);
// in [nstreams][nb] u8, one bit per element: each stream is nb / n words (at least 1), the tail
// is ignored. Word c goes through Bch::decode: msgs [nstreams][ncw * k] u8, status
// [nstreams][ncw] i32. Device pointers, one launch, asynchronous on s.
void bch_decode_batch(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                      int32_t* status, hipStream_t s);
void bch_decode_batch_host(size_t t, size_t info_bits, const uint8_t* in, size_t nstreams, size_t nb, uint8_t* msgs,
                           int32_t* status);
// bits [nstreams][nbits] u8 -> coded [nstreams][ceil(nbits / k) * n]: bch::encode_stream of
// each stream, the last message zero-padded.
void bch_encode_batch(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits, uint8_t* coded,
                      hipStream_t s);
void bch_encode_batch_host(size_t t, size_t info_bits, const uint8_t* bits, size_t nstreams, size_t nbits,
                           uint8_t* coded);

}  // namespace orion
