// rs_blocks.hpp — the outer code on the device (k_rs.hip): the batched Reed-Solomon decode
// with bit packing, the Forney deinterleaver and the energy dispersal fused into its fetch and
// store, the batched encoder, and the Forney frame interleaver. The scalar code they are held
// to is rs.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blocks.hpp"
#include "rs.hpp"

namespace orion {

// A call works on nstreams streams of ncw codewords each; all share the code (n, n_parity),
// and the fusions. Limits (std::invalid_argument otherwise, nothing is launched): 1 <= n <=
// 255, 1 <= n_parity <= 32, n_parity < n, 1 <= ncw <= 2^20, nstreams <= 2^24, nstreams * ncw
// <= 2^30, branches^2 * depth <= 2^24. nstreams == 0 does nothing.
constexpr size_t kRsMaxParity = 32, kRsMaxCw = size_t(1) << 20, kRsMaxStreams = size_t(1) << 24,
                 kRsMaxWords = size_t(1) << 30;

struct RsFusion {
  bool bits = false;                 // the stream is one bit per byte, MSB first (bit 0 of each byte is read)
  size_t branches = 0, depth = 0;    // 0, 0: none; else frame-mode Forney (de)interleaving
  bool disperse = false;             // k = 188 only: ts_energy_disperse, the group of a stream's word c being c / 8
};

// Bytes (bits: elements) of one input stream of rs_decode_batch: ncw * n, plus the round-trip
// delay with a deinterleaver (ncw * n must then be a multiple of branches), times 8 for bits.
size_t rs_decode_stream_len(size_t n, size_t n_parity, size_t ncw, const RsFusion& f);
// Per stream: the payload is the stream itself, or bits_to_bytes of it, or
// forney_frame_deinterleave of that; word c of it goes through decode_counted; messages
// [nstreams][ncw][k] u8 (with disperse: XORed with the dispersal sequence, failed words too),
// status [nstreams][ncw] i32 (the corrected-byte count, -1: uncorrectable, the message then
// received[:k]). Device pointers, one launch, asynchronous on s.
void rs_decode_batch(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw, const RsFusion& f,
                     uint8_t* msgs, int32_t* status, hipStream_t s);
void rs_decode_batch_host(size_t n, size_t n_parity, const uint8_t* in, size_t nstreams, size_t ncw,
                          const RsFusion& f, uint8_t* msgs, int32_t* status);

// msgs [nstreams][ncw][k] -> codewords [nstreams][ncw][n]; with disperse (k = 188) the message
// goes through ts_energy_disperse first. f.bits, f.branches must be unset.
void rs_encode_batch(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw, const RsFusion& f,
                     uint8_t* cws, hipStream_t s);
void rs_encode_batch_host(size_t n, size_t n_parity, const uint8_t* msgs, size_t nstreams, size_t ncw,
                          const RsFusion& f, uint8_t* cws);

// Elements of one output stream: forney_frame_len(len), times 8 with bits.
size_t forney_interleave_stream_len(size_t branches, size_t depth, size_t len, bool bits);
// Per stream: forney_frame_interleave(in [len] bytes), unpacked to one bit per byte with bits.
// 1 <= len <= 2^27. Device pointers, one launch, asynchronous on s.
void forney_interleave_batch(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len, bool bits,
                             uint8_t* out, hipStream_t s);
void forney_interleave_batch_host(size_t branches, size_t depth, const uint8_t* in, size_t nstreams, size_t len,
                                  bool bits, uint8_t* out);

}  // namespace orion
