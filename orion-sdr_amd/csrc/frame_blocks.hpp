// frame_blocks.hpp — the glue of the COFDM frame chain on the device (k_frame.hip): what lies
// between the batched codes. Pack (bytes or header fields -> CRC -> whitener -> bits or bytes),
// unpack (the inverse, with the CRC check and the decoders' verdicts folded per frame), the
// coded-bit and LLR rows with the after-inner PN, and bytes -> bits. The scalar code they are
// held to is frame.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "blocks.hpp"
#include "frame.hpp"

namespace orion {

// Limits (std::invalid_argument otherwise, nothing is launched): nframes <= 2^24, a block of
// at most 2^16 info bytes, rows of at most 2^24 elements. nframes == 0 does nothing.
constexpr size_t kFrameMaxFrames = size_t(1) << 24, kFrameMaxInfo = size_t(1) << 16, kFrameMaxRow = size_t(1) << 24;

// The whitener of a pack / unpack call: scheme's scrambler when it sits before the outer code.
// seeds [nframes] i64 (the low 32 bits are SeedMode::PerFrameRandom's drawn seed) or null for
// the scheme's fixed seed.
//
// payload [nframes][info_len] u8, or for header (info_len = 14) fields [nframes][5] i64:
// mcs_index, payload_len, sequence_num, flags, scrambler_seed. out: [nframes][framed * 8] u8
// bits, MSB first, or with out_bytes [nframes][framed] u8: frame.hpp's append_crc then
// scramble_bytes of every row. Device pointers, one launch, asynchronous on s.
void frame_pack_batch(const frame::Scheme& sch, const uint8_t* payload, const long long* fields,
                      const long long* seeds, size_t nframes, size_t info_len, bool out_bytes, uint8_t* out,
                      hipStream_t s);
void frame_pack_batch_host(const frame::Scheme& sch, const uint8_t* payload, const long long* fields,
                           const long long* seeds, size_t nframes, size_t info_len, bool out_bytes, uint8_t* out);

// in [nframes][in_stride] u8: the first framed * 8 elements of a row are the framed bits (bit 0
// of each), or with in_bytes the first framed elements its bytes. unsat [nframes][n_inner] i32
// or null (inner_ok = all zero; true when null), status [nframes][n_outer] i32 or null
// (outer_ok = all >= 0; true when null). Writes payload [nframes][info_len] u8 (descrambled,
// CRC stripped), flags [nframes][4] u8 = inner_ok, outer_ok, crc_ok, is_valid, corrected
// [nframes] i32 (the sum of the non-negative status entries) and, for header, fields
// [nframes][5] i64.
void frame_unpack_batch(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, bool in_bytes,
                        const long long* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                        size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                        int32_t* corrected, long long* fields, hipStream_t s);
void frame_unpack_batch_host(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, bool in_bytes,
                             const long long* seeds, const int32_t* unsat, size_t n_inner, const int32_t* status,
                             size_t n_outer, size_t nframes, size_t info_len, uint8_t* payload, uint8_t* flags,
                             int32_t* corrected, long long* fields);

// The rows ofdm_modulate_batch takes: out [nframes][out_len] = the first nbits elements of in
// [nframes][in_stride], scramble_bits applied when the scheme's Additive scrambler sits after
// the inner code, then zeros. nbits <= in_stride, nbits <= out_len.
void frame_coded_bits_batch(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, size_t nbits,
                            const long long* seeds, size_t nframes, size_t out_len, uint8_t* out, hipStream_t s);
void frame_coded_bits_batch_host(const frame::Scheme& sch, const uint8_t* in, size_t in_stride, size_t nbits,
                                 const long long* seeds, size_t nframes, size_t out_len, uint8_t* out);
// The mirror: out [nframes][n] = the first n LLRs of in [nframes][in_stride], apply_pn_to_llrs
// applied under the same condition; every other bit of an element is kept.
void frame_llr_prepare_batch(const frame::Scheme& sch, const float* in, size_t in_stride, size_t n,
                             const long long* seeds, size_t nframes, float* out, hipStream_t s);
void frame_llr_prepare_batch_host(const frame::Scheme& sch, const float* in, size_t in_stride, size_t n,
                                  const long long* seeds, size_t nframes, float* out);
// The frames' IQ (cf32, interleaved): out [nframes][lead_len + hdr_len + pay_len] = the shared
// lead [lead_len] (S&C repeats and training symbol), hdr [nframes][hdr_len], pay
// [nframes][pay_len]. With ramp [ramp_len] (SymbolWindow's, 2 ramp_len <= sps) every whole
// symbol of sps samples from win_start on is tapered as the host's window post-pass does.
void frame_assemble_batch(const float* lead, size_t lead_len, const float* hdr, size_t hdr_len, const float* pay,
                          size_t pay_len, size_t nframes, size_t sps, size_t win_start, const float* ramp,
                          size_t ramp_len, float* out, hipStream_t s);
// in [nframes][nbytes] u8 -> out [nframes][nbytes * 8] u8, MSB first.
void frame_bytes_to_bits_batch(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out, hipStream_t s);
void frame_bytes_to_bits_batch_host(const uint8_t* in, size_t nframes, size_t nbytes, uint8_t* out);

}  // namespace orion
