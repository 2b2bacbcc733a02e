// code_dev.hpp — small device helpers that the code kernels share (k_fec.hip, k_ldpc.hip,
// k_ldpc_family.hip). The Viterbi engine that k_fec.hip shares with k_psk31.hip is
// trellis_wave.hpp, the GF(2^8) algebra of k_rs.hip and k_bch.hip gf256_wave.hpp.
#pragma once
#include "hip_common.hpp"

namespace orion {

// The block interleaver of the frame chain, out[r cols + c] = in[c rows + r] within a block of
// rows * cols: offset q = r cols + c of one side is offset c rows + r of the other. The inverse
// map is the same with rows and cols exchanged.
__device__ __forceinline__ uint32_t block_il_offset(uint32_t q, uint32_t rows, uint32_t cols) {
  const uint32_t r = q / cols, c = q - r * cols;
  return c * rows + r;
}

// ldpc.rs:644-663, ldpc_codes.rs:560-580: the reference's rational tanh and atanh, op for op
// (no contraction: these TUs are built with -ffp-contract=off, and the division is IEEE).
__device__ __forceinline__ float fast_tanh(float x) {
  if (x < -4.97f) return -1.0f;
  if (x > 4.97f) return 1.0f;
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (105.0f + x2));
  const float b = 945.0f + x2 * (420.0f + x2 * 15.0f);
  return a / b;
}
__device__ __forceinline__ float fast_atanh(float x) {
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (-735.0f + x2 * 64.0f));
  const float b = 945.0f + x2 * (-1050.0f + x2 * 225.0f);
  return a / b;
}

}  // namespace orion
