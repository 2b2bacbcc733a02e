// trellis.hpp — the scratch of the batched Viterbi decoders (trellis_wave.hpp), host side (no
// device code): per step and stream the survivor word(s), laid out [step][padded stream].
#pragma once
#include <cstddef>

namespace orion {
namespace trellis {
// Streams rounded up to the 64 >> reg_bits that share a wave (reg_bits = K - 1 = 4 or 6).
constexpr size_t padded_streams(int reg_bits, size_t nstreams) {
  const size_t spw = size_t(64) >> reg_bits;
  return (nstreams + spw - 1) / spw * spw;
}
// K = 5: one uint32 per step and stream (16 + 16 bits). K = 7: two uint64.
constexpr size_t work_bytes(int reg_bits, size_t nstreams, size_t n_steps) {
  return padded_streams(reg_bits, nstreams) * n_steps * (reg_bits == 4 ? 4 : 16);
}
}  // namespace trellis
}  // namespace orion
