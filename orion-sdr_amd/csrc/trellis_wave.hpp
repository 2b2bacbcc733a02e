// trellis_wave.hpp — the Viterbi engine of one wave64 over a rate 1/2 shift-register code with
// RB = K - 1 register bits (4 or 6): one lane per trellis state, W = 2^RB lanes per stream,
// 64 / W streams per wave, 64 threads by ceil(nstreams / (64 / W)) workgroups. What
// k_psk31_viterbi (k_psk31.hip) and k_conv_viterbi (k_fec.hip) share: the lane's place, the
// add-compare-select of a step, the survivor words and the traceback. The caller's: the input
// fetch, the branch metrics, the sense, the step loop, the end state and the bits it wants.
//
// State s is reached from the two states p0 = (s << 1) & (W - 1) and p0 + 1 with input bit
// s >> (RB - 1). Each step leaves the stream's share of two ballots in the scratch array
// (trellis.hpp work_bytes), [step][padded stream]: bit s of upper says that state s took
// p0 + 1, bit s of taken that it took a predecessor at all. Lane 0 of the stream runs the
// traceback over the words it wrote itself, so its own program order suffices.
//
// Exactness. The reference decoders (codec/psk31.rs:95-160, fec/conv.rs:304-398) and the host
// decoders held to them (psk31.cpp, fec.cpp) visit the predecessor states in ascending order,
// skip one whose metric is at or beyond the start value, form cand = pm + branch metric with
// one rounding and replace a survivor on a strict comparison only; a next state's metric
// starts at the start value and its survivor entry at 0. A next state has exactly two
// predecessors, p0 < p0 + 1, and nothing else writes its entry, so the visit order restricted
// to it is: p0 first against the start value, then p0 + 1 against the result. That is what a
// lane computes, with the reference's own skip tests (!(pm >= start), !(pm <= start): NaN is
// not skipped) and comparisons, so ties, +-inf and NaN go the reference's way. An entry nobody
// wrote is "not taken" and leads to state 0, as the reference's zeroed table does. Every loop
// is bounded by the step count.
#pragma once
#include <type_traits>

#include "hip_common.hpp"
#include "trellis.hpp"

namespace orion {
namespace trellis {

constexpr int kTraceAhead = 8;  // survivor words fetched ahead of the traceback's chain of states

__device__ __forceinline__ uint32_t parity(uint32_t x) { return static_cast<uint32_t>(__popc(x)) & 1u; }

// The sense of a path metric: where it starts, when a predecessor is skipped, what wins.
struct Minimise {
  static __device__ __forceinline__ float start() { return 3.4028234663852886e38f / 2.0f; }  // f32::MAX / 2
  static __device__ __forceinline__ bool dead(float pm) { return pm >= start(); }
  static __device__ __forceinline__ bool better(float a, float b) { return a < b; }
};
struct Maximise {
  static __device__ __forceinline__ float start() { return -3.4028234663852886e38f / 2.0f; }  // f32::MIN / 2
  static __device__ __forceinline__ bool dead(float pm) { return pm <= start(); }
  static __device__ __forceinline__ bool better(float a, float b) { return a > b; }
};

template <int RB>
struct Wave {
  static_assert(RB == 4 || RB == 6, "K = 5 or K = 7");
  static constexpr int W = 1 << RB;   // states: lanes per stream
  static constexpr int SPW = 64 / W;  // streams per wave
  // The survivor word(s) of one step and stream. RB = 4: one uint32, upper | taken << 16. RB = 6:
  // two uint64, upper and taken.
  using Word = std::conditional_t<RB == 4, uint32_t, uint64_t>;
  static constexpr int kWords = RB == 4 ? 1 : 2;
  struct Survivor {
    Word word[kWords];
    __device__ __forceinline__ uint32_t upper(uint32_t s) const { return static_cast<uint32_t>(word[0] >> s) & 1u; }
    __device__ __forceinline__ bool taken(uint32_t s) const { return word[kWords - 1] >> s >> (RB == 4 ? 16 : 0) & 1u; }
  };

  const int lane = threadIdx.x;
  const int st = lane & (W - 1), gshift = lane & (64 - W);  // this lane's state; the stream's first lane
  const int p0 = (st << 1) & (W - 1);                       // the lower predecessor
  const uint32_t inbit = static_cast<uint32_t>(st) >> (RB - 1);  // the input bit of both branches into st
  const long long stream = static_cast<long long>(blockIdx.x) * SPW + (lane >> RB);
  const long long padded;
  const bool live;
  // the stream whose input to read: a group past the last stream runs the last stream's
  // arithmetic (the shuffles and ballots are wave-wide) and stores nothing
  const long long row;

  __device__ __forceinline__ explicit Wave(long long nstreams)
      : padded(static_cast<long long>(padded_streams(RB, static_cast<size_t>(nstreams)))),
        live(stream < nstreams),
        row(live ? stream : nstreams - 1) {}

  // One step: pm becomes this state's new metric, given the metrics bm0, bm1 of the branches
  // from p0 and p0 + 1. Every lane of the wave calls it.
  template <class Sense>
  __device__ __forceinline__ Survivor acs(float& pm, float bm0, float bm1) const {
    const float from[2] = {__shfl(pm, p0, W), __shfl(pm, p0 + 1, W)}, bm[2] = {bm0, bm1};
    float v = Sense::start();
    bool taken = false, upper = false;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!Sense::dead(from[k])) {
        const float cand = from[k] + bm[k];
        if (Sense::better(cand, v)) {
          v = cand;
          taken = true;
          upper = k == 1;
        }
      }
    }
    pm = v;
    const uint64_t mu = __ballot(upper) >> gshift, mt = __ballot(taken) >> gshift;
    if constexpr (RB == 4) {
      return {{static_cast<uint32_t>(mu & 0xFFFFu) | static_cast<uint32_t>(mt & 0xFFFFu) << 16}};
    } else {
      return {{mu, mt}};
    }
  }

  // [step][padded stream], 64-bit indices
  __device__ __forceinline__ void store(void* work, long long step, Survivor s) const {
    if (!live || st != 0) return;
#pragma unroll
    for (int i = 0; i < kWords; ++i) static_cast<Word*>(work)[kWords * (step * padded + stream) + i] = s.word[i];
  }
  __device__ __forceinline__ Survivor load(const void* work, long long step) const {
    Survivor s;
#pragma unroll
    for (int i = 0; i < kWords; ++i) s.word[i] = static_cast<const Word*>(work)[kWords * (step * padded + stream) + i];
    return s;
  }

  // From state at the end of n_steps back to step 0, on lane 0 of a live stream (the other
  // lanes return): B[t] = the input bit of step t for t < n_bits.
  __device__ __forceinline__ void traceback(const void* work, long long n_steps, uint32_t state, uint8_t* B,
                                            long long n_bits) const {
    if (!live || st != 0) return;
    const long long skip = n_steps - n_bits;  // the last steps, whose bits nobody wants
    for (long long d = 0; d < n_steps; d += kTraceAhead) {  // d steps back from the end
      Survivor w[kTraceAhead];
#pragma unroll
      for (int k = 0; k < kTraceAhead; ++k) w[k] = d + k < n_steps ? load(work, n_steps - 1 - d - k) : Survivor{};
#pragma unroll
      for (int k = 0; k < kTraceAhead; ++k) {
        if (d + k < n_steps) {
          if (d + k >= skip) B[n_steps - 1 - d - k] = static_cast<uint8_t>(state >> (RB - 1) & 1u);
          state = w[k].taken(state) ? ((state << 1) & (W - 1)) | w[k].upper(state) : 0u;
        }
      }
    }
  }
};

}  // namespace trellis
}  // namespace orion
