// k_acquire.hip — OFDM burst acquisition for a batch of captures (acquire.hpp):
//
//   k_sc_metric   the Schmidl & Cox sums of every candidate offset of every capture, one lane
//                 per offset. A lane walks its (num_repeats - 1) repeat_len terms in the host's
//                 order (acquire.cpp sc_metric: per-segment accumulators from zero, added to p
//                 and r in segment order, no contraction), so p, r and score carry the host's
//                 bits; a sliding-window update would round differently. A workgroup's 256
//                 offsets read 256 + num_repeats repeat_len consecutive samples: staged in LDS
//                 when they fit kScLdsSamples, read from global memory (L1 / L2 serve the
//                 overlap) otherwise. Consecutive lanes read consecutive cf32 values on either
//                 path (ds_read_b64 / 8-byte global loads, conflict-free and coalesced).
//   k_sc_select   one workgroup per capture: r_peak, the first five of the host's ranking
//                 (largest key = score (r / r_peak), the lower offset first among equals) and
//                 earliest_accepted's choice, by reductions.
//   k_icfo_gather each of the five candidates' training symbol from the CP boundary, rotated by
//                 the closed-form phasor of -cfo_hz; the batched transform (k_ofdm.hip) follows.
//   k_icfo_corr   the shift correlation against the known pattern, one lane per shift, bins
//                 summed in the host's order; the lowest shift wins a tie.
//   k_acq_correct every capture from its accepted start on, the total carrier offset taken out.
//   k_acq_weights the held equalizer weights from the corrected training symbol's transform.
//   k_frame_eq_cpe  the equalizer and the common-phase-error tracker of the frame demodulator,
//                 one wave per frame.
#include "acquire.hpp"
#include "hip_common.hpp"
#include "ofdm_dev.hpp"

namespace orion {

namespace {

constexpr int kSelThreads = 256;
constexpr float kTauF = 6.28318530717958647692f;

// (key, index) with the larger key, the lower index among equal keys; idx INT_MAX: none.
struct Pick {
  float key;
  int idx;
};
__device__ __forceinline__ Pick better(Pick a, Pick b) {
  const bool take = b.idx != 0x7fffffff && (a.idx == 0x7fffffff || b.key > a.key || (b.key == a.key && b.idx < a.idx));
  return take ? b : a;
}
__device__ __forceinline__ Pick block_pick(Pick v, Pick* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Pick o;
    o.key = __shfl_xor(v.key, off, 64);
    o.idx = __shfl_xor(v.idx, off, 64);
    v = better(v, o);
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();  // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  Pick out = sh[0];
  for (int k = 1; k < kSelThreads / 64; ++k) out = better(out, sh[k]);
  return out;
}

template <bool LDS>
__global__ __launch_bounds__(kScThreads) void k_sc_metric(const f2* __restrict__ iq, long long n, int R, int L,
                                                          long long start, long long nd, float den,
                                                          f2* __restrict__ p, float* __restrict__ r,
                                                          float* __restrict__ score, float* __restrict__ cfo) {
  extern __shared__ f2 sh[];
  const int t = threadIdx.x;
  const long long c = blockIdx.y;
  const f2* __restrict__ x = iq + c * n;
  const long long d0 = static_cast<long long>(blockIdx.x) * kScThreads;  // the group's first offset index
  const long long base = start + d0;
  if constexpr (LDS) {
    const int cnt = kScThreads + R * L;
    for (int i = t; i < cnt; i += kScThreads) {
      const long long g = base + i;
      sh[i] = g < n ? x[g] : f2{0.0f, 0.0f};
    }
    __syncthreads();
  }
  const long long di = d0 + t;
  if (di >= nd) return;  // di < nd: start + di + R L <= n, every read below is inside the capture
  float pr = 0.0f, pi = 0.0f, rr = 0.0f;
  for (int seg = 0; seg + 1 < R; ++seg) {
    float sr = 0.0f, si = 0.0f, se = 0.0f;
    const int o = seg * L;
    for (int i = 0; i < L; ++i) {
      f2 a, b;
      if constexpr (LDS) {
        a = sh[t + o + i];
        b = sh[t + o + L + i];
      } else {
        a = x[base + t + o + i];
        b = x[base + t + o + L + i];
      }
      const float ai = -a.y;  // conj(a) b, the plain product
      sr += a.x * b.x - ai * b.y;
      si += a.x * b.y + ai * b.x;
      se += b.x * b.x + b.y * b.y;
    }
    pr += sr;
    pi += si;
    rr += se;
  }
  const long long k = c * nd + di;
  p[k] = f2{pr, pi};
  r[k] = rr;
  float sc = -1.0f, f = 0.0f;
  if (!(rr <= 0.0f)) {
    sc = (pr * pr + pi * pi) / (rr * rr);
    sc = sc < 0.0f ? 0.0f : sc;
    sc = sc > 1.0f ? 1.0f : sc;
    f = atan2f(pi, pr) / den;
  }
  score[k] = sc;
  cfo[k] = f;
}

__global__ __launch_bounds__(kSelThreads) void k_sc_select(long long nd, long long start, float thr, long long cluster,
                                                           SyncOut o) {
  __shared__ Pick sh[kSelThreads / 64];
  const int t = threadIdx.x;
  const long long c = blockIdx.x;
  const float* __restrict__ r = o.r + c * nd;
  const float* __restrict__ score = o.score + c * nd;
  const int ndi = static_cast<int>(nd);
  // r_peak over the kept offsets (from 0, as the host's running maximum)
  Pick m{0.0f, 0x7fffffff};
  for (int d = t; d < ndi; d += kSelThreads) {
    const float v = r[d];
    if (!(v <= 0.0f) && (m.idx == 0x7fffffff || v > m.key)) m = Pick{v, d};
  }
  m = block_pick(m, sh);
  const float r_peak = m.idx == 0x7fffffff ? 0.0f : fmaxf(0.0f, m.key);
  const bool any = m.idx != 0x7fffffff && r_peak > 0.0f;
  int top[acquire::kTopN];
#pragma unroll
  for (int j = 0; j < static_cast<int>(acquire::kTopN); ++j) {
    Pick b{0.0f, 0x7fffffff};
    if (any) {
      for (int d = t; d < ndi; d += kSelThreads) {
        const float v = r[d];
        if (v <= 0.0f) continue;
        bool used = false;
#pragma unroll
        for (int q = 0; q < j; ++q) used |= top[q] == d;
        if (used) continue;
        const float key = score[d] * (v / r_peak);
        if (b.idx == 0x7fffffff || key > b.key) b = Pick{key, d};
      }
    }
    b = block_pick(b, sh);
    top[j] = b.idx == 0x7fffffff ? -1 : b.idx;
  }
  // earliest_accepted: the lowest accepted offset, then the best-ranked accepted one of its cluster
  Pick e{0.0f, 0x7fffffff};
  if (any) {
    for (int d = t; d < ndi; d += kSelThreads) {
      if (!(r[d] <= 0.0f) && score[d] >= thr) {
        e = Pick{0.0f, d};
        break;  // a lane's offsets ascend
      }
    }
  }
  e = block_pick(e, sh);  // equal keys: the lower index
  Pick a{0.0f, 0x7fffffff};
  if (e.idx != 0x7fffffff) {
    const long long span = cluster > 1 ? cluster : 1;
    for (int d = t; d < ndi; d += kSelThreads) {
      const float v = r[d];
      if (v <= 0.0f || !(score[d] >= thr) || d < e.idx || d - e.idx >= span) continue;
      const float key = score[d] * (v / r_peak);
      if (a.idx == 0x7fffffff || key > a.key) a = Pick{key, d};
    }
  }
  a = block_pick(a, sh);
  if (t == 0) {
    o.r_peak[c] = any ? r_peak : 0.0f;
    int in_top = -1;
#pragma unroll
    for (int j = 0; j < static_cast<int>(acquire::kTopN); ++j) {
      o.top_start[c * acquire::kTopN + j] = top[j] < 0 ? -1 : static_cast<int32_t>(start + top[j]);
      o.top_bins[c * acquire::kTopN + j] = 0;
      if (a.idx != 0x7fffffff && top[j] == a.idx) in_top = j;
    }
    const bool acc = a.idx != 0x7fffffff;
    o.accepted_start[c] = acc ? static_cast<int32_t>(start + a.idx) : -1;
    o.accepted_in_top[c] = in_top;
    o.accepted_bins[c] = 0;
    o.accepted_score[c] = acc ? score[a.idx] : 0.0f;
    o.accepted_cfo_hz[c] = acc ? o.cfo_hz[c * nd + a.idx] : 0.0f;
  }
}

// Rotator(f, fs): the f32 step phi = TAU f / fs; output k is the phasor of (k + 1) phi, here in
// closed form, phasor_q64(k + 1, step), from the step as a Q0.64 fraction of a turn (the f32
// step itself, rounded once more in f64).
__device__ __forceinline__ uint64_t rot_step_q64(float f, float fs) {
  const float phi = kTauF * f / fs;
  double turns = static_cast<double>(phi) * 0.15915494309189533577;
  turns -= rint(turns);
  if (turns >= 0.5) turns -= 1.0;
  return static_cast<uint64_t>(static_cast<long long>(llrint(ldexp(turns, 64))));
}

// Whether candidate cand has a training symbol to search (the host returns 0 bins otherwise).
__device__ __forceinline__ bool icfo_live(int st, long long n, int lead, int n_fft, int cp) {
  return st >= 0 && static_cast<long long>(st) + lead + cp + n_fft <= n;
}

__global__ __launch_bounds__(256) void k_icfo_gather(const f2* __restrict__ iq, long long n, long long nd, long long start,
                                                     int lead, int n_fft, int cp, float fs, SyncOut o,
                                                     f2* __restrict__ sym) {
  const long long cand = blockIdx.x, c = cand / static_cast<long long>(acquire::kTopN);
  const int st = o.top_start[cand];
  f2* __restrict__ out = sym + cand * n_fft;
  if (!icfo_live(st, n, lead, n_fft, cp)) {
    for (int i = threadIdx.x; i < n_fft; i += 256) out[i] = f2{0.0f, 0.0f};
    return;
  }
  const uint64_t step = rot_step_q64(-o.cfo_hz[c * nd + (st - start)], fs);
  const f2* __restrict__ x = iq + c * n + st + lead + cp;
  for (int i = threadIdx.x; i < n_fft; i += 256)
    out[i] = cmul_rot(x[i], phasor_q64(static_cast<uint64_t>(cp + i + 1), step));
}

__global__ __launch_bounds__(256) void k_icfo_corr(const f2* __restrict__ freq, const f2* __restrict__ known, long long n,
                                                   int lead, int n_fft, int cp, SyncOut o) {
  extern __shared__ f2 sh[];  // the candidate's spectrum; the known pattern is read at wave-uniform indices
  __shared__ Pick red[256 / 64];
  const long long cand = blockIdx.x, c = cand / static_cast<long long>(acquire::kTopN);
  const int j = static_cast<int>(cand - c * static_cast<long long>(acquire::kTopN));
  const int st = o.top_start[cand];
  if (!icfo_live(st, n, lead, n_fft, cp)) return;  // k_sc_select wrote the zeros; uniform over the workgroup
  f2* fq = sh;
  const auto* kn = uniform_table(known);
  for (int i = threadIdx.x; i < n_fft; i += 256) fq[i] = freq[cand * n_fft + i];
  __syncthreads();
  const int half = n_fft >> 1, mask = n_fft - 1;
  Pick b{0.0f, 0x7fffffff};
  for (int si = threadIdx.x; si <= n_fft; si += 256) {  // shift si - half, ascending per lane
    float cr = 0.0f, ci = 0.0f;
    for (int bin = 0; bin < n_fft; ++bin) {
      const f2 k = kn[bin], v = fq[(bin + si - half) & mask];
      const float ki = -k.y;  // conj(k) v, the plain product
      cr += k.x * v.x - ki * v.y;
      ci += k.x * v.y + ki * v.x;
    }
    const float mag = cr * cr + ci * ci;
    if (mag > -1.0f && (b.idx == 0x7fffffff || mag > b.key)) b = Pick{mag, si};
  }
  b = block_pick(b, red);
  if (threadIdx.x == 0) {
    const int bins = b.idx == 0x7fffffff ? 0 : b.idx - half;
    o.top_bins[cand] = bins;
    if (o.accepted_in_top[c] == j) o.accepted_bins[c] = bins;
  }
}

__global__ __launch_bounds__(256) void k_acq_correct(const f2* __restrict__ iq, long long n, float spacing, float fs,
                                                     SyncOut o, f2* __restrict__ rows, int32_t* __restrict__ avail,
                                                     float* __restrict__ total_cfo) {
  const long long c = blockIdx.y;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int st = o.accepted_start[c];
  if (st < 0) {
    rows[c * n + i] = f2{0.0f, 0.0f};
    if (i == 0) {
      avail[c] = 0;
      total_cfo[c] = 0.0f;
    }
    return;
  }
  const float total = o.accepted_cfo_hz[c] + static_cast<float>(o.accepted_bins[c]) * spacing;
  const long long src = st + i;
  f2 v{0.0f, 0.0f};
  if (src < n) v = cmul_rot(iq[c * n + src], phasor_q64(static_cast<uint64_t>(i + 1), rot_step_q64(-total, fs)));
  rows[c * n + i] = v;
  if (i == 0) {
    avail[c] = static_cast<int32_t>(n - st);
    total_cfo[c] = total;
  }
}

__global__ __launch_bounds__(256) void k_acq_weights(const f2* __restrict__ freq, const f2* __restrict__ known,
                                                     long long count, int n_fft, f2* __restrict__ w) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < count) w[i] = eq_weight(cdiv_nc(freq[i], known[i % n_fft]));
}

// The ideal point of v's hard decision: bit 1 where the LLR is <= 0 (a symbol on a BPSK / QPSK
// axis goes to the negative side), the QAM axes by the decider's thresholds.
__device__ __forceinline__ f2 ideal_point(int order, f2 v, const float* __restrict__ thr, const float* __restrict__ axis) {
  const float r = 0.70710678118654752440f;
  if (order == ofdm::kBpsk) return f2{v.x <= 0.0f ? -1.0f : 1.0f, 0.0f};
  if (order == ofdm::kQpsk) return f2{v.x <= 0.0f ? -r : r, v.y <= 0.0f ? -r : r};
  return f2{axis[decide_axis(v.x, order, thr)], axis[decide_axis(v.y, order, thr)]};
}

// One wave per frame: the frame's equalized symbols y = raw w[data bin] are recomputed where
// they are needed (a product per use, no intermediate store). Pass 1 is the decision-directed
// loop, serial over the symbols: lanes across the carriers, the accumulator by wave reduction
// (every lane ends with the same sums, so phase, freq and the running least-squares sums stay
// wave-uniform). Pass 2 takes the fitted ramp out. Fewer than 4 symbols: y as it is.
__global__ __launch_bounds__(64) void k_frame_eq_cpe(const f2* __restrict__ raw, const f2* __restrict__ weights, int nsym,
                                                     OfdmDev c, f2* __restrict__ out) {
  const long long f = blockIdx.x;
  const int lane = threadIdx.x, nd = c.nd;
  const f2* __restrict__ r = raw + f * nsym * nd;
  const f2* __restrict__ w = weights + f * c.n;
  f2* __restrict__ y = out + f * nsym * nd;
  const bool track = nsym >= 4 && nd > 0;
  float slope = 0.0f, intercept = 0.0f;
  bool apply = false;
  if (track) {
    float phase = 0.0f, freq = 0.0f, sum_y = 0.0f, sum_ky = 0.0f;
    for (int k = 0; k < nsym; ++k) {
      float s, co;
      sincos_cr(-phase, &s, &co);
      f2 acc{0.0f, 0.0f};
      for (int i = lane; i < nd; i += 64) {
        const f2 v = cmul_nc(cmul_nc(r[k * nd + i], w[c.data_bins[i]]), f2{co, s});
        const f2 id = ideal_point(c.order, v, c.thr, c.axis);
        const float ii = -id.y;  // v * conj(ideal), the plain product
        acc.x += v.x * id.x - v.y * ii;
        acc.y += v.x * ii + v.y * id.x;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        acc.x += __shfl_xor(acc.x, off, 64);
        acc.y += __shfl_xor(acc.y, off, 64);
      }
      const float err = (acc.x == 0.0f && acc.y == 0.0f) ? 0.0f : atan2f(acc.y, acc.x);
      const float m = phase + err;
      sum_y += m;
      sum_ky += static_cast<float>(k) * m;
      phase += freq + 0.5f * err;
      freq += 0.05f * err;
    }
    const float n = static_cast<float>(nsym);
    const float sum_k = n * (n - 1.0f) / 2.0f;
    const float sum_k2 = (n - 1.0f) * n * (2.0f * n - 1.0f) / 6.0f;
    const float denom = n * sum_k2 - sum_k * sum_k;
    if (!(fabsf(denom) <= 1.1920929e-7f)) {
      slope = (n * sum_ky - sum_k * sum_y) / denom;
      intercept = (sum_y - slope * sum_k) / n;
      apply = true;
    }
  }
  for (int k = 0; k < nsym; ++k) {
    float s = 0.0f, co = 1.0f;
    if (apply) sincos_cr(-(intercept + slope * static_cast<float>(k)), &s, &co);
    for (int i = lane; i < nd; i += 64) {
      const f2 v = cmul_nc(r[k * nd + i], w[c.data_bins[i]]);
      y[k * nd + i] = apply ? cmul_nc(v, f2{co, s}) : v;
    }
  }
}

}  // namespace

void launch_acq_correct(const f2* iq, long long ncap, long long n, float spacing, float fs, const SyncOut& o, f2* rows,
                        int32_t* avail, float* total_cfo, hipStream_t s) {
  if (ncap <= 0 || n <= 0) return;
  hipLaunchKernelGGL(k_acq_correct, dim3(static_cast<unsigned>(div_up(n, 256)), static_cast<unsigned>(ncap)), dim3(256), 0, s,
                     iq, n, spacing, fs, o, rows, avail, total_cfo);
  ORION_LAUNCH_CHECK();
}

void launch_acq_weights(const f2* freq, const f2* known, long long count, int n_fft, f2* weights, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_acq_weights, dim3(static_cast<unsigned>(div_up(count, 256))), dim3(256), 0, s, freq, known, count,
                     n_fft, weights);
  ORION_LAUNCH_CHECK();
}

void launch_frame_eq_cpe(const f2* raw, const f2* weights, long long frames, int nsym, const OfdmDev& c, f2* out,
                         hipStream_t s) {
  if (frames <= 0 || nsym <= 0) return;
  hipLaunchKernelGGL(k_frame_eq_cpe, dim3(static_cast<unsigned>(frames)), dim3(64), 0, s, raw, weights, nsym, c, out);
  ORION_LAUNCH_CHECK();
}

void launch_sc_metric(const f2* iq, long long ncap, long long n, int R, int L, long long start, long long nd, float den,
                      const SyncOut& o, hipStream_t s) {
  if (ncap <= 0 || nd <= 0) return;
  const dim3 grid(static_cast<unsigned>(div_up(nd, kScThreads)), static_cast<unsigned>(ncap));
  const long long staged = static_cast<long long>(kScThreads) + static_cast<long long>(R) * L;
  if (staged <= kScLdsSamples)
    hipLaunchKernelGGL(k_sc_metric<true>, grid, dim3(kScThreads), static_cast<size_t>(staged) * sizeof(f2), s, iq, n, R, L,
                       start, nd, den, o.p, o.r, o.score, o.cfo_hz);
  else
    hipLaunchKernelGGL(k_sc_metric<false>, grid, dim3(kScThreads), 0, s, iq, n, R, L, start, nd, den, o.p, o.r, o.score,
                       o.cfo_hz);
  ORION_LAUNCH_CHECK();
}

void launch_sc_select(long long ncap, long long nd, long long start, float thr, long long cluster, const SyncOut& o,
                      hipStream_t s) {
  if (ncap <= 0) return;
  hipLaunchKernelGGL(k_sc_select, dim3(static_cast<unsigned>(ncap)), dim3(kSelThreads), 0, s, nd, start, thr, cluster, o);
  ORION_LAUNCH_CHECK();
}

void launch_icfo_gather(const f2* iq, long long ncap, long long n, long long nd, long long start, int lead, int n_fft,
                        int cp, float fs, const SyncOut& o, f2* sym, hipStream_t s) {
  if (ncap <= 0) return;
  hipLaunchKernelGGL(k_icfo_gather, dim3(static_cast<unsigned>(ncap * static_cast<long long>(acquire::kTopN))), dim3(256), 0,
                     s, iq, n, nd, start, lead, n_fft, cp, fs, o, sym);
  ORION_LAUNCH_CHECK();
}

void launch_icfo_corr(const f2* freq, const f2* known, long long ncap, long long n, int lead, int n_fft, int cp,
                      const SyncOut& o, hipStream_t s) {
  if (ncap <= 0) return;
  hipLaunchKernelGGL(k_icfo_corr, dim3(static_cast<unsigned>(ncap * static_cast<long long>(acquire::kTopN))), dim3(256),
                     static_cast<size_t>(n_fft) * sizeof(f2), s, freq, known, n, lead, n_fft, cp, o);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
