// k_sync.hip — FT8 / FT4 frame sync on the device: the symbol-rate Goertzel waterfall
// (sync/waterfall.rs:73-160), the Costas candidate search (sync/costas.rs:48-174,
// sync/ft4_sync.rs:122-219) and the max-log LLRs (sync/ft8_sync.rs:170-246,
// sync/ft4_sync.rs:227-292), each in the reference's own f32 operation order (this TU
// is built with -ffp-contract=off: every FMA below is written out).
#include "kernels.hpp"

namespace orion {

// ---------------------------------------------------------------- waterfall --
// One lane owns one tone and S consecutive symbol rows of one channel. The phasor
// recurrence p <- mul(p, w) (waterfall.rs:155-160) restarts at (1, 0) in every row, so
// the S rows share it: one dependent FMA chain per lane, hidden under the S independent
// accumulations. A row's samples are the same for every lane of the wave: they are read
// through the constant address space (scalar loads, hip_common.hpp uniform_table).
// Per cell, in sample order: acc += x * p with num-complex's non-fused product and two
// plain adds; e = re^2 + im^2 non-fused (norm_sqr). mode 0 stores ln(e + 1e-12), mode 1
// e itself. A row that starts at or past the end of the buffer stores 0.0 in both modes
// (waterfall.rs:99-102); a row the buffer ends inside uses the samples it has (:104-109).
template <int S>
__global__ __launch_bounds__(64) void k_waterfall(const f2* __restrict__ x, const f2* __restrict__ w,
                                                  float* __restrict__ out, long long n, int sps, int num_syms,
                                                  int num_tones, long long time_offset, int mode) {
  const int tone = blockIdx.x * 64 + threadIdx.x;
  const int row0 = blockIdx.y * S;
  const long long ch = blockIdx.z;
  const auto* xc = uniform_table(x + ch * n);
  long long start[S];
  int len[S];
  int full = sps, longest = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int r = row0 + s;
    start[s] = time_offset + static_cast<long long>(r) * sps;
    const long long left = n - start[s];
    len[s] = (r < num_syms && left > 0) ? static_cast<int>(left < sps ? left : sps) : 0;
    full = len[s] < full ? len[s] : full;
    longest = len[s] > longest ? len[s] : longest;
  }
  const f2 wk = tone < num_tones ? w[tone] : f2{1.0f, 0.0f};
  f2 p = {1.0f, 0.0f};
  f2 acc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = f2{0.0f, 0.0f};
  int i = 0;
  // every row of the group has sample i: no per-row test
#pragma unroll 4
  for (; i < full; ++i) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f2 v = xc[start[s] + i];
      const f2 m = {v.x * p.x - v.y * p.y, v.x * p.y + v.y * p.x};
      acc[s] += m;
    }
    p = cmul_rot(p, wk);
  }
  // the buffer ends inside this group: rows drop out as their samples run out
  for (; i < longest; ++i) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (i < len[s]) {
        const f2 v = xc[start[s] + i];
        const f2 m = {v.x * p.x - v.y * p.y, v.x * p.y + v.y * p.x};
        acc[s] += m;
      }
    }
    p = cmul_rot(p, wk);
  }
  if (tone >= num_tones) return;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int r = row0 + s;
    if (r >= num_syms) continue;
    const float e = acc[s].x * acc[s].x + acc[s].y * acc[s].y;
    float v = mode == 0 ? logf(e + 1e-12f) : e;
    if (len[s] == 0) v = 0.0f;
    out[(ch * num_syms + r) * num_tones + tone] = v;
  }
}

void launch_waterfall(const f2* x_dev, const f2* steps_dev, float* out_dev, int nch, long long n, int sps, int num_syms,
                      int num_tones, long long time_offset, int mode, int rows_per_lane, hipStream_t s) {
  if (nch < 1 || num_syms < 1 || num_tones < 1) return;
  const dim3 grid(div_up(num_tones, 64), div_up(num_syms, rows_per_lane), nch);
#define ORION_WF(S)                                                                                            \
  case S:                                                                                                      \
    k_waterfall<S><<<grid, 64, 0, s>>>(x_dev, steps_dev, out_dev, n, sps, num_syms, num_tones, time_offset, mode); \
    break;
  switch (rows_per_lane) {
    ORION_WF(1)
    ORION_WF(2)
    ORION_WF(4)
    ORION_WF(8)
    default:
      throw std::invalid_argument("waterfall: rows per lane must be 1, 2, 4 or 8");
  }
#undef ORION_WF
  ORION_LAUNCH_CHECK();
}

// ------------------------------------------------------------- Costas scores --
// One thread per (time_sym, freq_bin) of one channel: the clamped differences summed in
// the reference's (block, ci) order, with its skips (rows outside the waterfall, bins
// past its last column) and its -inf neighbours at the edges (costas.rs:58-108).
__global__ __launch_bounds__(256) void k_costas_score(const float* __restrict__ wf, float* __restrict__ score,
                                                      int num_syms, int num_tones, int t_min, int nt, int nfb,
                                                      CostasPattern pat) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nt * nfb) return;
  const long long ch = blockIdx.y;
  const float* g = wf + ch * num_syms * num_tones;
  const int time_sym = t_min + idx / nfb;
  const int freq_bin = idx % nfb;
  const float ninf = -__builtin_inff();
  float total = 0.0f;
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
    for (int ci = 0; ci < 7; ++ci) {
      if (blk >= pat.nblk || ci >= pat.len) continue;
      const int sym = time_sym + pat.pos[blk] + ci;
      if (sym < 0 || sym >= num_syms) continue;
      const int bin = freq_bin + pat.tone[blk][ci];
      if (bin >= num_tones) continue;
      const float* row = g + static_cast<long long>(sym) * num_tones;
      const float e_signal = row[bin];
      const float left = bin > 0 ? row[bin - 1] : ninf;
      const float right = bin + 1 < num_tones ? row[bin + 1] : ninf;
      const float prev = sym > 0 ? row[bin - num_tones] : ninf;
      const float next = sym + 1 < num_syms ? row[bin + num_tones] : ninf;
      const float diff = e_signal - fmaxf(fmaxf(left, right), fmaxf(prev, next));
      total += fmaxf(diff, 0.0f);
    }
  }
  score[ch * nt * nfb + idx] = total;
}

// The reference's keep-N scan (costas.rs:144-173), replayed over the finished score map
// by one wave per channel. Its list, ties included: the first N scores in scan order,
// sorted ascending by a stable sort; then every score > heap[0].score replaces heap[0]
// and the list is re-sorted (stable: the new entry, coming from index 0, lands after
// every smaller score and before every equal one); at the end a stable descending sort.
// The wave reads 64 scores at a time and skips the chunk when none beats heap[0].score,
// which only grows; survivors are replayed in scan order by lane 0, which alone touches
// the list (in the caller's candidate array).
__global__ __launch_bounds__(64) void k_costas_topn(const float* __restrict__ score, long long total, int nfb,
                                                    int t_min, int max_cand, SyncCandidate* __restrict__ out,
                                                    uint32_t* __restrict__ count) {
  const long long ch = blockIdx.x;
  const int lane = threadIdx.x;
  const float* sc = score + ch * total;
  SyncCandidate* heap = out + ch * max_cand;
  const int first = static_cast<int>(total < max_cand ? total : max_cand);
  const bool filled = first == max_cand;
  float thr = 0.0f;
  if (lane == 0) {
    for (int k = 0; k < first; ++k) heap[k] = SyncCandidate{t_min + k / nfb, static_cast<uint32_t>(k % nfb), sc[k]};
    if (filled) {
      for (int i = 1; i < first; ++i) {  // stable, ascending
        const SyncCandidate key = heap[i];
        int j = i - 1;
        for (; j >= 0 && heap[j].score > key.score; --j) heap[j + 1] = heap[j];
        heap[j + 1] = key;
      }
      thr = heap[0].score;
    }
  }
  thr = __shfl(thr, 0);
  if (filled) {
    for (long long base = first; base < total; base += 64) {
      const long long idx = base + lane;
      const float v = idx < total ? sc[idx] : -__builtin_inff();
      unsigned long long mask = __ballot(v > thr);
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float cand = __shfl(v, l);
        if (cand > thr) {  // wave-uniform
          if (lane == 0) {
            const long long k = base + l;
            int j = 1;
            for (; j < max_cand && heap[j].score < cand; ++j) heap[j - 1] = heap[j];
            heap[j - 1] = SyncCandidate{t_min + static_cast<int>(k / nfb), static_cast<uint32_t>(k % nfb), cand};
            thr = heap[0].score;
          }
          thr = __shfl(thr, 0);
        }
      }
    }
  }
  if (lane == 0) {
    for (int i = 1; i < first; ++i) {  // stable, descending
      const SyncCandidate key = heap[i];
      int j = i - 1;
      for (; j >= 0 && heap[j].score < key.score; --j) heap[j + 1] = heap[j];
      heap[j + 1] = key;
    }
    for (int k = first; k < max_cand; ++k) heap[k] = SyncCandidate{0, 0u, 0.0f};
    count[ch] = static_cast<uint32_t>(first);
  }
}

// No candidates at all (the waterfall is no wider than a frame, costas.rs:138-142).
__global__ __launch_bounds__(64) void k_costas_none(int nch, int max_cand, SyncCandidate* __restrict__ out,
                                                    uint32_t* __restrict__ count) {
  const long long total = static_cast<long long>(nch) * max_cand;
  for (long long i = blockIdx.x * 64LL + threadIdx.x; i < total; i += 64LL * gridDim.x) out[i] = SyncCandidate{0, 0u, 0.0f};
  for (long long i = blockIdx.x * 64LL + threadIdx.x; i < nch; i += 64LL * gridDim.x) count[i] = 0u;
}

void launch_costas_search(const float* wf_dev, float* score_dev, int nch, int num_syms, int num_tones,
                          const CostasPattern& pat, int t_min, int t_max, int max_cand, SyncCandidate* cand_dev,
                          uint32_t* count_dev, hipStream_t s) {
  if (nch < 1) return;
  if (num_tones <= pat.tones) {
    k_costas_none<<<div_up(static_cast<long long>(nch) * max_cand + nch, 64 * 16), 64, 0, s>>>(nch, max_cand, cand_dev,
                                                                                             count_dev);
    ORION_LAUNCH_CHECK();
    return;
  }
  const int nfb = num_tones - pat.tones + 1;
  const long long nt64 = t_max >= t_min ? static_cast<long long>(t_max) - t_min + 1 : 0;
  const long long total = nt64 * nfb;
  if (total > 0x7fffffffLL) throw std::invalid_argument("costas search: more than 2^31 - 1 (time_sym, freq_bin) cells");
  const int nt = static_cast<int>(nt64);
  if (total > 0) {
    k_costas_score<<<dim3(div_up(total, 256), nch), 256, 0, s>>>(wf_dev, score_dev, num_syms, num_tones, t_min, nt,
                                                                 nfb, pat);
    ORION_LAUNCH_CHECK();
  }
  k_costas_topn<<<nch, 64, 0, s>>>(score_dev, total, nfb, t_min, max_cand, cand_dev, count_dev);
  ORION_LAUNCH_CHECK();
}

// --------------------------------------------------------------------- LLRs --
__device__ __forceinline__ float max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }

// One lane per candidate: the Gray-reordered max-log differences, negated
// (ft8_sync.rs:198-224, ft4_sync.rs:257-274; a data symbol outside the waterfall leaves
// zeros), then normalise_llr (ft8_sync.rs:237-246): variance = (the sequential sum of
// x * x) / 174, and when it exceeds 1e-10 every value times sqrt(24 / variance) (IEEE
// divide and sqrt). Slots past a channel's count are zeroed. cand_out (optional): the
// record with time_sym - sym_adj, ft8_sync.rs:151.
__global__ __launch_bounds__(64) void k_sync_llr(const float* __restrict__ wf, int num_syms, int num_tones, int ft4,
                                                 const SyncCandidate* cand, const uint32_t* __restrict__ count,
                                                 int max_cand, float* __restrict__ llr, SyncCandidate* cand_out,
                                                 int sym_adj) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= max_cand) return;
  const long long ch = blockIdx.y;
  float* L = llr + (ch * max_cand + c) * kSyncLlr;
  if (static_cast<uint32_t>(c) >= count[ch]) {
    for (int k = 0; k < kSyncLlr; ++k) L[k] = 0.0f;
    return;
  }
  const SyncCandidate cd = cand[ch * max_cand + c];
  const float* g = wf + ch * num_syms * num_tones;
  const float ninf = -__builtin_inff();
  const long long fb = cd.freq_bin;
  if (!ft4) {
    for (int k = 0; k < 58; ++k) {
      const int frame_sym = k < 29 ? k + 7 : k + 14;  // data at [7, 36) and [43, 72)
      const long long r = static_cast<long long>(cd.time_sym) + frame_sym;
      float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
      if (r >= 0 && r < num_syms) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = fb + j < num_tones ? g[r * num_tones + fb + j] : ninf;
        // s2[j] = t[FT8_GRAY8[j]], FT8_GRAY8 = [0, 1, 3, 2, 5, 6, 4, 7]
        const float s0 = t[0], s1 = t[1], s2 = t[3], s3 = t[2], s4 = t[5], s5 = t[6], s6 = t[4], s7 = t[7];
        l0 = -(max4(s4, s5, s6, s7) - max4(s0, s1, s2, s3));
        l1 = -(max4(s2, s3, s6, s7) - max4(s0, s1, s4, s5));
        l2 = -(max4(s1, s3, s5, s7) - max4(s0, s2, s4, s6));
      }
      L[3 * k] = l0;
      L[3 * k + 1] = l1;
      L[3 * k + 2] = l2;
    }
  } else {
    for (int k = 0; k < 87; ++k) {
      const int frame_sym = k < 29 ? k + 5 : (k < 58 ? k + 9 : k + 13);
      const long long r = static_cast<long long>(cd.time_sym) + frame_sym;
      float l0 = 0.0f, l1 = 0.0f;
      if (r >= 0 && r < num_syms) {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = fb + j < num_tones ? g[r * num_tones + fb + j] : ninf;
        // s2[j] = t[FT4_GRAY4[j]], FT4_GRAY4 = [0, 1, 3, 2]
        const float s0 = t[0], s1 = t[1], s2 = t[3], s3 = t[2];
        l0 = -(fmaxf(s2, s3) - fmaxf(s0, s1));
        l1 = -(fmaxf(s1, s3) - fmaxf(s0, s2));
      }
      L[2 * k] = l0;
      L[2 * k + 1] = l1;
    }
  }
  float sum = 0.0f;
  for (int k = 0; k < kSyncLlr; ++k) {
    const float v = L[k];
    sum += v * v;
  }
  const float variance = sum / static_cast<float>(kSyncLlr);
  if (variance > 1e-10f) {
    const float scale = sqrtf(24.0f / variance);
    for (int k = 0; k < kSyncLlr; ++k) L[k] *= scale;
  }
  if (cand_out) cand_out[ch * max_cand + c] = SyncCandidate{cd.time_sym - sym_adj, cd.freq_bin, cd.score};
}

void launch_sync_llr(const float* wf_dev, int nch, int num_syms, int num_tones, bool ft4, const SyncCandidate* cand_dev,
                     const uint32_t* count_dev, int max_cand, float* llr_dev, SyncCandidate* cand_out_dev, int sym_adj,
                     hipStream_t s) {
  if (nch < 1 || max_cand < 1) return;
  k_sync_llr<<<dim3(div_up(max_cand, 64), nch), 64, 0, s>>>(wf_dev, num_syms, num_tones, ft4 ? 1 : 0, cand_dev, count_dev,
                                                            max_cand, llr_dev, cand_out_dev, sym_adj);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
