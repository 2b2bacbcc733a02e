// k_ftmod.hip — FT8 / FT4 on the transmit side and the hard demodulator: slot synthesis
// (Ft8Mod / Ft4Mod::modulate, modulate/ft8.rs:88-156, ft4.rs:106-173, as the closed form
// of the reference's own f32 steps) and detect_tone over every symbol of a frame
// (demodulate/ft8.rs:33-126, ft4.rs) in the reference's f32 operation order (this TU is
// built with -ffp-contract=off: every FMA below is written out).
#include "kernels.hpp"

namespace orion {

// ------------------------------------------------------------- synthesis --
// Output-centric: one thread per output sample of one channel, looping over that
// channel's signals in list order (rows[ch] .. rows[ch + 1] of the table sorted by
// channel). A signal whose frame covers sample i adds g e^{j 2 pi ph / 2^64}, ph =
// enter[s] + (k + 1) step[s] for t = i - offset, s = t / SPS, k = t % SPS: the phasor
// the reference's recurrence holds after that sample's step, but for its rounding drift.
// Plain f32 adds in a fixed order, every output written once, nothing read back (but the
// buffer's own value with accumulate): bit-reproducible. A signal's offset and gain are
// wave-uniform (scalar loads); enter[s] / step[s] differ inside a workgroup only where it
// straddles a symbol boundary (SPS >= 576 > 256 threads: at most two symbols).
// rot (optional): Rotator::rotate_block phasors, applied to the sum of sample i
// (rotator.rs:79-82); the host passes it only with i < the table's length.
template <int SPS, int TOTAL>
__global__ __launch_bounds__(256) void k_ft_synth(const FtSynthRecord* __restrict__ rec,
                                                  const uint32_t* __restrict__ rows, f2* __restrict__ out,
                                                  long long n, int accumulate, const f2* __restrict__ rot) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= n) return;
  const long long ch = blockIdx.y;
  const auto* row = uniform_table(rows);
  const uint32_t j0 = row[ch], j1 = row[ch + 1];
  f2* o = out + ch * n + i;
  f2 acc = accumulate ? *o : f2{0.0f, 0.0f};
  constexpr uint32_t kLen = static_cast<uint32_t>(SPS) * TOTAL;
  for (uint32_t j = j0; j < j1; ++j) {
    const auto* r = uniform_table(rec + j);
    const long long off = r->offset;
    const float g = r->gain;
    if (i < off) continue;
    const unsigned long long t64 = static_cast<unsigned long long>(i) - static_cast<unsigned long long>(off);
    if (t64 >= kLen) continue;
    const uint32_t t = static_cast<uint32_t>(t64);
    const uint32_t s = t / SPS, k = t - s * SPS;
    const uint64_t ph = rec[j].enter[s] + static_cast<uint64_t>(k + 1u) * rec[j].step[s];
    const f2 z = phasor_at(ph);
    acc += f2{g * z.x, g * z.y};
  }
  if (rot) acc = cmul_rot(acc, rot[i]);
  *o = acc;
}

void launch_ft_synth(bool ft4, const FtSynthRecord* rec_dev, const uint32_t* rows_dev, f2* out_dev, int nch, long long n,
                     bool accumulate, const f2* rot_dev, hipStream_t s) {
  if (nch < 1 || n < 1) return;
  // channels ride grid dimension y in slices of at most 65535
  for (int c0 = 0; c0 < nch; c0 += 65535) {
    const int c = nch - c0 < 65535 ? nch - c0 : 65535;
    const dim3 grid(div_up(n, 256), c);
    if (ft4)
      k_ft_synth<576, 105><<<grid, 256, 0, s>>>(rec_dev, rows_dev + c0, out_dev + c0 * n, n, accumulate ? 1 : 0, rot_dev);
    else
      k_ft_synth<1920, 79><<<grid, 256, 0, s>>>(rec_dev, rows_dev + c0, out_dev + c0 * n, n, accumulate ? 1 : 0, rot_dev);
    ORION_LAUNCH_CHECK();
  }
}

// ----------------------------------------------------------- demodulator --
// One wave owns R consecutive symbols of one frame, all T tones: lane = row * T + tone
// (8 x 8 for FT8, 16 x 4 for FT4), so that every lane works, where k_waterfall (one lane
// per tone) would keep 8 or 4 of 64 busy. The phasor restarts at (1, 0) in every symbol,
// so the lanes of one tone run the same chain. The R rows' samples are staged through LDS
// in tiles of kTile: the wave loads each row's tile coalesced, and every lane reads its
// row's samples back in order (the T lanes of a row read one address: a broadcast). The
// next tile's global loads are in flight while the current one is accumulated. Per cell,
// in sample order: acc += x * p with num-complex's non-fused product and two plain adds,
// p <- cmul_rot(p, w); e = re^2 + im^2 non-fused (detect_tone; goertzel_energy of
// waterfall.rs:126-160 is the same arithmetic). The argmax runs over a row's tone lanes in
// tone order with strict > from -1.0: a NaN never wins, an all-NaN symbol gives tone 0.
// The last group of a frame is partial (79 = 9 * 8 + 7, 105 = 6 * 16 + 9): its missing
// rows load nothing and store nothing.
constexpr int kDemodTile = 64;                 // samples per row and tile (SPS is a multiple)
constexpr int kDemodRowF2 = kDemodTile + 2;    // row stride in LDS (f2): 528 B, rows 4 banks apart
struct FtDemodSteps {
  f2 w[8];
};
template <int T, int R, int SPS, int TOTAL, int DATA>
__global__ __launch_bounds__(64) void k_ft_demod(const f2* __restrict__ x, long long n, FtDemodSteps st,
                                                 uint8_t* __restrict__ tones, float* __restrict__ energies) {
  static_assert(T * R == 64 && SPS % kDemodTile == 0, "one wave, whole tiles");
  __shared__ f2 lds[R * kDemodRowF2];
  const int lane = threadIdx.x;
  const int tone = lane % T, rl = lane / T;
  const int row0 = blockIdx.x * R;
  const long long frame = blockIdx.y;
  const f2* xf = x + frame * n + static_cast<long long>(row0) * SPS;
  const int rows = TOTAL - row0 < R ? TOTAL - row0 : R;  // >= 1
  f2 wk = st.w[0];
#pragma unroll
  for (int k = 1; k < T; ++k) wk = tone == k ? st.w[k] : wk;
  f2 p = {1.0f, 0.0f}, acc = {0.0f, 0.0f};
  f2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = r < rows ? xf[r * SPS + lane] : f2{0.0f, 0.0f};
  const f2* mine = lds + rl * kDemodRowF2;
  for (int t0 = 0; t0 < SPS; t0 += kDemodTile) {
#pragma unroll
    for (int r = 0; r < R; ++r) lds[r * kDemodRowF2 + lane] = v[r];
    wave_lds_fence();
    if (t0 + kDemodTile < SPS) {
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = r < rows ? xf[r * SPS + t0 + kDemodTile + lane] : f2{0.0f, 0.0f};
    }
#pragma unroll 8
    for (int i = 0; i < kDemodTile; ++i) {
      const f2 s = mine[i];
      const f2 m = {s.x * p.x - s.y * p.y, s.x * p.y + s.y * p.x};
      acc += m;
      p = cmul_rot(p, wk);
    }
    wave_lds_fence();
  }
  const float e = acc.x * acc.x + acc.y * acc.y;
  float best = -1.0f;
  int bk = 0;
#pragma unroll
  for (int k = 0; k < T; ++k) {
    const float ek = __shfl(e, rl * T + k);
    if (ek > best) {
      best = ek;
      bk = k;
    }
  }
  const int sym = row0 + rl;
  if (sym >= TOTAL) return;
  if (energies) energies[(frame * TOTAL + sym) * T + tone] = e;
  if (tone != 0) return;
  int d;  // the data index of frame symbol sym, or -1 (a Costas tone, an FT4 ramp)
  if (T == 8) {
    d = sym < 7 ? -1 : sym < 36 ? sym - 7 : sym < 43 ? -1 : sym < 72 ? sym - 14 : -1;
  } else {
    d = sym < 5 ? -1 : sym < 34 ? sym - 5 : sym < 38 ? -1 : sym < 67 ? sym - 9 : sym < 71 ? -1 : sym < 100 ? sym - 13 : -1;
  }
  if (d >= 0) tones[frame * DATA + d] = static_cast<uint8_t>(bk);
}

void launch_ft_demod(bool ft4, const f2* x_dev, int nframes, long long n, const float* steps, uint8_t* tones_dev,
                     float* energies_dev, hipStream_t s) {
  if (nframes < 1) return;
  FtDemodSteps st;
  for (int k = 0; k < 8; ++k) st.w[k] = k < (ft4 ? 4 : 8) ? f2{steps[2 * k], steps[2 * k + 1]} : f2{1.0f, 0.0f};
  // frames ride grid dimension y (the host side rejects more than 65535)
  if (ft4)
    k_ft_demod<4, 16, 576, 105, 87><<<dim3(div_up(105, 16), nframes), 64, 0, s>>>(x_dev, n, st, tones_dev, energies_dev);
  else
    k_ft_demod<8, 8, 1920, 79, 58><<<dim3(div_up(79, 8), nframes), 64, 0, s>>>(x_dev, n, st, tones_dev, energies_dev);
  ORION_LAUNCH_CHECK();
}

}  // namespace orion
