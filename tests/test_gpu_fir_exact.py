"""Per-sample tests of the FIR and decimator kernels (csrc/k_fir.hip), every path.

Each kernel instance is compared, sample for sample, with the float64 reference of
tests/fir_ref.py (validated against the C oracle in tests/test_fir_ref.py) on inputs
for which a FIR has one correct f32 answer whatever the summation order:

* integer   taps in [-7, 7] (asymmetric), samples in [-15, 15]: got == ref;
* impulse   impulses >= K apart, amplitudes +-2^e: got == ref for any f32 taps;
* dense     standard-normal samples: |got - ref64| <= gamma_K sum |g| |x| per sample
            (the a-priori bound; printed as `[parity] ... worst |err| / bound`).

Which launch each test reaches (conditions read from launch_fir_real, launch_fir_iq,
launch_fir_iq_aligned_inplace and launch_decim_batch) is in each docstring. The host
process() splits calls of >= 2^21 samples into chunks, so every size-dependent path is
driven through process_device on device tensors.
"""
import numpy as np
import pytest

import fir_ref as R

pytestmark = pytest.mark.gpu

NT = 256          # k_fir.hip: workgroup size
MAX_GRID = 2048   # k_fir.hip kMaxGrid: more tiles than this take the grid-stride pass
FIR4_TILES_PER_CU = 4  # k_fir.hip kFir4TilesPerCu

IQ_KS = [1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 301]
REAL_DESIGNS = [(48e3, 3000.0, 800.0, 61), (1.25e6, 15e3, 10e3, 125), (48e3, 1000.0, 250.0, 193),
                (48e3, 500.0, 150.0, 321)]
# (fs, m, cutoff, trans, taps): k_decim_w4<16>, k_decim_w4q, and k_decim_generic with
# m = 4 / 41 taps, m = 8 / 335 taps (> 256) and m = 4 / 161 taps (129..256, m != 8)
DECIM_DESIGNS = [(10e6, 8, 200e3, 79e3, 127), (10e6, 8, 190e3, 39370.0, 255), (96e3, 4, 10.8e3, 2.4e3, 41),
                 (10e6, 8, 100e3, 30e3, 335), (96e3, 4, 3e3, 600.0, 161)]


def float_taps(K, seed=0):
    """Arbitrary f32 taps with no symmetry."""
    return np.random.default_rng(500 + K + seed).standard_normal(K).astype(np.float32)


def odd_at_least(K):
    """Impulse spacing: >= K, and odd, so coprime to every tile length (a power of two)
    and to the decimation factors used here: a long train visits every position within
    a tile, and every residue of the tap index mod m."""
    return K | 1


def thr8(lib):
    """launch_fir_iq: calls of n_out * nch below this take 4 outputs per lane."""
    return FIR4_TILES_PER_CU * lib.device_cus() * 8 * NT


def exact(got, ref64, what):
    assert R.same(got, ref64), f"{what}: {R.first_diffs(got, ref64)}"


class Worst:
    """The worst |err| / bound of a dense-random test, printed and asserted once."""

    def __init__(self, name):
        self.name, self.w, self.where = name, 0.0, ""

    def add(self, got, ref64, b, what):
        assert got.shape == ref64.shape and np.all(np.isfinite(got)), what
        w = R.worst_ratio(got, ref64, b)
        if w > self.w:
            self.w, self.where = w, what
        return w

    def done(self):
        print(f"[parity] {self.name}: worst |err| / bound {self.w:.3f} ({self.where})")
        assert self.w <= 1.0, f"{self.name}: |err| / bound {self.w:.3f} at {self.where}"


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_impulses(n, pos, amp):
    """impulse_signal on the device (no n-sized host array)."""
    import torch

    x = torch.zeros(n, dtype=torch.complex64 if np.iscomplexobj(amp) else torch.float32, device="cuda")
    x[dev(pos)] = dev(amp)
    return x


def run_calls(blk, x, lens):
    return [blk.process(np.ascontiguousarray(c)) for c in R.split_calls(x, lens)]


# ======================================================================= FirLowpassIq ==
IQ_NS = [1, 3, 1023, 1024, 1025, 2049, 5000]


@pytest.mark.parametrize("K", IQ_KS)
def test_firiq_integer(gpu_lib, K):
    """Integer class, 4 outputs per lane (n * nch < thr8): k_fir_iq8<64|128|256, false, 4>
    for K <= 64 / 128 / 256, k_fir_iq_generic for K > 256; one tile, a tile and one
    sample, several tiles; 3 channels of 2049 (odd x_stride: the scalar store branch)."""
    g = R.int_taps(K)
    assert max(IQ_NS) * 3 < thr8(gpu_lib)
    x = R.int_samples(max(IQ_NS), K)
    for n in IQ_NS:
        F = gpu_lib.FirLowpassIq.from_taps(g)
        assert np.array_equal(F.taps(), g)
        exact(F.process(x[:n]), R.fir64(x[:n], g), f"K={K} n={n}")
    x3 = R.int_samples((3, 2049), K + 1)
    got = gpu_lib.FirLowpassIq.from_taps(g, channels=3).process(x3)
    for c in range(3):
        exact(got[c], R.fir64(x3[c], g), f"K={K} 3 ch n=2049 ch={c}")


@pytest.mark.parametrize("K", IQ_KS)
def test_firiq_impulse(gpu_lib, K):
    """Impulse class with arbitrary f32 taps, 4 outputs per lane (launches as
    test_firiq_integer). Short calls with shifted trains, then one train of d * 1024
    samples, d odd: its impulses fall on every position of the 1024-output tile, so
    every (output within a tile, tap) pair occurs, through the interior staging path."""
    g = float_taps(K)
    d = odd_at_least(K)
    for n in IQ_NS:
        for first in sorted({0, 1 % d, d // 2, d - 1}):
            pos, amp = R.impulses(n, d, first, K + n)
            got = gpu_lib.FirLowpassIq.from_taps(g).process(R.impulse_signal(n, pos, amp))
            exact(got, R.impulse_fir64(n, pos, amp, g), f"K={K} n={n} first={first}")
    n = min(d * 4 * NT + 4 * NT + 5, thr8(gpu_lib) - 1)
    pos, amp = R.impulses(n, d, 2, K)
    got = gpu_lib.FirLowpassIq.from_taps(g).process_device(dev_impulses(n, pos, amp)).cpu().numpy()
    exact(got, R.impulse_fir64(n, pos, amp, g), f"K={K} n={n} every tile position")
    x3 = np.stack([R.impulse_signal(2049, *R.impulses(2049, d, c, K)) for c in range(3)])
    got = gpu_lib.FirLowpassIq.from_taps(g, channels=3).process(x3)
    for c in range(3):
        exact(got[c], R.impulse_fir64(2049, *R.impulses(2049, d, c, K), g), f"K={K} 3 ch ch={c}")


@pytest.mark.parametrize("K", [64, 128, 256])
def test_firiq_eight_per_lane(gpu_lib, K):
    """8 outputs per lane, not in place (n * nch >= thr8 = 4 tiles of 2048 per CU):
    k_fir_iq8<64|128|256, false, 8>. Single channel n = thr8 + 2048 + 5, integer and
    impulse class (d odd: every position of the 2048-output tile), on device tensors."""
    n = thr8(gpu_lib) + 8 * NT + 5
    g = R.int_taps(K)
    x = R.int_samples(n, K)
    got = gpu_lib.FirLowpassIq.from_taps(g).process_device(dev(x)).cpu().numpy()
    exact(got, R.fir64(x, g), f"K={K} n={n} integer")
    g = float_taps(K)
    pos, amp = R.impulses(n, odd_at_least(K), 1, K)
    got = gpu_lib.FirLowpassIq.from_taps(g).process_device(dev_impulses(n, pos, amp)).cpu().numpy()
    exact(got, R.impulse_fir64(n, pos, amp, g), f"K={K} n={n} impulse")


def test_firiq_eight_per_lane_batched(gpu_lib):
    """k_fir_iq8<128, false, 8> with blockIdx.y channels: 3 channels whose total is just
    over thr8 (each channel alone is below it), odd x_stride."""
    K = 128
    n = (thr8(gpu_lib) // 3 + 8 * NT + 5) | 1
    assert n < thr8(gpu_lib) <= 3 * n
    g = R.int_taps(K)
    x = R.int_samples((3, n), 77)
    got = gpu_lib.FirLowpassIq.from_taps(g, channels=3).process_device(dev(x)).cpu().numpy()
    for c in range(3):
        exact(got[c], R.fir64(x[c], g), f"K={K} 3 ch n={n} ch={c}")


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("K", IQ_KS)
def test_firiq_streaming(gpu_lib, K, nch):
    """One block over calls shorter than, equal to and longer than the carried history
    (hist_next fused into k_fir_iq8<KP, false, 4>; k_hist_update after k_fir_iq_generic),
    every call compared: integer class, then an impulse train across the calls."""
    lens = [v for v in [1, 2, K - 1, K, K + 1, 1000, 1, 2049] if v > 0]
    n = sum(lens)
    d = odd_at_least(K)
    for cls in ("integer", "impulse"):
        if cls == "integer":
            g = R.int_taps(K)
            x = R.int_samples((nch, n), K)
        else:
            g = float_taps(K)
            x = np.stack([R.impulse_signal(n, *R.impulses(n, d, c % d, K)) for c in range(nch)])
        ref = np.stack([R.fir64(x[c], g) for c in range(nch)])
        if nch == 1:
            x, ref = x[0], ref[0]
        F = gpu_lib.FirLowpassIq.from_taps(g, channels=nch)
        for i, (got, r) in enumerate(zip(run_calls(F, x, lens), R.split_calls(ref, lens))):
            exact(got, r, f"K={K} {nch} ch {cls} call {i} of {lens}")


@pytest.mark.parametrize("K", [1, 2, 64, 89, 128, 255, 256, 301])
def test_firiq_filter_aligned(gpu_lib, K):
    """filter_aligned (host copy) and filter_aligned_device (in place), integer class:
    k_hist_aligned + k_fir_edges (more than one tile) + k_fir_iq8<64|128|256, true, 8>
    for K <= 256, the copy + k_fir_iq_generic fall-back for K = 301; even and odd K
    (d = (K - 1) // 2). Then a process() of 3000 samples on the same block continues
    the stream [x | 0^d | z] exactly (the history filter_aligned leaves behind)."""
    g = R.int_taps(K)
    d = (K - 1) // 2
    z = R.int_samples(3000, K + 5)
    for n in (1, 7, 2047, 2048, 2049, 6157):
        x = R.int_samples(n, K + n)
        xz = np.concatenate([x, np.zeros(d, np.complex64), z])
        full = R.fir64(xz, g)
        for where in ("host", "device"):
            F = gpu_lib.FirLowpassIq.from_taps(g)
            if where == "host":
                got = F.filter_aligned(x)
            else:
                t = dev(x)
                assert F.filter_aligned_device(t) is t
                got = t.cpu().numpy()
            exact(got, full[d:d + n], f"K={K} n={n} {where} aligned")
            exact(F.process(z), full[n + d:], f"K={K} n={n} {where} process after aligned")


def test_firiq_dense(gpu_lib):
    """Dense random within the a-priori bound, per sample: K = 64, 255, 301 streamed
    (k_fir_iq8<64|256, false, 4>, k_fir_iq_generic), in place (k_fir_iq8<.., true, 8>)
    and 8 per lane (K = 64, 255)."""
    for K in (64, 255, 301):
        W = Worst(f"firiq dense K={K}")
        g = float_taps(K)
        lens = [5000, K - 1, 2049, 1]
        x = R.dense_samples(sum(lens), K)
        ref, b = R.fir64(x, g), R.bound(x, g)
        F = gpu_lib.FirLowpassIq.from_taps(g)
        for i, (got, r, bb) in enumerate(zip(run_calls(F, x, lens), R.split_calls(ref, lens), R.split_calls(b, lens))):
            W.add(got, r, bb, f"streamed call {i}")
        d = (K - 1) // 2
        xz = np.concatenate([x, np.zeros(d, np.complex64)])
        W.add(gpu_lib.FirLowpassIq.from_taps(g).filter_aligned(x), R.fir64(xz, g)[d:], R.bound(xz, g)[d:], "aligned")
        if K <= 256:
            n = thr8(gpu_lib) + 8 * NT + 5
            x = R.dense_samples(n, K + 1)
            got = gpu_lib.FirLowpassIq.from_taps(g).process_device(dev(x)).cpu().numpy()
            W.add(got, R.fir64(x, g), R.bound(x, g), "8 per lane")
        W.done()


@pytest.mark.parametrize("form", ["in_place", "eight_per_lane"])
def test_firiq_grid_stride(gpu_lib, form):
    """The grid-stride second pass (more than kMaxGrid = 2048 tiles of 2048): n = 2048 *
    2048 + 2048 + 5, K = 128, device tensors, impulse class (the expected output is a
    scatter of taps). in_place: k_fir_iq8<128, true, 8> via filter_aligned_device;
    eight_per_lane: k_fir_iq8<128, false, 8> via process_device. One of the largest
    cases of this file (4.2 M samples)."""
    K = 128
    n = MAX_GRID * 8 * NT + 8 * NT + 5
    assert n >= thr8(gpu_lib)
    g = float_taps(K)
    d = (K - 1) // 2
    pos, amp = R.impulses(n, odd_at_least(K), 3, 9)
    x = dev_impulses(n, pos, amp)
    F = gpu_lib.FirLowpassIq.from_taps(g)
    if form == "in_place":
        got = F.filter_aligned_device(x).cpu().numpy()
        ref = R.impulse_fir64(n + d, pos, amp, g)[d:]
    else:
        got = F.process_device(x).cpu().numpy()
        ref = R.impulse_fir64(n, pos, amp, g)
    exact(got, ref, f"{form} n={n}")


# ========================================================================= FirLowpass ==
REAL_NS = [1, 5, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 77]


def real_block(lib, design):
    *args, K = design
    F = lib.FirLowpass(*args)
    g = R.standard_taps(F.taps())
    assert len(g) == K, f"FirLowpass{tuple(args)}: {len(g)} taps, expected {K}"
    return F, g


@pytest.mark.parametrize("design", REAL_DESIGNS, ids=lambda d: f"{d[3]}taps")
def test_fir_real_impulse(gpu_lib, design):
    """k_fir_real8<64> (61 taps), <128> (125), <256> (193), k_fir_real_generic (321):
    short calls around the 2048-output halves and the 4096-output tile with shifted
    trains; an output pointer 4 bytes off 16-byte alignment (the scalar store branch);
    then, for the tiled kernels, one train of d * 4096 samples, d odd, whose impulses
    fall on every position of the tile (both packed halves), interior staging path."""
    import torch

    K = design[3]
    d = odd_at_least(K + 1)
    for n in REAL_NS:
        for first in sorted({0, 1, d // 2, d - 1}):
            F, g = real_block(gpu_lib, design)
            pos, amp = R.impulses(n, d, first, K + n, complex_=False)
            exact(F.process(R.impulse_signal(n, pos, amp)), R.impulse_fir64(n, pos, amp, g), f"{K} taps n={n} first={first}")
    n = 3 * 4096 + 77
    F, g = real_block(gpu_lib, design)
    pos, amp = R.impulses(n, d, 7, K, complex_=False)
    out = torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda")
    assert out[1:].data_ptr() % 16 == 4
    got = F.process_device(dev_impulses(n, pos, amp), out[1:]).cpu().numpy()
    exact(got, R.impulse_fir64(n, pos, amp, g), f"{K} taps n={n} unaligned out")
    if K <= 256:
        n = d * 4096 + 4096 + 77
        F, g = real_block(gpu_lib, design)
        pos, amp = R.impulses(n, d, 2, K + 1, complex_=False)
        got = F.process_device(dev_impulses(n, pos, amp)).cpu().numpy()
        exact(got, R.impulse_fir64(n, pos, amp, g), f"{K} taps n={n} every tile position")


@pytest.mark.parametrize("design", REAL_DESIGNS, ids=lambda d: f"{d[3]}taps")
def test_fir_real_streaming(gpu_lib, design):
    """Calls of [1, K-1, K+1, 4097, 3] on one block, every call compared: hist_next of
    k_fir_real8<KP> (k_hist_update after k_fir_real_generic) with calls shorter and
    longer than the history. Impulse class (exact), then dense random (bound)."""
    K = design[3]
    lens = [1, K - 1, K + 1, 4097, 3]
    n = sum(lens)
    d = odd_at_least(K + 1)
    for first in sorted({0, 1, d // 2, d - 1}):
        F, g = real_block(gpu_lib, design)
        pos, amp = R.impulses(n, d, first, K, complex_=False)
        ref = R.impulse_fir64(n, pos, amp, g)
        for i, (got, r) in enumerate(zip(run_calls(F, R.impulse_signal(n, pos, amp), lens), R.split_calls(ref, lens))):
            exact(got, r, f"{K} taps first={first} call {i} of {lens}")
    W = Worst(f"fir real dense streamed {K} taps")
    F, g = real_block(gpu_lib, design)
    x = R.dense_samples(n, K, complex_=False)
    ref, b = R.fir64(x, g), R.bound(x, g)
    for i, (got, r, bb) in enumerate(zip(run_calls(F, x, lens), R.split_calls(ref, lens), R.split_calls(b, lens))):
        W.add(got, r, bb, f"call {i}")
    W.done()


@pytest.mark.parametrize("design", REAL_DESIGNS, ids=lambda d: f"{d[3]}taps")
def test_fir_real_dense(gpu_lib, design):
    """Dense random within the a-priori bound at every size of REAL_NS (launches as
    test_fir_real_impulse)."""
    K = design[3]
    W = Worst(f"fir real dense {K} taps")
    x = R.dense_samples(max(REAL_NS), K, complex_=False)
    for n in REAL_NS:
        F, g = real_block(gpu_lib, design)
        W.add(F.process(x[:n]), R.fir64(x[:n], g), R.bound(x[:n], g), f"n={n}")
    W.done()


def test_fir_real_grid_stride(gpu_lib):
    """The grid-stride second pass of k_fir_real8<128> (125 taps; more than kMaxGrid =
    2048 tiles of 4096): one impulse-train call of 2048 * 4096 + 4096 + 77 samples on
    device tensors. One of the largest cases of this file (8.4 M samples)."""
    design = REAL_DESIGNS[1]
    n = MAX_GRID * 16 * NT + 16 * NT + 77
    F, g = real_block(gpu_lib, design)
    pos, amp = R.impulses(n, odd_at_least(len(g) + 1), 5, 11, complex_=False)
    got = F.process_device(dev_impulses(n, pos, amp)).cpu().numpy()
    exact(got, R.impulse_fir64(n, pos, amp, g), f"n={n}")


# ======================================================================= FirDecimator ==
DECIM_NS = [1, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 5]
DECIM_IDS = [f"m{d[1]}_{d[4]}taps" for d in DECIM_DESIGNS]


def decim_block(lib, design, nch=1):
    fs, m, cut, tr, K = design
    D = lib.FirDecimator(fs, m, cut, tr, channels=nch)
    g = R.standard_taps(D.taps())
    assert len(g) == K, f"FirDecimator{(fs, m, cut, tr)}: {len(g)} taps, expected {K}"
    return D, g


def decim_impulse_case(n, nch, d, seed, g, m):
    """An [nch, n] batch of shifted impulse trains and its decimated reference."""
    trains = [R.impulses(n, d, (3 * c + seed) % d, seed + c) for c in range(nch)]
    x = np.stack([R.impulse_signal(n, *t) for t in trains])
    ref = np.stack([R.impulse_fir64(n, *t, g)[::m] for t in trains])
    return x, ref


@pytest.mark.parametrize("design", DECIM_DESIGNS, ids=DECIM_IDS)
def test_decimator_impulse(gpu_lib, design):
    """Impulse class, d odd (coprime to m: every residue of the tap index mod m occurs),
    1, 2, 3 and 5 channels (the ragged last workgroup of k_decim_w4q's four waves),
    n across the CLAMP switch at 2048; odd n with several channels is the non-A16 form,
    as is the device input 8 bytes off 16-byte alignment. Launches: 127 taps m = 8
    k_decim_w4<16, A16, CLAMP>; 255 taps m = 8 k_decim_w4q<32, A16, CLAMP>; 41 taps
    m = 4, 335 taps m = 8 and 161 taps m = 4 k_decim_generic (+ k_hist_update). Then
    one single-channel train of d * 1024 samples: its impulses fall on every position
    of the 1024-input (128-output) tile. (The designed taps end in exact zeros, the Hann
    window's end points, so g[0] and g[1] are not observable through this block; n = 1
    is the call with no whole sample pair, which dw_load's CLAMP form must not load.)"""
    m, K = design[1], design[4]
    d = odd_at_least(K + 1)
    for nch in (1, 2, 3, 5):
        for n in DECIM_NS:
            for seed in (0, 1, d // 2):
                D, g = decim_block(gpu_lib, design, nch)
                x, ref = decim_impulse_case(n, nch, d, seed, g, m)
                got = D.process(x if nch > 1 else x[0])
                exact(got, ref if nch > 1 else ref[0], f"{K} taps m={m} {nch} ch n={n} seed={seed}")
    for n in (2047, 2048, 3 * 1024 + 5):  # xd[1:]: 8-byte but not 16-byte aligned
        D, g = decim_block(gpu_lib, design)
        x, ref = decim_impulse_case(n + 1, 1, d, 2, g, m)
        xd = dev(x[0])[1:]
        assert xd.data_ptr() % 16 == 8
        exact(D.process_device(xd).cpu().numpy(), R.fir64(x[0][1:], g)[::m], f"{K} taps m={m} n={n} unaligned in")
    n = d * 1024 + 1024 + 5
    D, g = decim_block(gpu_lib, design)
    pos, amp = R.impulses(n, d, 4, K)
    got = D.process_device(dev_impulses(n, pos, amp)).cpu().numpy()
    exact(got, R.impulse_fir64(n, pos, amp, g)[::m], f"{K} taps m={m} n={n} every tile position")


@pytest.mark.parametrize("design", DECIM_DESIGNS, ids=DECIM_IDS)
def test_decimator_dense(gpu_lib, design):
    """Dense random within the a-priori bound, same shapes and launches as
    test_decimator_impulse."""
    m, K = design[1], design[4]
    W = Worst(f"decimator dense {K} taps m={m}")
    x = R.dense_samples((5, max(DECIM_NS)), K)
    for nch in (1, 2, 3, 5):
        for n in DECIM_NS:
            D, g = decim_block(gpu_lib, design, nch)
            xs = np.ascontiguousarray(x[:nch, :n])
            ref = np.stack([R.fir64(xs[c], g)[::m] for c in range(nch)])
            b = np.stack([R.bound(xs[c], g)[::m] for c in range(nch)])
            got = D.process(xs if nch > 1 else xs[0])
            W.add(got if nch > 1 else got[None], ref, b, f"{nch} ch n={n}")
    W.done()


@pytest.mark.parametrize("lens", [[8, 1024, 2048, 8], [3333, 1, 7, 2049]], ids=["multiples_of_m", "ragged"])
@pytest.mark.parametrize("design", DECIM_DESIGNS, ids=DECIM_IDS)
def test_decimator_streaming(gpu_lib, design, lens):
    """One block (1 and 3 channels) over calls that are and are not multiples of m, every
    call compared: the history carried by dw_hist_next (k_hist_update on the generic
    path) and the kept phase restarting at every call (decim.rs:66-71). Impulse class
    (exact), then dense random (bound)."""
    m, K = design[1], design[4]
    d = odd_at_least(K + 1)
    n = sum(lens)
    for nch in (1, 3):
        for seed in (0, d // 2):
            D, g = decim_block(gpu_lib, design, nch)
            trains = [R.impulses(n, d, (3 * c + seed) % d, seed + c) for c in range(nch)]
            x = np.stack([R.impulse_signal(n, *t) for t in trains])
            refs = [R.decim_pick(R.impulse_fir64(n, *t, g), lens, m) for t in trains]
            outs = run_calls(D, x if nch > 1 else x[0], lens)
            for i, got in enumerate(outs):
                for c in range(nch):
                    exact(got[c] if nch > 1 else got, refs[c][i], f"{K} taps m={m} {nch} ch seed={seed} call {i} of {lens} ch={c}")
        W = Worst(f"decimator dense streamed {K} taps m={m} {nch} ch {lens}")
        D, g = decim_block(gpu_lib, design, nch)
        x = R.dense_samples((nch, n), K + nch)
        refs = [R.decim_pick(R.fir64(x[c], g), lens, m) for c in range(nch)]
        bs = [R.decim_pick(R.bound(x[c], g), lens, m) for c in range(nch)]
        for i, got in enumerate(run_calls(D, x if nch > 1 else x[0], lens)):
            for c in range(nch):
                W.add(got[c] if nch > 1 else got, refs[c][i], bs[c][i], f"call {i} ch={c}")
        W.done()


def test_decimator_many_tiles_per_wave(gpu_lib):
    """k_decim_w4q<32, true, false> at the 24 x 2,000,000 geometry of the 255-tap
    design: each wave walks many 128-output tiles, carrying Q + 2 columns from tile to
    tile inside LDS. Impulse class, compared exactly; input and output stay on the
    device and the reference is built one channel at a time. The largest case of this
    file (48 M input samples)."""
    import torch

    design = DECIM_DESIGNS[1]
    nch, n, m = 24, 2_000_000, 8
    D, g = decim_block(gpu_lib, design, nch)
    d = odd_at_least(len(g) + 1)
    x = torch.zeros((nch, n), dtype=torch.complex64, device="cuda")
    trains = [R.impulses(n, d, (11 * c) % d, c) for c in range(nch)]
    for c, (pos, amp) in enumerate(trains):
        x[c, dev(pos)] = dev(amp)
    got = D.process_device(x)
    assert tuple(got.shape) == (nch, n // m)
    for c, (pos, amp) in enumerate(trains):
        exact(got[c].cpu().numpy(), R.impulse_fir64(n, pos, amp, g)[::m], f"ch={c}")
