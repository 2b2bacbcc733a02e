"""tests/fir_ref.py (the float64 FIR reference and its a-priori bound) against the C
oracle, an independent f32 implementation of the same blocks, on every input class
the GPU tests use, before any kernel is judged by it. No GPU.

* exact classes (integer, impulse train): oracle == fir64 / decim64 rounded to f32;
* dense random: the oracle's f32 sums (unfused, tap order) stay within bound().
"""
import numpy as np
import pytest

import fir_ref as R

REAL_DESIGNS = [(48e3, 3000.0, 800.0, 61), (1.25e6, 15e3, 10e3, 125), (48e3, 1000.0, 250.0, 193),
                (48e3, 500.0, 150.0, 321)]
DECIM_DESIGNS = [(10e6, 8, 200e3, 79e3, 127), (10e6, 8, 190e3, 39370.0, 255), (96e3, 4, 10.8e3, 2.4e3, 41),
                 (10e6, 8, 100e3, 30e3, 335), (96e3, 4, 3e3, 600.0, 161)]


def float_taps(K, seed=0):
    """Arbitrary f32 taps with no symmetry."""
    return np.random.default_rng(500 + K + seed).standard_normal(K).astype(np.float32)


def test_reference_self_consistency():
    g = float_taps(37)
    x = R.dense_samples(500, 1)
    y = R.fir64(x, g)
    loop = np.array([sum(float(g[k]) * complex(x[n - k]) for k in range(37) if n - k >= 0) for n in range(500)])
    assert np.allclose(y, loop, rtol=1e-12, atol=1e-12)
    assert np.array_equal(R.fir64(x[200:], g, hist=x[:200]), y[200:])  # the history is the stream before
    pos, amp = R.impulses(500, 37, 5, 2)
    assert np.array_equal(R.impulse_fir64(500, pos, amp, g), R.fir64(R.impulse_signal(500, pos, amp), g))
    calls = R.split_calls(x, [7, 100, 1, 392])
    d = R.decim64(calls, g, 8)
    assert [len(c) for c in d] == [1, 13, 1, 49]
    assert d[1][3] == y[7 + 24] and d[3][0] == y[108]
    assert R.gamma(255) == pytest.approx(256 * 2.0 ** -24, rel=1e-4)
    h = np.arange(5, dtype=np.float32)
    assert R.standard_taps(h).tolist() == [4, 0, 1, 2, 3]
    t = R.int_taps(129)
    assert len({t[0], t[64], t[128]}) == 3 and 0 not in (t[0], t[64], t[128]) and not np.array_equal(t, t[::-1])
    assert np.abs(t).max() <= 7 and np.abs(R.int_samples(1000).real).max() <= 15
    assert R.worst_ratio(np.float32([1.0, 2.0]), np.array([1.0, 2.5]), np.array([0.0, 1.0])) == 0.5
    assert R.worst_ratio(np.float32([1.5]), np.array([1.0]), np.array([0.0])) == np.inf


@pytest.mark.parametrize("K", [1, 2, 64, 65, 129, 256, 301])
def test_oracle_firiq_integer(oracle, K):
    g = R.int_taps(K)
    x = R.int_samples(3 * K + 1111, K)
    ref = R.fir64(x, g)
    for chunk in (0, 1, K + 1, 1000):
        got = oracle.fir_lowpass_iq(x, g, chunk=chunk)
        assert R.same(got, ref), f"K={K} chunk={chunk}: {R.first_diffs(got, ref)}"


@pytest.mark.parametrize("K", [1, 2, 64, 129, 301])
def test_oracle_firiq_impulse(oracle, K):
    g = float_taps(K)
    n = 40 * K + 333
    for first in (0, K // 2, K - 1):
        pos, amp = R.impulses(n, K, first, K)
        x = R.impulse_signal(n, pos, amp)
        ref = R.impulse_fir64(n, pos, amp, g)
        got = oracle.fir_lowpass_iq(x, g, chunk=777)
        assert R.same(got, ref), f"K={K} first={first}: {R.first_diffs(got, ref)}"


@pytest.mark.parametrize("K", [1, 2, 64, 89, 128, 255, 256, 301])
def test_oracle_firiq_aligned_integer(oracle, K):
    """fir.rs:260-276: y[i] = streamed[i + d] over [x | 0^d], d = (K - 1) // 2."""
    g = R.int_taps(K)
    d = (K - 1) // 2
    for n in (1, 7, 2049):
        x = R.int_samples(n, K + n)
        ref = R.fir64(np.concatenate([x, np.zeros(d, np.complex64)]), g)[d:]
        got = oracle.fir_lowpass_iq_aligned(x, g)
        assert R.same(got, ref), f"K={K} n={n}: {R.first_diffs(got, ref)}"


@pytest.mark.parametrize("design", REAL_DESIGNS)
def test_oracle_fir_real_impulse(oracle, design):
    *args, K = design
    g = R.standard_taps(oracle.fir_lowpass_taps(*args))
    assert len(g) == K
    n = 3 * 4096 + 77
    for first in (0, 1, K - 1):
        pos, amp = R.impulses(n, K + 2, first, K, complex_=False)
        ref = R.impulse_fir64(n, pos, amp, g)
        got = oracle.fir_lowpass(R.impulse_signal(n, pos, amp), *args, chunk=4097)
        assert R.same(got, ref), f"{K} taps first={first}: {R.first_diffs(got, ref)}"


@pytest.mark.parametrize("design", DECIM_DESIGNS)
@pytest.mark.parametrize("chunk", [1024, 3333])
def test_oracle_decimator_impulse(oracle, design, chunk):
    fs, m, cut, tr, K = design
    g = R.standard_taps(oracle.fir_lowpass_taps(fs, cut, tr))
    assert len(g) == K
    n = 20_000
    d = K + 2 if (K + 2) % 2 else K + 3  # odd: coprime to m, every tap residue mod m occurs
    pos, amp = R.impulses(n, d, 3, K)
    lens = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
    ref = np.concatenate(R.decim_pick(R.impulse_fir64(n, pos, amp, g), lens, m))
    got = oracle.fir_decimator(R.impulse_signal(n, pos, amp), fs, m, cut, tr, chunk=chunk)
    assert R.same(got, ref), f"{K} taps m={m} chunk={chunk}: {R.first_diffs(got, ref)}"


def test_oracle_dense_within_bound(oracle):
    worst = 0.0
    for K in (64, 255, 301):
        g = float_taps(K)
        x = R.dense_samples(6000, K)
        w = R.worst_ratio(oracle.fir_lowpass_iq(x, g, chunk=1000), R.fir64(x, g), R.bound(x, g))
        d = (K - 1) // 2
        xz = np.concatenate([x, np.zeros(d, np.complex64)])
        w = max(w, R.worst_ratio(oracle.fir_lowpass_iq_aligned(x, g), R.fir64(xz, g)[d:], R.bound(xz, g)[d:]))
        worst = max(worst, w)
    for *args, K in REAL_DESIGNS:
        g = R.standard_taps(oracle.fir_lowpass_taps(*args))
        x = R.dense_samples(6000, K, complex_=False)
        worst = max(worst, R.worst_ratio(oracle.fir_lowpass(x, *args, chunk=1000), R.fir64(x, g), R.bound(x, g)))
    for fs, m, cut, tr, K in DECIM_DESIGNS:
        g = R.standard_taps(oracle.fir_lowpass_taps(fs, cut, tr))
        x = R.dense_samples(6000, K)
        lens = [3333, 2667]
        ref = np.concatenate(R.decim_pick(R.fir64(x, g), lens, m))
        b = np.concatenate(R.decim_pick(R.bound(x, g), lens, m))
        worst = max(worst, R.worst_ratio(oracle.fir_decimator(x, fs, m, cut, tr, chunk=3333), ref, b))
    print(f"[parity] oracle vs fir64, dense random: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
