"""GPU: the OFDM transform and the fused modem kernels (csrc/k_ofdm.hip) held to the host's
bits. Every comparison is R.same_bits (NaN in the same words, every other word byte-equal, the
sign of a zero or an inf included), against the library's scalar host entry and against the
numpy restatement (tests/np_ref_ofdm.py); tests/test_ofdm_oracle.py ties those two to each
other on the same inputs and shows that every input set used here notices the departure it is
there for (a contracted butterfly, a W^0 shortcut, recomputed twiddles, flushed subnormals, a
rotated twiddle, a reciprocal for a division, a fused interpolation, a strict floor).

Geometry: T = min(n / 4, 256) lanes serve one symbol and per = 256 / T symbols share a
workgroup, so every kernel is run with 1, per and per + 1 symbols (a full workgroup and one
symbol over), at all ten sizes (T = 2 at n = 8; 2 and 4 butterflies per lane per pass at 2048
and 4096; the leading radix-2 pass where log2 n is odd). Three channels cannot make per
(a power of two) symbols; they are given the fewest symbols that pass per."""
import itertools

import numpy as np
import pytest

import np_ref_ofdm as R

pytestmark = pytest.mark.gpu

S = R.same_bits
EPS = np.finfo(np.float32).eps
ONE_UP = float(np.nextafter(np.float32(1), np.float32(2)))  # |g - 1| == eps: not above it
ONE_UP2 = float(np.float32(1) + np.float32(2) * EPS)  # |g - 1| == 2 eps
GAINS = (1.0, ONE_UP, ONE_UP2)
ALL_ORDER_SIZES = (8, 64, 4096)
MODEM_CASES = [(n, o) for n in R.FFT_SIZES for o in (R.ORDERS if n in ALL_ORDER_SIZES else ["qam64"])]


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    if orion_sdr.device_count() < 1:
        pytest.fail("no HIP device visible")
    return orion_sdr


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def per_workgroup(n):
    return 256 // min(n // 4, 256)


def shapes(n):
    """(channels, symbols): one channel with 1 (n >= 2048: per is 1 or 2), per and per + 1 symbols, and
    three channels with the fewest symbols that pass per (exactly per + 1 where 3 divides it)."""
    per = per_workgroup(n)
    return sorted({(1, 1), (1, per), (1, per + 1), (3, -(-(per + 1) // 3))})


def rand_c(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def make_cfg(lib, n, order, cp, rf_hz=0.0, gain=1.0, backoff=0, roll=0, boost=False):
    guard, pi, pv = R.pilot_layout(n, boost)
    c = lib.OfdmConfig(n, cp, np.zeros(0, np.int32), pi, pv, 1e6, rf_hz, gain, order, edge_guard=guard)
    if backoff:
        c = c.with_rx_window_backoff(backoff)
    if roll:
        c = c.with_symbol_window(roll)
    r = R.Config(n, cp, R.contiguous_data(n, pi, guard, False), pi, pv, 1e6, rf_hz, gain, order, backoff, roll)
    assert R.validate(n, r.data, r.pilot_idx) == (0, 0) and len(pi) == (4 if n >= 32 else 2 if n == 16 else 1)
    assert S(c.data_carriers, r.data)
    return c, r


# ---- k_fft ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.FFT_SIZES)
def test_fft_kernel_gives_the_host_bits(lib, n):
    per = per_workgroup(n)
    for inv, blk in ((False, lib.FftBlock(n)), (True, lib.IfftBlock(n))):
        for name, x in R.input_sets(n).items():
            host = lib.fft_host(x.reshape(-1), n, inv).reshape(x.shape)
            ref = R.fft_radix2(x, inv)
            assert S(host, ref), (name, inv)
            for batch in sorted({1, per, per + 1}):
                got = blk.process_batch(R.cycle_rows(x, batch))
                d = R.diff_words(got, R.cycle_rows(host, batch))
                print(f"[exact] k_fft n={n} inverse={inv} {name} batch={batch}: {d} of {got.size * 2} words differ from the host's")
                assert S(got, R.cycle_rows(host, batch)) and S(got, R.cycle_rows(ref, batch)), (name, inv, batch)


@pytest.mark.parametrize("n", R.FFT_SIZES)
def test_fft_kernel_on_a_strided_view_gives_the_host_bits(lib, torch, n):
    """Symbols at an odd stride and an odd offset (a window inside longer symbols), 8-byte aligned only."""
    x = rand_c(np.random.default_rng([7301, n]), 5 * (n + 5)).reshape(5, n + 5)
    win = np.ascontiguousarray(x[:, 3: 3 + n])
    view = torch.from_numpy(x).cuda()[:, 3: 3 + n]
    for inv, blk in ((False, lib.FftBlock(n)), (True, lib.IfftBlock(n))):
        got = blk.process_batch(view).cpu().numpy()
        assert S(got, lib.fft_host(win.reshape(-1), n, inv).reshape(5, n)) and S(got, R.fft_radix2(win, inv))


# ---- k_ofdm_mod -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,order", MODEM_CASES)
def test_mod_kernel_gives_the_host_bits(lib, n, order):
    """cp in {0, 5, n / 4} x roll-off {0, 2}; over those six the three gains and rf_hz 0 / 125 kHz
    turn so that every gain meets both (the RF form over two calls of one handle: the phase
    carries, every channel from the same phase). The host and the restatement multiply by the
    gain whatever it is (the |g - 1| > eps rule is the demodulator's), so one ulp above 1 must
    already move the output: asserted on the restatement."""
    rng = np.random.default_rng([7302, n, R.ORDERS.index(order)])
    seen = set()
    for i, (cp, roll) in enumerate(itertools.product((0, 5, n // 4), (0, 2))):
        k = i + R.ORDERS.index(order)
        g, rf = GAINS[k % 3], (0.0, 125e3)[(k // 3) % 2]
        seen.add((g, rf))
        c, r = make_cfg(lib, n, order, cp, rf_hz=rf, gain=g, roll=roll)
        _, r1 = make_cfg(lib, n, order, cp, rf_hz=rf, gain=1.0, roll=roll)
        for nch, nsym in shapes(n):
            bits = rng.integers(0, 2, (nch, nsym * r.bps)).astype(np.uint8)
            per_ch = nsym * r.sym_len
            rot = lib.ofdm_rotator(rf, 1e6, 2 * per_ch) if rf else None  # the host Rotator (R.rotator's bits, CPU-tested)
            dev, hosts = lib.OfdmMod(c), [lib.OfdmMod(c) for _ in range(nch)]
            for call in range(2 if rf else 1):
                got = lib.ofdm_modulate_batch(dev, bits)
                assert got.shape == (nch, per_ch)
                for ch in range(nch):
                    ph = None if rot is None else rot[call * per_ch: (call + 1) * per_ch]
                    ref = R.modulate(r, bits[ch], ph)
                    assert S(got[ch], hosts[ch].modulate_host(bits[ch])) and S(got[ch], ref), (cp, roll, g, rf, nch, nsym, call, ch)
                    assert S(ref, R.modulate(r1, bits[ch], ph)) == (g == 1.0)
    assert seen == set(itertools.product(GAINS, (0.0, 125e3)))


# ---- k_ofdm_demod ---------------------------------------------------------------------------
def rx_signal(lib, c, r, nch, nsym, rng):
    """A received stream per channel: modulated symbols through the 3-tap channel plus a little noise."""
    bits = rng.integers(0, 2, (nch, nsym * r.bps)).astype(np.uint8)
    m = lib.OfdmMod(c)
    iq = np.stack([R.channel3(m.modulate_host(b)) for b in bits])
    return (iq + rand_c(rng, iq.size, 1e-3).reshape(iq.shape)).astype(np.complex64)


@pytest.mark.parametrize("n,order", MODEM_CASES)
def test_demod_kernel_gives_the_host_bits(lib, n, order):
    """The three equalizer modes x (cp n / 4 at back-off 0, 3 and cp; cp 5, an odd symbol stride,
    at back-off 3 and with the pilots boosted by 4/3); the gains 1.5, 1, one ulp above 1 (inside
    the |g - 1| > eps rule: no gain stage) and 1 + 2 eps (outside it) turn over the back-offs,
    so every mode meets every gain."""
    rng = np.random.default_rng([7303, n, R.ORDERS.index(order)])
    per = per_workgroup(n)
    tr = rand_c(rng, n)
    tr[n // 8 + 1] = 1e-4  # an erased bin
    gains = (1.5, 1.0, ONE_UP, ONE_UP2)
    for cp, backoffs in ((n // 4, (0, 3, n // 4)), (5, (3,))):
        boost = cp == 5  # pilots of 4/3 there: k_ofdm_demod's own division by |pilot|^2 is then no division by 1
        c0, r0 = make_cfg(lib, n, order, cp, boost=boost)
        iq = rx_signal(lib, c0, r0, 3, per + 1, rng)
        for eq, (bi, backoff) in itertools.product((None, "training_symbol", "pilot_interp"), enumerate(backoffs)):
            g = gains[bi if cp != 5 else 3]
            c, r = make_cfg(lib, n, order, cp, backoff=backoff, boost=boost)
            dev, hd = lib.OfdmDemod(c, eq), lib.OfdmDemod(c, eq)
            for d in (dev, hd):
                if eq:
                    d.estimate_channel_freq(tr)
                d.set_gain(g)
            for nch, nsym in shapes(n):
                part = np.ascontiguousarray(iq[:nch, : nsym * r.sym_len])
                soft, bits, llr = lib.ofdm_demodulate_batch(dev, part, bits=True, llr=True)
                assert soft.shape == (nch, nsym * len(r.data))
                for ch in range(nch):
                    req = R.Equalizer(r, eq) if eq else None
                    if eq:
                        req.estimate_from_training_symbol(tr)
                    ref = R.demodulate(r, part[ch], g, req)
                    assert S(soft[ch], hd.process_host(part[ch])) and S(soft[ch], ref), (cp, backoff, eq, g, nch, nsym, ch)
                    # which side of the rule the gain falls on, from the restatement
                    req1 = R.Equalizer(r, eq) if eq else None
                    if eq:
                        req1.estimate_from_training_symbol(tr)
                    assert S(ref, R.demodulate(r, part[ch], 1.0, req1)) == (g in (1.0, ONE_UP))
                    assert S(bits[ch], lib.ofdm_decide(order, ref)) and S(llr[ch], lib.ofdm_llr(order, ref))


# ---- k_ofdm_equalize and interp_est ---------------------------------------------------------
@pytest.mark.parametrize("boost", [False, True], ids=["unit_pilots", "boosted_pilots"])
@pytest.mark.parametrize("n", [8, 64, 4096])
def test_equalize_kernel_gives_the_host_bits(lib, n, boost):
    """pilot_interp over R.equalizer_case on one handle: a received pilot that is exactly 0, an
    estimate that crosses kEqualizerFloor between data bins, |h|^2 one ulp under the floor, on
    it and one ulp over it; n = 8 has a single pilot (np == 1: the held ratio everywhere).
    Boosted pilots (4/3) make the division by |pilot|^2 a division by something other than 1."""
    r, x = R.equalizer_case(n, boost)
    c, r2 = make_cfg(lib, n, "qam16", n // 4, boost=boost)
    assert S(r.data, r2.data) and S(r.pilot_val, r2.pilot_val)
    want, erased = R.equalizer_run(r, x)
    R.check_equalizer_erasures(r, erased)  # which bins are erased, on the restatement, before the device is looked at
    assert np.all((want == 0) == erased)
    eq, heq = lib.OfdmEqualizer(c, "pilot_interp"), lib.OfdmEqualizer(c, "pilot_interp")
    got = eq.process(x.reshape(-1)).reshape(x.shape)
    print(f"[exact] k_ofdm_equalize n_fft={n} boost={boost}: erased bins per symbol {erased.sum(1).tolist()}, "
          f"{R.diff_words(got, want)} words differ from the restatement's")
    assert S(got, heq.process_host(x.reshape(-1)).reshape(x.shape)) and S(got, want)
    # the same handle again, the symbols in the other order, then one at a time
    back = np.ascontiguousarray(x[::-1])
    assert S(eq.process(back.reshape(-1)).reshape(x.shape), R.equalizer_run(r, back)[0])
    for row, w in zip(x, want):
        assert S(eq.process(row), w)
