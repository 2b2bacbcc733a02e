"""GPU: the OFDM symbol layer's kernels (csrc/k_ofdm.hip) against the library's scalar host
code and tests/np_ref_ofdm.py.

The transform is held to the f64 DFT of the same f32 input: with e_host(n) the nrmse of the
host radix-2 transform on the test's own input, the device's nrmse must be <= 2 e_host(n)
(another radix and butterfly order moves the figure by under 30 %; a wrong twiddle or a
missed stage shows at 1e-3 and above). The modulator's IQ and the demodulator's soft symbols
are held end to end to the host path: max |delta| over the rms of the host output must be
<= 2 x the same measure of the host path against f64 truth. Everything else is bit for bit.
Each figure is printed before it is asserted."""
import numpy as np
import pytest

import np_ref_ofdm as R

pytestmark = pytest.mark.gpu

PILOT_IDX = np.array([-21, -7, 7, 21], np.int32)
PILOT_VAL = np.array([1, -1, 1j, 1], np.complex64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rand_c(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


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


def make_cfg(lib, order="qpsk", n_fft=64, cp=16, rf_hz=0.0, gain=1.0, pilots=True, edge_guard=4, backoff=0, roll=0):
    pi = PILOT_IDX if pilots else PILOT_IDX[:0]
    pv = PILOT_VAL if pilots else PILOT_VAL[:0]
    c = lib.OfdmConfig(n_fft, cp, np.zeros(0, np.int32), pi, pv, 1e6, rf_hz, gain, order, edge_guard=edge_guard)
    if backoff:
        c = c.with_rx_window_backoff(backoff)
    if roll:
        c = c.with_symbol_window(roll)
    r = R.Config(n_fft, cp, R.contiguous_data(n_fft, pi, edge_guard, False), pi, pv, 1e6, rf_hz, gain, order,
                 backoff, roll)
    return c, r


# ---- 1. the transform -----------------------------------------------------------------------
_FFT_INPUT = {}


def fft_case(lib, n):
    """257 symbols from default_rng(5), their f64 truth and the host transform's error, once per n."""
    if n not in _FFT_INPUT:
        x = rand_c(np.random.default_rng(5), 257 * n).reshape(257, n)
        e = {inv: R.nrmse(lib.fft_host(x.reshape(-1), n, inv).reshape(257, n), R.fft_truth(x, inv)) for inv in (False, True)}
        _FFT_INPUT[n] = (x, e)
    return _FFT_INPUT[n]


@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_transform_against_f64_truth(lib, n, batch):
    x257, e_host = fft_case(lib, n)
    x = np.ascontiguousarray(x257[:batch])
    for inv, blk in ((False, lib.FftBlock(n)), (True, lib.IfftBlock(n))):
        got = blk.process_batch(x)
        eh = R.nrmse(lib.fft_host(x.reshape(-1), n, inv).reshape(batch, n), R.fft_truth(x, inv))
        ed = R.nrmse(got, R.fft_truth(x, inv))
        print(f"[parity] k_fft n={n} batch={batch} inverse={inv}: e_host {eh:.3e} device {ed:.3e} ratio {ed / eh:.3f}")
        assert ed <= 2 * eh
        # batched output equals single calls bit for bit
        for row in sorted({0, batch // 2, batch - 1}):
            assert same(blk.process(x[row]), got[row])
    # the inverse of the forward of x is x within the transform's bound
    back = lib.IfftBlock(n).process_batch(lib.FftBlock(n).process_batch(x))
    eb = R.nrmse(back, x)
    print(f"[parity] k_fft n={n} batch={batch} inverse(forward(x)): nrmse {eb:.3e} (bound 2 e_host = {2 * e_host[False]:.3e})")
    assert eb <= 2 * e_host[False]


@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_transform_structure(lib, torch, n):
    f = lib.FftBlock(n)
    imp = np.zeros(n, np.complex64)
    imp[1] = 1
    row = np.exp(-2j * np.pi * np.arange(n) / n)
    d = float(np.max(np.abs(f.process(imp) - row)))
    print(f"[parity] k_fft n={n} impulse at 1: max |X[k] - W^k| {d:.3e}")
    assert d <= 2.0 ** -22
    c = f.process(np.ones(n, np.complex64))
    assert c[0] == n and np.max(np.abs(c[1:])) <= n * 2.0 ** -23
    assert f.process(imp[: n - 1]).size == 0  # a partial chunk is a no-op
    # symbols at an odd stride and an odd offset (a window inside longer symbols): 8-byte aligned only
    x = torch.from_numpy(rand_c(np.random.default_rng(1), 5 * (n + 5)).reshape(5, n + 5)).cuda()
    view = x[:, 3: 3 + n]
    assert same(f.process_batch(view).cpu().numpy(), f.process_batch(view.contiguous()).cpu().numpy())


# ---- 2. the fused stages --------------------------------------------------------------------
def mod_truth(r, bits, nch):
    """The modulator in f64 (numpy.fft), gain and window included: what both paths approximate."""
    syms = R.map_bits(r.order, bits.reshape(-1)).reshape(-1, len(r.data)).astype(np.complex128)
    f = np.zeros((len(syms), r.n_fft), np.complex128)
    f[:, r.data_bins] = syms
    f[:, r.pilot_bins] = r.pilot_val
    t = np.fft.ifft(f, axis=1)
    y = np.concatenate([t[:, r.n_fft - r.cp_len:], t], 1) if r.cp_len else t
    w = np.ones(r.sym_len)
    ramp = R.window_ramp(r.sym_len, r.roll_off).astype(np.float64)
    if len(ramp):
        w[: len(ramp)] = ramp
        w[-len(ramp):] = ramp[::-1]
    return (y * w * float(np.float32(r.gain))).reshape(nch, -1)


@pytest.mark.parametrize("nsym", [1, 7])
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cp", [0, 5, 16])
def test_mod_kernel_exact(lib, cp, nch, nsym):
    order = "qam64"
    c1, r1 = make_cfg(lib, order, cp=cp, gain=1.0)
    cw, rw = make_cfg(lib, order, cp=cp, gain=0.25, roll=2)
    bits = np.random.default_rng(21).integers(0, 2, (nch, nsym * r1.bps)).astype(np.uint8)
    plain = lib.ofdm_modulate_batch(lib.OfdmMod(c1), bits)
    assert plain.shape == (nch, nsym * r1.sym_len)
    s = plain.reshape(nch * nsym, r1.sym_len)
    assert cp == 0 or same(s[:, :cp], s[:, -cp:])  # the prefix is the tail
    # window and gain on the CPU in f32 over the device's own gain-1 output
    win = lib.ofdm_modulate_batch(lib.OfdmMod(cw), bits)
    want = R.gain(R.window_apply(s, R.window_ramp(r1.sym_len, 2)), 0.25).reshape(nch, -1)
    assert same(win, want)
    # end to end against the host path, within twice the host path's own error against f64 truth
    host = np.stack([lib.OfdmMod(cw).modulate_host(b) for b in bits])
    rms = float(np.sqrt(np.mean(np.abs(host.astype(np.complex128)) ** 2)))
    e_host = float(np.max(np.abs(host - mod_truth(rw, bits, nch)))) / rms
    e_dev = float(np.max(np.abs(win.astype(np.complex128) - host))) / rms
    print(f"[parity] k_ofdm_mod cp={cp} nch={nch} nsym={nsym}: host vs f64 {e_host:.3e}, device vs host {e_dev:.3e}")
    assert e_dev <= 2 * e_host
    # RF: the baseband output (window, gain 1) rotated by the host Rotator and gained on the CPU,
    # over two calls of one handle: the phase carries, every channel from the same phase
    cb, _ = make_cfg(lib, order, cp=cp, gain=1.0, roll=2)
    crf, _ = make_cfg(lib, order, cp=cp, gain=0.25, roll=2, rf_hz=125e3)
    base = lib.ofdm_modulate_batch(lib.OfdmMod(cb), bits)
    per = nsym * r1.sym_len
    rot = lib.ofdm_rotator(125e3, 1e6, 2 * per)
    m = lib.OfdmMod(crf)
    for call in range(2):
        got = lib.ofdm_modulate_batch(m, bits)
        want = np.stack([R.rotate_gain(base[ch], rot[call * per: (call + 1) * per], 0.25) for ch in range(nch)])
        assert same(got, want)
    m.reset()
    assert same(lib.ofdm_modulate_batch(m, bits)[0], R.rotate_gain(base[0], rot[:per], 0.25))


def rx_signal(lib, c, r, nch, nsym, seed):
    """A received stream per channel: modulated symbols through the 3-tap channel plus a little noise."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (nch, nsym * r.bps)).astype(np.uint8)
    m = lib.OfdmMod(c)
    iq = np.stack([R.channel3(m.modulate_host(b)) for b in bits])
    return (iq + rand_c(rng, iq.size, 1e-3).reshape(iq.shape)).astype(np.complex64)


@pytest.mark.parametrize("eq", [None, "training_symbol", "pilot_interp"])
@pytest.mark.parametrize("cp,backoff", [(16, 0), (16, 3), (16, 16), (5, 0), (5, 3), (5, 5)])
def test_demod_kernel_exact(lib, torch, cp, backoff, eq):
    """k_ofdm_demod equals FftBlock (the same device transform) on the selected window followed
    by the host's equalizer, gather, gain, decider and LLRs, bit for bit."""
    order, nch, nsym = "qam16", 3, 7
    c, r = make_cfg(lib, order, cp=cp, backoff=backoff)
    iq = rx_signal(lib, c, r, nch, nsym, 31)
    d = lib.OfdmDemod(c, eq)
    heq = lib.OfdmEqualizer(c, eq) if eq else None
    if eq:
        tr = rand_c(np.random.default_rng(32), 64)
        tr[9] = 1e-4  # an erased bin
        d.estimate_channel_freq(tr)
        heq.estimate_from_training_symbol(tr)
    d.set_gain(1.5)
    soft, bits, llr = lib.ofdm_demodulate_batch(d, iq, bits=True, llr=True)
    start = cp - min(backoff, cp)
    win = torch.from_numpy(iq).cuda().reshape(nch * nsym, r.sym_len)[:, start: start + 64]
    freq = lib.FftBlock(64).process_batch(win).cpu().numpy()
    if eq:
        freq = heq.process_host(freq.reshape(-1)).reshape(freq.shape)
    want = R.gain(freq[:, r.data_bins].reshape(-1), 1.5)
    assert same(soft.reshape(-1), want)
    assert same(bits.reshape(-1), lib.ofdm_decide(order, want)) and same(llr.reshape(-1), lib.ofdm_llr(order, want))
    # end to end against the host path (the scalar transform too)
    hd = lib.OfdmDemod(c, eq)
    if eq:
        hd.estimate_channel_freq(tr)
    hd.set_gain(1.5)
    host = np.concatenate([hd.process_host(ch) for ch in iq])
    req = R.Equalizer(r, eq) if eq else None
    if eq:
        req.estimate_from_training_symbol(tr)
    truth = np.concatenate([R.demodulate(r, ch, 1.5, req, transform=lambda w: R.fft_truth(w).astype(np.complex64))
                            for ch in iq])
    rms = float(np.sqrt(np.mean(np.abs(host.astype(np.complex128)) ** 2)))
    e_host = float(np.max(np.abs(host.astype(np.complex128) - truth))) / rms
    e_dev = float(np.max(np.abs(soft.reshape(-1).astype(np.complex128) - host))) / rms
    print(f"[parity] k_ofdm_demod cp={cp} backoff={backoff} eq={eq}: host vs f64 {e_host:.3e}, device vs host {e_dev:.3e}")
    assert e_dev <= 2 * e_host


@pytest.mark.parametrize("eq", ["training_symbol", "pilot_interp"])
def test_tables_replaced_between_two_device_demodulate_calls(lib, torch, eq):
    """n_fft 64, 2 symbols on device tensors: a demodulate call, then set_pilot_bins (the
    pilots in another order with other values, one data bin fewer) and estimate_channel, then
    the call again on the same handle. The first result has the bits of a fresh engine, the
    second those of a fresh engine configured the same way before its first call."""
    c, r = make_cfg(lib, "qam16")
    iq = torch.from_numpy(rx_signal(lib, c, r, 1, 2, 61)).cuda()
    tr = rand_c(np.random.default_rng(62), 64)
    pilots = np.array([b % 64 for b in PILOT_IDX[::-1]], np.uint32)

    def configure(d):
        lib.OfdmEqualizer.set_pilot_bins(d, pilots, np.array([1j, 1, -1, -1j], np.complex64),
                                         np.asarray(r.data_bins[1:], np.uint32))
        d.estimate_channel_freq(tr)
        return d

    def run(d):
        return [t.cpu().numpy() for t in lib.ofdm_demodulate_batch(d, iq, bits=True, llr=True)]

    want_first, want_second = run(lib.OfdmDemod(c, eq)), run(configure(lib.OfdmDemod(c, eq)))
    d = lib.OfdmDemod(c, eq)
    first = lib.ofdm_demodulate_batch(d, iq, bits=True, llr=True)  # left in flight: no read back before the tables change
    second = run(configure(d))
    assert all(same(g.cpu().numpy(), w) for g, w in zip(first, want_first))
    assert all(same(g, w) for g, w in zip(second, want_second))
    assert not same(second[0], want_first[0])


# ---- 3. the elementwise kernels -------------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
def test_decider_and_llr_kernels_exact(lib, order):
    c, r = make_cfg(lib, order, n_fft=8, cp=0, pilots=False, edge_guard=0)  # 6 data carriers per symbol
    v = R.edge_values(order, np.random.default_rng(41))  # 4099 soft symbols: 683 symbols and one over
    k = v.size // 6 * 6
    dec, sd = lib.OfdmDecider(c), lib.OfdmSoftDemod(c)
    assert same(dec.process(v), lib.ofdm_decide(order, v[:k])) and same(dec.process(v), R.decide(order, v[:k]))
    assert same(sd.process(v), lib.ofdm_llr(order, v[:k])) and same(sd.process(v), R.soft_llr(order, v[:k]))
    assert dec.process(v[:5]).size == 0 and sd.process(v[:5]).size == 0


@pytest.mark.parametrize("method", ["training_symbol", "pilot_interp"])
@pytest.mark.parametrize("n_fft", [64, 2048])
def test_equalizer_kernel_exact(lib, method, n_fft):
    c, r = make_cfg(lib, "qam16", n_fft=n_fft, cp=n_fft // 4)
    rng = np.random.default_rng(51)
    chan = rand_c(rng, n_fft, 0.7)
    edge = np.sqrt(np.float32(1e-6))
    chan[:6] = [edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1)), 0, 1e-3j, -1.0001e-3]
    x = (rand_c(rng, 5 * n_fft).reshape(5, n_fft).astype(np.complex128) * chan).astype(np.complex64).reshape(-1)
    eq = lib.OfdmEqualizer(c, method)
    assert same(eq.process(x), eq.process_host(x))  # before any estimate
    eq.estimate_from_training_symbol((R.training_pattern(n_fft).astype(np.complex128) * chan).astype(np.complex64))
    got, want = eq.process(x), eq.process_host(x)
    assert same(got, want) and got.size == 5 * n_fft
    if method == "training_symbol":
        # the null bin is erased; the bins at the floor fall either side of it by the estimate's own rounding
        assert np.all(got.reshape(5, n_fft)[:, 3] == 0) and np.all(got.reshape(5, n_fft)[:, 6:] != 0)
    assert eq.process(x[: n_fft - 1]).size == 0


# ---- 4. round trips -------------------------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("n_fft,cp", [(64, 16), (2048, 512)])
def test_round_trip_returns_the_bits(lib, order, n_fft, cp):
    """Noise free; tests/test_ofdm_oracle.py holds the restatement's soft symbols at least 30
    times the transform's error away from every threshold for these very configurations."""
    c, r = make_cfg(lib, order, n_fft=n_fft, cp=cp, pilots=n_fft == 64)
    bits = np.random.default_rng(8).integers(0, 2, 3 * r.bps).astype(np.uint8)
    iq = lib.OfdmMod(c).modulate(bits)
    soft = lib.OfdmDemod(c, None).process(iq)
    assert same(lib.OfdmDecider(c).process(soft), bits)
    assert same(lib.OfdmDemod(c).demodulate(iq), bits)  # the identity estimate
    # a static 3-tap channel under the training-symbol equalizer: the training symbol, then the data
    rx = R.channel3(np.concatenate([R.training_symbol(r), iq]))
    d = lib.OfdmDemod(c, "training_symbol")
    d.estimate_channel(rx[: r.sym_len])
    soft, got = d.demodulate_soft(np.ascontiguousarray(rx[r.sym_len:]))
    assert same(got, bits) and same(lib.OfdmDecider(c).process(soft), bits)
    fr = lib.build_ofdm_rx_frame(c, soft, got)
    print(f"[parity] round trip {order} n_fft={n_fft} through the 3-tap channel: EVM {fr.evm_db:.1f} dB")
    assert fr.num_symbols == 3 and fr.evm_db < -60


# ---- 5. the entry points agree --------------------------------------------------------------
def test_entry_points_agree(lib, torch):
    c, r = make_cfg(lib, "qam64", cp=5, gain=0.5, roll=2)
    bits = np.random.default_rng(61).integers(0, 2, 4 * r.bps).astype(np.uint8)
    m = lib.OfdmMod(c)
    a = m.modulate(bits)  # the handle's process, host pointers
    b = lib.ofdm_modulate_batch(m, bits.reshape(1, -1))[0]  # the Python batch, numpy
    t = lib.ofdm_modulate_batch(m, torch.from_numpy(bits).cuda().reshape(1, -1))  # the _device entry, resident
    assert t.is_cuda and same(a, b) and same(a, t.cpu().numpy()[0])
    assert same(m.modulate(torch.from_numpy(bits[:-3]).cuda()).cpu().numpy(), m.modulate(bits[:-3]))  # zero padding
    d = lib.OfdmDemod(c, "pilot_interp")
    s1 = d.process(a)
    s2, b2, l2 = lib.ofdm_demodulate_batch(d, a.reshape(1, -1), bits=True, llr=True)
    s3, b3, l3 = lib.ofdm_demodulate_batch(d, torch.from_numpy(a).cuda().reshape(1, -1), bits=True, llr=True)
    assert same(s1, s2[0]) and same(s1, s3.cpu().numpy()[0]) and same(b2, b3.cpu().numpy()) and same(l2, l3.cpu().numpy())
    assert same(lib.OfdmDecider(c).process(s1), b2[0]) and same(lib.OfdmSoftDemod(c).process(s1), l2[0])
    assert same(lib.OfdmDecider(c).process(s3.reshape(-1)).cpu().numpy(), b2[0])
    assert same(lib.OfdmSoftDemod(c).process(s3.reshape(-1)).cpu().numpy(), l2[0])
    # two channels of the same bits give the one channel twice
    two = lib.ofdm_modulate_batch(m, np.stack([bits, bits]))
    assert same(two[0], a) and same(two[1], a)
    # a short input gives a zero report and leaves the output alone
    out = np.full(r.sym_len, 7, np.complex64)
    wr = m.process_into(bits[: r.bps - 1], out)
    assert (wr.in_read, wr.out_written) == (0, 0) and np.all(out == 7)
    wr = m.process_into(bits, out)  # room for one symbol
    assert (wr.in_read, wr.out_written) == (r.bps, r.sym_len) and same(out, a[: r.sym_len])
    sout = np.zeros(len(r.data), np.complex64)
    wr = d.process_into(a[: r.sym_len - 1], sout)
    assert (wr.in_read, wr.out_written) == (0, 0)
    with pytest.raises(ValueError):
        d.demodulate(a[: r.sym_len - 1])
    with pytest.raises(ValueError):
        lib.ofdm_modulate_batch(m, bits[:-1].reshape(1, -1))
    with pytest.raises(ValueError):
        lib.ofdm_demodulate_batch(d, torch.from_numpy(a).cuda().reshape(1, -1).to(torch.complex128))
    for n_fft in (0, 6, 8192):
        with pytest.raises(ValueError):
            lib.FftBlock(n_fft)
        with pytest.raises(ValueError):
            lib.OfdmConfig(n_fft, 0, np.array([1], np.int32), PILOT_IDX[:0], PILOT_VAL[:0], 1e6, 0.0, 1.0, "qpsk")
