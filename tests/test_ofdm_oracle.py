"""CPU: the library's host side of the OFDM symbol layer (csrc/ofdm.cpp through the C ABI)
against tests/np_ref_ofdm.py bit for bit, the reference's own unit properties
(tests/unit/ofdm.rs) on it, the argument errors, and the host code under the sanitizers as
a stand-alone program. No kernel is launched here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_ofdm as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILOT_IDX = np.array([-21, -7, 7, 21], np.int32)
PILOT_VAL = np.array([1, -1, 1j, 1], np.complex64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


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


def rand_c(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


# ---- tables, plans, grids -----------------------------------------------------------------
@pytest.mark.parametrize("order", ["qam16", "qam64", "qam256"])
def test_axis_and_threshold_tables(lib, order):
    axis, thr, _, _, _ = lib.ofdm_tables(order)
    assert same(axis, R.axis_table(R.BITS[order])) and same(thr, R.threshold_table(R.BITS[order]))
    m = 1 << (R.BITS[order] // 2)
    lv = np.sort(axis[:m])
    assert np.allclose(np.mean(2 * lv.astype(np.float64) ** 2), 1.0, atol=1e-6)  # unit average energy
    assert np.allclose(thr[: m - 1], (lv[:-1] + lv[1:]) / 2, atol=1e-7)


def test_training_pattern_twiddles_and_ramp(lib):
    for n in (8, 64, 2048):
        _, _, tr, tw, ramp = lib.ofdm_tables("qpsk", n, n + 16, 5)
        assert same(tr, R.training_pattern(n)) and same(tw, R.twiddles(n)) and same(ramp, R.window_ramp(n + 16, 5))
        assert np.all(np.abs(np.abs(tr) - 1) < 1e-6)
    # roll_off is clamped to symbol_len / 2; the ramp rises from near 0 to near 1
    assert lib.ofdm_tables("qpsk", 0, 10, 99)[4].size == 5
    r = lib.ofdm_tables("qpsk", 0, 80, 8)[4]
    assert 0 < r[0] < 0.05 and 0.95 < r[-1] < 1 and np.all(np.diff(r) > 0)


def test_plan_contiguous_data_grid_and_occupied_bins(lib):
    for n_fft, g, pil in [(64, 0, False), (64, 4, True), (8, 1, False), (1024, 0, False)]:
        c, r = make_cfg(lib, n_fft=n_fft, cp=n_fft // 4, pilots=pil, edge_guard=g)
        assert same(c.data_carriers, r.data)
        d, p = c.grid()
        assert same(d, r.data_bins) and same(p, r.pilot_bins)
        assert same(c.occupied_bins(), R.occupied_bins(n_fft, r.data, r.pilot_idx))
        assert c.occupied_half_carriers == R.occupied_half_carriers(r.data, r.pilot_idx)
        assert c.bits_per_ofdm_symbol == r.bps and c.samples_per_ofdm_symbol == r.sym_len
        assert c.data_carriers[0] == -(n_fft // 2) + 1 + g and 0 not in c.data_carriers
        c.validate_edge_guard(g)
    assert make_cfg(lib, n_fft=1024, cp=128, pilots=False, edge_guard=0)[0].num_data_carriers == 1022
    with pytest.raises(ValueError, match="in_guard_band"):
        make_cfg(lib, edge_guard=4)[0].validate_edge_guard(5)
    assert lib.ofdm_max_pilot_safe_backoff(2048, 12) == 85 and lib.ofdm_max_pilot_safe_backoff(64, 0) == 32


def test_validate_errors_and_rejected_sizes(lib):
    z32, zc = np.zeros(0, np.int32), np.zeros(0, np.complex64)

    def cfg(n_fft, cp, data, pi=z32, pv=zc, **kw):
        return lib.OfdmConfig(n_fft, cp, np.asarray(data, np.int32), pi, pv, 1e6, 0.0, 1.0, "qpsk", **kw)

    with pytest.raises(ValueError, match="empty_data_set"):
        cfg(64, 16, [])
    with pytest.raises(ValueError, match=r"out_of_range \(carrier index 32\)"):
        cfg(64, 16, [1, 32])
    with pytest.raises(ValueError, match=r"out_of_range \(carrier index -33\)"):
        cfg(64, 16, [1], np.array([-33], np.int32), np.ones(1, np.complex64))
    with pytest.raises(ValueError, match=r"overlap \(carrier index 3\)"):
        cfg(64, 16, [1, 2, 3], np.array([3], np.int32), np.ones(1, np.complex64))
    with pytest.raises(ValueError, match=r"overlap \(carrier index 2\)"):
        cfg(64, 16, [1, 2, 2])
    assert cfg(64, 16, [-32, 31]).num_data_carriers == 2  # the bounds themselves are in range
    for n_fft in (0, 6, 8192):
        with pytest.raises(ValueError, match="power of two"):
            cfg(n_fft, 0, [1])
        with pytest.raises(ValueError, match="power of two"):
            lib.FftBlock(n_fft)
        with pytest.raises(ValueError, match="power of two"):
            lib.IfftBlock(n_fft)
        with pytest.raises(ValueError):
            lib.fft_host(np.zeros(16, np.complex64), n_fft)
    with pytest.raises(ValueError, match="cp_len"):
        cfg(64, 65, [1])
    with pytest.raises(ValueError, match="edge_guard"):
        cfg(64, 16, [1], edge_guard=2)
    with pytest.raises(ValueError, match="same length"):
        cfg(64, 16, [1], np.array([3], np.int32), zc)
    with pytest.raises(ValueError, match="constellation"):
        lib.OfdmConfig(64, 16, np.array([1], np.int32), z32, zc, 1e6, 0.0, 1.0, "qam32")
    with pytest.raises(ValueError):
        lib.OfdmConfig(64, 16, np.array([1], np.int64), z32, zc, 1e6, 0.0, 1.0, "qpsk")
    c = cfg(64, 16, [1, 2])
    with pytest.raises(ValueError):
        lib.OfdmMod(c).modulate(np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        lib.OfdmMod(c).modulate(np.zeros((2, 4), np.uint8))
    with pytest.raises(ValueError):
        lib.OfdmDemod(c).demodulate(np.zeros(160, np.complex64)[::2])
    with pytest.raises(ValueError, match="equalizer"):
        lib.OfdmDemod(c, "zero_forcing")


# ---- mappers, deciders, LLRs ----------------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
def test_mapper_decider_llr_bit_exact(lib, order):
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 256, 4099 * R.BITS[order]).astype(np.uint8)  # only the LSB counts
    syms = lib.ofdm_map(order, bits)
    assert same(syms, R.map_bits(order, bits))
    assert same(lib.ofdm_decide(order, syms), bits & 1)
    v = R.edge_values(order, rng)
    hard, llr = lib.ofdm_decide(order, v), lib.ofdm_llr(order, v)
    assert same(hard, R.decide(order, v)) and same(llr, R.soft_llr(order, v))
    # tests/unit/ofdm.rs: the LLR's sign is the hard decision wherever it is not near zero
    big = np.abs(llr) > 1e-3
    assert big.mean() > 0.9 and np.array_equal((llr[big] < 0).astype(np.uint8), hard[big])
    if order == "bpsk":
        assert syms[0] == (1 if bits[0] & 1 == 0 else -1)


# ---- the transform --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 16, 64, 256, 1024, 2048, 4096])
def test_host_transform_is_the_restatement(lib, n):
    x = rand_c(np.random.default_rng(5), 3 * n)
    for inv in (False, True):
        got = lib.fft_host(x, n, inv)
        assert same(got, R.fft_radix2(x.reshape(3, n), inv).reshape(-1))
        e = R.nrmse(got.reshape(3, n), R.fft_truth(x.reshape(3, n), inv))
        print(f"[parity] host radix-2 n={n} inverse={inv}: nrmse vs f64 {e:.3e}")
        assert e < 5e-7
    assert R.nrmse(lib.fft_host(lib.fft_host(x, n), n, True), x) < 5e-7
    # tests/unit/ofdm.rs: the inverse of a DC bin is 1 / n everywhere; a partial chunk is a no-op
    dc = np.zeros(n, np.complex64)
    dc[0] = 1
    assert np.max(np.abs(lib.fft_host(dc, n, True) - 1.0 / n)) < 1e-5
    assert lib.fft_host(x[: n - 1], n).size == 0


# ---- window, rotator, modulator ---------------------------------------------------------------
def test_window_and_rotator_bit_exact(lib):
    x = rand_c(np.random.default_rng(2), 3 * 69)
    for roll in (0, 2, 5, 34, 60):
        assert same(lib.ofdm_window(x, 69, roll), R.window_apply(x.reshape(3, 69), R.window_ramp(69, roll)).reshape(-1))
    assert same(lib.ofdm_rotator(12345.0, 1e6, 2500), R.rotator(12345.0, 1e6, 2500))


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("cp,rf,roll", [(16, 0.0, 0), (5, 0.0, 2), (0, 0.0, 0), (16, 125e3, 3)])
def test_modulator_bit_exact_and_its_properties(lib, order, cp, rf, roll):
    c, r = make_cfg(lib, order, cp=cp, rf_hz=rf, gain=0.25, roll=roll)
    bits = np.random.default_rng(3).integers(0, 2, 3 * r.bps - 7).astype(np.uint8)
    m = lib.OfdmMod(c)
    got = m.modulate_host(bits)
    rot = R.rotator(rf, 1e6, 2 * got.size) if rf else None
    assert got.size == 3 * r.sym_len
    assert same(got, R.modulate(r, bits, None if rot is None else rot[: got.size]))
    if rf:  # the phase carries across calls
        assert same(m.modulate_host(bits), R.modulate(r, bits, rot[got.size:]))
    # a partial chunk is a no-op; whole symbols only
    out = np.zeros(2 * r.sym_len, np.complex64)
    wr = m.process_host_into(bits[: r.bps - 1], out)
    assert (wr.in_read, wr.out_written) == (0, 0)
    wr = lib.OfdmMod(c).process_host_into(bits, out)
    assert (wr.in_read, wr.out_written) == (2 * r.bps, 2 * r.sym_len)
    if not rf and not roll:
        s = got.reshape(3, r.sym_len)
        assert cp == 0 or same(s[:, :cp], s[:, -cp:])  # the prefix is the tail, exactly
        f = np.fft.fft(s[:, cp:].astype(np.complex128), axis=1) / 0.25
        null = np.setdiff1d(np.arange(64), np.concatenate([r.data_bins, r.pilot_bins]))
        assert np.max(np.abs(f[:, null])) < 1e-3  # null carriers are silent
        assert np.max(np.abs(f[:, r.pilot_bins] - PILOT_VAL)) < 1e-3
        # zero padding: the last symbol equals the modulation of the padded bits
        padded = np.concatenate([bits, np.zeros(7, np.uint8)])
        assert same(lib.OfdmMod(c).modulate_host(padded), got)


# ---- demodulator, equalizer ---------------------------------------------------------------
@pytest.mark.parametrize("backoff", [0, 3, 16])
@pytest.mark.parametrize("eq", [None, "training_symbol", "pilot_interp"])
def test_demodulator_bit_exact(lib, backoff, eq):
    c, r = make_cfg(lib, "qam16", backoff=backoff)
    rng = np.random.default_rng(4)
    iq = rand_c(rng, 5 * r.sym_len + 9, 0.2)
    d = lib.OfdmDemod(c, eq)
    req = R.Equalizer(r, eq) if eq else None
    if eq:
        tr = rand_c(rng, 64)
        d.estimate_channel_freq(tr)
        req.estimate_from_training_symbol(tr)
    assert same(d.process_host(iq), R.demodulate(r, iq, 1.0, req))
    d.set_gain(1.0 + 1e-7)  # within f32::EPSILON of 1: no gain stage
    req = R.Equalizer(r, eq) if eq else None
    if eq:
        req.estimate_from_training_symbol(tr)
    assert same(d.process_host(iq), R.demodulate(r, iq, 1.0, req))
    d.set_gain(4.0)
    got = d.process_host(iq)
    assert same(got, R.demodulate(r, iq, 4.0, req)) and got.size == 5 * len(r.data)
    assert d.process_host(iq[: r.sym_len - 1]).size == 0


def test_equalizer_weights_interpolation_and_properties(lib):
    rng = np.random.default_rng(6)
    h = rand_c(rng, 4099, 0.5)
    h[:6] = np.array([1e-3, 1.0001e-3, 0.9999e-3, 0, 7.0710678e-4 + 7.0710678e-4j, 1e-20], np.complex64)
    h[6] = np.sqrt(np.float32(1e-6))
    h[7] = np.nextafter(np.sqrt(np.float32(1e-6)), np.float32(0))
    assert same(lib.ofdm_equalizer_weight(h), R.equalizer_weight(h))
    pb = np.array([3, 9, 10, 40, 61], np.uint32)
    ratios = rand_c(rng, 5)
    bins = np.arange(64, dtype=np.uint32)
    got = lib.ofdm_interpolate(pb, ratios, bins)
    assert same(got, np.array([R.interpolate_at(pb, ratios, int(b)) for b in bins], np.complex64))
    # tests/unit/ofdm.rs: held past the outer pilots, on a pilot its own ratio, between two
    # pilots between their ratios; one pilot is held everywhere
    assert np.all(got[:4] == ratios[0]) and np.all(got[61:] == ratios[4]) and got[40] == ratios[3]
    lo, hi = np.minimum(ratios[2].real, ratios[3].real), np.maximum(ratios[2].real, ratios[3].real)
    assert np.all((got[11:40].real >= lo - 1e-6) & (got[11:40].real <= hi + 1e-6))
    assert np.all(lib.ofdm_interpolate(pb[:1], ratios[:1], bins) == ratios[0])

    # a static channel through the training symbol: corrected, and a null bin erased
    c, r = make_cfg(lib, "qam16")
    eq = lib.OfdmEqualizer(c, "training_symbol")
    x = rand_c(rng, 2 * 64)
    assert same(eq.process_host(x), x)  # identity until an estimate is taken
    chan = rand_c(rng, 64, 0.7)
    chan[5] = 0
    eq.estimate_from_training_symbol((R.training_pattern(64).astype(np.complex128) * chan).astype(np.complex64))
    req = R.Equalizer(r, "training_symbol")
    req.estimate_from_training_symbol((R.training_pattern(64).astype(np.complex128) * chan).astype(np.complex64))
    y = (x.reshape(2, 64).astype(np.complex128) * chan).astype(np.complex64).reshape(-1)
    got = eq.process_host(y)
    assert same(got, np.concatenate([req.process(y[:64]), req.process(y[64:])]))
    keep = np.abs(chan) > 0.05
    assert np.max(np.abs(got.reshape(2, 64)[:, keep] - x.reshape(2, 64)[:, keep])) < 1e-4
    assert np.all(got.reshape(2, 64)[:, 5] == 0)

    # pilot interpolation, the estimate carried between calls; no pilots: a pass-through
    pe, rpe = lib.OfdmEqualizer(c, "pilot_interp"), R.Equalizer(r, "pilot_interp")
    assert same(pe.process_host(y), np.concatenate([rpe.process(y[:64]), rpe.process(y[64:])]))
    pe.set_pilot_bins(np.array([50, 4], np.uint32), np.array([1, 1j], np.complex64), np.arange(5, 50, dtype=np.uint32))
    rpe.pbins, rpe.pvals = np.array([4, 50], np.uint32), np.array([1j, 1], np.complex64)
    rpe.dbins = np.arange(5, 50, dtype=np.uint32)
    assert same(pe.process_host(y[:64]), rpe.process(y[:64]))
    c0, _ = make_cfg(lib, "qam16", pilots=False)
    assert same(lib.OfdmEqualizer(c0, "pilot_interp").process_host(x), x)
    with pytest.raises(ValueError):
        lib.OfdmEqualizer(c, "nearest")


# ---- round trips on the restatement and the host ---------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("n_fft,cp", [(64, 16), (2048, 512)])
def test_round_trip_margins_on_the_restatement(lib, order, n_fft, cp):
    """Noise free, the restatement's soft symbols lie at least 30 times the transform's error
    from any decision threshold (the GPU round trips rest on this), with and without a static
    3-tap channel under the training-symbol equalizer; the host library returns the bits."""
    c, r = make_cfg(lib, order, n_fft=n_fft, cp=cp, pilots=n_fft == 64, edge_guard=4)
    bits = np.random.default_rng(8).integers(0, 2, 3 * r.bps).astype(np.uint8)
    iq = R.modulate(r, bits)
    soft = R.demodulate(r, iq)
    ideal = R.map_bits(order, bits)
    nb = R.BITS[order]
    half = float(R.axis_scale(nb)) if nb >= 4 else (1.0 if order == "bpsk" else float(R.FRAC_1_SQRT_2))
    err = float(np.max(np.abs(soft.astype(np.complex128) - ideal)))
    print(f"[parity] {order} n_fft={n_fft}: max soft error {err:.3e}, half spacing {half:.3f}, margin {half / err:.0f}x")
    assert half >= 30 * err
    assert np.array_equal(R.decide(order, soft), bits)
    assert np.array_equal(lib.ofdm_decide(order, lib.OfdmDemod(c, None).process_host(lib.OfdmMod(c).modulate_host(bits))), bits)
    # the 3-tap channel: the training symbol first, then the data, one stream
    rx = R.channel3(np.concatenate([R.training_symbol(r), iq]))
    req = R.Equalizer(r, "training_symbol")
    req.estimate_from_training_symbol(R.symbol_freq(r, rx[: r.sym_len])[0])
    soft = R.demodulate(r, rx[r.sym_len:], 1.0, req)
    err = float(np.max(np.abs(soft.astype(np.complex128) - ideal)))
    print(f"[parity] {order} n_fft={n_fft} 3-tap channel: max soft error {err:.3e}, margin {half / err:.0f}x")
    assert half >= 30 * err and np.array_equal(R.decide(order, soft), bits)
    d = lib.OfdmDemod(c, "training_symbol")
    d.estimate_channel_freq(lib.fft_host(np.ascontiguousarray(rx[cp: r.sym_len]), n_fft))
    assert np.array_equal(lib.ofdm_decide(order, d.process_host(rx[r.sym_len:])), bits)


def test_gain_inverts_and_evm(lib):
    c, r = make_cfg(lib, "qam64", gain=0.25)
    bits = np.random.default_rng(9).integers(0, 2, 2 * r.bps).astype(np.uint8)
    d = lib.OfdmDemod(c, None)
    d.set_gain(4.0)
    soft = d.process_host(lib.OfdmMod(c).modulate_host(bits))
    assert np.max(np.abs(soft - R.map_bits("qam64", bits))) < 1e-4  # tests/unit/ofdm.rs: gain inverts
    # EVM of a known error: every symbol displaced by 0.1 of the unit average energy
    ideal = R.map_bits("qam64", bits)
    off = (ideal + np.complex64(0.06 + 0.08j)).astype(np.complex64)
    fr = lib.build_ofdm_rx_frame(c, off, bits)
    want = R.evm_db("qam64", off, bits)
    assert fr.num_symbols == 2 and np.array_equal(fr.bits, bits) and np.float32(fr.evm_db) == want
    assert abs(fr.evm_db - 10 * np.log10(0.01 / np.mean(np.abs(ideal.astype(np.complex128)) ** 2))) < 0.2
    assert fr.cfo_hz is None and fr.timing_offset_samples is None and fr.channel_mse is None and fr.sync_score is None
    assert lib.build_ofdm_rx_frame(c, off[:0], bits[:0]).evm_db is None
    assert lib.build_ofdm_rx_frame(c, off, bits[:-6]).evm_db is None  # the mapper comes up short


# ---- the exact GPU tests' reference, input sets and their sharpness ---------------------------
# tests/test_gpu_ofdm_exact.py holds the kernels to fft_host and to the restatement by R.same_bits on
# R.input_sets; here the two references are tied to each other on those very sets, the sets are
# shown to be what they claim, and every departure a kernel change could bring (R.FFT_VARIANTS,
# R.EQ_VARIANTS) is shown to change at least one word of a set named below.
NOTICED_BY = {"fma": "normal", "w0": "negzero", "f32tw": "normal", "ftz": "subnormal", "tw_rot": "impulse",
              "tw_rot_fused": "impulse"}
# tw_rot (W^(j + len/4) as -i W^j) reads (-0.0, -1) for the table's (6.1e-17, -1) at W^(len/4) and is the
# table's value everywhere else. Normal, integer, subnormal and top rows never see it. The negzero rows see it
# in every stage (tw_rot) but, placed where a kernel fusing two stages would place it (tw_rot_fused), only
# where log2 n is even; overflow rows (inf times +-0) see tw_rot at the sizes below only. The impulse rows
# are there for this: with one half of every butterfly an exact zero the 6.1e-17 itself comes out, at every size.
TW_ROT_SEEN_BY_OVERFLOW = (8, 16, 32)


def test_same_bits_rule():
    f = np.float32
    a = np.array([1.0, 0.0, np.inf, np.nan, 5e-42], f)
    assert R.same_bits(a, a.copy()) and R.same_bits(a[:4].view(np.complex64), a[:4].copy().view(np.complex64))
    quiet = a.copy()
    quiet.view(np.uint32)[3] = 0xFFC00001  # another NaN: sign and payload are not compared
    assert R.same_bits(a, quiet)
    for i, v in ((1, f(-0.0)), (2, f(-np.inf)), (3, f(1.0)), (0, f(np.nan)), (4, f(0.0)), (0, np.nextafter(f(1), f(2)))):
        b = a.copy()
        b[i] = v
        assert not R.same_bits(a, b) and R.diff_words(a, b) == 1
    assert not R.same_bits(a, a.astype(np.float64)) and not R.same_bits(a, a[:4])
    assert R.same_bits(np.arange(5, dtype=np.uint8), np.arange(5, dtype=np.uint8))
    assert not R.same_bits(np.arange(5, dtype=np.uint8), np.arange(5, dtype=np.uint8)[::-1])


def test_interpolation_in_one_pass_is_the_scalar_form(lib):
    rng = np.random.default_rng(12)
    for pb in ([5], [3, 9, 10, 40, 61], [0, 63], [7, 21, 43, 57]):
        ratios = rand_c(rng, len(pb))
        ratios[0] = R.cplx(-0.0, 0.0)[()]
        bins = rng.permutation(64)
        for variant in (None, "interp_fma"):
            want = np.array([R.interpolate_at(pb, ratios, int(b), variant) for b in bins], np.complex64)
            assert same(R.interpolate_bins(pb, ratios, bins, variant), want)
        assert same(R.interpolate_bins(pb, ratios, bins), lib.ofdm_interpolate(np.array(pb, np.uint32), ratios, bins))


@pytest.mark.parametrize("n", R.FFT_SIZES)
def test_host_transform_is_the_restatement_on_every_input_set(lib, n):
    for name, x in R.input_sets(n).items():
        for inv in (False, True):
            assert R.same_bits(lib.fft_host(x.reshape(-1), n, inv).reshape(x.shape), R.fft_radix2(x, inv)), (name, inv)


@pytest.mark.parametrize("n", R.FFT_SIZES)
def test_input_sets_are_what_they_claim(n):
    s = R.input_sets(n)
    assert list(s) == ["normal", "integers", "negzero", "impulse", "subnormal", "top", "overflow"]
    assert np.count_nonzero(s["impulse"]) == 4 and np.all(np.abs(s["impulse"]).sum(1) == 1)
    assert all(v.dtype == np.complex64 and v.ndim == 2 and v.shape[1] == n for v in s.values())
    again = R.input_sets(n)
    assert all(same(s[k], again[k]) for k in s)  # seeded
    ints = s["integers"].view(np.float32)
    assert np.all(ints == np.round(ints)) and np.abs(ints).max() == 8
    z = s["negzero"].view(np.float32)
    assert np.all(z == 0) and np.signbit(z[0]).all() and np.signbit(z[1]).sum() == 1
    for inv in (False, True):
        sub = R.fft_radix2(s["subnormal"], inv).view(np.float32)
        top = R.fft_radix2(s["top"], inv).view(np.float32)
        over = R.fft_radix2(s["overflow"], inv).view(np.float32)
        share = (np.abs(sub) < R.TINY).mean(1)
        print(f"[sets] n={n} inverse={inv}: subnormal-or-zero share {share.min():.4f}, nonzero {np.count_nonzero(sub)}; "
              f"overflow rows inf {np.isinf(over).sum(1).tolist()} NaN {np.isnan(over).sum(1).tolist()} of {over.shape[1]}")
        assert np.all(share >= 0.99) and np.count_nonzero(sub) > sub.size // 2
        assert np.all(np.isfinite(top)) and (inv or np.abs(top).max() > 1e37)  # finite, and near the top of the range
        assert np.all(np.isinf(over).sum(1) >= 1) and np.all(np.isnan(over).sum(1) <= over.shape[1] // 2)


@pytest.mark.parametrize("variant", R.FFT_VARIANTS)
def test_every_transform_departure_is_noticed_by_a_named_set(variant):
    for n in R.FFT_SIZES:
        s = R.input_sets(n)
        counts = {name: [R.diff_words(R.fft_radix2(x, inv, variant), R.fft_radix2(x, inv)) for inv in (False, True)]
                  for name, x in s.items()}
        print(f"[sharp] {variant} n={n}: words changed forward/inverse " +
              ", ".join(f"{k} {c[0]}/{c[1]} of {s[k].size * 2}" for k, c in counts.items()))
        assert min(counts[NOTICED_BY[variant]]) >= 1
        if variant == "w0":  # invisible on every input without a signed zero, as measured before these sets existed
            assert counts["normal"] == [0, 0] and counts["integers"] == [0, 0] and counts["negzero"] == [4, 4]
        if variant == "ftz":
            assert all(c == [0, 0] for k, c in counts.items() if k != "subnormal")
        if variant in ("tw_rot", "tw_rot_fused"):
            assert all(counts[k] == [0, 0] for k in ("normal", "integers", "subnormal", "top"))
        if variant == "tw_rot":
            assert (min(counts["overflow"]) >= 1) == (n in TW_ROT_SEEN_BY_OVERFLOW) and min(counts["negzero"]) >= 1
        if variant == "tw_rot_fused":  # the signed zeros alone would let it through at 8, 32, 128, 512 and 2048
            assert (min(counts["negzero"]) >= 1) == ((n.bit_length() - 1) % 2 == 0)


@pytest.mark.parametrize("boost", [False, True])
@pytest.mark.parametrize("n", [8, 64, 4096])
def test_every_equalizer_departure_is_noticed(n, boost):
    """R.equalizer_case is what tests/test_gpu_ofdm_exact.py feeds k_ofdm_equalize. recip needs a
    pilot whose |value|^2 is not 1 (boost); interp_fma needs two pilots (not n = 8); floor_strict
    changes exactly the bins that carry the estimate whose |h|^2 is on the floor."""
    cfg, x = R.equalizer_case(n, boost)
    assert R.validate(n, cfg.data, cfg.pilot_idx) == (0, 0)
    want, erased = R.equalizer_run(cfg, x)
    R.check_equalizer_erasures(cfg, erased)
    for variant in R.EQ_VARIANTS:
        got, _ = R.equalizer_run(cfg, x, variant)
        rows = [R.diff_words(got[i], want[i]) for i in range(len(x))]
        print(f"[sharp] {variant} n_fft={n} boost={boost}: words changed per row {rows}")
        can = {"recip": boost, "interp_fma": n > 8, "floor_strict": True}[variant]
        assert (sum(rows) >= 1) == can
        if variant == "floor_strict":
            assert [i for i, c in enumerate(rows) if c] == [R.EQ_ROWS["floor_on"]]


# ---- the host code under the sanitizers ---------------------------------------------------
def test_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/ofdm.cpp and tests/ofdm_host/main.cpp, built with the host compiler alone and
    -fsanitize=address,undefined into a stand-alone binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "ofdm_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src,
                    os.path.join(src, "ofdm.cpp"), os.path.join(ROOT, "tests", "ofdm_host", "main.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ofdm_host: ok" in out.stdout, out.stdout + out.stderr
