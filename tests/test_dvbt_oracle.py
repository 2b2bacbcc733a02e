"""CPU: the DVB-T 2K frame on the host (orion_sdr's dvb_t_* functions, TpsWord, DvbTFrameMod.modulate,
DvbTFrameDemod.decode) against tests/np_ref_dvbt.py, bit for bit (floats as uint32) in every
output, plus the known answers of EN 300 744 and the properties of the reference's
tests/roundtrip/dvb_t.rs ported to the host path. The noisy capture set that tests/test_gpu_dvbt.py
decodes on the device is built here and shown to hold every outcome on the host alone.

Not here: a frame shaped by the TX low-pass (the mask rows of the reference's zero-lead-in test);
the library's TX low-pass is a device filter, so that case lives in the GPU file."""
import numpy as np
import pytest

import np_ref_dvbt as R

F = np.float32


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def same32(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex64 if (a.dtype.kind == "c" or b.dtype.kind == "c") else np.float32
    a, b = np.atleast_1d(a.astype(dt)), np.atleast_1d(b.astype(dt))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits_int(bits):
    return int("".join(str(int(b)) for b in bits), 2)


def params(lib, guard="1/32", constellation="qpsk", rate="1/2", frame_number=2, cell_id=0x5A):
    return lib.DvbTFrameParams(guard, constellation, rate, frame_number, cell_id)


@pytest.fixture(scope="module")
def capstone(lib):
    """The capstone link's frame of sample_payload(184), modulated once for the module."""
    p = lib.DvbTFrameParams(*R.CAPTURE_PARAMS)
    return p, R.sample_payload(R.CAPTURE_PAYLOAD_LEN), lib.DvbTFrameMod(p).modulate(R.sample_payload(R.CAPTURE_PAYLOAD_LEN))


def outcome(lib, demod, iq, n_symbols, payload_len):
    try:
        return demod.decode(np.ascontiguousarray(iq), n_symbols, payload_len)
    except lib.DvbTRxError as e:
        return e.kind


# ---- constants and grid ---------------------------------------------------------------------
def test_constants_and_prbs(lib):
    assert list(lib.DVB_T_CONTINUAL_PILOTS_2K) == R.CONTINUAL and len(R.CONTINUAL) == 45
    assert list(lib.DVB_T_TPS_CARRIERS_2K) == R.TPS_CARRIERS and len(R.TPS_CARRIERS) == 17
    wk = lib.wk_prbs(1705)
    assert np.array_equal(wk, R.wk_prbs(1705))
    assert list(wk[:13]) == [1] * 11 + [0, 0]
    for w in (0, 1):
        assert same32(lib.boosted_pilot_value(w), R.boosted_pilot_value(w))
    assert same32(lib.boosted_pilot_value(0), np.complex64(F(4.0) / F(3.0)))
    assert lib.DVB_T_MAX_RX_WINDOW_BACKOFF == 85 == R.MAX_RX_WINDOW_BACKOFF
    assert list(lib.tps_carrier_bins()) == R.tps_carrier_bins()
    assert list(lib.continual_pilot_bins()) == R.continual_pilot_bins()
    for phase in range(6):
        assert list(lib.scattered_pilot_indices(phase)) == R.scattered_pilot_indices(phase)


@pytest.mark.parametrize("guard", ["1/32", "1/16", "1/8", "1/4"])
def test_plans_have_1512_data_carriers(lib, guard):
    plans = lib.dvb_t_2k_plans(guard)
    assert len(plans) == 4
    tps = set(R.tps_carrier_bins())
    for got, want in zip(plans, R.PLANS):
        assert got["cp_len"] == R.GUARD_CP[guard] == lib.dvb_t_cp_len_2k(guard)
        assert len(got["data_bins"]) == 1512 and np.array_equal(got["data_bins"], want["data_bins"])
        assert np.array_equal(got["pilot_bins"], want["pilot_bins"]) and same32(got["pilot_values"], want["pilot_values"])
        assert np.array_equal(got["ref_bins"], want["ref_bins"]) and same32(got["ref_values"], want["ref_values"])
        assert list(got["ref_bins"]) == sorted(got["ref_bins"]) and not (set(got["ref_bins"]) & tps)
        assert len(got["ref_bins"]) == len(got["pilot_bins"]) - 17 <= 193
        role = got["role"]
        assert np.array_equal(np.flatnonzero(role >= 0)[np.argsort(role[role >= 0])], want["data_bins"])
        assert np.count_nonzero(role == -1) == 2048 - 1705
        assert [int(np.flatnonzero(role == -4 - j)[0]) for j in range(17)] == R.tps_carrier_bins()


# ---- constellation --------------------------------------------------------------------------
@pytest.mark.parametrize("v", [2, 4, 6])
def test_constellation(lib, v):
    every = np.array([[(i >> (v - 1 - j)) & 1 for j in range(v)] for i in range(1 << v)], np.uint8)
    pts = lib.dvb_t_map_symbol(every)
    assert same32(pts, R.map_symbols(every, v))
    assert abs(float(np.mean(np.abs(pts.astype(np.complex128)) ** 2)) - 1.0) < 1e-6  # unit average energy
    assert np.array_equal(lib.dvb_t_demap_symbol(pts, v), every)
    assert same32(lib.dvb_t_map_symbol(every[3]), pts[3]) and np.array_equal(lib.dvb_t_demap_symbol(pts[3], v), every[3])
    # even bits move I only, odd bits Q only
    flip0, flip1 = every[0].copy(), every[0].copy()
    flip0[0], flip1[1] = 1, 1
    a, b0, b1 = pts[0], lib.dvb_t_map_symbol(flip0), lib.dvb_t_map_symbol(flip1)
    assert b0.imag == a.imag and b0.real != a.real and b1.real == a.real and b1.imag != a.imag
    rng = np.random.default_rng(90 + v)
    noisy = (np.repeat(pts, 8) + (rng.standard_normal(8 << v) + 1j * rng.standard_normal(8 << v)) * 0.3).astype(np.complex64)
    edge = np.array([0, -0.0, 1e-30, -1e-30, 3.0 + 3.0j, -5 - 0.5j, np.inf, complex(0.1, -np.inf)], np.complex64)
    x = np.concatenate([pts, noisy, edge])
    assert same32(lib.dvb_t_soft_llr(x, v), R.soft_llrs(x, v))
    assert np.array_equal(lib.dvb_t_demap_symbol(x, v), R.demap_symbols(x, v))
    clean = lib.dvb_t_soft_llr(pts, v)
    assert np.array_equal((clean <= 0).astype(np.uint8), every)  # positive means 0
    assert lib.dvb_t_map_symbol(np.zeros(3, np.uint8)) is None and lib.dvb_t_soft_llr(pts, 8) is None


# ---- TPS ------------------------------------------------------------------------------------
def test_bch_known_answers(lib):
    one = np.zeros(53, np.uint8)
    one[52] = 1
    assert bits_int(lib.tps_bch_encode(one)[53:]) == 0x377 == R.tps_bch_parity(one)
    assert bits_int(lib.tps_bch_encode(np.ones(53, np.uint8))[53:]) == 0x3CD1
    assert not lib.tps_bch_encode(np.zeros(53, np.uint8)).any()
    rng = np.random.default_rng(7)
    for _ in range(8):
        info = rng.integers(0, 2, 53, dtype=np.uint8)
        cw = lib.tps_bch_encode(info)
        assert np.array_equal(cw, R.tps_bch_encode(info)) and np.array_equal(cw[:53], info)
        assert np.array_equal(lib.tps_bch_decode(cw), info)


def test_bch_corrects_one_and_two_errors(lib):
    info = np.random.default_rng(8).integers(0, 2, 53, dtype=np.uint8)
    cw = lib.tps_bch_encode(info)
    for i in range(67):
        bad = cw.copy()
        bad[i] ^= 1
        assert np.array_equal(lib.tps_bch_decode(bad), info), i
    rng = np.random.default_rng(9)
    pairs = {(0, 66), (0, 1), (65, 66), (0, 53), (52, 53), (33, 34)} | {tuple(sorted(rng.choice(67, 2, replace=False))) for _ in range(60)}
    for i, j in sorted(pairs):
        bad = cw.copy()
        bad[[i, j]] ^= 1
        assert np.array_equal(lib.tps_bch_decode(bad), info), (i, j)
        assert np.array_equal(R.tps_bch_decode(bad), info), (i, j)


def test_bch_three_errors_as_the_restatement(lib):
    info = np.random.default_rng(10).integers(0, 2, 53, dtype=np.uint8)
    cw = lib.tps_bch_encode(info)
    rng = np.random.default_rng(11)
    triples = [(0, 1, 2), (0, 33, 66), (64, 65, 66)] + [tuple(rng.choice(67, 3, replace=False)) for _ in range(80)]
    rejected = 0
    for t in triples:
        bad = cw.copy()
        bad[list(t)] ^= 1
        got, want = lib.tps_bch_decode(bad), R.tps_bch_decode(bad)
        assert (got is None) == (want is None) and (got is None or np.array_equal(got, want)), t
        assert got is None or not np.array_equal(got, info)  # never the word that was sent
        rejected += got is None
    assert 0 < rejected  # the code is not perfect: some triples are rejected (the rest miscorrect)
    assert lib.tps_bch_decode(np.zeros(66, np.uint8)) is None


def test_tps_word(lib):
    for fn in range(4):
        for con, rate, guard, cell in (("qpsk", "1/2", "1/32", 0x5A), ("qam16", "3/4", "1/8", 0), ("qam64", "7/8", "1/4", 255),
                                      ("qam16", "2/3", "1/16", 0x33), ("qpsk", "5/6", "1/4", 1)):
            w = lib.TpsWord(fn, con, rate, guard, cell)
            bits = w.pack()
            assert np.array_equal(bits, R.tps_pack(fn, con, rate, guard, cell))
            assert bits[0] == 0 and bits_int(bits[1:17]) == (0x35EE if fn % 2 == 0 else 0xCA11)
            assert lib.TpsWord.unpack(bits) == w and R.tps_unpack(bits) == (fn, con, rate, guard, cell)
            flipped = bits.copy()
            flipped[0] = 1  # s0 is ignored
            flipped[[3, 60]] ^= 1
            assert lib.TpsWord.unpack(flipped) == w
    assert lib.TPS_SYNC_WORD_13 == 0x35EE and lib.TPS_SYNC_WORD_24 == 0xCA11
    # reserved codes: constellation 0b11, rate 0b101 and 0b111 (valid BCH words): None
    base = R.tps_pack(1, "qpsk", "1/2", "1/32", 7)
    for field, value in (((24, 26), 0b11), ((29, 32), 0b101), ((29, 32), 0b111)):
        info = base[1:54].copy()
        a, b = field
        info[a:b] = [(value >> (b - a - 1 - j)) & 1 for j in range(b - a)]
        bits = np.concatenate([[0], R.tps_bch_encode(info)]).astype(np.uint8)
        assert lib.TpsWord.unpack(bits) is None and R.tps_unpack(bits) is None
    assert lib.TpsWord.unpack(np.zeros(67, np.uint8)) is None


def test_tps_encoder_and_decoder(lib):
    bits = R.tps_pack(3, "qam64", "2/3", "1/8", 0xC3)
    enc, got = lib.TpsEncoder(), []
    for s in range(70):
        got.append(enc.next_symbol(bits[s % 68]))
        if (s + 1) % 68 == 0:
            enc.reset()
    want = R.tps_encode(bits, 70)
    assert same32(np.array(got), want)
    assert same32(want[68], want[0]) and np.all(want.imag == 0) and np.all(np.abs(want.real) == 1)
    rng = np.random.default_rng(12)
    rx = (want[:68] * np.complex64(0.3 - 0.8j) + (rng.standard_normal((68, 17)) + 1j * rng.standard_normal((68, 17))) * 0.2)
    rx = rx.astype(np.complex64)
    rx[9] = 0  # every product of symbols 9 and 10 is zero: the sums are exactly 0, the bits 0
    rx[30, :16] = [1, -1] * 8  # symbol 31 against this: the 16 products cancel exactly where the next row is constant
    rx[31, :16], rx[30, 16], rx[31, 16] = 1, 0, 0
    dec = lib.TpsDecoder()
    for row in rx:
        dec.feed_symbol(row)
    assert dec.is_complete() and np.array_equal(dec.bits(), R.tps_decide(rx))
    assert dec.bits()[9] == 0 and dec.bits()[10] == 0 and dec.bits()[31] == 0
    half = lib.TpsDecoder()
    for row in rx[:67]:
        half.feed_symbol(row)
    assert not half.is_complete() and half.word() is None and len(half.bits()) == 67
    clean = lib.TpsDecoder()
    for row in want[:68]:
        clean.feed_symbol(row)
    assert clean.word() == lib.TpsWord(3, "qam64", "2/3", "1/8", 0xC3)


# ---- guard-interval acquisition ---------------------------------------------------------------
def gi_same(lib, iq, n_fft, cp, fs, search_len, **cfg):
    want = R.gi_sync(iq, n_fft, cp, fs, search_len, detail=True, **cfg)
    got, metric = lib.dvb_t_gi_metric(np.ascontiguousarray(iq), n_fft, cp, float(fs), search_len, lib.GiSyncConfig(**cfg))
    if want is None:
        assert got is None and metric is None
        return None
    assert got is not None and got.start_sample == want["start"]
    assert same32(metric, want["metric"])
    for a, b in ((got.gamma, want["gamma"]), (got.phi, want["phi"]), (got.score, want["score"]), (got.cfo_hz, want["cfo_hz"])):
        assert same32(a, b), (a, b)
    return got


def test_gi_sync_edge_cases(lib, capstone):
    p, _, fr = capstone
    sps, fs = fr.samples_per_symbol, R.fs_1mhz()
    six = fr.iq[:6 * sps]
    for lead in (0, 200, sps - 1):
        got = gi_same(lib, R.place(six, lead, sps), 2048, 64, fs, sps)
        assert got.start_sample == lead and got.score > 0.999
    noisy = R.awgn(R.place(six, 300, sps), 0.3 * R.rms(six), 21)
    for ms in (1, 4):
        got = gi_same(lib, noisy, 2048, 64, fs, sps, max_symbols=ms)
        assert abs(got.start_sample - 300) <= 2
    # a silent lead-in that ends just below a period boundary: the peak is within cp / 2 of the
    # boundary, but the origin is silence (score 0), so the unwrap's second condition keeps the peak
    got = gi_same(lib, R.place(six, 2100, sps), 2048, 64, fs, sps)
    assert got.start_sample == 2100 and got.score > 0.999
    # a frequency offset is reported with its sign
    cfo = float(fs) / 2048 * 0.2
    got = gi_same(lib, R.rotate(R.place(six, 200, sps), cfo, fs), 2048, 64, fs, sps)
    assert got.start_sample == 200 and abs(float(got.cfo_hz) - cfo) < 0.02 * cfo
    # all zero: every metric ties at 0, the last offset wins, then the unwrap (0 >= 0.5 * 0) takes the origin
    zero = np.zeros(2 * sps + 5, np.complex64)
    got = gi_same(lib, zero, 2048, 64, fs, sps)
    assert got.start_sample == 0 and got.score == 0 and got.cfo_hz == 0
    got = gi_same(lib, zero, 2048, 64, fs, sps, origin_score_ratio=0.0)
    assert got.start_sample == sps - 1
    got = gi_same(lib, zero, 2048, 64, fs, sps - 40)  # the last offset is not near a boundary: no unwrap
    assert got.start_sample == sps - 41
    # one sample too short, and the degenerate arguments
    exact = R.place(six, 0, 0)[:2 * sps - 1]
    assert gi_same(lib, exact, 2048, 64, fs, sps) is not None
    assert gi_same(lib, exact[:-1], 2048, 64, fs, sps) is None
    assert gi_same(lib, exact, 2048, 64, fs, 0) is None and gi_same(lib, exact, 2048, 0, fs, 8) is None
    # a second geometry, and refine
    p4 = params(lib, "1/4", "qam16", "3/4")
    f4 = lib.DvbTFrameMod(p4).with_symbol_window(16).modulate(R.sample_payload(100))
    got = gi_same(lib, R.place(f4.iq[:5 * 2560], 333, 2560), 2048, 512, fs, 2560)
    assert abs(got.start_sample - 333) <= 8
    want = R.gi_refine(noisy, 2048, 64, fs, 290, 20)
    ref = lib.dvb_t_gi_refine(noisy, 2048, 64, float(fs), 290, 20)
    assert ref.start_sample == want["start"] and same32(ref.cfo_hz, want["cfo_hz"]) and same32(ref.score, want["score"])


def test_integer_cfo(lib, capstone):
    _, _, fr = capstone
    freq = lib.fft_host(np.ascontiguousarray(fr.iq[64:64 + 2048]), 2048)
    for k in (0, -7, -1, 3, 12):
        shifted = np.ascontiguousarray(np.roll(freq, k))
        got, want = lib.dvb_t_integer_cfo(shifted, 2048, 32), R.integer_cfo(shifted, 2048, 32)
        assert got[0] == want[0] == k and same32(got[1], want[1]) and got[1] > 1.3
    assert lib.dvb_t_integer_cfo(freq, 2048, 0) is None and R.integer_cfo(freq, 2048, 0) is None
    assert lib.dvb_t_integer_cfo(freq[:2047].copy(), 2048, 32) is None
    assert lib.dvb_t_integer_cfo(np.zeros(2048, np.complex64), 2048, 4) == (-4, 0.0)  # the first of equal maxima


# ---- the frame ------------------------------------------------------------------------------
def test_frame_known_answers(lib):
    assert lib.block_plan(188, params(lib).scheme()).coded_bits == 39180 == R.coded_bits_for_packets(1, "1/2")
    fr = lib.DvbTFrameMod(params(lib))
    n_symbols, target = fr.plan(184)
    assert (n_symbols, target) == R.frame_plan(184, "qpsk", "1/2") and n_symbols == 68
    assert n_symbols * 1512 * 2 == 205632
    assert same32(np.float32(params(lib).fs), R.fs_1mhz())
    sch = params(lib, rate="3/4").scheme()
    assert (sch.crc, sch.outer, sch.inner, sch.outer_interleaver, sch.scrambler) == \
        ("none", ("rs", 204, 16), ("conv", "3/4", "dvb_k7"), ("forney", 12, 17), None)


MCS = [("1/32", "qpsk", "1/2", 184), ("1/16", "qpsk", "2/3", 37), ("1/8", "qam16", "3/4", 400), ("1/4", "qam64", "7/8", 184)]


@pytest.mark.parametrize("guard,con,rate,n", MCS)
def test_noiseless_round_trip(lib, guard, con, rate, n):
    p = params(lib, guard, con, rate, 1, 0x33)
    payload = R.sample_payload(n)
    fr = lib.DvbTFrameMod(p).modulate(payload)
    iq, n_symbols, sps = R.modulate(payload, guard, con, rate, 1, 0x33)
    assert (fr.n_symbols, fr.samples_per_symbol) == (n_symbols, sps) and same32(fr.iq, iq)
    buf = R.place(fr.iq, 200, sps)
    got = lib.DvbTFrameDemod(p).decode(buf, n_symbols, n)
    assert np.array_equal(got.payload, payload) and got.tps == p.tps_word()
    d = got.diagnostics
    assert d["timing_offset_samples"] == 200 and d["integer_cfo_bins"] is None and d["outer_fec_ok"] is True
    assert d["evm_db"] is None and d["channel_ber"] is None and d["inner_ber"] is None
    want = R.decode(buf, n_symbols, n, guard, con, rate)
    assert np.array_equal(want["payload"], payload) and want["tps"] == (1, con, rate, guard, 0x33)
    assert same32(d["cfo_hz"], want["cfo_hz"]) and same32(d["sync_score"], want["sync_score"])
    assert d["rs_corrected_bytes"] == want["rs_corrected_bytes"] and d["timing_offset_samples"] == want["timing_offset_samples"]


@pytest.mark.parametrize("v,cp,roll,short", [(2, 64, 0, 0), (4, 512, 16, 77), (6, 128, 200, 3000)])
def test_symbols_level_against_the_restatement(lib, v, cp, roll, short):
    rng = np.random.default_rng(40 + v)
    n_symbols = 70  # both phase cycles and the TPS reset after symbol 67
    bits = rng.integers(0, 2, n_symbols * 1512 * v - short, dtype=np.uint8)
    tps = R.tps_pack(3, "qam16", "5/6", "1/8", 0xA5)
    iq = lib.dvb_t_mod_symbols(bits, v, cp, tps, n_symbols, roll)
    assert same32(iq, R.mod_symbols(bits, v, cp, tps, n_symbols, roll))
    sps = 2048 + cp
    rx = R.awgn(R.two_tap(iq[:9 * sps]), 0.1 * R.rms(iq), 50 + v)
    rx[3 * sps:4 * sps] = 0  # a silent symbol: every estimate is under the floor, the erasure branch
    for backoff in (0, cp // 2, cp + 5):
        llr, cells, syms = lib.dvb_t_demod_symbols(rx, 9, cp, backoff, v, syms=True)
        l2, c2, s2 = R.demod_symbols(rx, 9, cp, backoff, v)
        assert same32(llr, l2) and same32(cells, c2) and same32(syms, s2)
        assert not syms[3].any() and syms[2].any()


def test_two_tap_multipath_decodes(lib, capstone):
    p, payload, fr = capstone
    buf = R.place(R.two_tap(fr.iq), 200, fr.samples_per_symbol)
    got = lib.DvbTFrameDemod(p).decode(buf, fr.n_symbols, payload.size)
    assert np.array_equal(got.payload, payload) and got.tps == p.tps_word()


def test_window_with_backoff_is_transparent(lib, capstone):
    p, payload, _ = capstone
    fr = lib.DvbTFrameMod(p).with_symbol_window(32).modulate(payload)
    buf = R.place(fr.iq, 200, fr.samples_per_symbol)
    got = lib.DvbTFrameDemod(p).with_rx_window_backoff(32).decode(buf, fr.n_symbols, payload.size)
    assert np.array_equal(got.payload, payload) and got.tps == p.tps_word()
    want = R.decode(buf, fr.n_symbols, payload.size, "1/32", "qpsk", "1/2", backoff=32)
    assert np.array_equal(want["payload"], payload) and same32(got.diagnostics["cfo_hz"], want["cfo_hz"])
    assert got.diagnostics["timing_offset_samples"] == want["timing_offset_samples"]


@pytest.mark.parametrize("con,rate", [("qpsk", "1/2"), ("qpsk", "3/4"), ("qam16", "3/4")])
def test_short_payload_leaves_no_data_carrier_zero(lib, con, rate):
    p = params(lib, "1/8", con, rate, 0, 0)
    fr = lib.DvbTFrameMod(p).modulate(R.sample_payload(184))
    sps = fr.samples_per_symbol
    plans = lib.dvb_t_2k_plans("1/8")
    for s in range(fr.n_symbols):
        freq = lib.fft_host(np.ascontiguousarray(fr.iq[s * sps + 256:(s + 1) * sps]), 2048)
        assert np.all(np.abs(freq[plans[s % 4]["data_bins"]]) >= 1e-6), s


def test_integer_cfo_builder(lib):
    p = params(lib, "1/8", "qpsk", "1/2", 0, 0)
    payload = R.sample_payload(184)
    fr = lib.DvbTFrameMod(p).modulate(payload)
    fs = R.fs_1mhz()
    shifted = lib.ofdm_rotate_block(fr.iq, float(F(5.0) * F(fs / F(2048))), float(fs))
    buf = R.place(shifted, 200, fr.samples_per_symbol)
    assert isinstance(outcome(lib, lib.DvbTFrameDemod(p), buf, fr.n_symbols, 184), str)  # off: the offset breaks the decode
    got = lib.DvbTFrameDemod(p).with_integer_cfo_correction(True).decode(buf, fr.n_symbols, 184)
    assert np.array_equal(got.payload, payload) and got.diagnostics["integer_cfo_bins"] == 5
    want = R.decode(buf, fr.n_symbols, 184, "1/8", "qpsk", "1/2", integer_cfo_on=True)
    assert want["integer_cfo_bins"] == 5 and same32(got.diagnostics["cfo_hz"], want["cfo_hz"])
    assert abs(float(got.diagnostics["cfo_hz"]) - 5.0 * float(fs) / 2048) < 1.0
    on = lib.DvbTFrameDemod(p).with_integer_cfo_correction(True).decode(R.place(fr.iq, 200, fr.samples_per_symbol), fr.n_symbols, 184)
    assert on.diagnostics["integer_cfo_bins"] == 0 and np.array_equal(on.payload, payload)  # measured, nothing to rotate


@pytest.mark.parametrize("roll", [0, 8, 32])
def test_shaped_frame_with_no_lead_in_acquires_at_zero(lib, roll):
    p = params(lib, "1/8", "qpsk", "1/2", 1, 0x33)
    payload = R.sample_payload(184)
    fr = lib.DvbTFrameMod(p).with_symbol_window(roll).modulate(payload)
    got = lib.DvbTFrameDemod(p).with_rx_window_backoff(32).decode(fr.iq, fr.n_symbols, 184)
    assert got.diagnostics["timing_offset_samples"] == 0 and np.array_equal(got.payload, payload) and got.tps.guard == "1/8"


# ---- the capture set of the GPU test ----------------------------------------------------------
def test_capture_set_holds_every_outcome(lib, capstone):
    p, payload, fr = capstone
    rows, names, short = R.capture_set(fr.iq, fr.n_symbols, fr.samples_per_symbol)
    demod = lib.DvbTFrameDemod(p)
    got = {n: outcome(lib, demod, r, fr.n_symbols, payload.size) for r, n in zip(rows, names)}
    got["short"] = outcome(lib, demod, short, fr.n_symbols, payload.size)
    kinds = {n: (g if isinstance(g, str) else "decoded") for n, g in got.items()}
    assert kinds == {"clean": "decoded", "noisy": "decoded", "multipath": "decoded", "payload_fails": "payload_decode",
                     "tps_fails": "tps_decode", "truncated": "incomplete", "short": "acquisition"}
    for n in ("clean", "noisy", "multipath"):
        assert np.array_equal(got[n].payload, payload) and got[n].tps == p.tps_word()
    assert got["noisy"].diagnostics["rs_corrected_bytes"] >= 1
    # the restatement agrees on one decoded and on every failed capture
    for n, r in list(zip(names, rows)) + [("short", short)]:
        if n in ("clean", "multipath"):
            continue
        want = R.decode(r, fr.n_symbols, payload.size, "1/32", "qpsk", "1/2")
        assert (want if isinstance(want, str) else "decoded") == kinds[n], n
    with pytest.raises(lib.DvbTRxError) as e:
        demod.decode(short, fr.n_symbols, payload.size)
    assert e.value.code == lib.DVB_T_RX_ERRORS["acquisition"] and e.value == "acquisition"
