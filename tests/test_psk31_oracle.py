"""CPU: the library's host side of PSK31 (csrc/psk31.cpp through the C ABI:
orion_varicode_*, orion_conv_encode, orion_psk31_viterbi_host / _hard_host,
orion_psk31_streaming_viterbi_*, orion_psk31_tables, orion_psk31_mod_*, orion_psk31_demod_*,
orion_bpsk31_decide) against tests/np_ref_psk31.py, byte for byte, the argument errors of
the entry points that reach no device, and the host code under the sanitizers as a
stand-alone program.

The restatement decodes each Viterbi case once (np_ref_psk31.viterbi_case caches it); the
GPU tests share the same cases."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_psk31 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


# ---- Varicode ---------------------------------------------------------------------------
def test_varicode_table_is_the_alphabet(lib):
    cw, ln, exp = lib.psk31_tables()
    assert [(int(c), int(n)) for c, n in zip(cw, ln)] == P.VARICODE
    assert exp.tobytes() == np.array(P.DQPSK_EXP, np.float32).tobytes()
    # what the alphabet must be whatever its source: distinct codewords of 1..10 bits that
    # begin and end with 1 and hold no "00"; and a few every PSK31 text shows
    words = [format(c, "b").zfill(n) for c, n in P.VARICODE]
    assert len(set(words)) == 128
    assert all(1 <= len(w) <= P.VARICODE_MAX_BITS and w[0] == "1" and w[-1] == "1" and "00" not in w for w in words)
    assert [words[ord(c)] for c in " eto"] == ["1", "11", "101", "111"] and words[0] == "1010101011"
    assert lib.VARICODE_MAX_BITS == P.VARICODE_MAX_BITS and lib.PSK31_TRACEBACK_DEPTH == P.TRACEBACK_DEPTH


def test_every_byte_round_trips(lib):
    for b in range(256):
        cw, n = lib.varicode_encode(b)
        assert (cw, n) == P.varicode_encode(b)
        assert lib.varicode_decode(cw, n) == (b if b < 128 else 0)
    # codewords not in the table: a known word at another length, "00" inside, nothing at all
    for cw, n in [(0b11, 3), (0b1001, 4), (0, 0), (0, 5), (0b1, 2), (0xFFFF, 16), (0b11111111111, 11)]:
        assert lib.varicode_decode(cw, n) is None and P.varicode_decode(cw, n) is None


@pytest.mark.parametrize("preamble", [None, 0, 5, 32])
def test_encoder_framing(lib, preamble):
    """With and without a preamble, a postamble, and bytes pushed after both: the first
    flag decides where the "00" gaps go (varicode.rs:216-252)."""
    text = b"CQ CQ de \x00\xff~"
    e, r = lib.VaricodeEncoder(), P.VaricodeEncoder()
    assert e.is_empty()
    for enc in (e, r):
        if preamble is not None:
            enc.push_preamble(preamble)
        for b in text:
            enc.push_byte(b)
        enc.push_postamble(7)
        enc.push_byte(ord("x"))  # after a postamble: first is false, so a gap
        enc.push_preamble(3)
        enc.push_byte(ord("y"))  # after a preamble: no gap
        enc.push_postamble(0)
    assert not e.is_empty()
    got, want = e.drain_bits(), r.drain_bits()
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert e.is_empty() and e.drain_bits().size == 0
    # a postamble on a fresh encoder has no gap before it
    # and draining does not make it fresh: first stays false
    fresh = lib.VaricodeEncoder()
    fresh.push_postamble(4)
    assert fresh.drain_bits().tolist() == [1, 1, 1, 1]
    e.push_postamble(4)
    assert e.drain_bits().tolist() == [0, 0, 1, 1, 1, 1]


def test_decoder_is_the_restatement(lib):
    rng = np.random.default_rng(31)
    streams = [P.text_bits(bytes(range(128)), 32, 32), P.text_bits(b"hello world", 0, 0),
               rng.integers(0, 2, 4000).astype(np.uint8),                       # arbitrary bits
               (rng.random(4000) < 0.85).astype(np.uint8),                      # long runs of ones: the len cap
               np.concatenate([np.ones(40, np.uint8), [0, 0, 1, 1, 0, 0]]).astype(np.uint8)]
    for bits in streams:
        d, r = lib.VaricodeDecoder(), P.VaricodeDecoder()
        got = b""
        for a in range(0, len(bits), 997):  # ragged pushes: the state carries over
            d.push_bits(bits[a:a + 997])
            got += d.pop_bytes()
        for b in bits:
            r.push_bit(int(b))
        assert got == r.pop_bytes()
        assert d.pop_bytes() == b""
    d = lib.VaricodeDecoder()
    d.push_bits(P.text_bits(bytes(range(128)), 32, 32))
    assert d.pop_bytes() == bytes(range(128))
    # bit 0 alone is shifted in, but only a zero byte is a zero bit (varicode.rs:291): 2, 2 is no "00"
    d.push_bits(np.array([3, 2, 2, 0, 0], np.uint8))
    r = P.VaricodeDecoder()
    for b in (3, 2, 2, 0, 0):
        r.push_bit(b)
    assert d.pop_bytes() == r.pop_bytes()


# ---- the convolutional code -------------------------------------------------------------
def test_conv_encode(lib):
    rng = np.random.default_rng(5)
    for n in (0, 1, 4, 5, 33, 300):
        bits = rng.integers(0, 2, n).astype(np.uint8)
        got = lib.conv_encode(bits)
        assert got.dtype == np.uint8 and got.tobytes() == P.conv_encode(bits).tobytes()
        assert lib.conv_encode(bits | 0xFE).tobytes() == got.tobytes()  # only bit 0 is read
    # the impulse response is the two generators, 25 and 23 octal, newest bit first
    imp = lib.conv_encode(np.array([1, 0, 0, 0, 0], np.uint8)).reshape(5, 2)
    assert imp[:, 0].tolist() == [1, 0, 1, 0, 1] and imp[:, 1].tolist() == [1, 0, 0, 1, 1]


@pytest.mark.parametrize("kind", P.VITERBI_KINDS)
@pytest.mark.parametrize("n_syms", P.VITERBI_LENGTHS)
def test_viterbi_decode_is_the_restatement(lib, n_syms, kind):
    for k in range(3):
        soft, want = P.viterbi_case(n_syms, kind, k)
        got = lib.viterbi_decode(soft)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (n_syms, kind, k)
    if kind == "zero":
        assert not want.any()  # ties keep the lower predecessor and the first final state
    if kind == "clean" and n_syms >= 33:
        bits = np.random.default_rng(1000 * n_syms).integers(0, 2, n_syms).astype(np.uint8)
        assert np.array_equal(P.viterbi_case(n_syms, kind, 0)[1][:-4], bits[:-4])


def test_viterbi_edge_inputs(lib):
    """Empty input; NaN, infinite and huge values (outside the contract: defined all the
    same, and the same in both); metrics pinned at the start value."""
    assert lib.viterbi_decode(np.zeros(0, np.float32)).size == 0
    rng = np.random.default_rng(9)
    base = P.dqpsk_soft(rng.integers(0, 2, 40).astype(np.uint8), 0.3, 3)
    for v in (np.nan, np.inf, -np.inf, 3.0e38, 1.0e19, -1.0e19):
        for where in (slice(None), slice(10, 11), slice(0, 1), slice(78, 80)):
            soft = base.copy()
            soft[where] = v
            assert lib.viterbi_decode(soft).tobytes() == P.viterbi_decode(soft).tobytes(), (v, where)


def test_viterbi_decode_hard(lib):
    rng = np.random.default_rng(6)
    for n in (0, 1, 2, 5, 33, 300):
        bits = rng.integers(0, 2, n).astype(np.uint8)
        coded = P.conv_encode(bits)
        got = lib.viterbi_decode_hard(coded)
        assert got.tobytes() == P.viterbi_decode_hard(coded).tobytes()
        assert np.array_equal(got, bits)  # clean hard input decodes exactly, tail included
        flipped = coded.copy()
        flipped[::17] ^= 1
        assert lib.viterbi_decode_hard(flipped).tobytes() == P.viterbi_decode_hard(flipped).tobytes()


def test_streaming_viterbi_across_its_normalisation(lib):
    """600 symbols: the metrics lose their minimum after symbols 256 and 512, and the ring of
    128 rows wraps four times; fed in ragged pieces; flush gives the last 32 bits."""
    bits = np.random.default_rng(8).integers(0, 2, 600).astype(np.uint8)
    for sigma in (0.0, 0.5):
        soft = P.dqpsk_soft(bits, sigma, 21)
        v, r = lib.StreamingViterbi(), P.StreamingViterbi()
        got = []
        for a, b in ((0, 31), (31, 32), (32, 33), (33, 255), (255, 257), (257, 600)):
            out = v.feed(soft[2 * a:2 * b])
            assert out.dtype == np.uint8 and out.size == max(0, b - max(a, P.TRACEBACK_DEPTH))
            got.append(out)
        got.append(v.flush())
        want = np.concatenate([r.feed(soft), r.flush()])
        assert np.concatenate(got).tobytes() == want.tobytes()
        assert want.size == 600
        if sigma == 0.0:
            assert np.array_equal(want[:-4], bits[:-4])
        # a second flush keeps feeding zero symbols: still the restatement's
        assert v.flush().tobytes() == r.flush().tobytes()


# ---- modulators and demodulators ---------------------------------------------------------
FS_CASES = (8000.0, 12000.0)
RF = 1000.0
N_SYMS = 14


def _mod(lib, mode, *a):
    return (lib.Bpsk31Mod if mode == P.BPSK else lib.Qpsk31Mod)(*a)


def _demod(lib, mode, *a):
    return (lib.Bpsk31Demod if mode == P.BPSK else lib.Qpsk31Demod)(*a)


@pytest.mark.parametrize("fs", FS_CASES)
def test_sps_hann_and_text_bits(lib, fs):
    assert lib.psk31_sps(fs) == P.psk31_sps(fs) == {8000.0: 256, 12000.0: 384}[fs]
    for f in (31.25, 46.874, 46.876, 11025.0, 48000.0, 0.0, -8000.0, float("nan")):
        assert lib.psk31_sps(f) == (P.psk31_sps(f) if f == f else 0), f
    assert lib.psk31_text_bits(b"CQ CQ", 64, 32).tobytes() == P.text_bits(b"CQ CQ", 64, 32).tobytes()
    assert lib.psk31_text_bits(b"", 0, 0).size == 0
    # a constant phase (all ones) leaves gain * (1 + h * 0); the window itself shows in a flip
    m = lib.Bpsk31Mod(fs, 0.0, 1.0)
    flip = m.modulate_bits(np.array([0], np.uint8))
    want = (np.float32(1.0) + P.make_hann(P.psk31_sps(fs)) * np.float32(-2.0)).astype(np.float32)
    assert flip.real.tobytes() == want.tobytes() and not flip.imag.any()


@pytest.mark.parametrize("mode", [P.BPSK, P.QPSK])
@pytest.mark.parametrize("fs", FS_CASES)
def test_host_modulators_are_the_restatement(lib, fs, mode):
    """rf_hz 0 and 1000; the phasor (and QPSK31's register) carried into a second call, whose
    Rotator starts afresh; reset; set_gain. QPSK31's phasor products give -0.0: bytes compare."""
    bits = np.random.default_rng(3).integers(0, 2, 12).astype(np.uint8)
    for rf in (0.0, RF):
        m, r = _mod(lib, mode, fs, rf, 0.7), P.Mod(mode, fs, rf, 0.7)
        for b in (bits, bits[:5], bits[5:]):
            got, want = m.modulate_bits(b), r.modulate_bits(b)
            assert got.dtype == np.complex64 and got.shape == (len(b) * P.psk31_sps(fs),)
            assert got.tobytes() == want.tobytes(), (fs, mode, rf)
        m.reset(), r.reset()
        m.set_gain(0.25)
        r.gain = np.float32(0.25)
        assert m.modulate_bits(bits).tobytes() == r.modulate_bits(bits).tobytes()
        m.reset(), r.reset()
        text = m.modulate_text(b"hi", 3, 2)
        assert text.tobytes() == r.modulate_bits(P.text_bits(b"hi", 3, 2)).tobytes()
    if mode == P.QPSK:
        zeros = np.flatnonzero(P.Mod(mode, fs, 0.0, 1.0).modulate_bits(bits).view(np.uint32) == 0x80000000)
        assert zeros.size  # the fixture does hold negative zeros
    m = _mod(lib, mode, fs, 0.0, 1.0)
    sps = P.psk31_sps(fs)
    out, nread = m.process(bits, 3 * sps + 17)  # Block::process: whole symbols only
    assert nread == 3 and out.shape == (3 * sps,)
    assert out.tobytes() == P.Mod(mode, fs, 0.0, 1.0).modulate_bits(bits[:3]).tobytes()
    assert m.process(bits, sps - 1)[1] == 0


def _channels(fs):
    """Four channels of N_SYMS symbols + 37 samples: BPSK31 and QPSK31 at rf 0 and RF, gain
    0.8, with Gaussian noise of deviation 0.05 per component."""
    rng = np.random.default_rng(int(fs))
    rows = []
    for mode in (P.BPSK, P.QPSK):
        for rf in (0.0, RF):
            bits = rng.integers(0, 2, N_SYMS + 1).astype(np.uint8)
            rows.append(P.Mod(mode, fs, rf, 0.8).modulate_bits(bits)[:N_SYMS * P.psk31_sps(fs) + 37])
    x = np.stack(rows)
    noise = rng.normal(0.0, 0.05, x.shape + (2,)).astype(np.float32)
    return (x + noise.view(np.complex64)[..., 0]).astype(np.complex64)


def _records(fs):
    sps = P.psk31_sps(fs)
    rec = []
    for ch, (mode, rf) in enumerate([(P.BPSK, 0.0), (P.BPSK, RF), (P.QPSK, 0.0), (P.QPSK, RF)]):
        for offset in (0, 1, sps - 1, sps, sps + 7):
            rec.append(P.stream_record(mode, ch, rf, 1.25, 0, offset))
        rec.append(P.stream_record(mode, ch, rf, 1.25, 0, 0, out_cap=5))  # the capacity cuts the call short
    return rec


@pytest.mark.parametrize("fs", FS_CASES)
def test_host_demodulators_are_the_restatement(lib, fs):
    """rf_hz 0 and non-zero, new_with_offset at 0, 1, sps - 1, sps, sps + 7, and an output of 5
    values: BPSK stops after the sample that wrote the fifth (5 symbols), QPSK when one slot
    is left (2 symbols, 4 values), so their in_read differ."""
    x, rec = _channels(fs), _records(fs)
    soft, in_read, out_written = P.DemodBank(fs, rec).process(x)
    sps = P.psk31_sps(fs)
    for k, r in enumerate(rec):
        d = _demod(lib, r["mode"], fs, r["rf_hz"], r["gain"], r["offset"])
        cap = r["out_cap"] if r["out_cap"] < 100 else None
        got, nread = d.process_host(x[r["channel"]], cap)
        assert got.tobytes() == soft[k].tobytes(), (fs, k, r)
        assert nread == in_read[k] and got.size == out_written[k]
        if cap:
            assert (nread, got.size) == ((5 * sps, 5) if r["mode"] == P.BPSK else (2 * sps, 4))
    assert min(float(np.abs(s).max()) for s in soft) > 0.5  # the streams do demodulate something


@pytest.mark.parametrize("mode", [P.BPSK, P.QPSK])
def test_host_demodulator_chunked_calls_equal_one_call(lib, mode):
    fs = 8000.0
    x = _channels(fs)[1 if mode == P.BPSK else 3]
    whole, _ = _demod(lib, mode, fs, RF, 1.0, 3).process_host(x)
    d = _demod(lib, mode, fs, RF, 1.0, 3)
    parts, at = [], 0
    for n in (1000, 1, 5000, len(x)):
        got, nread = d.process_host(x[at:at + n])
        assert nread == min(n, len(x) - at)
        parts.append(got)
        at += nread
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    d.reset()  # reset: count 0 as well (demodulate/psk31.rs:136-144), so it is new(.., offset 0) again
    again, _ = d.process_host(x)
    assert again.tobytes() == _demod(lib, mode, fs, RF, 1.0, 0).process_host(x)[0].tobytes()
    # and the restatement carries its state the same way
    r = P.DemodBank(fs, [P.stream_record(mode, 0, RF, 1.0, 0, 3)])
    a, _, _ = r.process(x[None, :1000])
    b, _, _ = r.process(x[None, 1000:])
    assert np.concatenate([a[0], b[0]]).tobytes() == whole.tobytes()


def test_decider_and_clean_text_round_trips(lib):
    """Bpsk31Decider is soft >= 0 (-0.0 and 0.0 give 1, NaN 0); the reference's clean text
    round trips (tests/roundtrip/psk31.rs): BPSK31 through the decider, QPSK31 through the
    Viterbi decoder, both through Varicode."""
    soft = np.array([1.0, -1.0, 0.0, -0.0, np.nan, 1e-30, -1e-30], np.float32)
    assert lib.Bpsk31Decider().process(soft).tolist() == [1, 0, 1, 1, 0, 1, 0]
    for mode, text in ((P.BPSK, b"CQ CQ DE TEST"), (P.QPSK, b"TEST de orion 599")):
        for rf in (0.0, 1500.0):
            iq = _mod(lib, mode, 8000.0, rf, 1.0).modulate_text(text, 32, 32)
            soft, nread = _demod(lib, mode, 8000.0, rf, 1.0).process_host(iq)
            assert nread == iq.size
            bits = lib.Bpsk31Decider().process(soft) if mode == P.BPSK else lib.viterbi_decode(soft)
            d = lib.VaricodeDecoder()
            d.push_bits(bits)
            assert d.pop_bytes() == text


# ---- carrier search on hand-made waterfalls -----------------------------------------------
LOW, HIGH = np.float32(-27.6), np.float32(-2.0)  # ln(1e-12) and a carrier's log energy


def _wf(num_syms, num_bins, runs, rng=None):
    """A quiet waterfall (LOW plus a little seeded unevenness) with (bin, first, last+1, level) runs."""
    wf = np.full((num_syms, num_bins), LOW, np.float32)
    if rng is not None:
        wf += rng.uniform(0.0, 0.5, wf.shape).astype(np.float32)
    for b, a, e, level in runs:
        wf[a:e, b] = level
    return wf


def _same(lib, wf, min_run, margin, max_cand):
    got = lib.psk31_find_carriers(wf, min_run, margin, max_cand)
    want = P.find_carriers(wf, min_run, margin, max_cand)
    assert got.dtype == lib.CANDIDATE_DTYPE
    assert [(int(c["time_sym"]), int(c["freq_bin"]), np.float32(c["score"]).tobytes()) for c in got] == \
        [(t, b, sc.tobytes()) for t, b, sc in want]
    return [(int(c["time_sym"]), int(c["freq_bin"])) for c in got]


def test_search_runs_edges_and_min_run(lib):
    rng = np.random.default_rng(7)
    # a run that reaches the end of the buffer is flushed; one that starts at symbol 0
    assert _same(lib, _wf(40, 7, [(2, 30, 40, HIGH), (5, 0, 9, HIGH + 1)], rng), 8, 6.0, 10) == [(0, 5), (30, 2)]
    # one symbol short of min_run: nothing; exactly min_run: found
    assert _same(lib, _wf(40, 7, [(3, 10, 17, HIGH)], rng), 8, 6.0, 10) == []
    assert _same(lib, _wf(40, 7, [(3, 10, 18, HIGH)], rng), 8, 6.0, 10) == [(10, 3)]
    # min_carrier_syms 0 counts as 1
    assert _same(lib, _wf(12, 3, [(1, 5, 6, HIGH)]), 0, 6.0, 10) == [(5, 1)]
    # the first and the last bin have no neighbour on one side
    assert _same(lib, _wf(30, 4, [(0, 2, 12, HIGH), (3, 15, 30, HIGH)], rng), 8, 6.0, 10) == [(2, 0), (15, 3)]


def test_search_plateau_global_threshold_and_medians(lib):
    # a carrier between two bins: both hold the same energy, and >= keeps both
    assert _same(lib, _wf(30, 6, [(2, 5, 17, HIGH), (3, 5, 17, HIGH)]), 8, 6.0, 10) == [(5, 2), (5, 3)]
    # a constant full-length carrier never exceeds its own bin's median; the cross-bin floor finds it
    assert _same(lib, _wf(24, 9, [(4, 0, 24, HIGH)]), 8, 6.0, 10) == [(0, 4)]
    # even and odd counts, in time and across bins (even: the f32 mean of the two middle values)
    rng = np.random.default_rng(11)
    for num_syms in (23, 24):
        for num_bins in (8, 9):
            wf = _wf(num_syms, num_bins, [(3, 4, 14, HIGH)], rng)  # under half the symbols: the median stays low
            assert _same(lib, wf, 8, 6.0, 10) == [(4, 3)]
    a = np.array([3.0, 1.0, 2.0, 10.0], np.float32)
    assert P.median_f32(a) == np.float32(2.5) and P.median_f32(a[:3]) == np.float32(2.0)
    # exactly half the symbols high: the even median is the mean of LOW and HIGH, which lies above the
    # cross-bin floor by more than the margin, so the global rule takes the bin's quiet half as well
    assert _same(lib, _wf(24, 5, [(2, 12, 24, HIGH)]), 8, 6.0, 10) == [(0, 2)]
    # one symbol fewer: the median is LOW again and the run is the burst alone
    assert _same(lib, _wf(24, 5, [(2, 13, 24, HIGH)]), 8, 6.0, 10) == [(13, 2)]


def test_search_order_of_equal_scores_and_max_cand(lib):
    """Equal scores are ordered by freq_bin, then time_sym (the reference's unstable sort
    leaves it open); max_cand keeps the best."""
    runs = [(5, 20, 30, HIGH), (1, 20, 30, HIGH), (1, 0, 10, HIGH), (3, 5, 15, HIGH + 2), (7, 8, 18, HIGH - 1)]
    wf = _wf(60, 9, runs)  # bin 1's two runs stay under half the symbols, so its median stays low
    assert _same(lib, wf, 8, 6.0, 10) == [(5, 3), (0, 1), (20, 1), (20, 5), (8, 7)]
    assert _same(lib, wf, 8, 6.0, 3) == [(5, 3), (0, 1), (20, 1)]
    assert _same(lib, wf, 8, 6.0, 1) == [(5, 3)]
    three = lib.psk31_find_carriers(np.stack([wf, _wf(60, 9, []), wf[:, ::-1].copy()]), 8, 6.0, 10)
    assert [len(c) for c in three] == [5, 0, 5] and int(three[2][0]["freq_bin"]) == 5
    with pytest.raises(ValueError):
        lib.psk31_find_carriers(wf, 8, 6.0, 0)
    with pytest.raises(ValueError):
        lib.psk31_find_carriers(wf.astype(np.float64), 8, 6.0, 4)
    with pytest.raises(ValueError):
        lib.psk31_find_carriers(wf[0], 8, 6.0, 4)
    with pytest.raises(ValueError):
        lib.psk31_sync(np.zeros(8192, np.complex64), 8000.0, 900.0, 1100.0, max_cand=0)
    with pytest.raises(ValueError):
        lib.psk31_sync(np.zeros((2, 8192), np.complex64), 8000.0, 900.0, 1100.0)
    with pytest.raises(ValueError):
        lib.psk31_decode(np.zeros(8192, np.float32), 8000.0, 900.0, 1100.0)
    assert lib.psk31_sync(np.zeros(100, np.complex64), 8000.0, 900.0, 1100.0) == []  # under one symbol: no device call
    cands = [{"carrier_hz": 1000.0, "score": 1.0}, {"carrier_hz": 1031.25, "score": 3.0}, {"carrier_hz": 1200.0, "score": 9.0}]
    assert lib.best_psk31_sync(cands, 1010.0)["score"] == 3.0 and lib.best_psk31_sync(cands, 1400.0) is None


@pytest.mark.parametrize("mode,base_hz,bin_,text", [(0, 900.0, 3, b"CQ CQ"), (1, 1400.0, 2, b"TEST")])
def test_sync_round_trip_on_the_host(lib, mode, base_hz, bin_, text):
    """roundtrip_psk31_sync_finds_bpsk31 and its QPSK31 twin (tests/roundtrip/psk31.rs) with no
    device: the restated waterfall (np_ref_sync.compute_waterfall), the library's host search
    and host demodulator as record_candidate starts it. fs 8000, the carrier on a bin, 64 / 32
    preamble / postamble bits, a 4 s buffer, (.., 4, 3.0, 256, 5): a candidate, the best within
    40 Hz; the search equals the restated search."""
    import np_ref_sync as S

    fs, sps = 8000.0, 256
    carrier = base_hz + bin_ * 31.25
    iq = _mod(lib, mode, fs, carrier, 1.0).modulate_text(text, 64, 32)
    buf = np.zeros(32000, np.complex64)
    buf[:min(len(iq), 32000)] = iq[:32000]  # the reference's test cuts the signal at the buffer's end too
    wf = np.asarray(S.compute_waterfall(buf, fs, base_hz, 31.25, sps, 32000 // sps, 8, 0), np.float32)
    found = _same(lib, wf, 4, 3.0, 5)
    assert found and abs(base_hz + found[0][1] * 31.25 - carrier) < 40.0
    if mode == P.BPSK:
        texts = []
        for t, b in found:
            soft, _ = lib.Bpsk31Demod(fs, base_hz + b * 31.25, 1.0).process_host(buf[t * sps:], 258)
            texts.append(lib._varicode_text(soft[:256] >= 0))
        assert text.decode() in texts


@pytest.mark.parametrize("mode", ["bpsk", "qpsk"])
def test_stream_text_is_the_restatement(lib, mode):
    """Psk31Stream on the host demodulator, fed in ragged pieces, against the restated stream:
    the QPSK31 gate (a silent lead-in is skipped), the printable-ASCII filter (a BEL is sent
    and dropped), fed_up_to / set_fed_up_to."""
    fs, carrier = 8000.0, 1000.0
    text = b"CQ \x07de TEST"
    iq = _mod(lib, P.BPSK if mode == "bpsk" else P.QPSK, fs, carrier, 1.0).modulate_text(text, 32, 40)
    iq = np.concatenate([np.zeros(3 * 256, np.complex64), iq])  # whole symbols: the stream has no timing recovery
    s, r = lib.Psk31Stream(mode, fs, carrier, 1.0, device=False), P.Psk31Stream(mode, fs, carrier, 1.0)
    got = want = ""
    for a in range(0, iq.size, 3001):
        got += s.feed(iq[a:a + 3001])
        want += r.feed(iq[a:a + 3001])
    got, want = got + s.flush(), want + r.flush()
    # the decoder pairs zeros up, so the lead-in's extra symbols can cost the first character
    # (in the reference as here); the rest of the text, without the BEL, must be there
    assert got == want and "Q de TEST" in got and "\x07" not in got
    assert s.feed(np.zeros(0, np.complex64)) == ""
    s.set_fed_up_to(123)
    assert s.fed_up_to == 123
    with pytest.raises(ValueError):
        lib.Psk31Stream("fsk", fs, carrier)


# ---- argument errors ----------------------------------------------------------------------
def test_argument_errors(lib):
    with pytest.raises(ValueError):
        lib.conv_encode(np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        lib.conv_encode(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        lib.conv_encode([0, 1])
    with pytest.raises(ValueError):
        lib.viterbi_decode(np.zeros(4, np.float64))
    with pytest.raises(ValueError):
        lib.viterbi_decode(np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        lib.viterbi_decode(np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        lib.viterbi_decode_hard(np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        lib.psk31_viterbi_batch(np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        lib.psk31_viterbi_batch(np.zeros((2, 7), np.float32))
    with pytest.raises(ValueError):
        lib.psk31_viterbi_batch(np.zeros((2, 8), np.complex64))
    with pytest.raises(ValueError):
        lib.StreamingViterbi().feed(np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        lib.VaricodeDecoder().push_bits(np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        lib.VaricodeEncoder().push_byte(256)
    with pytest.raises(ValueError):
        lib.VaricodeEncoder().push_preamble(-1)
    with pytest.raises(ValueError):
        lib.VaricodeEncoder().push_preamble((1 << 30) + 1)
    with pytest.raises(ValueError):
        lib.varicode_encode(-1)
    for bad in (np.zeros(4, np.float32), np.zeros((2, 4), np.complex64), np.zeros(4, np.complex128), [1j]):
        with pytest.raises(ValueError):
            lib.Bpsk31Demod(8000.0, 0.0).process_host(bad)
        with pytest.raises(ValueError):
            lib.Qpsk31Demod(8000.0, 0.0).process(bad)
    with pytest.raises(ValueError):
        lib.Bpsk31Mod(8000.0, 0.0).modulate_bits(np.zeros(4, np.int8))
    with pytest.raises(ValueError):
        lib.Bpsk31Mod(10.0, 0.0)  # round(10 / 31.25) = 0 samples per symbol
    with pytest.raises(ValueError):
        lib.Qpsk31Demod(float("nan"), 0.0)
    with pytest.raises(ValueError):
        lib.Bpsk31Decider().process(np.zeros(3, np.float64))
    rec = np.zeros(2, lib.PSK31_STREAM_DTYPE)
    assert lib.PSK31_STREAM_DTYPE.itemsize == 32 and lib.PSK31_REPORT_DTYPE.itemsize == 16
    rec["out_cap"] = 8
    for field, value in (("channel", 1), ("mode", 2), ("out_cap", (1 << 30) + 1)):
        bad = rec.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            lib.Psk31DemodBank(8000.0, bad, 1)
    with pytest.raises(ValueError):
        lib.Psk31DemodBank(8000.0, rec, 0)
    with pytest.raises(ValueError):
        lib.Psk31DemodBank(8000.0, rec[:0], 1)
    with pytest.raises(ValueError):
        lib.Psk31DemodBank(8000.0, np.zeros(2, np.float32), 1)
    bank = lib.Psk31DemodBank(8000.0, rec, 1)  # no device is touched until a process call
    with pytest.raises(ValueError):
        bank.process(np.zeros(16, np.complex64))
    with pytest.raises(ValueError):
        bank.process(np.zeros((1, 16), np.float32))
    with pytest.raises(ValueError):
        bank.process(np.zeros((2, 16), np.complex64))  # not the bank's nch
    with pytest.raises(ValueError):
        bank.set_gain(2, 1.0)
    # an empty batch reaches no device
    assert lib.psk31_viterbi_batch(np.zeros((0, 8), np.float32)).shape == (0, 4)
    assert lib.psk31_viterbi_batch(np.zeros((3, 0), np.float32)).shape == (3, 0)


def test_c_abi_limits_and_nulls(lib):
    L = ctypes.CDLL(lib.lib_path())
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    L.orion_psk31_viterbi_work_bytes.restype = sz
    L.orion_psk31_viterbi_work_bytes.argtypes = [sz, sz]
    assert L.orion_psk31_viterbi_work_bytes(1, 1) == 16 and L.orion_psk31_viterbi_work_bytes(5, 300) == 8 * 300 * 4
    assert L.orion_psk31_viterbi_work_bytes(0, 9) == 0 and L.orion_psk31_viterbi_work_bytes(1 << 31, 1) == 0
    L.orion_psk31_viterbi_device.argtypes = [vp, sz, sz, vp, vp, sz, vp]
    L.orion_psk31_viterbi.argtypes = [vp, sz, sz, vp]
    L.orion_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert L.orion_psk31_viterbi_device(None, 1, 1, None, None, 0, None) == -1
    assert L.orion_psk31_viterbi_device(p, 1 << 31, 1, p, p, 64, None) == -3 and b"2^31" in L.orion_last_error()
    assert L.orion_psk31_viterbi_device(p, 2, 2, p, p, 31, None) == -3 and b"work" in L.orion_last_error()  # needs 32
    assert L.orion_psk31_viterbi_device(p, 1, 1, p, p + 2, 64, None) == -3 and b"aligned" in L.orion_last_error()
    assert L.orion_psk31_viterbi(p, 1 << 31, 1, p) == -3
    assert L.orion_psk31_viterbi(None, 1, 1, None) == -1
    L.orion_varicode_encoder_drain.argtypes = [vp, vp, sz, vp]
    L.orion_varicode_encoder_new.restype = vp
    L.orion_varicode_encoder_push_byte.argtypes = [vp, ctypes.c_uint8]
    L.orion_varicode_encoder_free.argtypes = [vp]
    e = L.orion_varicode_encoder_new()
    n = sz(0)
    assert L.orion_varicode_encoder_push_byte(e, 65) == 0
    assert L.orion_varicode_encoder_drain(e, p, 3, ctypes.addressof(n)) == -3  # 'A' is 7 bits: nothing removed
    assert L.orion_varicode_encoder_drain(e, p, 7, ctypes.addressof(n)) == 0 and n.value == 7
    assert L.orion_varicode_encoder_drain(None, p, 7, ctypes.addressof(n)) == -1
    L.orion_varicode_encoder_free(e)


# ---- the host code under the sanitizers ---------------------------------------------------
def test_host_codec_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/psk31.cpp and tests/psk31_host/main.cpp, built with the host compiler alone and
    -fsanitize=address,undefined into a stand-alone binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "psk31_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src,
                    os.path.join(src, "psk31.cpp"), os.path.join(ROOT, "tests", "psk31_host", "main.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "psk31_host: ok" in out.stdout, out.stdout + out.stderr
