"""CPU: the frame layer at a known start on the host (orion_sdr.OfdmFrameMod.modulate_frame,
OfdmFrameDemod.decode, generate_ofdm_preamble, the MCS table and the frame fields of OfdmConfig)
against tests/np_ref_frame.py: the preamble and the frame's IQ bit for bit (complex64 as uint32)
over the default ladder's constellations, both reference concatenations and the DVB-style one,
window roll-off 0 and 2, gain != 1 and the preamble fallback; the reference's published frame
lengths; the window applied exactly once; decode's packet or RxError on clean, noisy, corrupted
and truncated input; the known-start cases of the reference's tests/roundtrip/ofdm_frame.rs as
properties; a noisy set that holds all three kinds of frame; goldens with IQ."""
import os

import numpy as np
import pytest

import np_ref_frame as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_layer_golden.npz")
Z32, ZC = np.zeros(0, np.int32), np.zeros(0, np.complex64)


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def table(lib, triples):
    return lib.McsTable([lib.Mcs(c, i, o) for c, i, o in triples])


def links(lib, gain=1.0, roll_off=0, mcs=None, preamble=(2, 32), training=True, n_fft=64, cp_len=8, data=None, **frame):
    """The same link for the library (cfg, table, OfdmPreamble) and the restatement; the plan is
    64 / 8 with 62 data carriers unless n_fft, cp_len and data (carrier indices) say otherwise."""
    data = R.DATA62 if data is None else np.asarray(data, np.int32)
    cfg = lib.OfdmConfig(n_fft, cp_len, data, Z32, ZC, 1e6, 0.0, gain, "qpsk")
    if roll_off:
        cfg = cfg.with_symbol_window(roll_off)
    for k in ("outer_interleaver", "inner_interleaver"):
        if frame.get(k):
            cfg = cfg.with_interleaver(k.split("_")[0], *frame[k])
    if "payload_crc" in frame:
        cfg = cfg.with_payload_crc(frame["payload_crc"])
    if "header_crc" in frame:
        cfg = cfg.with_header_crc(frame["header_crc"])
    sc = frame.get("scrambler")
    if sc == "dvbt":
        cfg = cfg.with_dvbt_energy_dispersal()
    elif sc:
        cfg = cfg.with_scrambler(sc[1], sc[2], 1 if sc[3] == "per_frame" else sc[3], sc[3] == "per_frame",
                                 frame.get("scrambler_pos", "before_outer"))
    if "ldpc_decode_rule" in frame:
        r = frame["ldpc_decode_rule"]
        cfg = cfg.with_ldpc_decode_rule(*(r if isinstance(r, tuple) else (r,)))
    link = R.Link(n_fft, cp_len, data, gain=gain, roll_off=roll_off, mcs=mcs, preamble=preamble, training=training, **frame)
    pre = lib.OfdmPreamble(*preamble)
    if training:
        pre = pre.with_training_symbol(n_fft, cp_len)
    return cfg, table(lib, link.mcs), pre, link


def same32(a, b):
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def decoded(lib, demod, iq):
    try:
        p = demod.decode(np.ascontiguousarray(iq))
        return p.metadata.mcs_index, p.metadata.sequence_num, p.metadata.flags, p.payload
    except lib.RxError as e:
        return e.code


def same_result(got, want):
    if isinstance(want, int) or isinstance(got, int):
        assert got == want
    else:
        assert got[:3] == want[:3] and np.array_equal(got[3], want[3])


GRID = [
    dict(), dict(roll_off=2), dict(gain=0.5), dict(gain=1.75, roll_off=2), dict(preamble=(3, 24)), dict(preamble=(2, 16), roll_off=2),
    dict(training=False, roll_off=2), dict(mcs=R.CONV_RS_TABLE), dict(mcs=R.CONV_RS_TABLE, roll_off=2),
    dict(mcs=R.DVB_TABLE, **R.DVB_FRAME), dict(mcs=R.DVB_TABLE, roll_off=2, **R.DVB_FRAME),
    dict(scrambler=("additive", 0b1001, 7, "per_frame"), scrambler_pos="after_inner"),
    dict(scrambler=("additive", 0b11, 15, 0x2B), payload_crc="crc16", header_crc="crc32"),
    dict(mcs=[("qpsk", ("conv", "1/2", "dvb_k7"), ("rs", 60, 8))], scrambler=("additive", 0x80200003, 32, "per_frame"),
         scrambler_pos="after_inner", inner_interleaver=("block", 7, 9)),
    dict(ldpc_decode_rule="min_sum"), dict(payload_crc="none", header_crc="none"),
]


# ---- preamble ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(gain=0.5), dict(preamble=(3, 24)), dict(preamble=(4, 16)),
                                dict(training=False), dict(preamble=(0, 32))], ids=str)
def test_preamble_against_the_restatement(lib, kw):
    cfg, _, pre, link = links(lib, **kw)
    tr = pre.training or (None, None)
    got = lib.generate_ofdm_preamble(cfg, pre.num_repeats, pre.repeat_len, tr[0], tr[1])
    assert got.dtype == np.complex64 and got.size == pre.total_len and same32(got, R.preamble(link))
    n, rl = pre.num_repeats, pre.repeat_len
    for k in range(1, n):  # the repeats are exact copies
        assert same32(got[:rl], got[k * rl:(k + 1) * rl])
    if rl and 64 % rl == 0 and n:  # band-limited and boosted: twice a data symbol's RMS, times the gain
        rms = float(np.sqrt(np.mean(np.abs(got[:rl].astype(np.complex128)) ** 2)))
        assert abs(rms - 2 * np.sqrt(62) / 64 * kw.get("gain", 1.0)) < 1e-5
    elif n:  # the wideband fallback: unit magnitude
        assert np.allclose(np.abs(got[:rl]), kw.get("gain", 1.0), atol=1e-6)
    if pre.training:  # the training symbol loads the occupied bins alone, and carries its prefix
        t = got[n * rl:]
        assert same32(t[:8], t[-8:])
        f = np.fft.fft(t[8:].astype(np.complex128))
        assert np.max(np.abs(f[[0, 32]])) < 1e-5 and np.min(np.abs(f[1:32])) > 0.9 * kw.get("gain", 1.0)


# ---- modulate_frame ------------------------------------------------------------------------
def test_published_frame_lengths(lib):
    cfg, t, pre, _ = links(lib)
    m = lib.OfdmFrameMod(cfg, t, pre)
    assert m.header_plan.coded_bits == 512 and m.header_symbols == 9
    assert m.frame_len(1, 96) == 2584 == m.modulate_frame(lib.FramePacket(lib.FrameMetadata(0, 1), R.payload(96, 0))).size
    cfg, t, pre, _ = links(lib, mcs=R.CONV_RS_TABLE)
    m = lib.OfdmFrameMod(cfg, t, pre)
    assert m.frame_len(0, 96) == 1936 == m.modulate_frame(lib.FramePacket(lib.FrameMetadata(0, 0), R.payload(96, 0))).size


@pytest.mark.parametrize("idx", range(len(GRID)))
def test_modulate_and_decode_against_the_restatement(lib, idx):
    cfg, t, pre, link = links(lib, **GRID[idx])
    mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
    lead = pre.total_len
    for mi in range(len(t)):
        for n, seq, flags, seed in ((96, 7, 0, 0x12345678), (37, 0xFFFFFFFF, 255, 0)):
            data = R.payload(n, 16 * idx + mi)
            got = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(seq, mi, flags), data), seed)
            want = R.modulate_frame(link, mi, seq, flags, data, seed)
            assert got.size == mod.frame_len(mi, n) and same32(got, want), (mi, n)
            body = want[lead:]
            same_result(decoded(lib, dem, body), R.decode_frame(link, body))
            # the round trip (roundtrip_frame_noiseless_*); a taper without an RX window back-off reaches
            # into the transform's window, so it is asserted where there is none
            if GRID[idx].get("gain", 1.0) == 1.0 and not GRID[idx].get("roll_off"):
                p = dem.decode(np.ascontiguousarray(body))
                assert (p.metadata.mcs_index, p.metadata.sequence_num, p.metadata.flags) == (mi, seq, flags)
                assert np.array_equal(p.payload, data)
            noisy = R.awgn(body, 0.05 if mi < 2 else 0.02, idx)
            same_result(decoded(lib, dem, noisy), R.decode_frame(link, noisy))


@pytest.mark.parametrize("geometry", ["128_9", "256_16"])
def test_known_start_path_at_other_geometries(lib, geometry):
    """128 / 9 with 66 carriers (odd samples per symbol) and 256 / 16 with 200: the header's and
    the payload's symbol counts, the padding of the last symbol, the preamble and the frame's IQ
    bit for bit, decode clean and noisy, window roll-off 0 and 2."""
    import np_ref_acquire as A

    geo, frames = A.GEOMETRIES[geometry]
    for roll_off in (0, 2):
        cfg, t, pre, link = links(lib, roll_off=roll_off, **geo)
        mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
        n_data, sps = len(geo["data"]), geo["n_fft"] + geo["cp_len"]
        assert (mod.n_data, mod.sps, mod.header_symbols) == (n_data, sps, -(-512 // n_data)) and pre.total_len == geo["n_fft"] + sps
        for k, (mi, nbytes, nsym) in enumerate(frames):
            data = R.payload(nbytes, 70 + k)
            got = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(k, mi, k % 5), data), k)
            assert got.size == mod.frame_len(mi, nbytes) == pre.total_len + (mod.header_symbols + nsym) * sps
            assert same32(got, R.modulate_frame(link, mi, k, k % 5, data, k)), (mi, nbytes)
            body = got[pre.total_len:]
            if not roll_off:
                p = dem.decode(np.ascontiguousarray(body))
                assert (p.metadata.mcs_index, p.metadata.sequence_num, p.metadata.flags) == (mi, k, k % 5)
                assert np.array_equal(p.payload, data)
            for rx in (body, R.awgn(body, 0.05 if mi < 2 else 0.02, k), body[:-1]):
                same_result(decoded(lib, dem, rx), R.decode_frame(link, rx))


def test_every_symbol_is_windowed_exactly_once(lib):
    cfg, t, pre, _ = links(lib)
    cfgw = cfg.with_symbol_window(2)
    f = lib.FramePacket(lib.FrameMetadata(3, 2), R.payload(96, 3))
    plain, tapered = lib.OfdmFrameMod(cfg, t, pre).modulate_frame(f), lib.OfdmFrameMod(cfgw, t, pre).modulate_frame(f)
    assert same32(plain[:64], tapered[:64])  # the raw repeats are never tapered
    ramp = lib.ofdm_tables(symbol_len=72, roll_off=2)[4]
    w = np.ones(72, np.float32)
    w[:2], w[-2:] = ramp, ramp[::-1]
    sym = plain[64:].reshape(-1, 72)
    want = np.empty_like(sym)
    want.real, want.imag = sym.real * w, sym.imag * w
    assert same32(tapered[64:], want.reshape(-1))  # training, header and payload symbols: one multiply each
    # OfdmMod tapers by itself under this configuration; the frame modulator's symbol streams do not, so once
    own = lib.OfdmMod(cfgw.symbol_config("qam16")).modulate_host(np.zeros(248, np.uint8))
    assert same32(own, lib.OfdmMod(cfg.symbol_config("qam16")).modulate_host(np.zeros(248, np.uint8)))


# ---- decode: the error mapping -------------------------------------------------------------
def test_rx_error_mapping(lib):
    cfg, t, pre, link = links(lib)
    mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
    data = R.payload(96, 1)
    body = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(5, 1, 9), data))[pre.total_len:]
    E = lib.RX_ERRORS
    assert decoded(lib, dem, body[:9 * 72 - 1]) == E["malformed_header"] == R.decode_frame(link, body[:9 * 72 - 1])
    assert decoded(lib, dem, body[:-1]) == E["malformed_header"] == R.decode_frame(link, body[:-1])  # the payload cut short
    bad = body.copy()
    bad[72:144] = -bad[72:144]  # a header symbol turned over
    bad[144:216] = 0
    assert decoded(lib, dem, bad) == E["header_crc_mismatch"] == R.decode_frame(link, bad)
    bad = body.copy()
    bad[9 * 72 + 72:9 * 72 + 6 * 72] = 0  # five payload symbols erased
    assert decoded(lib, dem, bad) == E["crc_mismatch"] == R.decode_frame(link, bad)
    # a frame modulated under a longer table than the receiver's
    longer = table(lib, link.mcs + [("qpsk", ("ldpc", "n512r12"), None)])
    far = lib.OfdmFrameMod(cfg, longer, pre).modulate_frame(lib.FramePacket(lib.FrameMetadata(5, 4), data))
    assert decoded(lib, dem, far[pre.total_len:]) == E["malformed_header"]
    # extra samples after the frame are not read; the payload comes back at its declared length
    p = dem.decode(np.concatenate([body, np.ones(100, np.complex64)]))
    assert p.payload.size == 96 and np.array_equal(p.payload, data) and p == lib.FramePacket(lib.FrameMetadata(5, 1, 9), data)
    e = lib.RxError("crc_mismatch")
    assert (e.code, e.kind, str(e)) == (4, "crc_mismatch", "crc_mismatch") and e == lib.RxError(4)


def test_header_is_decoded_under_sum_product_whatever_the_rule(lib):
    """Headers noisy enough that min-sum and sum-product part ways on some of them."""
    cfg, t, pre, link = links(lib, ldpc_decode_rule="min_sum")
    dem = lib.OfdmFrameDemod(cfg, t)
    mod = lib.OfdmFrameMod(cfg, t, pre)
    body = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(1, 0), R.payload(20, 1)))[pre.total_len:]
    hs = lib.FrameScheme(crc="crc16", inner=("ldpc", "n512r12"))
    differ = 0
    for k in range(40):
        rx = R.awgn(body, 0.105, 300 + k)
        same_result(decoded(lib, dem, rx), R.decode_frame(link, rx))
        llr = dem._llrs_host("bpsk", rx, 9)
        a, b = lib.decode_chain(llr, 14, hs, 0, "sum_product"), lib.decode_chain(llr, 14, hs, 0, "min_sum")
        differ += a.is_valid() != b.is_valid()
        if a.is_valid() != b.is_valid():  # the header's verdict is sum-product's
            assert (decoded(lib, dem, rx) != lib.RX_ERRORS["header_crc_mismatch"]) == a.is_valid()
    assert differ >= 1


def test_noisy_frame_set_holds_every_kind(lib):
    """A condition on the inputs the GPU tests decode too, under the host decoder alone."""
    cfg, t, pre, link = links(lib)
    dem = lib.OfdmFrameDemod(cfg, t)
    sent, rx = R.noisy_frame_set()
    sch = dem.scheme(t.get(1))
    kinds = set()
    for k in range(len(rx)):
        got = decoded(lib, dem, rx[k])
        same_result(got, R.decode_frame(link, rx[k]))
        o = lib.decode_chain(dem._llrs_host("qpsk", rx[k][9 * 72:], 25), 96, sch)
        kinds.add("fails" if not o.crc_ok else "marginal" if not o.inner_ok else "clean")
        assert isinstance(got, int) == (not o.crc_ok)
        if o.crc_ok:
            assert got[:3] == (1, k, k % 7) and np.array_equal(got[3], sent[k])
        else:
            assert got == lib.RX_ERRORS["crc_mismatch"]
    assert kinds == {"fails", "marginal", "clean"}


# ---- configuration -------------------------------------------------------------------------
def test_frame_fields_defaults_and_checks(lib):
    cfg, t, pre, _ = links(lib)
    f = cfg.frame_fields
    assert (f["payload_crc"], f["header_crc"], f["header_format"], f["scrambler"], f["ldpc_decode_rule"], f["tx_lowpass"]) == \
        ("crc32", "crc16", "orion_sdr", None, "sum_product", None)
    c2 = cfg.with_scrambler(0b1001, 7, per_frame_random=True).with_symbol_window(2).with_rx_window_backoff(1)
    assert c2.frame_fields["scrambler"] == ("additive", 0b1001, 7, "per_frame") and c2.window_roll_off == 2  # builders keep each other
    assert c2.num_data_carriers == cfg.num_data_carriers and c2.samples_per_ofdm_symbol == 72
    for bad in (lambda: cfg.with_interleaver("inner", "block", 0, 4), lambda: cfg.with_interleaver("outer", "forney", 12, 0),
                lambda: cfg.with_header_format("none"), lambda: cfg.with_header_format("dvb_tps"),
                lambda: cfg.with_payload_crc("crc8"), lambda: cfg.with_scrambler(0b1001, 1),
                lambda: cfg.with_ldpc_decode_rule("best"), lambda: lib.Mcs("qpsk", None, ("bch", 0)),
                lambda: lib.OfdmFrameMod(lib.OfdmConfig(64, 8, R.DATA62, Z32, ZC, 1e6, 1e3, 1.0, "qpsk"), t, pre),
                lambda: lib.OfdmFrameMod(cfg, lib.McsTable(), pre),
                lambda: lib.OfdmFrameMod(cfg, t, pre).modulate_frame(lib.FramePacket(lib.FrameMetadata(0, 9), R.payload(4, 0)))):
        with pytest.raises(ValueError):
            bad()
    lad = lib.McsTable.default_ladder()  # mcs_table_lookup, mcs_custom_table
    assert len(lad) == 4 and lad.get(0).constellation == "bpsk" and lad.get(3).constellation == "qam64" and lad.get(99) is None
    assert lad.add("qpsk", ("ldpc", "n512r12")) == 4 and lad.get(4).outer is None


def test_goldens(lib):
    g = np.load(GOLDEN)
    for name, kw in (("ldpc_bch", dict(roll_off=2)), ("conv_rs", dict(mcs=R.CONV_RS_TABLE))):
        cfg, t, pre, link = links(lib, **kw)
        mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
        for k, data in enumerate(g[name + "_bytes"]):
            mi = min(1, len(t) - 1)
            iq = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(k, mi), data), k)
            assert same32(iq, g[name + "_iq"][k]) and same32(iq, R.modulate_frame(link, mi, k, 0, data, k))
            assert np.array_equal(dem.decode(np.ascontiguousarray(iq[pre.total_len:])).payload, data)
