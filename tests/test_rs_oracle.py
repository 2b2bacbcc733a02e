"""CPU: the library's host side of the outer code (csrc/rs.cpp through the C ABI and the
orion_sdr classes) against tests/np_ref_rs.py, byte for byte: GF(2^8), the Reed-Solomon
encoder and counted decoder on every path the decoder has, the Forney interleaver as a
streaming block and in frame mode, the PN scrambler, DVB-T energy dispersal and the
transport-stream layer; the reference's own properties (tests/unit/fec.rs:178-400, 807-940;
tests/unit/dvb_t_ts.rs); the argument errors of every entry, the device entries' before any
launch; and the host code under the sanitizers as a stand-alone program."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_rs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


@pytest.fixture(scope="module")
def decoded():
    """Every row's input set through the restatement, once: row -> (sent, words, msgs, counts, paths)."""
    out = {}
    for row in R.ROWS:
        sent, words = R.make_words(*row, R.words_per_row(row[0]), R.SEED)
        res = [R.rs_decode(row[0], row[1], w) for w in words]
        out[row] = (sent, words, np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res], np.int32),
                    [r[2] for r in res])
    return out


# ---- GF(2^8) --------------------------------------------------------------------------------
def test_gf_tables_and_arithmetic(lib):
    e, lg = lib.Gf256.tables()
    assert np.array_equal(e, R.EXP.astype(np.uint8)) and np.array_equal(lg[1:], R.LOG[1:].astype(np.uint8))
    G = lib.Gf256
    rng = np.random.default_rng(7)
    pairs = [(0, 0), (0, 5), (5, 0), (1, 1), (255, 255), (2, 128)] + [tuple(rng.integers(0, 256, 2)) for _ in range(200)]
    for a, b in pairs:
        a, b = int(a), int(b)
        assert G.mul(a, b) == R.gf_mul(a, b) and G.add(a, b) == a ^ b
        if b:
            assert G.div(a, b) == R.gf_div(a, b) and G.mul(G.div(a, b), b) == a
    for a in range(1, 256):
        assert G.inv(a) == R.gf_inv(a) and G.mul(a, G.inv(a)) == 1
    for a, n in [(0, 0), (0, 3), (2, 8), (2, 255), (7, 254), (200, 1000), (3, 255 * 4 + 1)]:
        assert G.pow(a, n) == R.gf_pow(a, n)
    assert [G.exp_of(i) for i in (0, 1, 8, 254, 255, 256)] == [1, 2, 29, R.gf_exp_of(254), 1, 2]


# ---- the Reed-Solomon code ------------------------------------------------------------------
def test_dvb_generator_and_parity_known_answers(lib):
    rs = lib.ReedSolomon.dvb()
    assert (rs.n, rs.k, rs.t, rs.parity_bytes) == (204, 188, 8, 16)
    assert list(rs.generator()) == [59, 36, 50, 98, 229, 41, 65, 163, 8, 30, 209, 68, 189, 104, 13, 59, 1]
    cw = rs.encode(np.arange(188, dtype=np.uint8))
    assert list(cw[188:192]) == [49, 29, 120, 214] and np.array_equal(cw[:188], np.arange(188, dtype=np.uint8))


@pytest.mark.parametrize("n,n_parity", sorted({(r[0], r[1]) for r in R.ROWS}) + [(255, 254), (5, 1)])
def test_encode_matches_restatement(lib, n, n_parity):
    rng = np.random.default_rng([3, n, n_parity])
    msgs = rng.integers(0, 256, (5, n - n_parity), dtype=np.uint8)
    rs = lib.ReedSolomon(n, n_parity)
    assert list(rs.generator()) == R.rs_generator(n_parity)
    got = rs.encode(msgs)
    for m, g in zip(msgs, got):
        assert np.array_equal(g, R.rs_encode(n, n_parity, m))
    assert np.array_equal(rs.encode(msgs[0]), got[0])


@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: f"rs{r[0]}_{r[1]}_e{r[2]}")
def test_decode_counted_matches_restatement(lib, decoded, row):
    sent, words, msgs, counts, paths = decoded[row]
    got_m, got_c = lib.ReedSolomon(row[0], row[1]).decode_counted(words)
    assert np.array_equal(got_c, counts), (np.flatnonzero(got_c != counts)[:5], paths)
    assert np.array_equal(got_m, msgs)
    k = row[0] - row[1]
    assert np.array_equal(got_m[counts < 0], words[counts < 0][:, :k])  # a failure hands back received[:k]


def test_input_set_reaches_every_decoder_path(decoded):
    """From the restatement alone: the words above take every path of the decoder, and at least
    one corrected word is a miscorrection."""
    seen = collections.Counter()
    miscorrected = 0
    for row, (sent, words, msgs, counts, paths) in decoded.items():
        seen.update(paths)
        miscorrected += sum(1 for i, p in enumerate(paths) if p == "fixed" and not np.array_equal(msgs[i], sent[i]))
    for path in ("zero", "fixed", "roots", "degt", "resid_outside", "resid"):
        assert seen[path] > 0, (path, dict(seen))
    assert miscorrected > 0
    assert "degt" in decoded[(12, 4, 4)][4]  # the locator grows past t inside Berlekamp-Massey
    # the placements asked for: position 0, position n - 1, parity only
    sent, words, msgs, counts, paths = decoded[(204, 16, 8)]
    clean = np.array([R.rs_encode(204, 16, m) for m in sent[:3]])
    diff = words[:3] != clean
    assert diff[0, 0] and diff[1, 203] and not diff[2, :188].any() and diff[2].sum() == 8
    assert counts[2] == 8  # parity bytes count


def test_counted_equals_plain_decode_and_failure_reports(lib):
    rs = lib.ReedSolomon.dvb()
    rng = np.random.default_rng(11)
    msg = rng.integers(0, 256, 188, dtype=np.uint8)
    cw = rs.encode(msg)
    assert rs.decode_counted(cw)[1] == 0 and np.array_equal(rs.decode(cw), msg)
    r = cw.copy()
    r[[3, 50, 190, 203]] ^= np.array([1, 0x80, 0xFF, 7], np.uint8)
    m, c = rs.decode_counted(r)
    assert c == 4 and np.array_equal(m, msg) and np.array_equal(rs.decode(r), msg)
    r = cw.copy()
    r[:9] ^= 0x55
    m, c = rs.decode_counted(r)
    assert c == -1 and np.array_equal(m, r[:188])
    with pytest.raises(lib.RsUncorrectable) as ei:
        rs.decode(r)
    assert np.array_equal(ei.value.message, r[:188])


# ---- the Forney interleaver -----------------------------------------------------------------
@pytest.mark.parametrize("I,M", [(12, 17), (3, 2), (4, 1), (1, 5)])
def test_forney_stream_matches_restatement_chunked_and_reset(lib, I, M):
    rng = np.random.default_rng([5, I, M])
    data = rng.integers(0, 256, 3 * I * I * M + 7, dtype=np.uint8)
    for cls, ref_cls in ((lib.ConvInterleaver, R.ConvInterleaver), (lib.ConvDeinterleaver, R.ConvDeinterleaver)):
        a, ref = cls(I, M), ref_cls(I, M)
        assert a.roundtrip_delay == ref.roundtrip_delay == I * (I - 1) * M
        whole = a.feed(data)
        assert np.array_equal(whole, ref.feed(data))
        assert np.array_equal(a.flush(), ref.flush())
        a.reset()  # reset restarts; chunked feed equals one-shot feed
        cuts = [0, 1, 5, 5, 64, data.size]
        parts = [a.feed(data[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("I,M,n", [(12, 17, 204), (12, 17, 612), (12, 17, 100), (3, 2, 36), (3, 2, 1), (4, 1, 10),
                                   (1, 5, 9), (5, 3, 77)])
def test_forney_frame_mode_round_trip_and_closed_forms(lib, I, M, n):
    rng = np.random.default_rng([6, I, M, n])
    data = rng.integers(1, 256, n, dtype=np.uint8)
    D = I * (I - 1) * M
    padded = -(-n // I) * I
    il = lib.forney_frame_interleave(data, I, M)
    assert il.size == padded + D and np.array_equal(il, R.frame_interleave(data, I, M))
    back = lib.forney_frame_deinterleave(il, I, M)
    assert np.array_equal(back, R.frame_deinterleave(il, I, M))
    assert np.array_equal(back[:n], data) and not back[n:].any() and back.size == padded
    # the index maps the kernels use
    i = np.arange(il.size)
    src = i - (i % I) * M * I
    pad = np.concatenate([data, np.zeros(padded - n, np.uint8)])
    assert np.array_equal(il, np.where((src >= 0) & (src < padded), pad[np.clip(src, 0, padded - 1)], 0))
    q = np.arange(padded)
    assert np.array_equal(il[D + q - (I - 1 - q % I) * M * I], pad)
    assert lib.forney_frame_deinterleave(il[:D], I, M).size == 0


# ---- scramblers -----------------------------------------------------------------------------
@pytest.mark.parametrize("taps,width,seed", [(0b1001, 7, 0x7F), (0x3, 15, 0x4A80), (0x80200003, 32, 0xDEADBEEF), (3, 2, 1)])
def test_pn_scrambler_matches_restatement_self_inverse_stream(lib, taps, width, seed):
    rng = np.random.default_rng([8, width])
    data = rng.integers(0, 256, 300, dtype=np.uint8)
    s = lib.PnScrambler(taps, width, seed)
    out = s.scramble(data)
    assert np.array_equal(out, R.pn_scramble(taps, width, seed, data))
    assert np.array_equal(s.scramble(out), data) and np.array_equal(s.scramble(data), out)
    st, ref = s.into_stream(), R.PnStream(taps, width, seed)
    assert np.array_equal(st.feed(data), out) and np.array_equal(ref.feed(data), out)  # one feed equals one-shot
    assert np.array_equal(st.feed(data[:50]), ref.feed(data[:50]))  # the register is carried on
    st.reset()
    assert np.array_equal(np.concatenate([st.feed(data[:13]), st.feed(data[13:200]), st.feed(data[200:])]), out)


def test_dvbt_dispersal_known_answer_stream_and_advance(lib):
    d = lib.DvbTEnergyDispersal()
    z = np.zeros(40, np.uint8)
    seq = d.feed(z)
    assert list(seq[:3]) == [0x03, 0xF6, 0x08] and np.array_equal(seq, R.Dispersal().feed(z))
    d.reset()
    assert np.array_equal(np.concatenate([d.feed(z[:1]), d.feed(z[1:17]), d.feed(z[17:])]), seq)
    d.reset()
    d.advance_byte()
    assert np.array_equal(d.feed(z[:39]), seq[1:])
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, 64, dtype=np.uint8)
    d.reset()
    w = d.feed(data)
    d.reset()
    assert np.array_equal(d.feed(w), data) and np.array_equal(w, data ^ R.Dispersal().feed(np.zeros(64, np.uint8)))


# ---- the transport-stream layer -------------------------------------------------------------
@pytest.mark.parametrize("npk", [1, 7, 8, 9, 17])
def test_ts_energy_dispersal_matches_restatement_and_is_self_inverse(lib, npk):
    rng = np.random.default_rng([10, npk])
    ts = lib.ts_packetize(rng.integers(0, 256, npk * 187, dtype=np.uint8))
    assert ts.size == npk * 188
    d = lib.ts_energy_disperse(ts)
    assert np.array_equal(d, R.ts_energy_disperse(ts)) and np.array_equal(lib.ts_energy_disperse(d), ts)
    sync = d.reshape(-1, 188)[:, 0]
    assert all(sync[i] == (0xB8 if i % 8 == 0 else 0x47) for i in range(npk))
    assert np.array_equal(ts.reshape(-1, 188)[:, 0], np.full(npk, 0x47, np.uint8))


def test_ts_dispersal_mask_is_the_dispersal_of_zero_packets(lib):
    L = ctypes.CDLL(lib.lib_path())
    mask = np.zeros(1504, np.uint8)
    assert L.orion_rs_ts_dispersal_mask(ctypes.c_void_p(mask.ctypes.data)) == 0
    assert np.array_equal(mask, lib.ts_energy_disperse(np.zeros(1504, np.uint8)))
    assert np.array_equal(mask, R.ts_energy_disperse(np.zeros(1504, np.uint8)))


@pytest.mark.parametrize("n", [0, 1, 186, 187, 188, 400])
def test_ts_packetize_depacketize_null_and_stuffing(lib, n):
    rng = np.random.default_rng([12, n])
    payload = rng.integers(0, 256, n, dtype=np.uint8)
    ts = lib.ts_packetize(payload)
    assert np.array_equal(ts, R.ts_packetize(payload))
    dep = lib.ts_depacketize(ts)
    assert np.array_equal(dep, R.ts_depacketize(ts)) and np.array_equal(dep[:n], payload) and not dep[n:].any()
    assert lib.ts_depacketize(ts[:-1]) is None and lib.ts_depacketize(ts[:0]) is None
    null = lib.ts_null_packet()
    assert np.array_equal(null, R.ts_null_packet()) and list(null[:5]) == [0x47, 0x1F, 0xFF, 0x10, 0xFF]
    have = ts.size // 188
    for target in (0, have, have + 3):
        st = lib.ts_stuff_null_packets(ts, target)
        assert np.array_equal(st, R.ts_stuff_null_packets(ts, target)) and st.size == max(have, target) * 188


# ---- argument errors ------------------------------------------------------------------------
def test_argument_errors_of_the_host_entries(lib):
    L = ctypes.CDLL(lib.lib_path())
    sz, vp, i32, u32 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    E_NULL, E_ARG = -1, -3
    buf = np.zeros(4096, np.uint8)
    st = np.zeros(16, np.int32)
    p, q = vp(buf.ctypes.data), vp(st.ctypes.data)
    for name in ("orion_rs_forney_new", "orion_rs_pn_stream_new", "orion_rs_dispersal_new"):
        getattr(L, name).restype = vp
    for name in ("orion_rs_forney_delay", "orion_rs_forney_frame_len", "orion_rs_ts_packetized_len"):
        getattr(L, name).restype = sz
    assert L.orion_rs_gf_div(5, 0) == E_ARG and L.orion_rs_gf_inv(0) == E_ARG and L.orion_rs_gf_mul(256, 1) == E_ARG
    assert L.orion_rs_gf_tables(None, p) == E_NULL
    for n, npar in ((0, 0), (256, 16), (10, 10), (10, 11)):
        assert L.orion_rs_generator(sz(n), sz(npar), p) == E_ARG
        assert L.orion_rs_encode(sz(n), sz(npar), p, sz(1), p) == E_ARG
        assert L.orion_rs_decode_counted(sz(n), sz(npar), p, sz(1), p, q) == E_ARG
    assert L.orion_rs_generator(sz(10), sz(2), None) == E_NULL
    assert L.orion_rs_encode(sz(10), sz(0), p, sz(1), p) == E_ARG  # no parity: the reference's register is empty
    assert L.orion_rs_decode_counted(sz(10), sz(0), p, sz(1), p, q) == 0 and st[0] == 0  # and its decoder passes
    assert L.orion_rs_encode(sz(10), sz(2), None, sz(1), p) == E_NULL
    assert L.orion_rs_decode_counted(sz(10), sz(2), p, sz(1), p, None) == E_NULL
    assert L.orion_rs_forney_new(sz(0), sz(17), 0) is None and L.orion_rs_forney_new(sz(12), sz(0), 1) is None
    assert L.orion_rs_forney_new(sz(4097), sz(1), 0) is None
    assert L.orion_rs_forney_feed(None, p, sz(1), p) == E_NULL and L.orion_rs_forney_flush(None, p) == E_NULL
    assert L.orion_rs_forney_reset(None) == E_NULL
    assert L.orion_rs_forney_delay(sz(0), sz(1)) == 0 and L.orion_rs_forney_delay(sz(12), sz(17)) == 2244
    assert L.orion_rs_forney_frame_len(sz(12), sz(0), sz(5)) == 0 and L.orion_rs_forney_frame_len(sz(12), sz(17), sz(5)) == 2256
    assert L.orion_rs_forney_frame_interleave(sz(0), sz(1), p, sz(4), p) == E_ARG
    assert L.orion_rs_forney_frame_interleave(sz(3), sz(2), None, sz(4), p) == E_NULL
    assert L.orion_rs_forney_frame_deinterleave(sz(3), sz(0), p, sz(40), p) == E_ARG
    assert L.orion_rs_forney_frame_deinterleave(sz(3), sz(2), p, sz(40), None) == E_NULL
    for taps, width, seed in ((1, 1, 1), (1, 33, 1), (1, 7, 0), (1, 7, 0x80), (0x80, 7, 1)):
        assert L.orion_rs_pn_scramble(u32(taps), u32(width), u32(seed), p, sz(4)) == E_ARG
        assert L.orion_rs_pn_stream_new(u32(taps), u32(width), u32(seed)) is None
    assert L.orion_rs_pn_scramble(u32(9), u32(7), u32(1), None, sz(4)) == E_NULL
    assert L.orion_rs_pn_stream_feed(None, p, sz(1)) == E_NULL and L.orion_rs_pn_stream_reset(None) == E_NULL
    assert L.orion_rs_dispersal_feed(None, p, sz(1)) == E_NULL and L.orion_rs_dispersal_advance_byte(None) == E_NULL
    assert L.orion_rs_dispersal_reset(None) == E_NULL
    assert L.orion_rs_ts_energy_disperse(p, sz(187)) == E_ARG and L.orion_rs_ts_energy_disperse(None, sz(188)) == E_NULL
    assert L.orion_rs_ts_dispersal_mask(None) == E_NULL and L.orion_rs_ts_null_packet(None) == E_NULL
    assert L.orion_rs_ts_packetize(p, sz(10), None) == E_NULL
    assert L.orion_rs_ts_depacketize(p, sz(0), p) == E_ARG and L.orion_rs_ts_depacketize(p, sz(189), p) == E_ARG
    assert L.orion_rs_ts_stuff_null_packets(p, sz(100), sz(2), p) == E_ARG
    for bad in (lambda: lib.ReedSolomon(0, 0), lambda: lib.ReedSolomon(256, 2), lambda: lib.ReedSolomon(5, 5),
                lambda: lib.ReedSolomon(10, 2).encode(np.zeros(9, np.uint8)),
                lambda: lib.ReedSolomon(10, 2).decode_counted(np.zeros(11, np.uint8)),
                lambda: lib.ReedSolomon(10, 0).encode(np.zeros(10, np.uint8)),
                lambda: lib.ConvInterleaver(0, 1), lambda: lib.ConvDeinterleaver(1, 0),
                lambda: lib.ConvInterleaver(3, 2).feed(np.zeros(4, np.float32)),
                lambda: lib.forney_frame_interleave(np.zeros(4, np.uint8), 0, 2),
                lambda: lib.PnScrambler(1, 1, 1), lambda: lib.PnScramblerStream(1, 7, 0),
                lambda: lib.Gf256.div(1, 0), lambda: lib.Gf256.inv(0), lambda: lib.Gf256.mul(256, 0),
                lambda: lib.ts_energy_disperse(np.zeros(187, np.uint8)),
                lambda: lib.ts_stuff_null_packets(np.zeros(10, np.uint8), 1)):
        with pytest.raises(ValueError):
            bad()


def test_device_entries_refuse_bad_arguments_before_any_launch(lib):
    """No device is needed: every one of these returns before the first device call."""
    L = ctypes.CDLL(lib.lib_path())
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    E_NULL, E_ARG = -1, -3
    buf = np.zeros(4096, np.uint8)
    p = vp(buf.ctypes.data)
    L.orion_rs_decode_stream_len.restype = sz
    L.orion_rs_forney_interleave_len.restype = sz

    def dec(n, npar, ns, ncw, bits=0, I=0, M=0, derand=0, inp=p, msgs=p, status=p):
        return L.orion_rs_decode_batch_device(sz(n), sz(npar), inp, sz(ns), sz(ncw), bits, sz(I), sz(M), derand, msgs,
                                              status, None)

    assert dec(204, 0, 1, 1) == E_ARG and dec(204, 33, 1, 1) == E_ARG and dec(255, 34, 1, 1) == E_ARG
    assert dec(256, 16, 1, 1) == E_ARG and dec(0, 0, 1, 1) == E_ARG and dec(16, 16, 1, 1) == E_ARG
    assert dec(204, 16, 1, 0) == E_ARG and dec(204, 16, 1, (1 << 20) + 1) == E_ARG
    assert dec(204, 16, (1 << 24) + 1, 1) == E_ARG and dec(204, 16, 1 << 12, 1 << 19) == E_ARG
    assert dec(204, 16, 1, 1, I=12, M=0) == E_ARG and dec(204, 16, 1, 1, I=0, M=17) == E_ARG
    assert dec(204, 16, 1, 1, I=8, M=2) == E_ARG  # 204 is no multiple of 8 branches
    assert dec(12, 4, 1, 1, derand=1) == E_ARG  # k != 188
    assert dec(204, 16, 1, 1, inp=None) == E_NULL and dec(204, 16, 1, 1, status=None) == E_NULL
    assert dec(204, 16, 1, 1, status=vp(buf.ctypes.data + 1)) == E_ARG
    assert dec(204, 16, 0, 1, inp=None, msgs=None, status=None) == 0  # no streams: nothing to do
    assert L.orion_rs_decode_batch(sz(204), sz(40), p, sz(1), sz(1), 0, sz(0), sz(0), 0, p, p) == E_ARG
    assert L.orion_rs_decode_stream_len(sz(204), sz(16), sz(3), 1, sz(12), sz(17)) == (3 * 204 + 2244) * 8
    assert L.orion_rs_decode_stream_len(sz(204), sz(16), sz(3), 0, sz(8), sz(17)) == 0
    assert L.orion_rs_encode_batch_device(sz(204), sz(40), p, sz(1), sz(1), 0, p, None) == E_ARG
    assert L.orion_rs_encode_batch_device(sz(12), sz(4), p, sz(1), sz(1), 1, p, None) == E_ARG
    assert L.orion_rs_encode_batch_device(sz(204), sz(16), None, sz(1), sz(1), 0, p, None) == E_NULL
    assert L.orion_rs_encode_batch(sz(204), sz(16), p, sz(1), sz(0), 0, p) == E_ARG
    assert L.orion_rs_forney_interleave_batch_device(sz(0), sz(17), p, sz(1), sz(8), 0, p, None) == E_ARG
    assert L.orion_rs_forney_interleave_batch_device(sz(12), sz(17), p, sz(1), sz(0), 0, p, None) == E_ARG
    assert L.orion_rs_forney_interleave_batch_device(sz(12), sz(17), p, sz(1), sz((1 << 27) + 1), 0, p, None) == E_ARG
    assert L.orion_rs_forney_interleave_batch_device(sz(12), sz(17), p, sz(1), sz(8), 0, None, None) == E_NULL
    assert L.orion_rs_forney_interleave_batch(sz(12), sz(17), p, sz((1 << 24) + 1), sz(8), 0, p) == E_ARG
    assert L.orion_rs_forney_interleave_len(sz(12), sz(17), sz(100), 1) == (108 + 2244) * 8
    x = np.zeros((2, 204), np.uint8)
    for bad in (lambda: lib.rs_decode_batch(x, n_parity=33), lambda: lib.rs_decode_batch(x[:, :203]),
                lambda: lib.rs_decode_batch(x.astype(np.int32)), lambda: lib.rs_decode_batch(x, bits=True),
                lambda: lib.rs_decode_batch(x, deinterleave=(12, 17)),
                lambda: lib.rs_decode_batch(np.zeros((1, 12), np.uint8), n=12, n_parity=4, derandomize=True),
                lambda: lib.rs_encode_batch(x), lambda: lib.rs_encode_batch(x, n_parity=0),
                lambda: lib.rs_encode_batch(np.zeros((1, 8), np.uint8), n=12, n_parity=4, disperse=True),
                lambda: lib.forney_interleave_batch(x, 0, 17), lambda: lib.forney_interleave_batch(x[:, :0], 12, 17)):
        with pytest.raises(ValueError):
            bad()


# ---- the host code under the sanitizers -----------------------------------------------------
def test_host_rs_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/rs.cpp and tests/rs_host/main.cpp, built with the host compiler alone and
    -fsanitize=address,undefined into a stand-alone binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "rs_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src,
                    os.path.join(src, "rs.cpp"), os.path.join(ROOT, "tests", "rs_host", "main.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "rs_host: ok" in out.stdout, out.stdout + out.stderr
