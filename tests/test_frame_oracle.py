"""CPU: the library's host side of the frame layer's coding chain (csrc/frame.cpp through the C
ABI and orion_sdr) against tests/np_ref_frame.py, byte for byte: the CRCs (and against binascii
and zlib, which no one here wrote), the bit/byte and header helpers, the scrambler seed and its
three drivers, block_plan at the reference's published geometries, encode_chain and every
field of decode_chain's ChainOutcome over a grid of configurations, the reference's own unit
tests (tests/unit/ofdm_frame.rs:20-140), a noisy set that holds all three kinds of frame, and
the goldens under tests/golden/."""
import binascii
import os
import zlib

import numpy as np
import pytest

import np_ref_frame as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_golden.npz")


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def both(lib, **kw):
    return lib.FrameScheme(**kw), R.scheme(**kw)


def decoded(lib, *args):
    """decode_chain's ChainOutcome, or the code of the RxError it raised."""
    try:
        return lib.decode_chain(*args)
    except lib.RxError as e:
        return e.code


def same_outcome(got, want):
    if isinstance(want, int):
        assert got == want
        return
    assert np.array_equal(got.bytes, want["bytes"]) and np.array_equal(got.inner_out_bits, want["inner_out_bits"])
    for f in ("inner_ok", "outer_ok", "crc_ok", "crc_present", "outer_present", "outer_corrected_bytes"):
        assert getattr(got, f) == want[f], f
    assert got.is_valid() == want["valid"]


# ---- CRCs ----------------------------------------------------------------------------------
def test_crc_known_answers_and_outside_references(lib):
    assert lib.crc16(b"123456789") == 0x29B1 and lib.crc32(b"123456789") == 0xCBF43926
    assert R.crc16(b"123456789") == 0x29B1 and R.crc32(b"123456789") == 0xCBF43926
    rng = np.random.default_rng(7)
    for n in list(range(0, 301, 7)) + [1, 2, 3, 299, 300]:
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert lib.crc16(d) == binascii.crc_hqx(d.tobytes(), 0xFFFF) == R.crc16(d), n
        assert lib.crc32(d) == zlib.crc32(d.tobytes()) == R.crc32(d), n


def test_append_and_check_crc(lib):
    data = np.frombuffer(b"frame payload bytes", np.uint8)
    for crc, clen in (("none", 0), ("crc16", 2), ("crc32", 4)):  # crc_kind_lengths, append_and_check_crc_round_trip
        framed = lib.append_crc(crc, data)
        assert framed.size == data.size + clen and np.array_equal(framed, R.append_crc(crc, data))
        rec, ok = lib.check_and_strip_crc(crc, framed)
        assert np.array_equal(rec, data) and ok
        if clen:
            assert lib.check_and_strip_crc(crc, framed[:clen - 1]) is None
    for crc in ("crc16", "crc32"):  # crc_detects_corruption
        framed = lib.append_crc(crc, np.frombuffer(b"important", np.uint8))
        framed[0] ^= 1
        assert lib.check_and_strip_crc(crc, framed)[1] is False and R.check_and_strip_crc(crc, framed)[1] is False
    big = lib.append_crc("crc32", np.frombuffer(b"123456789", np.uint8))
    assert big[-4:].tolist() == [0xCB, 0xF4, 0x39, 0x26]  # big-endian
    assert lib.check_and_strip_crc("crc32", np.zeros(3, np.uint8)) is None
    with pytest.raises(ValueError):
        lib.append_crc("crc8", data)


# ---- helpers -------------------------------------------------------------------------------
def test_bytes_bits_round_trip(lib):
    b = np.array([0x00, 0xFF, 0xA5, 0x3C, 0x81], np.uint8)
    bits = lib.bytes_to_bits(b)
    assert bits.size == 40 and bits[16:24].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
    assert np.array_equal(lib.bits_to_bytes(bits), b)
    assert np.array_equal(lib.bits_to_bytes(bits | 0xFE), b)  # bit 0 of an element alone
    with pytest.raises(ValueError):
        lib.bits_to_bytes(bits[:-1])


def test_header_fields_pack_big_endian(lib):
    f = lib.pack_header_fields(0x07, 0x00010203, 0x04050607, 0x09, 0x0A0B0C0D)
    assert f.tolist() == [7, 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13] and lib.HEADER_FIELD_BYTES == 14
    assert np.array_equal(f, R.pack_header_fields(0x07, 0x00010203, 0x04050607, 0x09, 0x0A0B0C0D))
    assert lib.unpack_header_fields(f) == (0x07, 0x00010203, 0x04050607, 0x09, 0x0A0B0C0D)
    top = (255, 0xFFFFFFFF, 0xFFFFFFFF, 255, 0xFFFFFFFF)
    assert lib.unpack_header_fields(lib.pack_header_fields(*top)) == top
    with pytest.raises(ValueError):
        lib.pack_header_fields(256, 0, 0, 0, 0)


# ---- scramblers ----------------------------------------------------------------------------
def test_seed_reduction(lib):
    assert lib.scrambler_seed(7, 0) == 1 and lib.scrambler_seed(7, 0x80) == 1 and lib.scrambler_seed(7, 0xFF) == 0x7F
    assert lib.scrambler_seed(15, 0x18001) == 1 and lib.scrambler_seed(15, 0x8000) == 1
    assert lib.scrambler_seed(32, 0xFFFFFFFF) == 0xFFFFFFFF and lib.scrambler_seed(32, 0) == 1
    assert lib.scrambler_seed(40, 0x80000000) == 0x80000000  # width >= 32 takes the whole mask
    for taps, width in R.ADDITIVE:
        for raw in R.SEEDS:
            sch = R.scheme(scrambler=("additive", taps, width, "per_frame"))
            assert lib.scrambler_seed(width, raw) == R.build_scrambler(sch, raw)[2]


@pytest.mark.parametrize("taps,width", R.ADDITIVE)
def test_scramble_drivers(lib, taps, width):
    rng = np.random.default_rng(width)
    data = rng.integers(0, 256, 259, dtype=np.uint8)
    bits = rng.integers(0, 2, 1932, dtype=np.uint8)
    llr = rng.standard_normal(1932).astype(np.float32)
    llr[:8] = [np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, 1.0]
    for seed in (R.SEEDS[0], R.SEEDS[3], "per_frame"):
        for raw in ([0] if seed != "per_frame" else R.SEEDS):
            ls, rs = both(lib, scrambler=("additive", taps, width, seed))
            s3 = R.build_scrambler(rs, raw)
            sb = lib.scramble_bytes(ls, data, raw)
            assert np.array_equal(sb, R.scramble_bytes(rs, raw, data))
            assert np.array_equal(lib.scramble_bytes(ls, sb, raw), data)  # self-inverse
            got = lib.scramble_bits(ls, bits, raw)
            assert np.array_equal(got, R.scramble_bits(s3, bits))
            # packed MSB first, whitened LSB first: bit i meets PN step 8 (i // 8) + 7 - i % 8
            pn = np.unpackbits(R.scramble_bytes(rs, raw, np.zeros(242, np.uint8)), bitorder="little")
            i = np.arange(1932)
            assert np.array_equal(got ^ bits, pn[8 * (i // 8) + 7 - i % 8])
            fl = lib.apply_pn_to_llrs(ls, llr, raw)
            assert np.array_equal(fl.view(np.uint32), R.apply_pn_to_llrs(s3, llr).view(np.uint32))
            assert np.array_equal((fl.view(np.uint32) ^ llr.view(np.uint32)) >> 31, got ^ bits)
            assert np.array_equal((fl.view(np.uint32) ^ llr.view(np.uint32)) & 0x7FFFFFFF, np.zeros(1932, np.uint32))


def test_dispersal_and_none_drivers(lib):
    data = np.random.default_rng(3).integers(0, 256, 300, dtype=np.uint8)
    ls, rs = both(lib, scrambler="dvbt")
    assert np.array_equal(lib.scramble_bytes(ls, data), R.scramble_bytes(rs, 0, data))
    assert not np.array_equal(lib.scramble_bytes(ls, data), data)
    bits = data[:100] & 1
    assert np.array_equal(lib.scramble_bits(ls, bits), bits)  # byte-domain only
    none = lib.FrameScheme()
    assert np.array_equal(lib.scramble_bytes(none, data), data) and np.array_equal(lib.scramble_bits(none, bits), bits)


# ---- block_plan ----------------------------------------------------------------------------
def test_block_plan_published_geometries(lib):
    # n_fft 64, cp 8, 62 data carriers: the reference's two benchmark rows (docs/performance.md:253-269),
    # frames of 2584 and 1936 samples behind a 136-sample preamble and training symbol
    sps, carriers, lead = 72, 62, 136
    hdr = lib.block_plan(14, lib.FrameScheme(**R.HEADER))
    assert hdr.astuple() == (14, 16, 128, 128, 512, 512)
    n_hdr = lib.symbols_for_coded_bits(carriers, 1, hdr.coded_bits)
    assert n_hdr == 9
    p = lib.block_plan(96, lib.FrameScheme(**R.LDPC_BCH))
    assert p.astuple() == (96, 100, 1288, 1288, 3072, 3072)
    n = lib.symbols_for_coded_bits(carriers, 2, p.coded_bits)
    assert n == 25 and lead + (n_hdr + n) * sps == 2584
    p = lib.block_plan(96, lib.FrameScheme(**R.CONV_RS))
    assert p.astuple() == (96, 100, 960, 960, 1928, 1928)
    n = lib.symbols_for_coded_bits(carriers, 2, p.coded_bits)
    assert n == 16 and lead + (n_hdr + n) * sps == 1936
    p = lib.block_plan(96, lib.FrameScheme(outer=("rs", 60, 8), inner=("conv", "1/2", "dvb_k7")))
    assert p.coded_bits == 1932 and p.coded_bits % 8 != 0


def test_block_plan_reference_unit_tests(lib):
    p = lib.block_plan(10, lib.FrameScheme(crc="none"))  # block_plan_no_coding_is_bits
    assert p.framed_bytes == 10 and p.coded_bits == 80
    p = lib.block_plan(40, lib.FrameScheme(**R.LDPC_BCH))  # block_plan_ldpc_bch_fragments
    n_bch = -(-44 * 8 // lib.BCH_INFO_BITS)
    assert p.framed_bytes == 44 and p.outer_coded_bits >= 44 * 8 and p.outer_coded_bits % n_bch == 0
    assert p.coded_bits % 512 == 0


GRID = [
    dict(R.LDPC_BCH), dict(R.CONV_RS), dict(R.DVB), dict(R.HEADER),
    dict(crc="none"), dict(crc="crc16", inner=("ldpc", "n576r23")), dict(crc="none", **R.LDPC_BCH),
    dict(crc="crc16", **R.CONV_RS), dict(outer=("rs", 60, 8), inner=("conv", "1/2", "dvb_k7")),
    dict(inner=("ldpc", "n512r34"), inner_interleaver=("block", 16, 32), outer=("bch", 4)),
    dict(inner=("conv", "2/3", "k5"), inner_interleaver=("block", 7, 9)),
    dict(outer=("bch", 8), outer_interleaver=("block", 8, 23), inner=("ldpc", "n512r12")),
    dict(outer_interleaver=("block", 5, 7), inner_interleaver=("block", 3, 11)),
    dict(outer_interleaver=("forney", 4, 3), outer=("bch", 2)),
    dict(outer=("rs", 204, 16), outer_interleaver=("forney", 12, 17), inner=("conv", "7/8", "dvb_k7")),
] + [dict(R.LDPC_BCH, scrambler=("additive", t, w, sd), scrambler_pos=pos)
     for (t, w) in R.ADDITIVE for sd in (0, 0x2B, "per_frame") for pos in ("before_outer", "after_inner")
     ] + [dict(R.CONV_RS, scrambler=("additive", R.ADDITIVE[1][0], 15, "per_frame"), scrambler_pos="after_inner"),
          dict(outer=("rs", 60, 8), inner=("conv", "1/2", "dvb_k7"), scrambler=("additive", 0b1001, 7, "per_frame"),
               scrambler_pos="after_inner")]


@pytest.mark.parametrize("n", [0, 1, 14, 96, 259])
def test_block_plan_against_the_restatement(lib, n):
    for kw in GRID:
        ls, rs = both(lib, **kw)
        assert lib.block_plan(n, ls).astuple() == R.block_plan(n, rs), kw


# ---- the chain -----------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(GRID)))
def test_chain_against_the_restatement(lib, idx):
    kw = GRID[idx]
    ls, rs = both(lib, **kw)
    long = R.block_plan(96, rs)[5] > 10000  # the Forney(12,17) frames: one payload, two inputs (the restatement is slow)
    for n, seed in ((96, 0x12345678), (37, 0))[:1 if long else 2]:
        data = R.payload(n, idx)
        plan = R.block_plan(n, rs)
        oil, coded = lib.encode_chain_stages(data, ls, seed)
        w_oil, w_coded = R.encode_chain_stages(data, rs, seed)
        assert coded.size == plan[5] and np.array_equal(coded, w_coded) and np.array_equal(oil, w_oil)
        assert np.array_equal(lib.encode_chain(data, ls, seed), w_coded)
        # clean, then noisy enough that some decoders give up, then a row cut short
        for llr in (R.clean_llrs(coded), R.noisy_llrs(coded, 0.9, idx), R.clean_llrs(coded)[:plan[5] // 2],
                    np.concatenate([R.clean_llrs(coded), np.ones(33, np.float32)]))[:2 if long else 4]:
            got = decoded(lib, llr, n, ls, seed)
            same_outcome(got, R.decode_chain(llr, plan, rs, seed))
        got = lib.decode_chain(R.clean_llrs(coded), n, ls, seed)
        assert got.is_valid() and np.array_equal(got.bytes, data) and got.inner_ok and got.outer_ok and got.crc_ok
        assert got.crc_present == (kw.get("crc", "crc32") != "none") and got.outer_present == ("outer" in kw)
        if ls.per_frame_seed and n > 20:  # the wrong seed does not descramble
            bad = decoded(lib, R.clean_llrs(coded), n, ls, seed ^ 0x55)
            assert isinstance(bad, int) or not np.array_equal(bad.bytes, data)


def test_ldpc_rule_reaches_the_decoder(lib):
    ls, rs = both(lib, **R.LDPC_BCH)
    data = R.payload(96, 5)
    llr = R.noisy_llrs(lib.encode_chain(data, ls), 0.78, 11)
    plan = R.block_plan(96, rs)
    for rule in ("sum_product", "min_sum", ("scaled_min_sum", 0.75)):
        same_outcome(decoded(lib, llr, 96, ls, 0, rule), R.decode_chain(llr, plan, rs, 0, rule))


def test_valid_precedence(lib):
    # a CRC decides alone; without one the outer code; without either the inner decoder
    data = R.payload(40, 1)
    ls = lib.FrameScheme(crc="none", outer=("bch", 8))
    llr = R.clean_llrs(lib.encode_chain(data, ls))
    llr[:20] = -llr[:20]  # twenty errors in a word of t = 8
    got = lib.decode_chain(llr, 40, ls)
    assert got.crc_ok and not got.crc_present and not got.outer_ok and not got.is_valid()
    ls = lib.FrameScheme(crc="none", inner=("ldpc", "n512r12"))
    got = lib.decode_chain(R.noisy_llrs(lib.encode_chain(data, ls), 1.5, 2), 40, ls)
    assert not got.inner_ok and got.outer_ok and not got.outer_present and not got.is_valid()
    ls = lib.FrameScheme(**R.LDPC_BCH)
    coded = lib.encode_chain(data, ls)
    got = lib.decode_chain(R.noisy_llrs(coded, 0.8, 1018), 40, ls)
    assert got.is_valid() == got.crc_ok


def test_noisy_set_holds_every_kind(lib):
    # a condition on the inputs the GPU tests decode too (np_ref_frame.noisy_set), not a measurement
    ls = lib.FrameScheme(**R.LDPC_BCH)
    sent, llr = R.noisy_set()
    out = [lib.decode_chain(row, 96, ls) for row in llr]
    assert any(not o.crc_ok for o in out)
    assert any(o.crc_ok and not o.inner_ok for o in out)
    assert any(o.crc_ok and o.inner_ok and o.outer_ok for o in out)
    for o, d in zip(out, sent):
        assert o.crc_ok == np.array_equal(o.bytes, d)


def test_goldens(lib):
    g = np.load(GOLDEN)
    for name, kw in (("ldpc_bch", R.LDPC_BCH), ("conv_rs", R.CONV_RS), ("dvb", R.DVB)):
        ls, rs = both(lib, **kw)
        data, coded = g[name + "_bytes"], g[name + "_coded"]
        for k in range(len(data)):
            assert np.array_equal(np.unpackbits(coded[k])[:R.block_plan(96, rs)[5]], lib.encode_chain(data[k], ls, 0))
            assert np.array_equal(lib.encode_chain(data[k], ls), R.encode_chain(data[k], rs))


def test_argument_errors(lib):
    for kw in (dict(crc="crc8"), dict(outer=("bch", 0)), dict(outer=("rs", 300, 16)), dict(inner=("ldpc", "n1024")),
               dict(inner=("conv", "9/10")), dict(inner_interleaver=("block", 0, 4)),
               dict(outer_interleaver=("forney", 0, 17)), dict(scrambler=("additive", 0x48, 1, 1)),
               dict(scrambler=("additive", 0x100, 7, 1)), dict(scrambler_pos="middle"), dict(scrambler="fancy")):
        with pytest.raises(ValueError):
            lib.FrameScheme(**kw)
    with pytest.raises(ValueError):
        lib.block_plan(-1, lib.FrameScheme())
    with pytest.raises(ValueError):
        lib.block_plan(1 << 25, lib.FrameScheme())
    with pytest.raises(ValueError):
        lib.decode_chain(np.zeros(3072, np.float32), 96, lib.FrameScheme(**R.LDPC_BCH), 0, "best")
    with pytest.raises(ValueError):
        lib.encode_chain(np.zeros(4, np.uint8), "ldpc")
