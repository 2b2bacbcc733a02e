"""CPU: the library's host side of the inner code (csrc/fec.cpp through the C ABI:
orion_fec_punctured_coded_len, orion_fec_conv_encode, orion_fec_viterbi_host, the block
interleaver calls) against tests/np_ref_fec.py, byte for byte; the reference's own properties
(tests/unit/fec.rs:666-802); the argument errors of the entry points that reach no device;
and the host code under the sanitizers as a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_fec as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = ("k5", "dvb_k7")
INFO_BITS = (1, 2, 5, 33, 120, 188)


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


# ---- encode, coded length, decode against the restatement -----------------------------------
@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("rate", R.RATES)
def test_encode_and_length_match_the_restatement(lib, code, rate):
    for n in INFO_BITS:
        info, coded = R.frame(code, rate, n)
        got = lib.conv_encode_punctured(info, rate, code)
        assert got.dtype == np.uint8 and np.array_equal(got, coded), (code, rate, n)
        assert lib.punctured_coded_len(n, rate, code) == len(coded) == R.punctured_coded_len(code, n, rate)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("rate", R.RATES)
@pytest.mark.parametrize("kind", R.INPUT_KINDS)
def test_decode_matches_the_restatement(lib, code, rate, kind):
    for n in INFO_BITS:
        info, coded = R.frame(code, rate, n)
        llr = R.llr_input(kind, coded, seed=n)
        got = lib.viterbi_decode_soft(llr, n, rate, code)
        want = R.viterbi_decode_soft(code, llr, n, rate)
        assert np.array_equal(got, want), (code, rate, kind, n)
        if kind == "clean":
            assert np.array_equal(got, info)
        if kind == "zeros":
            assert not got.any()


def test_the_noisy_input_has_ties_and_the_huge_input_overflows():
    """What the inputs are for: half-integer LLRs (so equal candidates occur) and +-inf."""
    _, coded = R.frame("dvb_k7", "1/2", 188)
    x = R.llr_input("noisy", coded, seed=188)
    assert np.array_equal(x * 2, np.round(x * 2)) and len(np.unique(x)) < 30
    assert np.isinf(R.llr_input("huge", coded, seed=188)).any()


# ---- the reference's own properties (tests/unit/fec.rs:666-802) -----------------------------
@pytest.mark.parametrize("code,n", [("k5", 120), ("dvb_k7", 188)])
@pytest.mark.parametrize("rate", R.RATES)
def test_noiseless_round_trip_at_every_rate(lib, code, n, rate):
    info = ((np.arange(n) * 7 + 3) % 5 < 2).astype(np.uint8)
    coded = lib.conv_encode_punctured(info, rate, code)
    assert coded.size == lib.punctured_coded_len(n, rate, code)
    llr = (4.0 - 8.0 * coded.astype(np.float32)).astype(np.float32)
    assert np.array_equal(lib.viterbi_decode_soft(llr, n, rate, code), info)


def test_k5_rate_half_corrects_weakened_llrs(lib):
    info = ((np.arange(96) * 5 + 1) % 3 == 0).astype(np.uint8)
    coded = lib.conv_encode_punctured(info, "1/2", "k5")
    llr = (4.0 - 8.0 * coded.astype(np.float32)).astype(np.float32)
    for i in (3, 44, 90, 150):
        llr[i] *= np.float32(-0.5)
    assert np.array_equal(lib.viterbi_decode_soft(llr, 96, "1/2", "k5"), info)


def test_k7_rate_half_corrects_negated_llrs(lib):
    info = ((np.arange(188) * 11 + 2) % 7 < 3).astype(np.uint8)
    coded = lib.conv_encode_punctured(info, "1/2", "dvb_k7")
    llr = (4.0 - 8.0 * coded.astype(np.float32)).astype(np.float32)
    for i in (7, 33, 61, 100, 140, 200, 260):
        llr[i] = -llr[i]
    assert np.array_equal(lib.viterbi_decode_soft(llr, 188, "1/2", "dvb_k7"), info)


def test_k7_impulse_response_is_the_dvb_generators(lib):
    coded = lib.conv_encode_punctured(np.array([1], np.uint8), "1/2", "dvb_k7")  # 1 then six zeros
    assert coded[0::2].tolist() == [1, 1, 1, 1, 0, 0, 1]  # G0 = 171 octal
    assert coded[1::2].tolist() == [1, 0, 1, 1, 0, 1, 1]  # G1 = 133 octal


def test_k5_mother_code_is_the_existing_conv_encode(lib):
    info = np.random.default_rng(5).integers(0, 2, 77).astype(np.uint8)
    want = lib.conv_encode(np.concatenate([info, np.zeros(4, np.uint8)]))
    assert np.array_equal(lib.conv_encode_punctured(info, "1/2", "k5"), want)
    assert np.array_equal(lib.conv_encode_punctured(info, "1/2"), want)  # k5 is the default


# ---- the block interleaver ------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(4, 4), (3, 5), (32, 32)])
def test_interleaver_round_trip_and_index_map(lib, rows, cols):
    bi = lib.BlockInterleaver(rows, cols)
    n = rows * cols
    assert bi.block_len == n
    rng = np.random.default_rng(rows * 100 + cols)
    for x in (rng.integers(0, 256, n).astype(np.uint8), rng.normal(size=n).astype(np.float32)):
        y = bi.interleave(x)
        assert y.dtype == x.dtype and np.array_equal(y, R.interleave(rows, cols, x))
        for r in range(rows):
            for c in range(cols):
                assert y[c * rows + r] == x[r * cols + c]
        assert np.array_equal(bi.deinterleave(y), x)
        assert np.array_equal(bi.deinterleave(x), R.deinterleave(rows, cols, x))


def test_interleave_bits_pads_the_tail_to_a_full_block(lib):
    bi = lib.BlockInterleaver(4, 6)
    bits = np.random.default_rng(1).integers(0, 2, 85).astype(np.uint8)  # three blocks and a 13-bit tail
    for b in (bits, bits[:37], bits[:24], bits[:0]):
        got = bi.interleave_bits(b)
        assert got.size == -(-b.size // 24) * 24
        assert np.array_equal(got, R.interleave_bits(4, 6, b))
    tail = bi.interleave_bits(bits[:37])[24:]
    padded = np.concatenate([bits[24:37], np.zeros(11, np.uint8)])
    assert np.array_equal(tail, bi.interleave(padded))


def test_deinterleave_llrs_leaves_a_short_tail_as_it_is(lib):
    bi = lib.BlockInterleaver(4, 6)
    x = np.random.default_rng(2).normal(size=2 * 24 + 7).astype(np.float32)
    got = bi.deinterleave_llrs(x)
    assert np.array_equal(got, R.deinterleave_llrs(4, 6, x))
    assert np.array_equal(got[48:], x[48:])
    assert np.array_equal(got[:24], bi.deinterleave(x[:24])) and np.array_equal(got[24:48], bi.deinterleave(x[24:48]))
    assert np.array_equal(bi.deinterleave_llrs(x[:7]), x[:7])
    # with whole blocks the two drivers are inverses
    bits = np.random.default_rng(3).integers(0, 2, 72).astype(np.uint8)
    assert np.array_equal(bi.deinterleave_llrs(bi.interleave_bits(bits).astype(np.float32)), bits.astype(np.float32))


def test_host_decoder_with_an_interleaver_is_deinterleave_then_decode(lib):
    L = ctypes.CDLL(lib.lib_path())
    sz, vp, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    L.orion_fec_viterbi_host.argtypes = [i, i, vp, sz, sz, sz, sz, vp]
    info, coded = R.frame("dvb_k7", "3/4", 120)
    x = R.llr_input("noisy", coded, seed=9)[:6 * 24 + 7]
    got = np.zeros(120, np.uint8)
    assert L.orion_fec_viterbi_host(1, 2, x.ctypes.data, x.size, 120, 4, 6, got.ctypes.data) == 0
    want = lib.viterbi_decode_soft(lib.BlockInterleaver(4, 6).deinterleave_llrs(x), 120, "3/4", "dvb_k7")
    assert np.array_equal(got, want)


# ---- argument errors of the entries that reach no device -------------------------------------
def test_argument_errors(lib):
    L = ctypes.CDLL(lib.lib_path())
    sz, vp, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    L.orion_fec_punctured_coded_len.restype = sz
    L.orion_fec_punctured_coded_len.argtypes = [i, sz, i]
    L.orion_fec_viterbi_work_bytes.restype = sz
    L.orion_fec_viterbi_work_bytes.argtypes = [i, sz, sz]
    L.orion_fec_encoded_len.restype = sz
    L.orion_fec_encoded_len.argtypes = [i, sz, i, sz, sz]
    L.orion_fec_conv_encode.argtypes = [i, i, vp, sz, vp]
    L.orion_fec_viterbi_host.argtypes = [i, i, vp, sz, sz, sz, sz, vp]
    L.orion_fec_interleave_u8.argtypes = [sz, sz, vp, vp]
    L.orion_fec_viterbi_device.argtypes = [i, i, vp, sz, sz, sz, sz, sz, vp, vp, sz, vp]
    L.orion_fec_conv_encode_batch_device.argtypes = [i, i, vp, sz, sz, sz, sz, vp, vp]
    a = np.zeros(64, np.uint8)
    f = np.zeros(64, np.float32)
    p, q = a.ctypes.data, f.ctypes.data
    E_NULL, E_ARG = -1, -3
    assert L.orion_fec_punctured_coded_len(0, 10, 0) == 28 and L.orion_fec_punctured_coded_len(1, 10, 0) == 32
    assert L.orion_fec_punctured_coded_len(2, 10, 0) == 0 and L.orion_fec_punctured_coded_len(0, 10, 5) == 0
    assert L.orion_fec_punctured_coded_len(0, 0, 0) == 0 and L.orion_fec_punctured_coded_len(0, (1 << 24) + 1, 0) == 0
    assert L.orion_fec_viterbi_work_bytes(0, 5, 10) == 8 * 14 * 4 and L.orion_fec_viterbi_work_bytes(1, 5, 10) == 5 * 16 * 16
    assert L.orion_fec_viterbi_work_bytes(2, 5, 10) == 0 and L.orion_fec_viterbi_work_bytes(0, 5, 0) == 0
    assert L.orion_fec_encoded_len(0, 10, 0, 4, 6) == 48 and L.orion_fec_encoded_len(0, 10, 0, 0, 0) == 28
    assert L.orion_fec_encoded_len(0, 10, 0, 4, 0) == 0
    assert L.orion_fec_conv_encode(0, 0, None, 4, p) == E_NULL and L.orion_fec_conv_encode(0, 0, p, 4, None) == E_NULL
    assert L.orion_fec_conv_encode(7, 0, p, 4, p) == E_ARG and L.orion_fec_conv_encode(0, -1, p, 4, p) == E_ARG
    assert L.orion_fec_conv_encode(0, 0, p, 0, p) == E_ARG
    assert L.orion_fec_viterbi_host(0, 0, None, 8, 2, 0, 0, p) == E_NULL
    assert L.orion_fec_viterbi_host(0, 0, q, 8, 2, 0, 0, None) == E_NULL
    assert L.orion_fec_viterbi_host(0, 0, q, 8, 0, 0, 0, p) == E_ARG
    assert L.orion_fec_viterbi_host(0, 9, q, 8, 2, 0, 0, p) == E_ARG
    assert L.orion_fec_viterbi_host(0, 0, q, 8, 2, 4, 0, p) == E_ARG
    assert L.orion_fec_viterbi_host(0, 0, None, 0, 2, 0, 0, p) == 0  # no LLRs at all: every one reads 0.0
    assert L.orion_fec_interleave_u8(0, 4, p, p) == E_ARG and L.orion_fec_interleave_u8(4, 4, None, p) == E_NULL
    # the device entries refuse these before any device call
    assert L.orion_fec_viterbi_device(0, 0, q, 1, 8, 0, 0, 0, p, p, 1 << 20, None) == E_ARG
    assert L.orion_fec_viterbi_device(3, 0, q, 1, 8, 2, 0, 0, p, p, 1 << 20, None) == E_ARG
    assert L.orion_fec_viterbi_device(0, 0, q, 1, 8, 2, 0, 0, p, None, 1 << 20, None) == E_NULL
    assert L.orion_fec_viterbi_device(0, 0, q, (1 << 24) + 1, 8, 2, 0, 0, p, p, 1 << 20, None) == E_ARG
    assert L.orion_fec_conv_encode_batch_device(0, 5, p, 1, 8, 0, 0, p, None) == E_ARG
    assert L.orion_fec_conv_encode_batch_device(0, 0, p, 1, 0, 0, 0, p, None) == E_ARG
    with pytest.raises(ValueError):
        lib.punctured_coded_len(10, "1/3")
    with pytest.raises(ValueError):
        lib.conv_encode_punctured(a, "1/2", "k9")
    with pytest.raises(ValueError):
        lib.viterbi_decode_soft(f, 0, "1/2")
    with pytest.raises(ValueError):
        lib.BlockInterleaver(0, 4)
    with pytest.raises(ValueError):
        lib.BlockInterleaver(4, 4).interleave(a[:15])


# ---- the host code under the sanitizers -----------------------------------------------------
def test_host_fec_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/fec.cpp and tests/fec_host/main.cpp, built with the host compiler alone and
    -fsanitize=address,undefined into a stand-alone binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "fec_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src,
                    os.path.join(src, "fec.cpp"), os.path.join(ROOT, "tests", "fec_host", "main.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "fec_host: ok" in out.stdout, out.stdout + out.stderr
