"""GPU: the inner code's kernels (csrc/k_fec.hip) against the library's scalar host code.
Everything is exact: the device decoder's bits equal the host decoder's (viterbi_decode_soft of
deinterleave_llrs of the same input, which tests/test_fec_oracle.py holds to the numpy
restatement), the device encoder's bytes equal the host encoder's and interleave_bits'.

Information bits. k_conv_viterbi fetches LLRs in groups of W / 2 trellis steps (W lanes per
stream): H = 8 steps for K = 5 and H = 32 for K = 7, and a frame has info_bits + K - 1 steps. Its
traceback reads survivor words in groups of kTraceAhead = 8. INFO_BITS is chosen against those:

  info_bits   K = 5 steps (H = 8)                K = 7 steps (H = 32)
  1, 2        5, 6: inside the first group       7, 8: inside; not every state reachable yet
  4           8: ends exactly on the first group 10: inside
  5           9: one past the first group        11: inside
  26          30: three groups and 6             32: ends exactly on the first group
  27          31: three groups and 7             33: one past the first group
  33          37: four groups and 5              39: one group and 7
  300         304: 38 groups                     306: nine groups and 18

All five rates run at 33 and 300 bits, rate 1/2 at the rest. Streams: K = 5 with 1, 4, 5 and 9
(one lane group, a full wave, a wave plus one, three workgroups with the last partly empty),
K = 7 with 1, 2 and 3; every stream has its own seeded input."""
import ctypes

import numpy as np
import pytest

import np_ref_fec as R

pytestmark = pytest.mark.gpu

INFO_BITS = (1, 2, 4, 5, 26, 27, 33, 300)
ALL_RATE_BITS = (33, 300)
STREAMS = [("k5", 1), ("k5", 4), ("k5", 5), ("k5", 9), ("dvb_k7", 1), ("dvb_k7", 2), ("dvb_k7", 3)]
KINDS = ("noisy", "zeros", "short", "huge")


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


def shapes():
    return [(n, rate) for n in INFO_BITS for rate in (R.RATES if n in ALL_RATE_BITS else ("1/2",))]


def batch_llrs(lib, code, rate, info_bits, nstreams, kind, n_llr=None):
    """(nstreams, n_llr) LLRs, every stream from its own frame and its own noise. n_llr
    defaults to the coded length (half of it for "short"); a longer n_llr continues the
    half-integer noise past the coded bits."""
    coded_len = lib.punctured_coded_len(info_bits, rate, code)
    if n_llr is None:
        n_llr = coded_len // 2 if kind == "short" else coded_len
    out = np.zeros((nstreams, n_llr), np.float32)
    if kind == "zeros":
        return out
    for k in range(nstreams):
        _, coded = R.frame(code, rate, info_bits, seed=k)
        bits = np.zeros(max(n_llr, coded_len), np.uint8)
        bits[:coded_len] = coded
        out[k] = R.noisy_llrs(bits, seed=1000 * info_bits + k)[:n_llr]
    if kind == "huge":
        with np.errstate(over="ignore"):
            out = (out * np.float32(1e38)).astype(np.float32)
    return out


def host_decode(lib, llr, info_bits, rate, code, il=None):
    bi = lib.BlockInterleaver(*il) if il else None
    return np.stack([lib.viterbi_decode_soft(bi.deinterleave_llrs(row) if bi else row, info_bits, rate, code)
                     for row in llr])


# ---- the decoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("code,nstreams", STREAMS)
def test_decoder_equals_the_host_decoder(lib, code, nstreams):
    """Every shape of the module docstring, on the four inputs: half-integer noise (ties), all
    zeros (all-zero bits), n_llr at half the coded length, and the noise scaled by 1e38."""
    for info_bits, rate in shapes():
        for kind in KINDS:
            llr = batch_llrs(lib, code, rate, info_bits, nstreams, kind)
            got = lib.conv_viterbi_batch(llr, info_bits, rate, code)
            assert got.dtype == np.uint8 and got.shape == (nstreams, info_bits)
            want = host_decode(lib, llr, info_bits, rate, code)
            assert np.array_equal(got, want), (code, nstreams, info_bits, rate, kind)
            if kind == "zeros":
                assert not got.any()


@pytest.mark.parametrize("code,nstreams", [("k5", 5), ("dvb_k7", 3)])
def test_decoder_recovers_clean_frames(lib, code, nstreams):
    for info_bits, rate in shapes():
        info = np.stack([R.frame(code, rate, info_bits, seed=k)[0] for k in range(nstreams)])
        coded = np.stack([R.frame(code, rate, info_bits, seed=k)[1] for k in range(nstreams)])
        llr = (4.0 - 8.0 * coded.astype(np.float32)).astype(np.float32)
        assert np.array_equal(lib.conv_viterbi_batch(llr, info_bits, rate, code), info), (code, info_bits, rate)


@pytest.mark.parametrize("code,nstreams", [("k5", 5), ("dvb_k7", 3)])
def test_decoder_with_the_fused_deinterleaver(lib, code, nstreams):
    """4 x 6 with n_llr = whole blocks + 7 (the short tail passes through unpermuted), at 33 and
    300 bits and every rate; 32 x 32 on a frame of more than one block (1100 bits: two blocks
    and a tail at rate 1/2, one block and a tail at 7/8), and on whole blocks only."""
    cases = [((4, 6), n, rate, None) for n in ALL_RATE_BITS for rate in R.RATES]
    cases += [((32, 32), 1100, "1/2", None), ((32, 32), 1100, "7/8", None), ((32, 32), 1100, "1/2", 3072)]
    for il, info_bits, rate, n_llr in cases:
        block = il[0] * il[1]
        coded_len = lib.punctured_coded_len(info_bits, rate, code)
        if n_llr is None:
            n_llr = coded_len // block * block + 7 if block == 24 else coded_len
        for kind in ("huge", "noisy"):
            llr = batch_llrs(lib, code, rate, info_bits, nstreams, kind, n_llr)
            got = lib.conv_viterbi_batch(llr, info_bits, rate, code, interleaver=il)
            want = host_decode(lib, llr, info_bits, rate, code, il)
            assert np.array_equal(got, want), (code, il, info_bits, rate, n_llr, kind)
        if n_llr % block:  # the permutation is in play: the full blocks read differently deinterleaved
            assert not np.array_equal(lib.BlockInterleaver(*il).deinterleave_llrs(llr[0])[:n_llr // block * block],
                                      llr[0][:n_llr // block * block])


def test_decoder_on_resident_tensors_and_a_stream(lib, torch):
    """The _device entry: torch tensors in and out, on torch's current stream and on a stream
    of the caller's; an interleaver object or a (rows, cols) pair."""
    llr = batch_llrs(lib, "dvb_k7", "3/4", 300, 3, "noisy", 17 * 24 + 7)
    want = host_decode(lib, llr, 300, "3/4", "dvb_k7", (4, 6))
    t = torch.from_numpy(llr).cuda()
    got = lib.conv_viterbi_batch(t, 300, "3/4", "dvb_k7", interleaver=lib.BlockInterleaver(4, 6))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = lib.conv_viterbi_batch(t, 300, "3/4", "dvb_k7", interleaver=(4, 6), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        lib.conv_viterbi_batch(t.double(), 300, "3/4", "dvb_k7")
    with pytest.raises(ValueError):
        lib.conv_viterbi_batch(t, 0, "3/4", "dvb_k7")
    with pytest.raises(ValueError):
        lib.conv_viterbi_batch(llr, 300, "3/5", "dvb_k7")
    assert lib.conv_viterbi_batch(llr[:0], 300, "3/4", "dvb_k7").shape == (0, 300)


@pytest.mark.parametrize("code", ["k5", "dvb_k7"])
def test_workspace_too_small_is_refused_and_its_contents_do_not_matter(lib, torch, code):
    L = ctypes.CDLL(lib.lib_path())
    sz, vp, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    L.orion_fec_viterbi_work_bytes.restype = sz
    L.orion_fec_viterbi_work_bytes.argtypes = [i, sz, sz]
    L.orion_fec_viterbi_device.argtypes = [i, i, vp, sz, sz, sz, sz, sz, vp, vp, sz, vp]
    c, ns, n = lib.FEC_CODES[code], 5, 33
    llr = batch_llrs(lib, code, "2/3", n, ns, "noisy")
    want = host_decode(lib, llr, n, "2/3", code)
    t = torch.from_numpy(llr).cuda()
    wb = L.orion_fec_viterbi_work_bytes(c, ns, n)
    assert wb == ((8 * 37 * 4) if code == "k5" else (5 * 39 * 16))
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device="cuda")
    bits = torch.full((ns, n), 7, dtype=torch.uint8, device="cuda")
    args = (c, 1, t.data_ptr(), ns, llr.shape[1], n, 0, 0, bits.data_ptr(), work.data_ptr())
    assert L.orion_fec_viterbi_device(*args, wb - 1, None) == -3  # ORION_E_ARG
    torch.cuda.synchronize()
    assert bool((bits == 7).all()) and bool((work == 0xFF).all())  # nothing was launched
    assert L.orion_fec_viterbi_device(*args, wb, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy(), want)


# ---- the encoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("code", ["k5", "dvb_k7"])
def test_encoder_equals_the_host_encoder(lib, torch, code):
    cases = [(None, n, rate) for n, rate in shapes()]
    cases += [((4, 6), n, rate) for n in ALL_RATE_BITS for rate in R.RATES]
    cases += [((32, 32), 1100, "1/2"), ((32, 32), 1100, "7/8")]
    for il, info_bits, rate in cases:
        info = np.stack([R.frame(code, rate, info_bits, seed=k)[0] for k in range(3)]) if info_bits <= 300 else \
            np.random.default_rng(info_bits).integers(0, 2, (3, info_bits)).astype(np.uint8)
        want = [lib.conv_encode_punctured(row, rate, code) for row in info]
        if il:
            want = [lib.BlockInterleaver(*il).interleave_bits(w) for w in want]
        want = np.stack(want)
        got = lib.conv_encode_batch(info, rate, code, interleaver=il)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (code, il, info_bits, rate)
        if il:
            assert got.shape[1] % (il[0] * il[1]) == 0
    t = lib.conv_encode_batch(torch.from_numpy(info).cuda(), rate, code, interleaver=il)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)
    with pytest.raises(ValueError):
        lib.conv_encode_batch(info[:, :0], rate, code)
    with pytest.raises(ValueError):
        lib.conv_encode_batch(info, rate, code, interleaver=(4, 0))


# ---- payload bits -> coded bits -> OfdmMod -> OfdmDemod LLRs -> payload bits, on the device --
def test_payload_round_trip_through_the_ofdm_symbol_layer(lib, torch):
    """K = 7 at rate 3/4 behind a 4 x 6 interleaver over QAM-16 symbols, two channels, a
    noiseless channel: no tensor leaves the device between the payload and its decode."""
    pilots = np.array([-21, -7, 7, 21], np.int32)
    cfg = lib.OfdmConfig(64, 16, np.zeros(0, np.int32), pilots, np.array([1, -1, 1j, 1], np.complex64), 1e6, 0.0,
                         1.0, "qam16", edge_guard=4)
    mod, demod = lib.OfdmMod(cfg), lib.OfdmDemod(cfg, None)
    info_bits, il = 400, (4, 6)
    payload = torch.from_numpy(np.random.default_rng(77).integers(0, 2, (2, info_bits)).astype(np.uint8)).cuda()
    coded = lib.conv_encode_batch(payload, "3/4", "dvb_k7", interleaver=il)
    bps = mod.bits_per_ofdm_symbol
    nsym = -(-coded.shape[1] // bps)
    assert 2 <= nsym <= 8
    tx_bits = torch.zeros((2, nsym * bps), dtype=torch.uint8, device="cuda")
    tx_bits[:, :coded.shape[1]] = coded
    iq = lib.ofdm_modulate_batch(mod, tx_bits)
    _, _, llr = lib.ofdm_demodulate_batch(demod, iq, bits=False, llr=True)
    assert llr.is_cuda and llr.shape == (2, nsym * bps)
    got = lib.conv_viterbi_batch(llr, info_bits, "3/4", "dvb_k7", interleaver=il)
    assert got.is_cuda and torch.equal(got, payload)
