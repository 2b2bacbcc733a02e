"""GPU: the outer-code kernels (csrc/k_rs.hip) against the library's host layer (csrc/rs.cpp,
itself held to tests/np_ref_rs.py by tests/test_rs_oracle.py), byte for byte: the batched
Reed-Solomon decoder on every shape, error count and decoder path of the oracle's input set,
its three fusions alone and together, the encoder, the Forney frame interleaver, one chain
from transport-stream packets through both codes and back on the device, and torch input."""
import numpy as np
import pytest

import np_ref_rs as R

pytestmark = pytest.mark.gpu
WAVES = 4  # codewords per workgroup of k_rs_decode


@pytest.fixture(scope="module")
def rows(gpu_lib):
    """Every row's received words and the host decode of them, once: row -> (words, msgs, status)."""
    out = {}
    for row in R.ROWS:
        _, words = R.make_words(*row, R.words_per_row(row[0]), R.SEED)
        msgs, status = gpu_lib.ReedSolomon(row[0], row[1]).decode_counted(words)
        out[row] = (words, msgs, status)
    return out


def dvb_words(lib, ncw, seed, nstreams=1):
    """(nstreams, ncw, 204) received words, mixed: clean, 1..8 errors, 9..12 errors."""
    rng = np.random.default_rng([21, ncw, seed])
    rs = lib.ReedSolomon.dvb()
    cws = rs.encode(rng.integers(0, 256, (nstreams * ncw, 188), dtype=np.uint8))
    for i, cw in enumerate(cws):
        n_err = (0, 3, 11, 8, 9, 1, 12, 5)[i % 8]
        pos = rng.choice(204, n_err, replace=False)
        cw[pos] ^= rng.integers(1, 256, n_err, dtype=np.uint8)
    return cws.reshape(nstreams, ncw, 204)


def host_decode(lib, words, n=204, n_parity=16):
    m, s = lib.ReedSolomon(n, n_parity).decode_counted(words.reshape(-1, n))
    return m.reshape(words.shape[:-1] + (n - n_parity,)), s.reshape(words.shape[:-1])


# ---- the decoder against the host decode_counted --------------------------------------------
@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: f"rs{r[0]}_{r[1]}_e{r[2]}")
def test_decode_equals_host_on_every_row(gpu_lib, rows, row):
    """All the row's words in one launch: a last workgroup partly empty (26 or 302 words), and
    clean, correctable and uncorrectable words side by side in a workgroup."""
    words, msgs, status = rows[row]
    assert len(words) % WAVES != 0
    got_m, got_s = gpu_lib.rs_decode_batch(words, n=row[0], n_parity=row[1])
    assert got_s.dtype == np.int32 and np.array_equal(got_s, status), np.flatnonzero(got_s != status)[:8]
    assert np.array_equal(got_m, msgs)


@pytest.mark.parametrize("ncw", [1, WAVES, WAVES + 1])
@pytest.mark.parametrize("nstreams", [1, 3])
def test_decode_codeword_and_stream_counts(gpu_lib, rows, ncw, nstreams):
    """One word; exactly one workgroup; one more than that; one stream and three. The words
    mix the paths: from the 8-, 9-, 0- and 1-error rows of the DVB code, and from the (12, 4)
    rows that hold the locator that outgrows t."""
    for code, picks in (((204, 16), (8, 9, 0, 1)), ((12, 4), (4, 3, 2, 4))):
        pool = np.concatenate([rows[code + (e,)][0][i::7][:6] for i, e in enumerate(picks)])
        words = pool[np.arange(nstreams * ncw) * 5 % len(pool)].reshape(nstreams, ncw, code[0])
        want_m, want_s = host_decode(gpu_lib, words, *code)
        got_m, got_s = gpu_lib.rs_decode_batch(words, n=code[0], n_parity=code[1])
        assert got_m.shape == want_m.shape and got_s.shape == want_s.shape
        assert np.array_equal(got_s, want_s) and np.array_equal(got_m, want_m)
        if nstreams == 1:  # a 2-D input is one stream
            m2, s2 = gpu_lib.rs_decode_batch(words[0], n=code[0], n_parity=code[1])
            assert np.array_equal(m2, want_m[0]) and np.array_equal(s2, want_s[0])


def test_one_workgroup_mixes_clean_correctable_and_uncorrectable_words(gpu_lib):
    words = dvb_words(gpu_lib, 2 * WAVES, 0)
    hm, hs = host_decode(gpu_lib, words)
    assert hs[0, :WAVES].tolist() == [0, 3, -1, 8] and hs[0, WAVES:].tolist() == [-1, 1, -1, 5]
    got_m, got_s = gpu_lib.rs_decode_batch(words)
    assert np.array_equal(got_s, hs) and np.array_equal(got_m, hm)


# ---- the fused paths ------------------------------------------------------------------------
def test_bit_input_equals_byte_input(gpu_lib):
    words = dvb_words(gpu_lib, 5, 1, nstreams=2)
    want_m, want_s = gpu_lib.rs_decode_batch(words)
    bits = np.unpackbits(words.reshape(2, -1), axis=1)
    for b in (bits, bits | 0xFE):  # only bit 0 of an element is read
        got_m, got_s = gpu_lib.rs_decode_batch(b, bits=True)
        assert np.array_equal(got_m, want_m) and np.array_equal(got_s, want_s)
    hm, hs = host_decode(gpu_lib, words)
    assert np.array_equal(want_m, hm) and np.array_equal(want_s, hs) and (hs < 0).any() and (hs > 0).any()


@pytest.mark.parametrize("I,M,code,ncw", [(12, 17, (204, 16), 1), (12, 17, (204, 16), 3), (3, 2, (12, 4), 5)])
def test_deinterleave_fusion_equals_host_deinterleaver_then_host_decode(gpu_lib, rows, I, M, code, ncw):
    n, n_parity = code
    src = dvb_words(gpu_lib, ncw, 2, nstreams=2) if n == 204 else \
        np.concatenate([rows[(12, 4, e)][0][:5] for e in (2, 4)]).reshape(2, ncw, n)
    streams = np.array([gpu_lib.forney_frame_interleave(s.reshape(-1), I, M) for s in src])
    rng = np.random.default_rng([22, I, ncw])
    streams[:, :I * (I - 1) * M:7] ^= rng.integers(0, 256, streams[:, :I * (I - 1) * M:7].shape, dtype=np.uint8)
    payload = np.array([gpu_lib.forney_frame_deinterleave(s, I, M) for s in streams])  # host ConvDeinterleaver
    assert payload.shape == (2, ncw * n)
    want_m, want_s = host_decode(gpu_lib, payload.reshape(2, ncw, n), n, n_parity)
    got_m, got_s = gpu_lib.rs_decode_batch(streams, n=n, n_parity=n_parity, deinterleave=(I, M))
    assert np.array_equal(got_s, want_s) and np.array_equal(got_m, want_m)
    m1, s1 = gpu_lib.rs_decode_batch(streams[1], n=n, n_parity=n_parity, deinterleave=(I, M))
    assert np.array_equal(m1, want_m[1]) and np.array_equal(s1, want_s[1])


@pytest.mark.parametrize("ncw", [1, 8, 9, 17])
def test_derandomize_equals_host_dispersal_of_host_decode(gpu_lib, ncw):
    """ncw = 9 and 17: the PRBS restarts inside the stream and the last group is partial; the
    words include failed ones (every fifth of eight has 9 errors), dispersed like the rest."""
    words = dvb_words(gpu_lib, ncw, 3, nstreams=2)
    hm, hs = host_decode(gpu_lib, words)
    want = np.array([gpu_lib.ts_energy_disperse(m.reshape(-1)) for m in hm]).reshape(hm.shape)
    got_m, got_s = gpu_lib.rs_decode_batch(words, derandomize=True)
    assert np.array_equal(got_s, hs) and np.array_equal(got_m, want)
    assert ncw < 5 or (hs < 0).any()


def test_all_three_fusions_together(gpu_lib):
    ncw = 9
    words = dvb_words(gpu_lib, ncw, 4, nstreams=2)
    hm, hs = host_decode(gpu_lib, words)
    want = np.array([gpu_lib.ts_energy_disperse(m.reshape(-1)) for m in hm]).reshape(hm.shape)
    streams = np.array([gpu_lib.forney_frame_interleave(s.reshape(-1), 12, 17) for s in words])
    bits = np.unpackbits(streams, axis=1)
    got_m, got_s = gpu_lib.rs_decode_batch(bits, bits=True, deinterleave=(12, 17), derandomize=True)
    assert np.array_equal(got_s, hs) and np.array_equal(got_m, want)


# ---- the encoder and the interleaver --------------------------------------------------------
@pytest.mark.parametrize("n,n_parity", [(204, 16), (255, 32), (12, 4), (7, 3), (2, 1), (40, 31)])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (3, 17)])
def test_encode_equals_host(gpu_lib, n, n_parity, shape):
    rng = np.random.default_rng([23, n, n_parity, shape[1]])
    msgs = rng.integers(0, 256, shape + (n - n_parity,), dtype=np.uint8)
    want = gpu_lib.ReedSolomon(n, n_parity).encode(msgs.reshape(-1, n - n_parity)).reshape(shape + (n,))
    assert np.array_equal(gpu_lib.rs_encode_batch(msgs, n=n, n_parity=n_parity), want)
    assert np.array_equal(gpu_lib.rs_encode_batch(msgs[0], n=n, n_parity=n_parity), want[0])


@pytest.mark.parametrize("ncw", [1, 8, 9, 17])
def test_encode_with_dispersal_equals_host_disperse_then_encode(gpu_lib, ncw):
    rng = np.random.default_rng([24, ncw])
    ts = np.array([gpu_lib.ts_packetize(rng.integers(0, 256, ncw * 187, dtype=np.uint8)) for _ in range(2)])
    want = np.array([gpu_lib.ReedSolomon.dvb().encode(gpu_lib.ts_energy_disperse(s).reshape(ncw, 188)) for s in ts])
    assert np.array_equal(gpu_lib.rs_encode_batch(ts.reshape(2, ncw, 188), disperse=True), want)


@pytest.mark.parametrize("I,M,length", [(12, 17, 204), (12, 17, 3 * 204), (12, 17, 100), (3, 2, 60), (4, 1, 10),
                                        (1, 5, 9), (5, 3, 77)])
def test_forney_interleave_equals_host_frame_mode(gpu_lib, I, M, length):
    rng = np.random.default_rng([25, I, length])
    x = rng.integers(1, 256, (3, length), dtype=np.uint8)
    want = np.array([gpu_lib.forney_frame_interleave(s, I, M) for s in x])
    assert np.array_equal(gpu_lib.forney_interleave_batch(x, I, M), want)
    assert np.array_equal(gpu_lib.forney_interleave_batch(x[1], I, M), want[1])
    assert np.array_equal(gpu_lib.forney_interleave_batch(x, I, M, bits=True), np.unpackbits(want, axis=1))


# ---- the chain on the device ----------------------------------------------------------------
def test_chain_from_ts_packets_through_both_codes_and_back_on_the_device(gpu_lib):
    """TS packets -> rs_encode_batch(disperse) -> forney_interleave_batch(bits) ->
    conv_encode_batch (K = 7, rate 2/3) -> LLRs of +-4 with a fixed set negated ->
    conv_viterbi_batch -> rs_decode_batch(bits, deinterleave, derandomize) = the packets, every
    tensor staying on the device."""
    import torch

    ncw, ns = 9, 2
    rng = np.random.default_rng(26)
    ts = np.array([gpu_lib.ts_packetize(rng.integers(0, 256, ncw * 187, dtype=np.uint8)) for _ in range(ns)])
    d_ts = torch.from_numpy(ts.reshape(ns, ncw, 188)).cuda()
    cws = gpu_lib.rs_encode_batch(d_ts, disperse=True)
    il = gpu_lib.forney_interleave_batch(cws, 12, 17, bits=True)
    assert il.is_cuda and tuple(il.shape) == (ns, (ncw * 204 + 2244) * 8)
    coded = gpu_lib.conv_encode_batch(il, "2/3", code="dvb_k7")
    llr = 4.0 - 8.0 * coded.to(torch.float32)  # positive means bit 0
    flip = torch.arange(llr.shape[1], device=llr.device) % 97 == 5  # isolated channel errors
    burst = (torch.arange(llr.shape[1], device=llr.device) // 40) % 300 == 7  # and bursts the inner code loses
    llr = torch.where(flip | burst, -llr, llr).contiguous()
    bits = gpu_lib.conv_viterbi_batch(llr, il.shape[1], "2/3", code="dvb_k7")
    assert bits.is_cuda and not torch.equal(bits, il)  # the inner code left errors for the outer code
    msgs, status = gpu_lib.rs_decode_batch(bits, bits=True, deinterleave=(12, 17), derandomize=True)
    assert msgs.is_cuda and status.is_cuda and status.dtype == torch.int32
    status = status.cpu().numpy()
    assert (status >= 0).all() and status.sum() > 0, status
    assert np.array_equal(msgs.cpu().numpy().reshape(ns, -1), ts)


# ---- input checks ---------------------------------------------------------------------------
def test_torch_tensor_gives_the_same_bytes_as_numpy(gpu_lib):
    import torch

    words = dvb_words(gpu_lib, 6, 5, nstreams=2)
    m, s = gpu_lib.rs_decode_batch(words, derandomize=True)
    tm, tst = gpu_lib.rs_decode_batch(torch.from_numpy(words).cuda(), derandomize=True)
    assert np.array_equal(tm.cpu().numpy(), m) and np.array_equal(tst.cpu().numpy(), s)
    bits = np.unpackbits(np.array([gpu_lib.forney_frame_interleave(w.reshape(-1), 12, 17) for w in words]), axis=1)
    d_bits = torch.from_numpy(bits).cuda()
    tm, tst = gpu_lib.rs_decode_batch(d_bits, bits=True, deinterleave=(12, 17), derandomize=True)
    assert np.array_equal(tm.cpu().numpy(), m) and np.array_equal(tst.cpu().numpy(), s)
    # a stream that does not start on an 8-byte boundary takes the byte loads
    odd = torch.zeros(bits.size + 3, dtype=torch.uint8, device="cuda")[3:].view(bits.shape)
    odd.copy_(d_bits)
    assert odd.data_ptr() % 8 != 0
    tm, tst = gpu_lib.rs_decode_batch(odd, bits=True, deinterleave=(12, 17), derandomize=True)
    assert np.array_equal(tm.cpu().numpy(), m) and np.array_equal(tst.cpu().numpy(), s)
    msgs = words[:, :, :188].copy()
    enc = gpu_lib.rs_encode_batch(torch.from_numpy(msgs).cuda(), disperse=True)
    assert np.array_equal(enc.cpu().numpy(), gpu_lib.rs_encode_batch(msgs, disperse=True))
    il = gpu_lib.forney_interleave_batch(enc, 12, 17)
    assert np.array_equal(il.cpu().numpy(), gpu_lib.forney_interleave_batch(enc.cpu().numpy(), 12, 17))
    for bad in (lambda: gpu_lib.rs_decode_batch(torch.from_numpy(words)),  # a CPU tensor
                lambda: gpu_lib.rs_decode_batch(torch.from_numpy(words).cuda()[:, :, ::2]),
                lambda: gpu_lib.rs_decode_batch(torch.from_numpy(words).cuda().to(torch.int32)),
                lambda: gpu_lib.rs_decode_batch(torch.from_numpy(words).cuda(), n_parity=40)):
        with pytest.raises(ValueError):
            bad()
