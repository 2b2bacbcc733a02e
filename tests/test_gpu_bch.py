"""GPU: the outer BCH code's kernels (csrc/k_bch.hip) against the library's host layer
(csrc/bch.cpp, itself held to tests/np_ref_bch.py by tests/test_bch_oracle.py), byte for byte:
the batched decoder on every row and decoder path of the oracle's input set, at every word and
stream count, reading a stream with a tail; the encoder with its padding; torch tensors on a
stream of the caller's. The device entries take (t, info_bits), so a row (n, t, errors) runs
as info_bits = k. The chain through both frame codes is in tests/test_gpu_ldpc_family.py."""
import numpy as np
import pytest

import np_ref_bch as R

pytestmark = pytest.mark.gpu
WAVES = 4  # words per workgroup of k_bch_decode


@pytest.fixture(scope="module")
def rows(gpu_lib):
    """Every row's received words and the host decode of them, once: row -> (k, words, msgs, status)."""
    out = {}
    for row in R.ROWS:
        n, t, _ = row
        _, words = R.make_words(*row)
        code = gpu_lib.Bch(t, n)
        msgs, status = code.decode_counted(words)
        out[row] = (code.k, words, msgs, status)
    return out


def host_decode(lib, t, k, streams):
    """(nstreams, nb) -> (nstreams, ncw * k), (nstreams, ncw) by the host decoder, the tail dropped."""
    code = lib.Bch.for_info_bits(t, k)
    ncw = streams.shape[1] // code.n
    m, s = code.decode_counted(np.ascontiguousarray(streams[:, :ncw * code.n]).reshape(-1, code.n))
    return m.reshape(len(streams), ncw * k), s.reshape(len(streams), ncw)


@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: f"bch{r[0]}_t{r[1]}_e{r[2]}")
def test_decode_equals_host_on_every_row(gpu_lib, rows, row):
    """All the row's 26 words in one launch as one stream: the last workgroup is partly empty,
    and clean, corrected, rejected and miscorrected words sit side by side in a workgroup."""
    n, t, _ = row
    k, words, msgs, status = rows[row]
    assert len(words) % WAVES != 0
    got_m, got_s = gpu_lib.bch_decode_batch(words.reshape(-1), t, info_bits=k)
    assert got_s.dtype == np.int32 and np.array_equal(got_s, status), np.flatnonzero(got_s != status)[:8]
    assert np.array_equal(got_m, msgs.reshape(-1))


@pytest.mark.parametrize("ncw", [1, WAVES, WAVES + 1])
@pytest.mark.parametrize("nstreams", [1, 3])
def test_decode_word_and_stream_counts_with_a_tail(gpu_lib, rows, ncw, nstreams):
    """One word; exactly one workgroup; one more than that; one stream and three. The frame's
    code with 0, 1, 8, 9 and 12 errors mixed, and the shortest code; every stream ends in a
    tail shorter than a word, which is ignored."""
    for (n, t), picks in (((184, 8), (8, 9, 0, 1, 12)), ((9, 1), (1, 2, 0))):
        pool = np.concatenate([rows[(n, t, e)][1][i::5][:5] for i, e in enumerate(picks)])
        k = rows[(n, t, picks[0])][0]
        words = pool[np.arange(nstreams * ncw) * 3 % len(pool)].reshape(nstreams, ncw * n)
        streams = np.concatenate([words, np.full((nstreams, n - 1), 1, np.uint8)], axis=1)
        want_m, want_s = host_decode(gpu_lib, t, k, streams)
        got_m, got_s = gpu_lib.bch_decode_batch(streams, t, info_bits=k)
        assert got_m.shape == (nstreams, ncw * k) and got_s.shape == (nstreams, ncw)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_m, want_m)
        if ncw > 1:
            assert (want_s < 0).any() and (want_s >= 0).any()


@pytest.mark.parametrize("t,info_bits", [(8, 120), (1, 1), (2, 239), (16, 124), (31, 7), (3, 100)])
def test_encode_equals_host(gpu_lib, t, info_bits):
    """An input length that is no multiple of info_bits (the last message is zero-padded), one
    that is, and one shorter than a message; byte values other than 0 and 1 are copied as
    they are and enter the parity with bit 0. t = 31 has 200 parity bits: a fourth cell in
    lanes 0 to 7."""
    code = gpu_lib.Bch.for_info_bits(t, info_bits)
    for nbits in (2 * info_bits + max(1, info_bits // 3), 3 * info_bits, max(1, info_bits - 1)):
        rng = np.random.default_rng([61, t, nbits])
        bits = rng.integers(0, 2, (3, nbits), dtype=np.uint8)
        bits[1] = rng.integers(0, 256, nbits, dtype=np.uint8)
        ncw = -(-nbits // info_bits)
        padded = np.zeros((3, ncw * info_bits), np.uint8)
        padded[:, :nbits] = bits
        want = code.encode(padded.reshape(-1, info_bits)).reshape(3, ncw * code.n)
        got = gpu_lib.bch_encode_batch(bits, t, info_bits=info_bits)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (t, info_bits, nbits)
        assert np.array_equal(gpu_lib.bch_encode_batch(bits[2], t, info_bits=info_bits), want[2])


def test_torch_tensors_on_a_stream_of_the_callers(gpu_lib, rows):
    import torch

    k, words, msgs, status = rows[(184, 8, 8)]
    streams = np.ascontiguousarray(words[:24].reshape(2, -1))
    t = torch.from_numpy(streams).cuda()
    got_m, got_s = gpu_lib.bch_decode_batch(t, 8)
    assert got_m.is_cuda and got_s.is_cuda and got_s.dtype == torch.int32
    assert np.array_equal(got_m.cpu().numpy().reshape(-1, k), msgs[:24])
    assert np.array_equal(got_s.cpu().numpy().reshape(-1), status[:24])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got_m, got_s = gpu_lib.bch_decode_batch(t, 8, stream=s.cuda_stream)
        enc = gpu_lib.bch_encode_batch(got_m, 8, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(got_s.cpu().numpy().reshape(-1), status[:24])
    assert enc.is_cuda and np.array_equal(enc.cpu().numpy(), gpu_lib.bch_encode_batch(got_m.cpu().numpy(), 8))
    for bad in (lambda: gpu_lib.bch_decode_batch(torch.from_numpy(streams), 8),  # a CPU tensor
                lambda: gpu_lib.bch_decode_batch(t[:, ::2], 8),
                lambda: gpu_lib.bch_decode_batch(t.to(torch.int32), 8),
                lambda: gpu_lib.bch_decode_batch(t, 32),
                lambda: gpu_lib.bch_decode_batch(t[:, :100].contiguous(), 8)):
        with pytest.raises(ValueError):
            bad()
