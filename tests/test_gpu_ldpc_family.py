"""GPU: the LDPC family's kernels (csrc/k_ldpc_family.hip) against the library's host layer
(csrc/ldpc_family.cpp, itself held to tests/np_ref_ldpc_family.py by
tests/test_ldpc_family_oracle.py), equal in every output: bits, unsatisfied checks and
iteration counts of the batched decoder under all three rules, on the whole oracle input set,
at every codeword and stream count, with the deinterleaver fused; the encoder with its padding
and its interleaver; torch tensors on a stream of the caller's; and one chain through both
frame codes and the OFDM symbol layer that stays on the device. k_ldpcf_decode runs one
codeword per workgroup, so 1 codeword is one workgroup and 2 is one more than that."""
import numpy as np
import pytest

import np_ref_ldpc_family as R

pytestmark = pytest.mark.gpu
# The chain's noise: its standard deviation per complex sample over the signal's RMS. 0.25 is
# 12 dB, where QAM-16 leaves raw bit errors (a few in a hundred) and the rate-1/2 code has margin.
CHAIN_NOISE = 0.25


@pytest.fixture(scope="module")
def sets():
    """code -> the oracle input set, (125, N) float32, unchanged by the tests."""
    out = {name: R.input_set(name) for name in R.NAMES}
    for v in out.values():
        v.setflags(write=False)
    return out


def host_decode(lib, code, llr, max_iter=50, rule="sum_product", interleaver=None):
    """(nstreams, n_llr) through the host deinterleaver and the host decoder."""
    c = lib.Ldpc(code)
    rows = [lib.BlockInterleaver(*interleaver).deinterleave_llrs(r) if interleaver else r for r in llr]
    nb = llr.shape[1] // c.n
    words = np.stack(rows)[:, :nb * c.n].reshape(-1, c.n)
    b, u, i = c.decode_soft(words, max_iter, rule)
    return b.reshape(len(llr), nb * c.k), u.reshape(len(llr), nb), i.reshape(len(llr), nb)


def assert_same(got, want):
    for g, w, what in zip(got, want, ("bits", "unsat", "iterations")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w), (what, np.argwhere(g != w)[:8])


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: r if isinstance(r, str) else r[0])
@pytest.mark.parametrize("code", R.NAMES)
def test_decode_equals_host_on_the_whole_oracle_set(gpu_lib, sets, code, rule):
    """All 125 words in one launch, five streams of 25: valid, converging and failing words
    side by side, NaN, infinities and 1e30 among them; max_iter 50, 1 and 0."""
    llr = sets[code].reshape(5, -1)
    want = host_decode(gpu_lib, code, llr, 50, rule)
    assert (want[2] == 0).any() and (want[2] == 1).any() and (want[2] == 50).any() and (want[1] > 0).any()
    assert_same(gpu_lib.ldpc_family_decode_batch(llr, code, rule=rule), want)
    for max_iter in (1, 0):
        assert_same(gpu_lib.ldpc_family_decode_batch(llr, code, max_iter=max_iter, rule=rule),
                    host_decode(gpu_lib, code, llr, max_iter, rule))


@pytest.mark.parametrize("nblocks", [1, 2, 3])
@pytest.mark.parametrize("nstreams", [1, 3])
def test_decode_codeword_and_stream_counts(gpu_lib, sets, nblocks, nstreams):
    """One word, two, three; one stream and three; the words alternate between the sigma =
    0.3 (valid at once), 0.6 (converging) and 0.9 (failing) parts of the set."""
    for code in R.NAMES:
        i = np.arange(nstreams * nblocks)
        pick = np.array([0, 2, 4])[i % 3] * R.WORDS + i * 5 % R.WORDS
        llr = sets[code][pick].reshape(nstreams, -1)
        want = host_decode(gpu_lib, code, llr)
        got = gpu_lib.ldpc_family_decode_batch(llr, code)
        assert got[0].shape == (nstreams, nblocks * gpu_lib.Ldpc(code).k) and got[1].shape == (nstreams, nblocks)
        assert_same(got, want)


@pytest.mark.parametrize("il", [(32, 32), (24, 24), (7, 11)])
@pytest.mark.parametrize("code", R.NAMES)
def test_decode_with_the_fused_deinterleaver(gpu_lib, sets, code, il):
    """The stream is whole interleaver blocks, one and two codewords' worth; codeword LLR j is
    element j of its deinterleaving. With (7, 11) and N = 512 a stream of 539 holds one word
    and a tail of 27 that is never read (it holds NaN here and changes nothing)."""
    n, block = gpu_lib.Ldpc(code).n, il[0] * il[1]
    for nwords in (1, 2):
        length = -(-nwords * n // block) * block
        nb = length // n
        plain = np.full((3, length), np.nan, np.float32)
        plain[:, :nb * n] = sets[code][np.arange(3 * nb) * 7 % 125].reshape(3, nb * n)
        stream = np.stack([np.concatenate([gpu_lib.BlockInterleaver(*il).interleave(r[b:b + block])
                                           for b in range(0, length, block)]) for r in plain])
        want = host_decode(gpu_lib, code, stream, interleaver=il)
        assert_same(want, host_decode(gpu_lib, code, plain))
        assert_same(gpu_lib.ldpc_family_decode_batch(stream, code, interleaver=il), want)
        if length == 539:
            assert nb == 1 and length - nb * n == 27


@pytest.mark.parametrize("il", [None, (32, 32), (7, 11)])
@pytest.mark.parametrize("code", R.NAMES)
def test_encode_equals_host(gpu_lib, code, il):
    """An input length that is no multiple of K (the last message is zero-padded), one that is,
    and one shorter than K; the coded stream zero-padded to whole interleaver blocks."""
    c = gpu_lib.Ldpc(code)
    for nbits in (c.k + 100, 2 * c.k, 5):
        rng = np.random.default_rng([51, c.index, nbits])
        bits = rng.integers(0, 2, (3, nbits), dtype=np.uint8)
        nb = -(-nbits // c.k)
        padded = np.zeros((3, nb * c.k), np.uint8)
        padded[:, :nbits] = bits
        want = c.encode(padded.reshape(-1, c.k)).reshape(3, nb * c.n)
        if il:
            want = np.stack([gpu_lib.BlockInterleaver(*il).interleave_bits(w) for w in want])
        got = gpu_lib.ldpc_family_encode_batch(bits, code, interleaver=il)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (code, il, nbits)


def test_torch_tensors_on_a_stream_of_the_callers(gpu_lib, sets):
    import torch

    code, il = "n576r23", (24, 24)
    llr = sets[code][40:46].reshape(2, -1).copy()
    want = host_decode(gpu_lib, code, llr, 50, "min_sum", il)
    t = torch.from_numpy(llr).cuda()
    got = gpu_lib.ldpc_family_decode_batch(t, code, rule="min_sum", interleaver=gpu_lib.BlockInterleaver(*il))
    assert all(g.is_cuda for g in got) and got[0].dtype == torch.uint8 and got[1].dtype == torch.int32
    assert_same([g.cpu().numpy() for g in got], want)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = gpu_lib.ldpc_family_decode_batch(t, code, rule="min_sum", interleaver=il, stream=s.cuda_stream)
        bits = torch.from_numpy(want[0]).cuda()
        enc = gpu_lib.ldpc_family_encode_batch(bits, code, interleaver=il, stream=s.cuda_stream)
    s.synchronize()
    assert_same([g.cpu().numpy() for g in got], want)
    assert enc.is_cuda and np.array_equal(enc.cpu().numpy(), gpu_lib.ldpc_family_encode_batch(want[0], code, interleaver=il))
    for bad in (lambda: gpu_lib.ldpc_family_decode_batch(torch.from_numpy(llr), code),  # a CPU tensor
                lambda: gpu_lib.ldpc_family_decode_batch(t[:, ::2], code),
                lambda: gpu_lib.ldpc_family_decode_batch(t.double(), code),
                lambda: gpu_lib.ldpc_family_decode_batch(t, code, interleaver=(7, 11)),
                lambda: gpu_lib.ldpc_family_encode_batch(bits.to(torch.int32), code)):
        with pytest.raises(ValueError):
            bad()


def test_chain_through_both_frame_codes_and_the_ofdm_symbol_layer_on_the_device(gpu_lib):
    """payload -> bch_encode_batch (t = 8) -> ldpc_family_encode_batch (N512R12 behind a 32 x 32
    interleaver) -> OfdmMod (QAM-16; the configuration of tests/test_gpu_fec.py's chain) ->
    noise -> ofdm_demodulate_batch LLRs -> ldpc_family_decode_batch (min-sum) -> bch_decode_batch = the
    payload, and = the host decoders on the same LLRs; no tensor leaves the device between
    the payload and its decode."""
    import torch

    lib = gpu_lib
    pilots = np.array([-21, -7, 7, 21], np.int32)
    cfg = lib.OfdmConfig(64, 16, np.zeros(0, np.int32), pilots, np.array([1, -1, 1j, 1], np.complex64), 1e6, 0.0,
                         1.0, "qam16", edge_guard=4)
    mod, demod = lib.OfdmMod(cfg), lib.OfdmDemod(cfg, None)
    il, nbits = (32, 32), 300  # 3 BCH words (the last padded) = 552 bits = 3 LDPC words (padded) = 1.5 blocks
    payload = torch.from_numpy(np.random.default_rng(78).integers(0, 2, (2, nbits)).astype(np.uint8)).cuda()
    outer = lib.bch_encode_batch(payload, 8)
    assert outer.is_cuda and tuple(outer.shape) == (2, 3 * 184)
    coded = lib.ldpc_family_encode_batch(outer, "n512r12", interleaver=il)
    assert coded.is_cuda and tuple(coded.shape) == (2, 2048)
    bps = mod.bits_per_ofdm_symbol
    nsym = -(-coded.shape[1] // bps)
    tx_bits = torch.zeros((2, nsym * bps), dtype=torch.uint8, device="cuda")
    tx_bits[:, :coded.shape[1]] = coded
    iq = lib.ofdm_modulate_batch(mod, tx_bits)
    gen = torch.Generator().manual_seed(79)
    noise = torch.view_as_complex(torch.randn(tuple(iq.shape) + (2,), generator=gen)).cuda()
    rms = iq.abs().pow(2).mean().sqrt()
    iq = (iq + (CHAIN_NOISE / 2 ** 0.5) * rms * noise).contiguous()  # randn is unit variance per component
    _, _, llr = lib.ofdm_demodulate_batch(demod, iq, bits=False, llr=True)
    llr = llr[:, :2048].contiguous()  # whole interleaver blocks: the symbol padding goes
    # the demodulator's max-log LLRs carry no noise-variance scale; min-sum does not need one
    inner, unsat, iters = lib.ldpc_family_decode_batch(llr, "n512r12", rule="min_sum", interleaver=il)
    assert inner.is_cuda and tuple(inner.shape) == (2, 4 * 256)
    got, status = lib.bch_decode_batch(inner, 8)
    assert got.is_cuda and status.is_cuda and tuple(got.shape) == (2, 5 * 120)  # 1024 // 184 words
    h_inner, h_unsat, h_iters = host_decode(lib, "n512r12", llr.cpu().numpy(), rule="min_sum", interleaver=il)
    assert_same([inner.cpu().numpy(), unsat.cpu().numpy(), iters.cpu().numpy()], [h_inner, h_unsat, h_iters])
    h_got, h_status = lib.Bch.for_info_bits(8).decode_counted(h_inner[:, :5 * 184].reshape(-1, 184))
    assert np.array_equal(got.cpu().numpy(), h_got.reshape(2, -1)) and np.array_equal(status.cpu().numpy().ravel(), h_status)
    print(f"[chain] ldpc iterations {h_iters.tolist()} unsat {h_unsat.tolist()} bch status {h_status.tolist()}")
    assert (h_iters[:, :3] >= 1).any(), "the noise left the inner code nothing to do"
    assert (h_unsat[:, :3] == 0).all() and (h_status.reshape(2, 5)[:, :3] >= 0).all()
    assert torch.equal(got[:, :nbits], payload)
