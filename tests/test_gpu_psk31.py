"""GPU: the PSK31 demodulator bank (csrc/k_psk31.hip k_psk31_demod) and the batched QPSK31
Viterbi decode (k_psk31_viterbi), both against the library's host layer (csrc/psk31.cpp, held
to tests/np_ref_psk31.py byte for byte by tests/test_psk31_oracle.py).

The bank. Its arithmetic is the host demodulator's operation for operation except phase_acc's
sine and cosine (glibc on the host, a correctly-rounded-but-for-near-ties pair on the device),
so soft values are held to a bound taken on the CPU for the very input: the restatement runs
twice, as is and with every sine and cosine moved one ulp in a seeded random direction; d1 is
the largest difference between the two runs' soft values, and the device may differ from the
host layer by 2 d1 (one random pattern is not the worst one). The loop is contractive (a
prev_sym error re-enters the next symbol scaled by about 1/3, the phase loop has gain 0.05),
so d1 is a few ulp. Reports and hard bits are exact. Each test that compares hard bits
first checks on the CPU that the smallest |soft| behind them exceeds 1000 d1, so no sign can
flip within the bound, and fails as a bad fixture otherwise. The bank writes hard bits for
BPSK31 streams only (a QPSK31 pair has one component that is noise about zero, which nobody
slices): a QPSK31 stream's rows of bits stay zero, and its decisions, the Viterbi decode of
the device's soft pairs, equal the Viterbi decode of the host's.
The band: fs 8000 (256 samples per symbol), 40 symbols + 37 samples, so every stream with a
rotator crosses its renormalisation at 1024 steps ten times and ends inside a symbol.
Channel 0 carries BPSK31 at 1000 Hz and another BPSK31 signal at 0 Hz (32 cycles per symbol
apart); channel 1 QPSK31 at 1531.25 Hz; both with Gaussian noise of deviation 0.05 per
component. 130 streams: even ones BPSK31 at 1000 Hz, odd ones QPSK31, stream 7 BPSK31 with
rf_hz == 0 (no rotator at all); starts (53 k) % 700 with the offset that keeps the symbol
clock; gains 1 and 0.5. 1, 64, 65 and 130 streams are the first streams of that list: one
lane, a full wave, a wave and a lane, two waves and two lanes.

The batched QPSK31 Viterbi decode (csrc/k_psk31.hip k_psk31_viterbi) against the
library's host decoder (csrc/psk31.cpp, itself held to tests/np_ref_psk31.py byte for byte by
tests/test_psk31_oracle.py). Everything is exact: the kernel keeps the reference's start
metric, skip, predecessor order, strict < and first-minimum rule, so its bits are the
host's for every input, ties and non-finite values included.

Shapes: 1, 4, 5 and 9 streams put one, four, and four-plus-one streams into a wave and use
one to three workgroups, with the last wave partly empty; 1, 2 and 5 symbols end before
every state is reachable and inside the first group of eight symbols the kernel fetches
ahead, 33 and 300 cross that group with and without a remainder; 7, 8, 9, 15, 16 and 17 sit
on either side of the first two edges of that group, which the step loop and the traceback
(eight survivor words ahead) both have."""
import functools

import numpy as np
import pytest

import np_ref_psk31 as P
from conftest import report

pytestmark = pytest.mark.gpu

STREAMS = (1, 4, 5, 9)
GROUP_EDGE_LENGTHS = (7, 8, 9, 15, 16, 17)

# ---- the demodulator bank ---------------------------------------------------------------
FS = 8000.0
SPS = 256
N = 40 * SPS + 37
NBANK = 130
CAP = 96


@functools.lru_cache(maxsize=None)
def _band():
    rng = np.random.default_rng(2031)
    nb = 42
    b0 = P.Mod(P.BPSK, FS, 1000.0, 1.0).modulate_bits(rng.integers(0, 2, nb).astype(np.uint8))[:N]
    b1 = P.Mod(P.BPSK, FS, 0.0, 1.0).modulate_bits(rng.integers(0, 2, nb).astype(np.uint8))[:N]
    q = P.Mod(P.QPSK, FS, 1531.25, 1.0).modulate_bits(rng.integers(0, 2, nb).astype(np.uint8))[:N]
    x = np.stack([b0 + b1, q])
    noise = rng.normal(0.0, 0.05, x.shape + (2,)).astype(np.float32)
    return (x + noise.view(np.complex64)[..., 0]).astype(np.complex64)


def _stream(k):
    start = (53 * k) % 700
    offset = (SPS - start % SPS) % SPS
    gain = 0.5 if k % 5 == 3 else 1.0
    if k == 7:
        return P.stream_record(P.BPSK, 0, 0.0, gain, start, offset, CAP)
    if k % 2 == 0:
        return P.stream_record(P.BPSK, 0, 1000.0, gain, start, offset, CAP)
    return P.stream_record(P.QPSK, 1, 1531.25, gain, start, offset, CAP)


def _records(lib, recs):
    out = np.zeros(len(recs), lib.PSK31_STREAM_DTYPE)
    for k, r in enumerate(recs):
        out[k] = (r["mode"], r["channel"], r["rf_hz"], r["gain"], r["start"], r["offset"], r["out_cap"])
    return out


@functools.lru_cache(maxsize=None)
def _reference():
    """-> (recs, host soft per stream, host in_read, d1 per stream): the host layer's output
    for each of the 130 streams, and the restatement's distance between its two runs."""
    import orion_sdr

    x = _band()
    recs = [_stream(k) for k in range(NBANK)]
    plain, _, _ = P.DemodBank(FS, recs).process(x)
    moved, _, _ = P.DemodBank(FS, recs, perturb=np.random.default_rng(99)).process(x)
    d1 = np.array([float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(plain, moved)])
    host, nread = [], []
    for r in recs:
        cls = orion_sdr.Bpsk31Demod if r["mode"] == P.BPSK else orion_sdr.Qpsk31Demod
        soft, n = cls(FS, r["rf_hz"], r["gain"], r["offset"]).process_host(x[r["channel"], r["start"]:], CAP)
        host.append(soft)
        nread.append(n)
    # the host layer is the restatement on this input too
    assert all(h.tobytes() == p.tobytes() for h, p in zip(host, plain))
    return recs, host, nread, d1


def _check_bank(lib, ns, soft, bits, rep, name):
    recs, host, nread, d1_all = _reference()
    d1 = float(d1_all[:ns].max())
    worst = 0.0
    for k in range(ns):
        w = int(rep["out_written"][k])
        assert (int(rep["in_read"][k]), w) == (nread[k], host[k].size), (name, k)
        worst = max(worst, float(np.max(np.abs(soft[k, :w].astype(np.float64) - host[k]))))
        assert not soft[k, w:].any()
        if recs[k]["mode"] == P.BPSK:
            # the fixture: no BPSK31 soft value within reach of a sign flip
            assert float(np.abs(host[k]).min()) > 1000 * d1, ("bad fixture", k, float(np.abs(host[k]).min()), d1)
            assert bits[k, :w].tobytes() == lib.Bpsk31Decider().process(host[k]).tobytes(), (name, k)
        else:
            assert not bits[k].any(), (name, k)  # no hard bits for QPSK31 pairs
            assert lib.viterbi_decode(np.ascontiguousarray(soft[k, :w])).tobytes() == lib.viterbi_decode(host[k]).tobytes()
    print(f"[parity] {name}: d1 {d1:.3e}")
    report(f"{name}: max |device soft - host soft|", worst, 2 * d1)


@pytest.mark.parametrize("ns", [1, 64, 65, 130])
def test_bank_follows_the_host_demodulators(gpu_lib, ns):
    recs = _reference()[0]
    bank = gpu_lib.Psk31DemodBank(FS, _records(gpu_lib, recs[:ns]), 2)
    soft, bits, rep = bank.process(_band())
    assert soft.shape == (ns, CAP) and bits.shape == (ns, CAP) and rep.shape == (ns,)
    _check_bank(gpu_lib, ns, soft, bits, rep, f"bank of {ns}")


def test_bank_chunked_calls_equal_one_call_and_reset(gpu_lib):
    """Calls of 1000, 1, 5000 and the rest give one call's bytes (the state, the rotator's
    included, lives on the device between calls; streams start inside the first chunk);
    after reset the bank gives them again; the listing order of the streams does not matter."""
    recs = _reference()[0]
    x = _band()
    rec = _records(gpu_lib, recs[:65])
    bank = gpu_lib.Psk31DemodBank(FS, rec, 2)
    whole, wbits, wrep = bank.process(x)
    bank.reset()
    parts = [[] for _ in range(65)]
    at = 0
    for n in (1000, 1, 5000, N):
        soft, bits, rep = bank.process(np.ascontiguousarray(x[:, at:at + n]))
        for k in range(65):
            parts[k].append(soft[k, :int(rep["out_written"][k])])
        at += n
    for k in range(65):
        w = int(wrep["out_written"][k])
        assert np.concatenate(parts[k]).tobytes() == whole[k, :w].tobytes(), k
    bank.reset()
    again, abits, arep = bank.process(x)
    assert again.tobytes() == whole.tobytes() and abits.tobytes() == wbits.tobytes() and arep.tobytes() == wrep.tobytes()
    perm = np.random.default_rng(5).permutation(65)
    psoft, pbits, prep = gpu_lib.Psk31DemodBank(FS, rec[perm], 2).process(x)
    assert psoft.tobytes() == whole[perm].tobytes() and prep.tobytes() == wrep[perm].tobytes()


def test_bank_capacity_cuts_a_call_short(gpu_lib):
    """out_cap 5: BPSK31 stops after its fifth symbol, QPSK31 with one slot left (4 values),
    as the host demodulators do; in_read says how far each came."""
    recs = [dict(_stream(k), out_cap=5) for k in (0, 1, 7, 9)]
    x = _band()
    soft, bits, rep = gpu_lib.Psk31DemodBank(FS, _records(gpu_lib, recs), 2).process(x)
    assert soft.shape == (4, 5)
    for k, r in enumerate(recs):
        cls = gpu_lib.Bpsk31Demod if r["mode"] == P.BPSK else gpu_lib.Qpsk31Demod
        want, nread = cls(FS, r["rf_hz"], r["gain"], r["offset"]).process_host(x[r["channel"], r["start"]:], 5)
        assert (int(rep["in_read"][k]), int(rep["out_written"][k])) == (nread, want.size)
        assert want.size == (5 if r["mode"] == P.BPSK else 4) and nread < N - r["start"]
        d1 = float(_reference()[3][[0, 1, 7, 9]].max())
        if r["mode"] == P.BPSK:
            assert float(np.abs(want).min()) > 1000 * d1, ("bad fixture", k, float(np.abs(want).min()), d1)
            assert bits[k, :want.size].tobytes() == gpu_lib.Bpsk31Decider().process(want).tobytes()
        else:
            assert not bits[k].any()
        assert not soft[k, want.size:].any()
        # these calls are the first symbols of streams 0, 1, 7 and 9 of the list: the same bound
        report(f"capacity 5, stream {k}: max |device soft - host soft|", float(np.max(np.abs(soft[k, :want.size] - want))),
               2 * float(_reference()[3][[0, 1, 7, 9]].max()))


def test_bank_stream_stopped_by_capacity_skips_the_rest_of_the_call(gpu_lib):
    """The documented contract, pinned over two calls: a stream stopped by out_cap is not fed
    the rest of that call again; the next call brings every stream its channel's next samples.
    So a BPSK31 stream of capacity 5 given 8 symbols and then 8 more gives what the host
    demodulator gives when it is fed the first call's in_read samples and then the second
    buffer, while a stream with room for all 16 is unaffected by its neighbour."""
    r0 = dict(_stream(0), out_cap=5)
    r1 = dict(_stream(0), out_cap=CAP)
    x = _band()
    a, b = x[:, :8 * SPS], x[:, 8 * SPS:16 * SPS]
    bank = gpu_lib.Psk31DemodBank(FS, _records(gpu_lib, [r0, r1]), 2)
    s1, _, rep1 = bank.process(np.ascontiguousarray(a))
    s2, _, rep2 = bank.process(np.ascontiguousarray(b))
    assert (int(rep1["in_read"][0]), int(rep1["out_written"][0])) == (5 * SPS, 5)
    assert (int(rep2["in_read"][0]), int(rep2["out_written"][0])) == (5 * SPS, 5)
    assert (int(rep1["out_written"][1]), int(rep2["out_written"][1])) == (8, 8)
    d = gpu_lib.Bpsk31Demod(FS, r0["rf_hz"], r0["gain"], r0["offset"])
    w1, n1 = d.process_host(a[0], 5)
    w2, n2 = d.process_host(b[0], 5)  # not a[0][n1:]: the skipped samples are gone
    assert (n1, n2) == (5 * SPS, 5 * SPS)
    # d1 for this very case: the restatement's two runs over the same two calls
    runs = []
    for rng in (None, np.random.default_rng(98)):
        r = P.DemodBank(FS, [r0, r1], perturb=rng)
        runs.append([np.concatenate(v) for v in zip(r.process(a)[0], r.process(b)[0])])
    tol = 2 * max(float(np.max(np.abs(p.astype(np.float64) - m))) for p, m in zip(*runs))
    assert runs[0][0].tobytes() == np.concatenate([w1, w2]).tobytes()  # the host layer is the restatement here too
    report("capacity then next call: max |device soft - host soft|",
           float(max(np.max(np.abs(s1[0, :5] - w1)), np.max(np.abs(s2[0, :5] - w2)))), tol)
    whole = gpu_lib.Bpsk31Demod(FS, r1["rf_hz"], r1["gain"], r1["offset"]).process_host(x[0, :16 * SPS])[0]
    report("its neighbour with room: max |device soft - host soft|",
           float(np.max(np.abs(np.concatenate([s1[1, :8], s2[1, :8]]) - whole))), tol)


def test_bank_device_tensors_and_single_stream_classes(gpu_lib):
    """Torch tensors in, torch tensors out, the host-slice call's bytes; Bpsk31Demod /
    Qpsk31Demod.process are banks of one stream, fed here in two ragged calls, and
    Qpsk31Demod.flush decodes what process returned."""
    import torch

    recs = _reference()[0]
    x = _band()
    rec = _records(gpu_lib, recs[:9])
    want = gpu_lib.Psk31DemodBank(FS, rec, 2).process(x)
    soft, bits, rep = gpu_lib.Psk31DemodBank(FS, rec, 2).process(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert soft.cpu().numpy().tobytes() == want[0].tobytes() and bits.cpu().numpy().tobytes() == want[1].tobytes()
    assert rep.cpu().numpy().tobytes() == want[2].tobytes()
    for k in (0, 1):  # stream 0 starts at sample 0 with offset 0: BPSK31 at 1000 Hz; stream 1: QPSK31 from sample 53
        r = recs[k]
        cls = gpu_lib.Bpsk31Demod if r["mode"] == P.BPSK else gpu_lib.Qpsk31Demod
        d = cls(FS, r["rf_hz"], r["gain"], r["offset"])
        row = x[r["channel"], r["start"]:]
        got = np.concatenate([d.process(row[:3001]), d.process(row[3001:])])
        assert got.tobytes() == want[0][k, :int(want[2]["out_written"][k])].tobytes()
        if r["mode"] == P.QPSK:
            assert d.flush().tobytes() == gpu_lib.viterbi_decode(got).tobytes()
            assert d.flush().size == 0


# ---- the batched Viterbi decode -----------------------------------------------------------


def _soft(n_syms, kind, k):
    bits = np.random.default_rng(1000 * n_syms + k).integers(0, 2, n_syms).astype(np.uint8)
    if kind == "zero":
        return np.zeros(2 * n_syms, np.float32)
    return P.dqpsk_soft(bits, 0.5 if kind == "noisy" else 0.0, 77 * n_syms + k)


def _batch(nstreams, n_syms, kind):
    return np.stack([_soft(n_syms, kind, k) for k in range(nstreams)])


def _host(lib, soft):
    return np.stack([lib.viterbi_decode(row) for row in soft]) if len(soft) else np.zeros((0, soft.shape[1] // 2), np.uint8)


@pytest.mark.parametrize("kind", P.VITERBI_KINDS)
@pytest.mark.parametrize("n_syms", P.VITERBI_LENGTHS)
def test_viterbi_batch_equals_the_host_decoder(gpu_lib, n_syms, kind):
    for nstreams in STREAMS:
        soft = _batch(nstreams, n_syms, kind)
        got = gpu_lib.psk31_viterbi_batch(soft)
        assert got.dtype == np.uint8 and got.shape == (nstreams, n_syms)
        assert got.tobytes() == _host(gpu_lib, soft).tobytes(), (nstreams, n_syms, kind)
    # the restatement's own bits for the first stream (cached by the CPU tests' cases)
    assert got[0].tobytes() == P.viterbi_case(n_syms, kind, 0)[1].tobytes()


@pytest.mark.parametrize("kind", P.VITERBI_KINDS)
@pytest.mark.parametrize("n_syms", GROUP_EDGE_LENGTHS)
def test_viterbi_batch_equals_the_host_decoder_at_the_group_edges(gpu_lib, n_syms, kind):
    for nstreams in STREAMS:
        soft = _batch(nstreams, n_syms, kind)
        got = gpu_lib.psk31_viterbi_batch(soft)
        assert got.dtype == np.uint8 and got.shape == (nstreams, n_syms)
        assert got.tobytes() == _host(gpu_lib, soft).tobytes(), (nstreams, n_syms, kind)


def test_viterbi_batch_is_independent_of_its_neighbours(gpu_lib):
    """A stream decodes to the same bits alone, in any slot of a wave and next to streams of
    another kind; 130 streams are 33 workgroups, the last with two live streams."""
    n_syms = 37
    soft = np.stack([_soft(n_syms, ("clean", "noisy", "zero")[k % 3], k) for k in range(130)])
    want = _host(gpu_lib, soft)
    got = gpu_lib.psk31_viterbi_batch(soft)
    assert got.tobytes() == want.tobytes()
    perm = np.random.default_rng(4).permutation(130)
    assert gpu_lib.psk31_viterbi_batch(np.ascontiguousarray(soft[perm])).tobytes() == want[perm].tobytes()
    for k in (0, 1, 129):
        assert gpu_lib.psk31_viterbi_batch(soft[k:k + 1]).tobytes() == want[k:k + 1].tobytes()


def test_viterbi_non_finite_and_huge_input_neither_faults_nor_differs(gpu_lib):
    """Outside the contract, and still the host's bits: NaN, infinities and values whose
    squares overflow, over a whole stream, in one symbol, and in the first and last ones;
    metrics that reach the start value are skipped as the reference skips them."""
    base = _soft(40, "noisy", 3)
    rows = []
    for v in (np.nan, np.inf, -np.inf, 3.0e38, 1.0e19, -1.0e19):
        for where in (slice(None), slice(10, 11), slice(0, 1), slice(78, 80)):
            row = base.copy()
            row[where] = v
            rows.append(row)
    soft = np.stack(rows)
    got = gpu_lib.psk31_viterbi_batch(soft)
    assert got.tobytes() == _host(gpu_lib, soft).tobytes()
    assert got.max() <= 1


def test_viterbi_device_tensors_equal_the_host_slices(gpu_lib):
    """The device entry on torch tensors (its scratch is a tensor the wrapper allocates) gives
    the host-slice call's bytes, and a second call on the same input the same bytes again."""
    import torch

    soft = _batch(9, 300, "noisy")
    want = gpu_lib.psk31_viterbi_batch(soft)
    d = torch.from_numpy(soft).cuda()
    a = gpu_lib.psk31_viterbi_batch(d)
    b = gpu_lib.psk31_viterbi_batch(d)
    torch.cuda.synchronize()
    assert a.dtype == torch.uint8 and a.is_cuda and tuple(a.shape) == (9, 300)
    assert a.cpu().numpy().tobytes() == want.tobytes() and b.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        gpu_lib.psk31_viterbi_batch(d[:, :599])
    with pytest.raises(ValueError):
        gpu_lib.psk31_viterbi_batch(d.double())


def test_text_through_the_code_and_back(gpu_lib):
    """Varicode -> conv_encode -> DQPSK phasors with noise -> the batched decode -> Varicode:
    three texts in one launch come back. The bits past the last character are the postamble's
    ones, so the few unprotected tail bits of the block code carry no text."""
    texts = [b"CQ CQ de TEST", b"the quick brown fox 0123456789", b"~"]
    streams = [P.text_bits(t, 8, 16) for t in texts]
    n = max(len(s) for s in streams)
    streams = [np.concatenate([s, np.ones(n - len(s), np.uint8)]) for s in streams]
    soft = np.stack([P.dqpsk_soft(s, 0.3, 50 + k) for k, s in enumerate(streams)])
    bits = gpu_lib.psk31_viterbi_batch(soft)
    for k, t in enumerate(texts):
        d = gpu_lib.VaricodeDecoder()
        d.push_bits(np.ascontiguousarray(bits[k]))
        assert d.pop_bytes() == t


# ---- the device modulator ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [P.BPSK, P.QPSK])
@pytest.mark.parametrize("fs", [8000.0, 12000.0])
def test_device_modulator_equals_the_host_modulator(gpu_lib, fs, mode):
    """k_psk31_mod: 1, 3 and 65 streams of 40 symbols (65 streams are 2.6 M samples at 12 kHz,
    many workgroups; 40 symbols at 8 kHz cross the Rotator's renormalisation ten times),
    rf_hz 0 and 1000: every stream's bytes equal the host modulator's (QPSK31's negative
    zeros included), a batch equals the single calls, device=True equals the host-returning
    call and carries the state into the next call as the host modulator does."""
    cls = gpu_lib.Bpsk31Mod if mode == P.BPSK else gpu_lib.Qpsk31Mod
    bits = np.random.default_rng(int(fs) + mode).integers(0, 2, (65, 40)).astype(np.uint8)
    for rf in (0.0, 1000.0):
        want = np.stack([cls(fs, rf, 0.7).modulate_bits(row) for row in bits])
        for ns in (1, 3, 65):
            got = cls(fs, rf, 0.7).modulate_batch(bits[:ns])
            assert got.dtype == np.complex64 and got.shape == (ns, 40 * gpu_lib.psk31_sps(fs))
            assert got.tobytes() == want[:ns].tobytes(), (fs, mode, rf, ns)
        dev = cls(fs, rf, 0.7).modulate_batch(bits[:3], device=True)
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == want[:3].tobytes()
        # one stateful stream: two calls on the device against two calls on the host
        h, d = cls(fs, rf, 0.7), cls(fs, rf, 0.7)
        for part in (bits[0, :17], bits[0, 17:], bits[1]):
            assert d.modulate_bits(part, device=True).cpu().numpy().tobytes() == h.modulate_bits(part).tobytes()
        d.set_gain(0.25), h.set_gain(0.25)
        d.reset(), h.reset()
        assert d.modulate_text(b"hi", 3, 2, device=True).cpu().numpy().tobytes() == h.modulate_text(b"hi", 3, 2).tobytes()
    assert cls(fs, 0.0, 1.0).modulate_batch(np.zeros((0, 4), np.uint8)).shape == (0, 4 * gpu_lib.psk31_sps(fs))
    with pytest.raises(ValueError):
        cls(fs, 0.0, 1.0).modulate_batch(bits[0])


# ---- band synthesis ----------------------------------------------------------------------------
def _d0(rf_hz, fs, length):
    """The distance between the Rotator's recurrence (restated: np_ref.rotator) and the f64
    closed form of its own f32 step (the Q0.64 angle the library states), over length outputs."""
    import orion_sdr
    from np_ref import rotator

    rec = rotator(np.ones(length, np.complex64), rf_hz, fs).astype(np.complex128)
    q = orion_sdr.psk31_rotator_q64(rf_hz, fs)
    turns = np.array([((j + 1) * q) % (1 << 64) for j in range(length)], np.float64) / 2.0 ** 64
    return float(np.max(np.abs(rec - np.exp(2j * np.pi * turns))))


def test_synth_sums_clipped_signals_within_the_closed_form_bound(gpu_lib):
    """2 channels x 3 signals of 3 symbols in n = 3 sps + 37 samples: channel 0 holds one
    signal clipped at the start (offset -300, BPSK31 at 1000 Hz) and one clipped at the end
    (offset 500, QPSK31 at 1531.25 Hz, gain -0.5) that overlap, plus a baseband one; channel 1
    one signal wholly outside and one baseband BPSK31 signal, which must be the host
    modulator's bytes (no RF stage: nothing is approximated). Against the host modulators
    placed, clipped and added in list order in f32: per sample within the sum over the
    signals of |gain| (2 d0 + 2e-6), d0 taken per signal on the CPU. The accumulate flag, a
    repeated call (bytewise stable), the table permuted within a channel (f32 addition order
    only: within 4 ulp of the largest partial sum), host slices against device tensors."""
    import torch

    n = 3 * SPS + 37
    rng = np.random.default_rng(77)
    spec = [(0, P.BPSK, -300, 1000.0, 1.0), (0, P.QPSK, 500, 1531.25, -0.5), (0, P.BPSK, 37, 0.0, 0.25),
            (1, P.BPSK, n + 10, 1000.0, 1.0), (1, P.BPSK, 100, 0.0, 0.7), (1, P.QPSK, -10 * SPS, 500.0, 1.0)]
    bits = [rng.integers(0, 2, 3).astype(np.uint8) for _ in spec]
    sig = np.zeros(len(spec), gpu_lib.PSK31_SIGNAL_DTYPE)
    for k, (ch, mode, off, rf, gain) in enumerate(spec):
        sig[k] = (ch, mode, off, rf, gain, 0)
    want = np.zeros((2, n), np.complex64)
    bound = np.zeros((2, n))
    for (ch, mode, off, rf, gain), b in zip(spec, bits):
        cls = gpu_lib.Bpsk31Mod if mode == P.BPSK else gpu_lib.Qpsk31Mod
        s = cls(FS, rf, gain).modulate_bits(b)
        lo, hi = max(off, 0), min(off + s.size, n)
        if lo < hi:
            want[ch, lo:hi] = want[ch, lo:hi] + s[lo - off:hi - off]  # complex64: one f32 add per component
            if rf != 0.0:
                bound[ch, lo:hi] += abs(gain) * (2 * _d0(rf, FS, s.size) + 2e-6)
    got = gpu_lib.psk31_synth(sig, bits, n, nch=2, fs=FS)
    assert got.dtype == np.complex64 and got.shape == (2, n)
    assert got[1].tobytes() == want[1].tobytes()  # baseband only: exact
    err = np.abs(got.astype(np.complex128) - want)
    assert np.all(err[bound == 0] == 0)
    k = int(np.argmax(err))  # the largest error and the bound of that very sample
    report("synth: largest |device - host sum|, with its sample's bound", float(err.flat[k]), float(bound.flat[k]))
    assert np.all(err <= bound)
    assert gpu_lib.psk31_synth(sig, bits, n, nch=2, fs=FS).tobytes() == got.tobytes()
    dev = gpu_lib.psk31_synth(sig, bits, n, nch=2, fs=FS, device=True)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == got.tobytes()
    # accumulate: onto a ramp, and twice the band
    ramp = (np.arange(2 * n, dtype=np.float32).reshape(2, n) * np.float32(0.001)).astype(np.complex64)
    acc = gpu_lib.psk31_synth(sig, bits, n, nch=2, fs=FS, out=ramp.copy(), accumulate=True)
    assert acc[1].tobytes() == (ramp[1] + want[1]).astype(np.complex64).tobytes()
    over = gpu_lib.psk31_synth(sig, bits, n, nch=2, fs=FS, out=ramp.copy(), accumulate=False)
    assert over.tobytes() == got.tobytes()
    # the table permuted within channel 0: f32 addition order only
    perm = [2, 0, 1, 3, 4, 5]
    other = gpu_lib.psk31_synth(sig[perm], [bits[k] for k in perm], n, nch=2, fs=FS)
    assert other[1].tobytes() == got[1].tobytes()
    assert float(np.max(np.abs(other[0] - got[0]))) <= 4 * np.finfo(np.float32).eps * 1.75
    with pytest.raises(ValueError):
        bad = sig.copy()
        bad["channel"][0] = 2
        gpu_lib.psk31_synth(bad, bits, n, nch=2, fs=FS)
    with pytest.raises(ValueError):
        gpu_lib.psk31_synth(sig, bits[:3], n, nch=2, fs=FS)


def test_synth_plans_and_modulator_batches_queued_back_to_back_on_one_stream(gpu_lib):
    """Two psk31_synth plans (one signal of 2 bits; three signals on 2 channels) and two
    batches of one modulator handle (2 streams of 3 symbols, 3 streams of 5) queued on one
    non-default stream with nothing between them, read back after a single synchronise: every
    plan is uploaded for its own launch, so each output has the bytes of the same call made
    alone (a fresh modulator for each batch). This pins the results, not the ordering: plans
    of a few hundred bytes are copied long before the next call rewrites the pinned space, so
    the test would rarely fail if a call did not wait for the previous one."""
    import torch

    rng = np.random.default_rng(31)
    n = 4 * SPS + 5
    spec = [[(0, P.BPSK, 10, 1000.0, 1.0, 2)],
            [(0, P.QPSK, -100, 1531.25, -0.5, 3), (1, P.BPSK, 300, 0.0, 0.7, 4), (0, P.BPSK, 37, 500.0, 0.25, 1)]]
    plans = []
    for rows in spec:
        sig = np.zeros(len(rows), gpu_lib.PSK31_SIGNAL_DTYPE)
        for k, (ch, mode, off, rf, gain, _) in enumerate(rows):
            sig[k] = (ch, mode, off, rf, gain, 0)
        plans.append((sig, [rng.integers(0, 2, r[5]).astype(np.uint8) for r in rows], 1 + max(r[0] for r in rows)))
    batches = [rng.integers(0, 2, shape).astype(np.uint8) for shape in ((2, 3), (3, 5))]
    alone = [gpu_lib.psk31_synth(sig, bits, n, nch=nch, fs=FS, device=True).cpu().numpy() for sig, bits, nch in plans]
    alone += [gpu_lib.Qpsk31Mod(FS, 1000.0, 0.7).modulate_batch(b, device=True).cpu().numpy() for b in batches]
    mod = gpu_lib.Qpsk31Mod(FS, 1000.0, 0.7)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = [gpu_lib.psk31_synth(sig, bits, n, nch=nch, fs=FS, device=True) for sig, bits, nch in plans]
        got += [mod.modulate_batch(b, device=True) for b in batches]
    torch.cuda.synchronize()
    for g, want in zip(got, alone):
        assert g.cpu().numpy().tobytes() == want.tobytes()


# ---- psk31_sync, the band browser and Psk31Stream ---------------------------------------------
def _embed(iq, total):
    buf = np.zeros(total, np.complex64)
    buf[:min(len(iq), total)] = iq[:total]
    return buf


def _sync_equals_the_host_search(lib, x, base_hz, max_hz, min_run, margin, n_bits, max_cand):
    """psk31_sync_batch (the device search, k_psk31_medians / _floor / _runs / _merge, inside
    orion_psk31_sync) against the restated search run on the device's own waterfall (its
    log differs from glibc's by up to 4 * 2^-23, DESIGN.md 3.3, so the waterfall is the
    device's): the list, the order and the scores' bytes; each carrier_hz the two-rounding
    f32 sum."""
    got = lib.psk31_sync_batch(x, FS, base_hz, max_hz, min_run, margin, n_bits, max_cand)
    num_bins = int(np.ceil(np.float32(max(max_hz - base_hz, 0.0)) / np.float32(31.25))) + 1
    wf = lib.compute_waterfall(x, FS, base_hz, 31.25, SPS, x.shape[1] // SPS, num_bins, 0)
    assert wf.shape == (x.shape[0], x.shape[1] // SPS, num_bins)
    for ch in range(x.shape[0]):
        want = P.find_carriers(wf[ch], min_run, margin, max_cand)
        assert [(c["time_sym"], c["freq_bin"], np.float32(c["score"]).tobytes()) for c in got[ch]] == \
            [(t, b, sc.tobytes()) for t, b, sc in want], ch
        for c in got[ch]:
            assert c["carrier_hz"] == float(np.float32(base_hz) + np.float32(c["freq_bin"]) * np.float32(31.25))
            assert c["soft_bits"].dtype == np.float32 and c["soft_bits"].size <= n_bits
    return got


def _soft_bits_follow_the_host(lib, row, cands, n_bits, name):
    """Each candidate's soft bits against the host demodulator started as record_candidate
    starts it, within 2 d1 (the restatement's two runs of the same streams); hard bits equal
    where the fixture check holds (it must hold for every value)."""
    recs = [P.stream_record(P.BPSK, 0, c["carrier_hz"], 1.0, c["time_sym"] * SPS, 0, n_bits + 2) for c in cands]
    runs = [P.DemodBank(FS, recs, perturb=rng).process(row[None, :])[0] for rng in (None, np.random.default_rng(97))]
    d1 = max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(*runs))
    worst = 0.0
    for c, plain in zip(cands, runs[0]):
        host, _ = lib.Bpsk31Demod(FS, c["carrier_hz"], 1.0).process_host(row[c["time_sym"] * SPS:], n_bits + 2)
        host = host[:n_bits]
        assert host.tobytes() == plain[:n_bits].tobytes() and c["soft_bits"].size == host.size
        assert float(np.abs(host).min()) > 1000 * d1, ("bad fixture", c["freq_bin"], float(np.abs(host).min()), d1)
        assert np.array_equal(c["soft_bits"] >= 0, host >= 0)
        worst = max(worst, float(np.max(np.abs(c["soft_bits"].astype(np.float64) - host))))
    print(f"[parity] {name}: d1 {d1:.3e}")
    report(f"{name}: max |candidate soft bits - host|", worst, 2 * d1)


@pytest.mark.parametrize("mode,base_hz,bin_,text", [("bpsk", 900.0, 3, b"CQ CQ"), ("qpsk", 1400.0, 2, b"TEST")])
def test_sync_finds_the_carrier_in_a_4_s_buffer(gpu_lib, mode, base_hz, bin_, text):
    """roundtrip_psk31_sync_finds_bpsk31 and its QPSK31 twin (tests/roundtrip/psk31.rs): fs
    8000, the carrier on a bin, 64 / 32 preamble / postamble bits, a 4 s buffer, psk31_sync(..,
    4, 3.0, 256, 5): a candidate, the best within 40 Hz of the carrier. 8 bins."""
    carrier = base_hz + bin_ * 31.25
    cls = gpu_lib.Bpsk31Mod if mode == "bpsk" else gpu_lib.Qpsk31Mod
    x = _embed(cls(FS, carrier, 1.0).modulate_text(text, 64, 32), 32000)[None, :]
    got = _sync_equals_the_host_search(gpu_lib, x, base_hz, base_hz + 200.0, 4, 3.0, 256, 5)[0]
    assert got and abs(got[0]["carrier_hz"] - carrier) < 40.0
    one = gpu_lib.psk31_sync(x[0], FS, base_hz, base_hz + 200.0, 4, 3.0, 256, 5)
    assert [c["soft_bits"].tobytes() for c in one] == [c["soft_bits"].tobytes() for c in got]
    assert gpu_lib.best_psk31_sync(got, carrier)["score"] == max(c["score"] for c in got if abs(c["carrier_hz"] - carrier) <= 62.5)
    if mode == "bpsk":
        assert any(gpu_lib._varicode_text(c["soft_bits"] >= 0) == text.decode() for c in got)


BAND = ((625.0, b"CQ CQ de K1ABC"), (1125.0, b"hello world 599"), (1750.0, b"TEST de orion"), (2500.0, b"73"),
        (2843.75, b"qrz?"))


@functools.lru_cache(maxsize=None)
def _browser_band(nch):
    """nch channels of 3 s: the five BPSK31 carriers of BAND (the channel's share of them,
    from sample 0, amplitude 1) plus Gaussian noise of deviation 0.05 per component."""
    import orion_sdr

    rng = np.random.default_rng(40 + nch)
    n = 3 * 8000
    x = np.zeros((nch, n), np.complex64)
    for k, (car, text) in enumerate(BAND):
        s = orion_sdr.Bpsk31Mod(FS, car, 1.0).modulate_text(text, 64, 32)
        x[k % nch, :min(n, len(s))] += s[:n]
    noise = rng.normal(0.0, 0.05, x.shape + (2,)).astype(np.float32)
    return (x + noise.view(np.complex64)[..., 0]).astype(np.complex64)


@pytest.mark.parametrize("nch", [1, 3])
def test_sync_over_97_bins(gpu_lib, nch):
    """0-3000 Hz (97 bins, past one wave of the waterfall kernel), 1 and 3 channels: the list
    equals the host search on the device's waterfall; every carrier sent has a candidate
    within one bin in its channel; the first channel's candidates' soft bits (30 each) follow
    the host demodulator."""
    x = _browser_band(nch)
    got = _sync_equals_the_host_search(gpu_lib, x, 0.0, 3000.0, 8, 6.0, 30, 10)
    for k, (car, _) in enumerate(BAND):
        assert any(abs(c["carrier_hz"] - car) <= 31.25 for c in got[k % nch]), car
    _soft_bits_follow_the_host(gpu_lib, x[0], got[0][:4], 30, f"sync, {nch} channel(s)")


SENT = ((625.0, 4, b"CQ K1ABC"), (1125.0, 20, b"hello 599"), (1750.0, 40, b"TEST 73"))


def _restated_text(bits):
    d = P.VaricodeDecoder()
    for b in list(bits) + [0, 0]:
        d.push_bit(int(b))
    return "".join(chr(c) for c in d.pop_bytes() if 0x20 <= c < 0x7F)


def test_decode_returns_each_text_at_its_carrier(gpu_lib):
    """psk31_decode on one channel of three BPSK31 carriers (625, 1125 and 1750 Hz, bins 4, 20
    and 40 of a search from 500 Hz: "CQ K1ABC", "hello 599", "TEST 73", from sample 0, 16 / 16
    preamble / postamble bits, 4 s) plus Gaussian noise of deviation 0.05 per component (power
    0.005). At that power the restatement alone (np_ref_psk31's modulator, demodulator and
    Varicode decoder, at the known carriers) decodes all three; the test checks that first.
    Where a text comes back is the reference's search's doing: while a carrier is keyed its
    energy peaks in the two neighbouring bins (its own bin is a local maximum only in the
    unmodulated postamble), so each text is found, from symbol 0, in exactly the bins one
    below and one above its carrier's, 31.25 Hz off (the reference's own round trip allows
    40 Hz), and the carrier's own bin holds a late run with no text. A text is followed by
    what the idle carrier and the noise after it decode to, so texts are compared at their
    start."""
    rng = np.random.default_rng(5)
    n = 4 * 8000
    x = np.zeros(n, np.complex64)
    for car, _, text in SENT:
        s = P.Mod(P.BPSK, FS, car, 1.0).modulate_bits(P.text_bits(text, 16, 16))
        x[:len(s)] += s
    x = (x + rng.normal(0.0, 0.05, (n, 2)).astype(np.float32).view(np.complex64)[:, 0]).astype(np.complex64)
    soft = P.DemodBank(FS, [P.stream_record(P.BPSK, 0, car, 1.0) for car, _, _ in SENT]).process(x[None, :])[0]
    for (car, _, text), sb in zip(SENT, soft):
        assert _restated_text(sb >= 0).startswith(text.decode()), ("bad fixture", car)
    got = gpu_lib.psk31_decode(x, FS, 500.0, 2000.0)
    assert got == gpu_lib.psk31_decode_batch(x[None, :], FS, 500.0, 2000.0)[0]
    assert all(set(c) == {"carrier_hz", "score", "time_sym", "text"} for c in got)
    for car, bin_, text in SENT:
        where = sorted(round((c["carrier_hz"] - 500.0) / 31.25) for c in got if c["text"].startswith(text.decode()))
        assert where == [bin_ - 1, bin_ + 1], (car, where, got)
        assert all(c["time_sym"] == 0 for c in got if c["text"].startswith(text.decode()))
        own = [c for c in got if c["carrier_hz"] == car]
        assert own and all(c["time_sym"] > 60 and not c["text"].startswith(text.decode()) for c in own)


def _search_cases():
    """Hand-made log waterfalls (channel, symbols, bins): the CPU suite's tie and edge cases
    and seeded waterfalls drawn from five levels, so equal energies, equal scores and equal
    medians are the rule; odd and even counts; one bin; one symbol."""
    low, high = np.float32(-27.6), np.float32(-2.0)
    a = np.full((3, 60, 9), low, np.float32)
    for b, t0, t1, v in [(5, 20, 30, high), (1, 20, 30, high), (1, 0, 10, high), (3, 5, 15, high + 2)]:
        a[0, t0:t1, b] = v
    a[1, 50:, 8] = high    # to the end of the buffer, last bin
    a[2, 10:17, 4] = high  # one short of min_run 8
    cases = [(a, 8, 6.0, 10), (a, 8, 6.0, 3), (a, 8, 6.0, 1)]
    plateau = np.full((1, 30, 6), low, np.float32)
    plateau[0, 5:17, 2:4] = high
    constant = np.full((1, 24, 9), low, np.float32)
    constant[0, :, 4] = high
    half = np.full((1, 24, 5), low, np.float32)
    half[0, 12:, 2] = high
    cases += [(plateau, 8, 6.0, 10), (constant, 8, 6.0, 10), (half, 8, 6.0, 10)]
    rng = np.random.default_rng(12)
    levels = np.array([-20.0, -19.5, 0.0, 0.5, 1.0], np.float32)
    for shape in [(2, 23, 8), (2, 24, 9), (1, 37, 1), (3, 1, 5), (1, 64, 70), (5, 40, 3)]:
        cases.append((rng.choice(levels, size=shape).astype(np.float32), 2, 3.0, 4))
        cases.append((rng.choice(levels, size=shape).astype(np.float32), 0, 6.0, 64))
    return cases


def _cand_tuples(c):
    return [(int(v["time_sym"]), int(v["freq_bin"]), np.float32(v["score"]).tobytes()) for v in c]


def test_device_search_equals_the_host_search_on_hand_made_waterfalls(gpu_lib):
    """k_psk31_medians / _floor / _runs / _merge (orion_psk31_find_carriers and _device)
    against the host search (psk31.cpp, held to the restatement by the CPU suite): the list,
    its order (score, then freq_bin, then time_sym) and the scores' bytes, for host slices
    and for device tensors; a repeated call gives the same bytes."""
    import torch

    for wf, min_run, margin, max_cand in _search_cases():
        want = gpu_lib.psk31_find_carriers(wf, min_run, margin, max_cand)
        got = gpu_lib.psk31_find_carriers_device(wf, min_run, margin, max_cand)
        dev = gpu_lib.psk31_find_carriers_device(torch.from_numpy(wf).cuda(), min_run, margin, max_cand)
        again = gpu_lib.psk31_find_carriers_device(wf, min_run, margin, max_cand)
        for ch in range(wf.shape[0]):
            assert _cand_tuples(got[ch]) == _cand_tuples(want[ch]), (wf.shape, ch, max_cand)
            assert _cand_tuples(dev[ch]) == _cand_tuples(want[ch]) and _cand_tuples(again[ch]) == _cand_tuples(want[ch])
    a = _search_cases()[0][0]
    got = gpu_lib.psk31_find_carriers_device(a, 8, 6.0, 10)
    assert [(t, b) for t, b, _ in _cand_tuples(got[0])] == [(5, 3), (0, 1), (20, 1), (20, 5)]
    assert [(t, b) for t, b, _ in _cand_tuples(got[1])] == [(50, 8)] and len(got[2]) == 0
    one = gpu_lib.psk31_find_carriers_device(a[0], 8, 6.0, 10)
    assert _cand_tuples(one) == _cand_tuples(got[0])
    with pytest.raises(ValueError):
        gpu_lib.psk31_find_carriers_device(a, 8, 6.0, 0)
    with pytest.raises(ValueError):
        gpu_lib.psk31_find_carriers_device(a.astype(np.float64), 8, 6.0, 4)


def test_sync_on_device_tensors_equals_the_host_slices(gpu_lib):
    """psk31_sync_batch on a torch CUDA tensor (nothing is uploaded, no stage returns to the
    host) gives the host-slice call's candidates and soft bits, byte for byte."""
    import torch

    x = _browser_band(3)
    want = gpu_lib.psk31_sync_batch(x, FS, 0.0, 3000.0, 8, 6.0, 40, 10)
    got = gpu_lib.psk31_sync_batch(torch.from_numpy(x).cuda(), FS, 0.0, 3000.0, 8, 6.0, 40, 10)
    assert [[(c["time_sym"], c["freq_bin"], c["score"], c["soft_bits"].tobytes()) for c in ch] for ch in got] == \
        [[(c["time_sym"], c["freq_bin"], c["score"], c["soft_bits"].tobytes()) for c in ch] for ch in want]
    assert sum(len(ch) for ch in got) >= 5


def test_stream_qpsk_in_ragged_chunks_returns_the_host_text(gpu_lib):
    """Psk31Stream("qpsk") on the device (a bank of one stream, the streaming Viterbi decoder
    and Varicode on the host) fed in ragged chunks gives the text the host stream gives."""
    iq = gpu_lib.Qpsk31Mod(FS, 1000.0, 1.0).modulate_text(b"TEST de orion 599", 32, 40)
    dev, host = gpu_lib.Psk31Stream("qpsk", FS, 1000.0), gpu_lib.Psk31Stream("qpsk", FS, 1000.0, device=False)
    got = want = ""
    at = 0
    for n in (1000, 1, 5000, 777, iq.size):
        got += dev.feed(iq[at:at + n])
        want += host.feed(iq[at:at + n])
        at += n
    got, want = got + dev.flush(), want + host.flush()
    assert got == want == "TEST de orion 599"
    b = gpu_lib.Psk31Stream("bpsk", FS, 1000.0)
    iq = gpu_lib.Bpsk31Mod(FS, 1000.0, 1.0).modulate_text(b"CQ CQ", 32, 32)
    assert b.feed(iq[:4097]) + b.feed(iq[4097:]) + b.flush() == "CQ CQ"
