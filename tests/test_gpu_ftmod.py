"""GPU: the FT8 / FT4 modulators, the slot synthesiser and the hard demodulators
(csrc/k_ftmod.hip) against the library's host functions (csrc/ftmod.cpp, held to
tests/np_ref_ftmod.py bit for bit by tests/test_ftmod_oracle.py) and the restatement.

Modulator: the device generates the closed form of the reference's f32 tone steps, so it
is held to the reference's recurrence at a bound taken per case on the CPU: d0 = max |dz|
between the recurrence and the f64 closed form of the restatement's own Q-steps, and the
device may be 2 d0 + 2e-6 away (times |g|; for a sum of signals, times each |g_j| and
summed). Demodulator: energies and tones bit for bit.

End to end: an encoded frame (payload bits from default_rng(7)) synthesised on the device
2 symbols late and 5 bins above 1000 Hz in a slot of T_MAX + total symbols, plus complex
Gaussian noise from default_rng(11) generated on the host and added on the device. The
noise powers were chosen on the CPU beforehand: with the restated recurrence frame plus
that noise, the restatement's own sync (np_ref_sync.sync) finds the frame as its top
candidate with 0 hard errors at
  FT8  power 150,   FT4  power 40
(the powers tests/test_gpu_ldpc.py uses for its table-lookup frames)."""
import functools

import numpy as np
import pytest

import np_ref_ftmod as F
import np_ref_ldpc as R
import np_ref_sync as S
from conftest import report

pytestmark = pytest.mark.gpu

FS = 12000.0
PROTOCOLS = ("ft8", "ft4")
BASES = (1000.0, 1531.25)
E2E_POWER = {"ft8": 150.0, "ft4": 40.0}


def _cls(lib, protocol, kind):
    return getattr(lib, f"Ft{protocol[2]}{kind}")


def _data(protocol, seed=None):
    return F.frame_data(F.MODES[protocol], (8 if protocol == "ft8" else 4) if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _d0(protocol, base, seed=None):
    """max |dz| between the reference's recurrence (the library's host modulator at gain 1,
    rf 0) and the f64 closed form of the restatement's Q-steps, for this case."""
    import orion_sdr

    mode = F.MODES[protocol]
    data = _data(protocol, seed)
    rec = _cls(orion_sdr, protocol, "Mod")(FS, base, 0.0, 1.0).modulate_host(data)
    return F.d0(rec, F.closed_form(mode, FS, base, data))


def _maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.complex128) - np.asarray(b, np.complex128))))


# ---- 1. the modulator's bound ---------------------------------------------------------------
@pytest.mark.parametrize("gain,rf", [(1.0, 0.0), (0.25, 0.0), (1.0, 1500.0)])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_modulator_within_the_closed_form_bound(gpu_lib, protocol, base, gain, rf):
    mode = F.MODES[protocol]
    data = _data(protocol)
    mod = _cls(gpu_lib, protocol, "Mod")(FS, base, rf, gain)
    want = mod.modulate_host(data)  # the reference's recurrence
    got = mod.modulate(data)
    assert got.dtype == np.complex64 and got.shape == (F.frame_len(mode),)
    d0 = _d0(protocol, base)
    print(f"[parity] {protocol} base {base} gain {gain} rf {rf}: d0 {d0:.3e}")
    report(f"{protocol} modulate base {base} gain {gain} rf {rf} max|dz|", _maxabs(got, want), abs(gain) * (2 * d0 + 2e-6))


# ---- 2. frame batch sizes, entry points ----------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_batches_equal_single_calls_and_entry_points_agree(gpu_lib, protocol):
    mode = F.MODES[protocol]
    for rf in (0.0, 1500.0):
        mod = _cls(gpu_lib, protocol, "Mod")(FS, 1000.0, rf, 0.5)
        tones = np.stack([_data(protocol, s) for s in (1, 2, 3)])
        single = [mod.modulate(t) for t in tones]
        one = mod.modulate(tones[:1])
        assert one.shape == (1, F.frame_len(mode)) and one[0].tobytes() == single[0].tobytes()
        three = mod.modulate(tones)
        assert three.shape == (3, F.frame_len(mode))
        for k in range(3):
            assert three[k].tobytes() == single[k].tobytes(), k
        dev = mod.modulate(tones, device=True)
        assert dev.is_cuda and tuple(dev.shape) == (3, F.frame_len(mode))
        assert dev.cpu().numpy().tobytes() == three.tobytes()
        assert mod.modulate(tones[1], device=True).cpu().numpy().tobytes() == single[1].tobytes()


# ---- 3. slot synthesis ------------------------------------------------------------------------
def _slot_case(lib, protocol):
    """2 channels x 3 signals, n = 3 sps + 37: channel 0 holds A (starts sps + 5 samples
    before the slot) and B (starts inside, runs past the end), listed around C, whose frame
    lies wholly past the end of channel 1."""
    mode = F.MODES[protocol]
    sps = mode["sps"]
    n = 3 * sps + 37
    sig = np.zeros(3, lib.SIGNAL_DTYPE)
    sig["channel"] = [0, 1, 0]
    sig["offset"] = [-(sps + 5), n + 10, sps + 3]
    sig["base_hz"] = [1000.0, 1200.0, 1531.25]
    sig["gain"] = [1.0, 0.7, -0.5]
    tones = np.stack([_data(protocol, s) for s in (11, 12, 13)])
    return mode, n, sig, tones


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_synth_one_signal_is_modulate(gpu_lib, protocol):
    mode = F.MODES[protocol]
    data = _data(protocol)
    synth = getattr(gpu_lib, f"{protocol}_synth")
    sig = np.zeros(1, gpu_lib.SIGNAL_DTYPE)
    sig["base_hz"], sig["gain"] = 1531.25, 0.25
    want = _cls(gpu_lib, protocol, "Mod")(FS, 1531.25, 0.0, 0.25).modulate(data)
    got = synth(sig, data[None, :], F.frame_len(mode))
    assert got.shape == (1, F.frame_len(mode)) and got[0].tobytes() == want.tobytes()
    dev = synth(sig, data[None, :], F.frame_len(mode), device=True)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_synth_clipped_overlapping_signals(gpu_lib, protocol):
    mode, n, sig, tones = _slot_case(gpu_lib, protocol)
    synth = getattr(gpu_lib, f"{protocol}_synth")
    got = synth(sig, tones, n, nch=2)
    assert got.dtype == np.complex64 and got.shape == (2, n)
    # the restated frames, clipped and summed in list order with f32 adds
    want = np.zeros((2, n), np.complex64)
    tol = np.zeros(2)
    for j in range(3):
        g, off, ch = float(sig["gain"][j]), int(sig["offset"][j]), int(sig["channel"][j])
        base = float(sig["base_hz"][j])
        frame = _cls(gpu_lib, protocol, "Mod")(FS, base, 0.0, g).modulate_host(tones[j])
        lo, hi = max(off, 0), min(off + len(frame), n)
        if lo < hi:
            want[ch, lo:hi] = want[ch, lo:hi] + frame[lo - off:hi - off]
        rec1 = frame if g == 1.0 else _cls(gpu_lib, protocol, "Mod")(FS, base, 0.0, 1.0).modulate_host(tones[j])
        d0 = F.d0(rec1, F.closed_form(mode, FS, base, tones[j]))
        print(f"[parity] {protocol} signal {j}: d0 {d0:.3e}")
        tol[ch] += abs(g) * (2 * d0 + 2e-6)
    assert not got[1].any() and not want[1].any()  # channel 1: its signal lies past the end
    report(f"{protocol} synth channel 0 max|dz|", _maxabs(got[0], want[0]), tol[0])
    # a second call with the same arguments is bit-identical
    assert synth(sig, tones, n, nch=2).tobytes() == got.tobytes()
    # accumulate on a ramp: a channel without a covering signal keeps the ramp; where one
    # signal covers a sample the result is the single f32 add ramp + signal
    ramp = (np.linspace(-1.0, 1.0, 2 * n).reshape(2, n) * (1 + 0.5j)).astype(np.complex64)
    buf = ramp.copy()
    out = synth(sig, tones, n, nch=2, out=buf, accumulate=True)
    assert out is buf
    assert buf[1].tobytes() == ramp[1].tobytes()
    only_a = int(sig["offset"][2])  # B starts here
    assert buf[0, :only_a].tobytes() == (ramp[0, :only_a] + got[0, :only_a]).tobytes()
    report(f"{protocol} synth accumulate max|dz|", _maxabs(buf[0], ramp[0].astype(np.complex128) + want[0]),
           tol[0] + 3 * 2.0 ** -23)  # three f32 adds on values below 4


def test_synth_more_channels_than_one_launch_slice(gpu_lib):
    """65537 channels of 8 samples: the channels ride a grid dimension in slices of 65535, so
    channels 65535 and 65536 come from a second launch. A signal at offset 0 (-3)
    gives the first samples of its modulated frame (from its sample 3), bit for bit."""
    nch, n = 65537, 8
    data = _data("ft4")
    sig = np.zeros(4, gpu_lib.SIGNAL_DTYPE)
    sig["channel"] = [65536, 0, 65535, 65534]
    sig["offset"] = [0, -3, 0, -3]
    sig["base_hz"] = 1531.25
    sig["gain"] = [1.0, 1.0, 0.5, 0.5]
    got = gpu_lib.ft4_synth(sig, np.stack([data] * 4), n, nch=nch)
    full = {g: gpu_lib.Ft4Mod(FS, 1531.25, 0.0, g).modulate(data) for g in (1.0, 0.5)}
    want = np.zeros((nch, n), np.complex64)
    for j in range(4):
        off = -int(sig["offset"][j])
        want[int(sig["channel"][j])] = full[float(sig["gain"][j])][off:off + n]
    assert got.tobytes() == want.tobytes()


# ---- 4. the demodulator, exact -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noisy_rows(protocol):
    """3 rows of frame length + 11: restated frames plus add_awgn at power 0.5, and the
    restatement's tones and energies of each."""
    import oracle
    import orion_sdr

    mode = F.MODES[protocol]
    rows, tones, energies, datas = [], [], [], []
    for k, seed in enumerate((21, 22, 23)):
        data = _data(protocol, seed)
        frame = _cls(orion_sdr, protocol, "Mod")(FS, 1000.0, 0.0, 1.0).modulate_host(data)
        x = oracle.add_awgn(np.concatenate([frame, frame[:11]]), 0.5, 700 + k)
        t, e = F.demodulate(mode, FS, 1000.0, x)
        rows.append(x)
        tones.append(t)
        energies.append(e)
        datas.append(data)
    return np.stack(rows), np.stack(tones), np.stack(energies), np.stack(datas)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_demodulator_is_the_restatement_bit_for_bit(gpu_lib, protocol):
    import torch

    x, want_t, want_e, datas = _noisy_rows(protocol)
    assert np.array_equal(want_t, datas)
    dem = _cls(gpu_lib, protocol, "Demod")(FS, 1000.0)
    one_t, one_e = dem.demodulate(x[0]), dem.energies(x[0])
    assert one_t.dtype == np.uint8 and one_t.shape == want_t[0].shape and one_e.dtype == np.float32
    assert one_t.tolist() == want_t[0].tolist() and one_e.tobytes() == want_e[0].tobytes()
    for arr in (x, torch.from_numpy(x).cuda()):
        t, e = dem.demodulate(arr), dem.energies(arr)
        assert t.shape == want_t.shape and e.shape == want_e.shape
        assert t.tobytes() == want_t.tobytes() and e.tobytes() == want_e.tobytes()
    t1 = dem.demodulate(torch.from_numpy(x[2]).cuda())
    assert t1.tolist() == want_t[2].tolist()


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_demodulator_nan_and_zeros(gpu_lib, protocol):
    mode = F.MODES[protocol]
    x = np.array(_noisy_rows(protocol)[0][0])
    x[40 * mode["sps"] + 17] = complex(np.nan, 0.25)
    want_t, want_e = F.demodulate(mode, FS, 1000.0, x)
    dem = _cls(gpu_lib, protocol, "Demod")(FS, 1000.0)
    t, e = dem.demodulate(x), dem.energies(x)
    assert np.isnan(e[40]).all() and np.isfinite(np.delete(e, 40, axis=0)).all()
    assert e.tobytes() == want_e.tobytes() and t.tolist() == want_t.tolist()
    pos = np.flatnonzero(F.data_positions(mode) == 40)  # symbol 40: a Costas symbol of FT8, data in FT4
    if len(pos):
        assert t[pos[0]] == 0
    # every energy NaN: tone 0 everywhere; all-zero input: every energy 0, tone 0 everywhere
    for fill in (complex(np.nan, np.nan), 0.0):
        z = np.full(F.frame_len(mode), fill, np.complex64)
        assert not dem.demodulate(z).any()
    assert not dem.energies(np.zeros(F.frame_len(mode), np.complex64)).any()


# ---- 5. loopback on the device ------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_device_loopback(gpu_lib, protocol):
    codec = _cls(gpu_lib, protocol, "Codec")
    mod = _cls(gpu_lib, protocol, "Mod")(FS, 1000.0, 0.0, 1.0)
    dem = _cls(gpu_lib, protocol, "Demod")(FS, 1000.0)
    payloads = [R.frame_payload(s) for s in (7, 8, 9)]
    tones = np.stack([codec.encode(p) for p in payloads])
    iq = mod.modulate(tones, device=True)
    back = dem.demodulate(iq)
    assert back.tobytes() == tones.tobytes()
    for k, p in enumerate(payloads):
        assert dem.demodulate(iq[k]).tolist() == tones[k].tolist()
        assert codec.decode_hard(back[k]) == p


# ---- 6. end to end ------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_end_to_end_synthesised_slot_decodes(gpu_lib, protocol):
    import torch

    mode = F.MODES[protocol]
    payload = R.frame_payload(7)
    tones = _cls(gpu_lib, protocol, "Codec").encode(payload)
    n = (S.T_MAX + mode["total"]) * mode["sps"]
    sig = np.zeros(1, gpu_lib.SIGNAL_DTYPE)
    sig["offset"] = S.LATE_SYMS * mode["sps"]
    sig["base_hz"] = np.float32(S.BASE_HZ) + np.float32(S.UP_BINS) * mode["spacing"]
    sig["gain"] = 1.0
    slot = getattr(gpu_lib, f"{protocol}_synth")(sig, tones[None, :], n, device=True)
    rng = np.random.default_rng(11)
    noise = (np.sqrt(E2E_POWER[protocol] / 2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    iq = (slot[0] + torch.from_numpy(noise).cuda()).contiguous()
    max_hz = float(np.float32(S.BASE_HZ) + np.float32(10.0) * mode["spacing"])
    out = getattr(gpu_lib, f"{protocol}_decode")(iq, S.FS, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX, S.MAX_CAND,
                                                 rule="sum_product")
    top = out["candidates"][0]
    print(f"{protocol}: first_ok {out['first_ok']}, top candidate ({top['time_sym']}, {top['freq_bin']})")
    assert out["first_ok"] >= 0 and out["payload"] == payload
    first = out["candidates"][out["first_ok"]]
    assert (first["time_sym"], first["freq_bin"]) == (S.LATE_SYMS, S.UP_BINS)


# ---- 7. interface ------------------------------------------------------------------------------
def test_interface(gpu_lib):
    import torch

    lib = gpu_lib
    assert (lib.FT8_FRAME_LEN, lib.FT4_FRAME_LEN) == (151680, 60480)
    for name in ("Ft8Mod", "Ft4Mod", "Ft8Demod", "Ft4Demod", "ft8_synth", "ft4_synth", "SIGNAL_DTYPE",
                 "FT8_FRAME_LEN", "FT4_FRAME_LEN"):
        assert name in lib.__all__
    m = lib.Ft8Mod(FS, 1000.0, 0.0, 1.0)
    data = _data("ft8")
    a, b = m.modulate(data), m.modulate(data)
    assert a is not b and not np.shares_memory(a, b) and a.tobytes() == b.tobytes()
    for bad in (np.zeros(57, np.uint8), np.zeros(58, np.int64), np.zeros((2, 59), np.uint8), [0] * 58):
        with pytest.raises(ValueError):
            m.modulate(bad)
    eight = data.copy()
    eight[3] = 8
    with pytest.raises(ValueError):
        m.modulate(eight)
    with pytest.raises(ValueError):
        lib.Ft4Mod(FS, 1000.0, 0.0, 1.0).modulate(np.full(87, 4, np.uint8), device=True)
    d = lib.Ft8Demod(FS, 1000.0)
    with pytest.raises(ValueError):
        d.demodulate(np.zeros(lib.FT8_FRAME_LEN - 1, np.complex64))
    with pytest.raises(ValueError):
        d.demodulate(torch.zeros(lib.FT8_FRAME_LEN - 1, dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        d.demodulate(np.zeros(lib.FT8_FRAME_LEN, np.complex128))
    with pytest.raises(ValueError):
        lib.Ft4Demod(FS, 1000.0).energies(np.zeros((2, lib.FT4_FRAME_LEN - 1), np.complex64))
    # more frames than a launch takes: rejected before the device is touched (a 1-byte-per-row view)
    many = np.lib.stride_tricks.as_strided(np.zeros(lib.FT4_FRAME_LEN, np.complex64), (65536, lib.FT4_FRAME_LEN), (0, 8))
    assert lib._L.orion_ft_demod_device(1, FS, 1000.0, many.ctypes.data, 65536, lib.FT4_FRAME_LEN,
                                        np.zeros(87, np.uint8).ctypes.data, None, None) == -3
    sig = np.zeros(2, lib.SIGNAL_DTYPE)
    sig["channel"] = [0, 2]
    with pytest.raises(ValueError):
        lib.ft8_synth(sig, np.zeros((2, 58), np.uint8), 100, nch=2)
    with pytest.raises(ValueError):
        lib.ft8_synth(sig[:1], np.zeros((1, 87), np.uint8), 100)
    with pytest.raises(ValueError):
        lib.ft8_synth(sig[:1], np.zeros((1, 58), np.uint8), 100, accumulate=True)
    # no signals: zeros
    assert not lib.ft4_synth(np.zeros(0, lib.SIGNAL_DTYPE), np.zeros((0, 87), np.uint8), 1000, nch=3).any()
