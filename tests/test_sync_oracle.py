"""CPU: the FT8 / FT4 sync restatement (tests/np_ref_sync.py) reproduces its committed
golden, has the properties the reference's own unit tests check (tests/unit/sync.rs:8-216),
finds the suite's test frames, and its two forms (vectorised, scalar) agree bit for bit.
No kernel is launched here; tests/test_gpu_sync.py holds the device to this restatement."""
import os
import re

import numpy as np
import pytest

import np_ref
import np_ref_sync as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sync_golden.npz"))
FS, BASE = 12_000.0, 1_000.0


def _tone(idx, n, spacing=6.25):
    """tests/unit/sync.rs:19-24: phi = TAU * f_tone * k / fs in f32, (cos, sin)."""
    f32 = np.float32
    f_tone = f32(f32(BASE) + f32(f32(idx) * f32(spacing)))
    k = np.arange(n, dtype=np.float32)
    phi = ((np_ref.TAU * f_tone) * k / f32(FS)).astype(np.float32)
    return (np.cos(phi.astype(np.float64)) + 1j * np.sin(phi.astype(np.float64))).astype(np.complex64)


def _ft8_zero_frame():
    return S.frame_samples(S.FT8, [0] * 58, 160)


def test_noise_is_np_ref_add_awgn():
    """The frames' noise comes through the C oracle's add_awgn: np_ref.add_awgn's values."""
    import oracle

    z = np.zeros(600, np.complex64)
    for seed in S.NOISE_SEED.values():
        assert np.array_equal(oracle.add_awgn(z, 0.5, seed).view(np.uint64), np_ref.add_awgn(z, 0.5, seed).view(np.uint64))


def test_restatement_reproduces_the_golden():
    mode, iq, _, max_hz = S.test_frame("ft8")
    res = S.ft8_sync(iq, S.FS, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX, S.MAX_CAND)
    num_bins, wf_syms, start, _, _ = S.sync_geometry(mode, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX)
    wf = S.compute_waterfall(iq, S.FS, S.BASE_HZ, mode["spacing"], mode["sps"], wf_syms, num_bins, start)
    assert wf.shape == (83, 19)
    assert np.array_equal(wf.view(np.uint32), GOLD["wf"].view(np.uint32))
    assert [r["time_sym"] for r in res] == GOLD["time_sym"].tolist()
    assert [r["freq_bin"] for r in res] == GOLD["freq_bin"].tolist()
    assert np.array_equal(np.array([r["score"] for r in res], np.float32).view(np.uint32), GOLD["score"].view(np.uint32))
    assert np.array_equal(np.stack([r["llr"] for r in res]).view(np.uint32), GOLD["llr"].view(np.uint32))


@pytest.mark.parametrize("tone_idx", [3, 5])
def test_waterfall_peak_bin_matches_tone_and_dominates(tone_idx):
    """sync.rs:8-82: the peak bin is the tone's and exceeds both neighbours by more than 10."""
    wf = S.compute_waterfall(_tone(tone_idx, 1920), FS, BASE, 6.25, 1920, 1, 8, 0)
    assert int(np.argmax(wf[0])) == tone_idx
    assert wf[0, tone_idx] - wf[0, tone_idx - 1] > 10.0
    assert wf[0, tone_idx] - wf[0, tone_idx + 1] > 10.0


def test_waterfall_time_offset_shifts_window():
    """sync.rs:84-121."""
    n = 1920
    buf = np.zeros(2 * n, np.complex64)
    buf[n:] = _tone(2, n)
    e_silence = S.compute_waterfall(buf, FS, BASE, 6.25, n, 1, 8, 0)[0, 2]
    wf1 = S.compute_waterfall(buf, FS, BASE, 6.25, n, 1, 8, n)
    assert wf1[0, 2] > e_silence + 10.0
    assert int(np.argmax(wf1[0])) == 2


def test_waterfall_rows_past_the_end_and_partial_rows():
    """waterfall.rs:99-109: a row starting at or past the end stays 0.0 (not ln 1e-12); a
    row the buffer ends inside uses the samples it has."""
    iq = _tone(1, 500)
    wf = S.compute_waterfall(iq, FS, BASE, 6.25, 200, 4, 3, 0)
    assert np.all(wf[3] == 0.0) and np.all(wf[:3] != 0.0)
    part = S.compute_waterfall(iq[400:], FS, BASE, 6.25, 200, 1, 3, 0)
    assert np.array_equal(wf[2].view(np.uint32), part[0].view(np.uint32))


def test_costas_score_peaks_at_correct_location():
    """sync.rs:125-167 on the restated Ft8Mod frame of all-zero data."""
    wf = S.compute_waterfall(_ft8_zero_frame(), FS, BASE, 6.25, 1920, 79, 16, 0)
    sm = S.costas_score_map(wf, S.FT8, 0, 5)
    assert sm[0, 0] > sm[0, 4] and sm[0, 0] > sm[5, 0]


def test_find_candidates_top_hit_at_correct_location():
    """sync.rs:171-216."""
    wf = S.compute_waterfall(_ft8_zero_frame(), FS, BASE, 6.25, 1920, 79, 16, 0)
    cands = S.find_candidates(wf, S.FT8, 0, 0, 5)
    assert cands and cands[0][:2] == (0, 0)


def test_top_n_is_the_reference_order_not_the_naive_one():
    """costas.rs:144-173 among equal scores: the keep-N scan with stable re-sorts is not
    (score descending, scan order ascending) — on integer-valued waterfalls it differs."""
    differs = 0
    for seed in range(6):
        wf = np.random.default_rng(seed).integers(0, 4, (85, 24)).astype(np.float32)
        sm = S.costas_score_map(wf, S.FT8, 0, 6)
        got = [(t, fb, float(s)) for t, fb, s in S.top_n(sm, 0, 5)]
        flat = [(i // sm.shape[1], i % sm.shape[1], float(v)) for i, v in enumerate(sm.ravel())]
        differs += got != sorted(flat, key=lambda c: -c[2])[:5]
        assert sorted(s for _, _, s in got) == sorted(c[2] for c in sorted(flat, key=lambda c: -c[2])[:5])
    assert differs == 6


@pytest.mark.parametrize("name", ["ft8", "ft4"])
def test_sync_finds_the_frame_and_its_bits(name):
    """A frame two symbols late and five bins up at noise power 0.5: the true location
    comes first, well clear of the runner-up, and the LLR signs are the transmitted bits
    through the Gray map (LLR > 0: bit 0)."""
    mode, iq, data, max_hz = S.test_frame(name)
    res = S.sync(iq, mode, S.FS, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX, S.MAX_CAND)
    assert len(res) == S.MAX_CAND
    assert (res[0]["time_sym"], res[0]["freq_bin"]) == (S.LATE_SYMS, S.UP_BINS)
    print(f"[sync] {name}: score {res[0]['score']:.2f}, runner-up {res[1]['score']:.2f}")
    assert res[0]["score"] > 2.0 * res[1]["score"]
    assert np.array_equal((res[0]["llr"] < 0).astype(np.int64), S.data_bits(mode, data))
    assert abs(float(np.mean(res[0]["llr"].astype(np.float64) ** 2)) - 24.0) < 1e-3


def test_sync_negative_t_min_reports_buffer_relative_time():
    """ft8_sync.rs:108-115, :151: with t_min < 0 the waterfall starts at sample 0 and the
    returned time_sym is relative to the buffer (candidate row minus -t_min)."""
    mode, iq, _, max_hz = S.test_frame("ft4")
    res = S.sync(iq, mode, S.FS, S.BASE_HZ, max_hz, -2, 2, 3)
    assert S.sync_geometry(mode, S.BASE_HZ, max_hz, -2, 2) == (16, 109, 0, 2, 4)
    assert (res[0]["time_sym"], res[0]["freq_bin"]) == (S.LATE_SYMS - 2, S.UP_BINS)


def test_scalar_restatement_agrees_bit_for_bit():
    """The project's rule of two restatements: plain scalar Python goertzel_energy and
    costas_score against the vectorised forms on a tiny geometry (partial last row,
    time offset, negative time_sym, bins past the last column)."""
    _, iq, _, _ = S.test_frame("ft4")
    iq = iq[1000:1000 + 3 * 50 + 27]
    e, present = S.waterfall_energy(iq, FS, BASE, 20.833334, 50, 5, 4, 7)
    assert present.tolist() == [True, True, True, True, False]
    wr, wi = S.steps(FS, BASE, 20.833334, 4)
    for r in range(5):
        for k in range(4):
            seg = iq[7 + r * 50:7 + (r + 1) * 50]
            assert S.goertzel_energy_scalar(seg, (wr[k], wi[k])).tobytes() == e[r, k].tobytes(), (r, k)
    rng = np.random.default_rng(3)
    for mode, shape in ((S.FT8, (81, 11)), (S.FT4, (107, 7))):
        wf = rng.normal(0, 3, shape).astype(np.float32)
        sm = S.costas_score_map(wf, mode, -3, 4)
        for t in range(-3, 5):
            for fb in range(sm.shape[1]):
                ref = S.costas_score_scalar(wf, mode["costas"], mode["pos"], t, fb)
                assert ref.tobytes() == sm[t + 3, fb].tobytes(), (mode["name"], t, fb)


def test_llr_missing_symbols_and_zero_variance():
    """ft8_sync.rs:181-185: data symbols outside the waterfall leave zeros;
    ft8_sync.rs:239: an all-zero vector is not scaled."""
    wf = np.random.default_rng(1).normal(0, 2, (83, 19)).astype(np.float32)
    llr = S.extract_llr(wf, S.FT8, 26, 3)  # frame symbols 57.. fall off the 83 rows
    assert np.all(llr[3 * 29 + 3 * 14:] == 0.0) and np.all(llr[:3 * 29 + 3 * 14] != 0.0)
    flat = S.normalise_llr(S.extract_llr(np.full((83, 19), 2.5, np.float32), S.FT8, 0, 0))
    assert np.all(flat == 0.0)


def test_header_declares_the_sync_entries():
    src = open(os.path.join(ROOT, "include", "orion_sdr_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(orion_[a-z0-9_]+)\s*\(", src))
    want = {"orion_sync_new", "orion_sync_free", "orion_waterfall_compute", "orion_waterfall_compute_device",
            "orion_costas_find_candidates_device", "orion_sync_llr_device", "orion_ft8_sync", "orion_ft8_sync_device",
            "orion_ft4_sync", "orion_ft4_sync_device", "orion_sync_geometry"}
    assert want <= names, want - names


def test_host_geometry_matches_the_restatement():
    """orion_sync_geometry (host only) restates ft8_sync.rs:99-131 as np_ref_sync does."""
    import orion_sdr

    for pat, mode in (("ft8", S.FT8), ("ft4", S.FT4)):
        for a in [(1000.0, 1062.5, 0, 4), (0.0, 3000.0, -2, 12), (1000.0, 900.0, 3, 3), (1000.0, 1208.3334, -5, -3),
                  (200.0, 2999.9, 0, 0)]:
            assert orion_sdr.sync_geometry(pat, *a) == S.sync_geometry(mode, *a), (pat, a)


def test_max_cand_zero_is_an_argument_error():
    """costas.rs:159 indexes an empty heap when max_candidates == 0: ORION_E_ARG here,
    before any device work."""
    import orion_sdr

    with pytest.raises(orion_sdr.OrionError, match="error -3"):
        orion_sdr.SyncEngine().sync_raw("ft8", np.zeros(100, np.complex64), 12e3, 1e3, 1.1e3, 0, 0, 0)
