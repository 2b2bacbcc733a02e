"""GPU: the FT8 / FT4 sync kernels (csrc/k_sync.hip) against tests/np_ref_sync.py.

Energies, Costas scores, candidate lists (ties included) and LLRs are held to the
restatement bit for bit; only the waterfall's ln() has a tolerance (device logf against
host libm logf). The restatement's values are computed once per geometry and shared."""
import functools

import numpy as np
import pytest

import np_ref_sync as S

pytestmark = pytest.mark.gpu

FS, BASE = 12_000.0, 1_000.0
# (samples_per_sym, num_syms, num_tones, time_offset, n, spacing, nch)
GEOMS = [
    (1920, 1, 8, 0, 1920, 6.25, 1),
    (1920, 5, 19, 0, 4 * 1920 + 700, 6.25, 1),     # partial last row
    (1920, 6, 19, 1920, 4 * 1920, 6.25, 1),        # rows past the end: exactly 0.0 in log mode
    (576, 7, 65, 3, 4000, 20.833334, 1),
    (577, 3, 1, 0, 2000, 20.833334, 1),            # sps not a multiple of 4, one tone
    (1920, 83, 130, 0, 158140, 6.25, 3),           # three channels holding different data
]
BIG = len(GEOMS) - 1


@functools.lru_cache(maxsize=None)
def _input(gi):
    """A frame plus AWGN (the suite's FT8 / FT4 search buffers), cut to the geometry; the
    channels of a batched case are different stretches and scalings of it."""
    sps, _, _, _, n, _, nch = GEOMS[gi]
    _, iq, _, _ = S.test_frame("ft8" if sps == 1920 else "ft4")
    x = np.empty((nch, n), np.complex64)
    for ch in range(nch):
        seg = np.roll(iq, -777 * ch)[:n]
        x[ch] = seg if ch == 0 else (seg * np.complex64(complex(0.5 + ch, -0.25 * ch))).astype(np.complex64)
    return x


@functools.lru_cache(maxsize=None)
def _ref(gi):
    """(energy, log waterfall) of every channel, from the restatement."""
    sps, ns, nt, off, n, spacing, nch = GEOMS[gi]
    x = _input(gi)
    e = np.empty((nch, ns, nt), np.float32)
    mag = np.empty((nch, ns, nt), np.float32)
    for ch in range(nch):
        e[ch], present = S.waterfall_energy(x[ch], FS, BASE, spacing, sps, ns, nt, off)
        mag[ch] = S._vlogf(e[ch] + np.float32(1e-12))
        mag[ch][~present, :] = 0.0
    return e, mag


@functools.lru_cache(maxsize=None)
def _dev_wf(gi, mode):
    import orion_sdr

    sps, ns, nt, off, n, spacing, nch = GEOMS[gi]
    x = _input(gi)
    return orion_sdr.SyncEngine().compute_waterfall(x if nch > 1 else x[0], FS, BASE, spacing, sps, ns, nt, off, mode)


def _cands(rec):
    return [(int(r["time_sym"]), int(r["freq_bin"]), np.float32(r["score"]).tobytes()) for r in rec]


def _ref_cands(wf, mode, t_min, t_max, n):
    return [(int(t), int(fb), np.float32(s).tobytes()) for t, fb, s in S.find_candidates(wf, mode, t_min, t_max, n)]


# ---- 1. energies bit-exact ------------------------------------------------------
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_energies_bit_exact(gpu_lib, gi):
    got = _dev_wf(gi, "energy").reshape(_ref(gi)[0].shape)
    assert np.array_equal(got.view(np.uint32), _ref(gi)[0].view(np.uint32))


@pytest.mark.parametrize("rows", [1, 2, 4, 8])
def test_energies_do_not_depend_on_rows_per_lane(gpu_lib, rows):
    """Every rows-per-lane form of the kernel on the geometries with a partial row, rows
    past the end and three channels: the same bits."""
    for gi in (1, 2, 4, BIG):
        sps, ns, nt, off, n, spacing, nch = GEOMS[gi]
        x = _input(gi)
        eng = gpu_lib.SyncEngine().set_rows_per_lane(rows)
        got = eng.compute_waterfall(x if nch > 1 else x[0], FS, BASE, spacing, sps, ns, nt, off, "energy")
        assert np.array_equal(got.reshape(_ref(gi)[0].shape).view(np.uint32), _ref(gi)[0].view(np.uint32)), (gi, rows)


# ---- 2. log power ----------------------------------------------------------------
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_log_power_within_four_ulp(gpu_lib, gi):
    """|d| <= 4 * 2^-23 * max(1, |v|) per cell: 1 ulp of host libm, 2 ulp of device logf,
    and a margin; rows past the end of the buffer are exactly 0.0."""
    got = _dev_wf(gi, "log").reshape(_ref(gi)[1].shape).astype(np.float64)
    ref = _ref(gi)[1].astype(np.float64)
    rel = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[parity] waterfall log geometry {gi}: max |d| / max(1, |v|) = {rel.max() / 2.0 ** -23:.3f} x 2^-23, "
          f"values in [{ref.min():.2f}, {ref.max():.2f}]")
    assert rel.max() <= 4 * 2.0 ** -23
    if gi == 2:
        assert np.all(got[0, 3:] == 0.0) and np.all(got[0, :3] != 0.0)


def test_host_and_device_entries_give_the_same_waterfall(gpu_lib):
    import torch

    sps, ns, nt, off, n, spacing, nch = GEOMS[BIG]
    x = _input(BIG)
    got = gpu_lib.SyncEngine().compute_waterfall(torch.from_numpy(x).cuda(), FS, BASE, spacing, sps, ns, nt, off, "log")
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _dev_wf(BIG, "log").view(np.uint32))


# ---- 3. search exact, ties included ----------------------------------------------
def test_search_constant_waterfall(gpu_lib):
    """(a) every score is 0: the list is the reference's tie order."""
    eng = gpu_lib.SyncEngine()
    for pat, mode, shape in (("ft8", S.FT8, (85, 24)), ("ft4", S.FT4, (110, 12))):
        wf = np.full(shape, 1.5, np.float32)
        for n in (1, 5, 20):
            assert _cands(eng.find_candidates(wf, pat, 0, 6, n)) == _ref_cands(wf, mode, 0, 6, n), (pat, n)


@pytest.mark.parametrize("seed", range(6))
def test_search_integer_waterfalls_ties(gpu_lib, seed):
    """(b) integer-valued random waterfalls: many equal scores, where the reference's
    order is not (score descending, scan order ascending)."""
    eng = gpu_lib.SyncEngine()
    for pat, mode, shape in (("ft8", S.FT8, (85, 24)), ("ft4", S.FT4, (110, 12))):
        wf = np.random.default_rng(seed).integers(0, 4, shape).astype(np.float32)
        assert _cands(eng.find_candidates(wf, pat, 0, 6, 5)) == _ref_cands(wf, mode, 0, 6, 5), pat


@pytest.mark.parametrize("n", [1, 5, 20])
def test_search_on_the_device_waterfall(gpu_lib, n):
    """(c) the device's own log waterfall of the three-channel geometry, batched."""
    wf = _dev_wf(BIG, "log")
    got = gpu_lib.SyncEngine().find_candidates(wf, "ft8", 0, 4, n)
    assert len(got) == 3
    for ch in range(3):
        assert _cands(got[ch]) == _ref_cands(wf[ch], S.FT8, 0, 4, n), ch


def test_search_narrow_waterfall_is_empty(gpu_lib):
    """(d) num_tones <= the frame's tones: no candidates."""
    eng = gpu_lib.SyncEngine()
    assert len(eng.find_candidates(np.zeros((85, 8), np.float32), "ft8", 0, 6, 5)) == 0
    assert len(eng.find_candidates(np.zeros((110, 4), np.float32), "ft4", 0, 6, 5)) == 0
    assert len(eng.find_candidates(np.zeros((85, 9), np.float32), "ft8", 3, 2, 5)) == 0  # empty time range


def test_search_negative_t_min_and_short_lists(gpu_lib):
    """(e) t_min < 0: skipped rows and -inf edge neighbours; fewer cells than max_cand."""
    eng = gpu_lib.SyncEngine()
    rng = np.random.default_rng(11)
    for pat, mode, shape in (("ft8", S.FT8, (81, 11)), ("ft4", S.FT4, (107, 7))):
        wf = rng.normal(0, 3, shape).astype(np.float32)
        for t_min, t_max, n in ((-3, 4, 5), (-80, -70, 7), (-2, -2, 20), (0, 30, 300)):
            assert _cands(eng.find_candidates(wf, pat, t_min, t_max, n)) == _ref_cands(wf, mode, t_min, t_max, n), \
                (pat, t_min, t_max, n)


def test_max_cand_zero_is_rejected(gpu_lib):
    with pytest.raises(gpu_lib.OrionError, match="error -3"):
        gpu_lib.SyncEngine().find_candidates(np.zeros((85, 24), np.float32), "ft8", 0, 6, 0)


# ---- 4. LLRs -----------------------------------------------------------------------
@pytest.mark.parametrize("pat", ["ft8", "ft4"])
def test_llrs_bit_exact_on_the_device_waterfall(gpu_lib, pat):
    """The restatement's extractor and normaliser on the device's own waterfall and
    candidates equal the device's LLRs bit for bit (IEEE divide and sqrt on both sides)."""
    mode, iq, _, max_hz = S.test_frame(pat)
    eng = gpu_lib.SyncEngine()
    num_bins, wf_syms, start, _, wf_t_max = S.sync_geometry(mode, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX)
    wf = eng.compute_waterfall(iq, S.FS, S.BASE_HZ, float(mode["spacing"]), mode["sps"], wf_syms, num_bins, start)
    cand = eng.find_candidates(wf, pat, 0, wf_t_max, 8)
    assert len(cand) == 8
    # by hand: data symbols that run off either end of the waterfall
    extra = np.array([(wf_syms - 40, 2, 1.0), (-30, 0, 2.0), (wf_syms + 5, 1, 0.0)], gpu_lib.CANDIDATE_DTYPE)
    allc = np.concatenate([cand, extra])
    got = eng.extract_llr(wf, pat, allc)
    for k, c in enumerate(allc):
        ref = S.normalise_llr(S.extract_llr(wf, mode, int(c["time_sym"]), int(c["freq_bin"])))
        assert np.array_equal(got[k].view(np.uint32), ref.view(np.uint32)), (k, c)
    assert np.all(got[len(cand) + 2] == 0.0)  # every symbol missing: zeros, never scaled
    assert np.any(got[len(cand)] == 0.0) and np.any(got[len(cand)] != 0.0)


def test_llrs_zero_variance_is_not_scaled(gpu_lib):
    wf = np.full((83, 19), 2.5, np.float32)
    got = gpu_lib.SyncEngine().extract_llr(wf, "ft8", np.array([(0, 0, 0.0), (2, 5, 0.0)], gpu_lib.CANDIDATE_DTYPE))
    assert got.shape == (2, 174) and np.all(got == 0.0)


# ---- 5. end to end --------------------------------------------------------------------
def _check_sync(name, got, ref):
    """Against the restatement run on its own waterfall: the slack is ln()'s ulps only."""
    assert len(got) == len(ref)
    scores = [float(r["score"]) for r in ref]
    ds = dl = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        near = [abs(scores[k] - scores[j]) for j in (k - 1, k + 1) if 0 <= j < len(ref)]
        if not near or min(near) > 1e-3:
            assert (g["time_sym"], g["freq_bin"]) == (r["time_sym"], r["freq_bin"]), (name, k)
            ds = max(ds, abs(g["score"] - float(r["score"])))
            dl = max(dl, float(np.max(np.abs(g["llr"].astype(np.float64) - r["llr"]))) / max(1e-30, float(np.max(np.abs(r["llr"])))))
    print(f"[parity] {name}: max |score - ref| {ds:.3e}, max |llr - ref| / full scale {dl:.3e}")
    assert ds <= 1e-4 and dl <= 1e-4


@functools.lru_cache(maxsize=None)
def _ref_sync(pat, ch):
    mode, iq, _, max_hz = S.test_frame(pat)
    return S.sync(_chan(iq, ch), mode, S.FS, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX, S.MAX_CAND)


def _chan(iq, ch):
    """Channel ch of the batched end-to-end case: the frame moved 0 / 1 / 2 symbols later."""
    sps = 1920 if len(iq) == 83 * 1920 else 576
    return np.ascontiguousarray(np.roll(iq, ch * sps))


@pytest.mark.parametrize("pat", ["ft8", "ft4"])
def test_sync_end_to_end(gpu_lib, pat):
    import torch

    mode, iq, data, max_hz = S.test_frame(pat)
    args = (S.FS, S.BASE_HZ, max_hz, S.T_MIN, S.T_MAX, S.MAX_CAND)
    eng = gpu_lib.SyncEngine()
    one = getattr(eng, f"{pat}_sync")(np.ascontiguousarray(iq), *args)
    _check_sync(f"{pat}_sync 1 channel", one, _ref_sync(pat, 0))
    assert (one[0]["time_sym"], one[0]["freq_bin"]) == (S.LATE_SYMS, S.UP_BINS)
    assert np.array_equal((one[0]["llr"] < 0).astype(np.int64), S.data_bits(mode, data))
    # the module-level drop-in call and the device-tensor entry: identical results
    for other in (getattr(gpu_lib, f"{pat}_sync")(np.ascontiguousarray(iq), *args),
                  getattr(eng, f"{pat}_sync")(torch.from_numpy(np.array(iq)).cuda(), *args)):
        assert [(r["time_sym"], r["freq_bin"], r["score"]) for r in other] == \
               [(r["time_sym"], r["freq_bin"], r["score"]) for r in one]
        assert all(np.array_equal(a["llr"].view(np.uint32), b["llr"].view(np.uint32)) for a, b in zip(other, one))
    # three channels: each against the restatement, and the batch against per-channel calls
    x = np.stack([_chan(iq, ch) for ch in range(3)])
    batch = getattr(eng, f"{pat}_sync_batch")(x, *args)
    assert len(batch) == 3
    for ch in range(3):
        _check_sync(f"{pat}_sync_batch channel {ch}", batch[ch], _ref_sync(pat, ch))
        assert (batch[ch][0]["time_sym"], batch[ch][0]["freq_bin"]) == (S.LATE_SYMS + ch, S.UP_BINS)
        single = getattr(eng, f"{pat}_sync")(x[ch].copy(), *args)
        assert [(r["time_sym"], r["freq_bin"], r["score"]) for r in single] == \
               [(r["time_sym"], r["freq_bin"], r["score"]) for r in batch[ch]]
        assert all(np.array_equal(a["llr"].view(np.uint32), b["llr"].view(np.uint32)) for a, b in zip(single, batch[ch]))


def test_sync_negative_t_min(gpu_lib):
    """t_min < 0: the waterfall starts at sample 0 and time_sym comes back buffer-relative."""
    mode, iq, _, max_hz = S.test_frame("ft4")
    got = gpu_lib.SyncEngine().ft4_sync(np.ascontiguousarray(iq), S.FS, S.BASE_HZ, max_hz, -2, 2, 3)
    ref = S.sync(iq, mode, S.FS, S.BASE_HZ, max_hz, -2, 2, 3)
    _check_sync("ft4_sync t_min -2", got, ref)
    assert (got[0]["time_sym"], got[0]["freq_bin"]) == (S.LATE_SYMS - 2, S.UP_BINS)


# ---- 6. handle reuse ---------------------------------------------------------------------
def test_handle_reuse_across_geometries(gpu_lib):
    """Two calls with different geometries on one handle, then the first again: identical
    results (the step table is rebuilt, the scratch waterfall and score map regrow)."""
    m8, iq8, _, hz8 = S.test_frame("ft8")
    m4, iq4, _, hz4 = S.test_frame("ft4")
    eng = gpu_lib.SyncEngine()
    a = eng.sync_raw("ft4", np.ascontiguousarray(iq4), S.FS, S.BASE_HZ, hz4, 0, 4, 5)
    b = eng.sync_raw("ft8", np.stack([iq8, iq8[::-1]]), S.FS, 900.0, 1400.0, -1, 6, 20)
    c = eng.sync_raw("ft4", np.ascontiguousarray(iq4), S.FS, S.BASE_HZ, hz4, 0, 4, 5)
    fresh = gpu_lib.SyncEngine().sync_raw("ft8", np.stack([iq8, iq8[::-1]]), S.FS, 900.0, 1400.0, -1, 6, 20)
    for x, y in zip(a, c):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(b, fresh):
        assert x.tobytes() == y.tobytes()


# ---- 7. the step table replaced under launches of another stream ------------------
def test_step_table_is_replaced_whatever_streams_the_earlier_calls_used(gpu_lib):
    """One engine on device tensors: geometry A (2 channels, 64 samples per symbol, 6
    symbols, 9 tones 6.25 Hz apart) on one stream, geometry B (5 tones 20.833334 Hz apart
    from another base) on a second stream with no host synchronisation between the
    enqueues, then A again on the first. compute_waterfall reads the handle's step table
    and no scratch, so the handle contract makes the three calls well defined; each gives
    the bits of the same call made alone on a fresh engine. This pins the contract's results,
    not the ordering: a launch this small ends long before the next table is uploaded, so
    the test would rarely fail if the table's guard were removed."""
    import torch

    rng = np.random.default_rng(20)
    sps, ns = 64, 6
    x = (rng.standard_normal((2, sps * ns)) + 1j * rng.standard_normal((2, sps * ns))).astype(np.complex64)
    xd = torch.from_numpy(x).cuda()
    geom_a, geom_b = (FS, BASE, 6.25, sps, ns, 9), (FS, 1500.0, 20.833334, sps, ns, 5)
    alone = [gpu_lib.SyncEngine().compute_waterfall(xd, *g).cpu().numpy() for g in (geom_a, geom_b)]
    eng = gpu_lib.SyncEngine()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a1 = eng.compute_waterfall(xd, *geom_a)
    with torch.cuda.stream(s2):
        b = eng.compute_waterfall(xd, *geom_b)
    with torch.cuda.stream(s1):
        a2 = eng.compute_waterfall(xd, *geom_a)
    torch.cuda.synchronize()
    assert a1.shape == (2, ns, 9) and b.shape == (2, ns, 5)
    for got, want in ((a1, alone[0]), (b, alone[1]), (a2, alone[0])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
