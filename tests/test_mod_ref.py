"""tests/mod_ref.py against the C oracle, on the CPU: the oscillator yardstick E is the
reference inside its table for every tuning and budget the GPU tests use, the f32
restatements are the oracle's op order, the PM / FM yardsticks are what their roundings
allow, and every criterion of tests/test_gpu_mod_exact.py and tests/test_gpu_osc_seam.py
passes on a faithful numpy model of the kernels' indexing and fails on each indexing
mistake those files have to catch (mod_ref.seam_phasors, mod_ref.fm_engine_model)."""
import numpy as np
import pytest

import iir_ref as IR
import mod_ref as M

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def _cnoise(n, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    return (amp * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))).astype(np.complex64)


# ------------------------------------------------------------------- the oscillator ==
@pytest.mark.parametrize("b", M.BUDGETS + (3900, 8000))
@pytest.mark.parametrize("f,fs", M.ACYCLIC)
def test_E_is_the_reference_inside_the_table(oracle, lib, f, fs, b):
    """E[:B] is the oracle's recurrence bit for bit, cyc_len == 0 and n_tab == B; past it
    the host's drift model (its distance from the reference's own random walk printed)."""
    n = M.N_SEAM
    e, cs, cl, nt = M.osc_E(lib, f, fs, n + 1, b)
    ref = oracle.nco(np.zeros(n + 1, np.complex64), f, fs, gen=True)
    assert cl == 0 and nt == b
    assert M.bits_equal(e[:b], ref[:b])
    d = np.abs(e[b:].astype(np.complex128) - ref[b:])
    assert np.all(np.isfinite(e.view(f32))) and d.max() < 1e-3  # the model follows the reference
    print(f"[parity] E {f}/{fs} budget {b}: table bit-exact, model vs reference over {n - b} outputs past it "
          f"max {d.max():.3e}, first {d[0]:.3e}")


@pytest.mark.parametrize("f,fs,cyc,n", [(-1.5e6, 10e6, (16384, 20480, 36864), M.N_CYC),
                                        (100e3, 10e6, (None, None, 49152), 80000)])
def test_E_cyclic_is_the_reference_forever(oracle, lib, f, fs, cyc, n):
    e, cs, cl, nt = M.osc_E(lib, f, fs, n, 1 << 20)
    assert nt == cyc[2] and cl >= 16384 and nt == cs + cl
    if cyc[0] is not None:
        assert (cs, cl) == cyc[:2]
    if f == 100e3:  # the first wrap sits on a tile boundary, the second mid-tile for both tile sizes
        assert nt % 4096 == 0 and nt + cl == 74752 and (nt + cl) % 2048 != 0 and n > nt + cl
    assert M.bits_equal(e, oracle.nco(np.zeros(n, np.complex64), f, fs, gen=True))
    print(f"[parity] E {f}/{fs}: cycle ({cs}, {cl}), n_tab {nt}, {n} outputs bit-exact")


@pytest.mark.parametrize("f,fs", M.ACYCLIC[:1] + M.CYCLIC[:1])
def test_restatements_are_the_oracles_op_order(oracle, lib, f, fs):
    """rot_rotate / rot_mix_usb / nco_mix / am_restate / cw_restate with the reference's
    phasors equal the oracle bit for bit (inside the default table E is the reference)."""
    n = M.N_SEAM
    x = _cnoise(n, 3)
    e = M.osc_E(lib, f, fs, n)[0]
    assert M.bits_equal(M.rot_rotate(x, e), oracle.rotator(x, f, fs))
    assert M.bits_equal(M.rot_mix_usb(x, e), oracle.rotator_retune(x, f, fs, n, f, usb=True))
    assert M.bits_equal(M.nco_mix(x, e), oracle.nco(x, f, fs))
    a = M.fm_input("noise", n, 5) * f32(3.0)
    for cl, mi, g, clamp in ((1.0, 0.8, 1.0, False), (0.5, 0.5, 1.3, True)):
        assert M.bits_equal(M.am_restate(a, e, cl, mi, g, clamp), oracle.am_mod(a, fs, f, cl, mi, g, clamp))
    key = np.clip(np.repeat(np.array([1.0, 0.0, 0.6, 1.4, -0.2], f32), 2459), -1, 2)[:n].astype(f32)
    assert M.bits_equal(M.cw_restate(M.cw_env(oracle, key, fs, 2.0, 8.0), e), oracle.cw_mod(key, fs, f, 2.0, 8.0))
    ad = M.OscAdapter(oracle, lib, 1 << 20)
    assert M.bits_equal(IR.phasors(ad, n, f, fs), IR.phasors(oracle, n, f, fs))
    assert ad.lp_cascade_coeffs(48e3, 2520.0) is not None  # everything else is the oracle's


@pytest.mark.parametrize("mistake", [None, "exponent", "rem+", "table"])
@pytest.mark.parametrize("b", [5001, 6144, 1])
def test_seam_criterion_sees_each_indexing_mistake(oracle, lib, b, mistake):
    """check_osc_product on the restatement with seam_phasors: passes when faithful; each
    mistake fails in at least one call split of the seam cases, for the 2048 tile (k_mod)
    and the 4096 tile (k_rotator, FM chunks). Budget 6144 is a k_mod tile boundary: there
    'rem+' and 'table' cannot occur for the 2048 tile (no mixed tile), by construction."""
    f, fs, n = 1500.0, 48e3, M.N_SEAM
    e = M.osc_E(lib, f, fs, n + 1, b)[0]
    x = _cnoise(n, 7)
    for tile in (M.MOD_TILE, M.ROT_TILE):
        seen = False
        for lens in M.seam_calls(n, b):
            p = M.seam_phasors(e, b, lens, tile, mistake)
            try:
                M.check_osc_product("model", M.rot_rotate(x, p), M.rot_rotate(x, e[:n]), np.abs(x), b)
            except AssertionError:
                seen = True
        mixed = any(t0 < b < min(t0 + tile, t1) for lens in M.seam_calls(n, b) for t0, t1 in _tiles(lens, tile))
        expect = mistake == "exponent" or (mistake is not None and mixed)
        assert seen == expect, (tile, mistake, seen)


def _tiles(lens, tile):
    """(first output, end of its call) of every tile of the calls `lens`."""
    k0 = 0
    for ln in lens:
        for t0 in range(k0, k0 + ln, tile):
            yield t0, k0 + ln
        k0 += ln


# --------------------------------------------------------------------------- PM / FM ==
@pytest.mark.parametrize("fs,kp,g,rf", [(48e3, 0.9, 1.0, 0.0), (48e3, 2.5, 0.7, 12e3), (10e6, 1.2, 1.0, -1.5e6)])
@pytest.mark.parametrize("kind", M.FM_CLASSES)
def test_pm_yardstick(oracle, fs, kp, g, rf, kind):
    """0 < e_ref <= 4 u g: 0.56 u sinf / cosf, the gain, two products and a sum."""
    x = M.fm_input(kind, 4101, 11)
    e = M.pm_e_ref(oracle, x, fs, kp, g, rf)
    print(f"[parity] pm e_ref {fs:g}/{kp}/{g}/{rf:g} {kind}: {e:.3e} ({e / (M.U * g):.2f} u g)")
    assert 0 < e <= 4 * M.U * g


@pytest.mark.parametrize("fs,dev,rf", [(48e3, 5e3, 0.0), (48e3, 5e3, 1500.0), (10e6, 75e3, 0.0), (10e6, 75e3, -1.5e6)])
@pytest.mark.parametrize("kind", M.FM_CLASSES)
def test_fm_yardstick_and_truth(oracle, fs, dev, rf, kind):
    """0 < e_ref < 1e-4 for every input class; the truth stays with the reference over a long
    run as far as the reference's own drift allows (printed), and kf is the oracle's."""
    n = 65 * M.FM_CH + 17
    x = M.fm_input(kind, n, 13)
    e = M.fm_e_ref(oracle, x, fs, dev, rf)
    r = oracle.nco(np.zeros(n, np.complex64), rf, fs, gen=True)
    far = float(np.max(np.abs(oracle.fm_mod(x, fs, dev, rf) - M.fm_truth(x, [n], M.kf32(dev, fs), 1.0, r))))
    print(f"[parity] fm e_ref {fs:g}/{dev:g}/{rf:g} {kind}: first 4096 {e:.3e}, over {n} samples {far:.3e}")
    assert 0 < e < 1e-4 and far < 1e-3
    assert float(M.kf32(dev, fs)) == pytest.approx(2 * np.pi * dev / fs, rel=1e-6)


@pytest.mark.parametrize("kind", M.FM_CLASSES)
def test_fm_criterion_on_the_engine_model(oracle, kind):
    """The faithful model of the FM kernels meets the criterion on streamed calls with a
    per-call kf and gain, and its single-pass and three-pass forms agree bit for bit."""
    fs, dev, rf = 48e3, 5e3, 1500.0
    lens = [1, 15, 4081, 4096, 4102]
    n = sum(lens)
    x = M.fm_input(kind, n, 17)
    r = oracle.nco(np.zeros(n, np.complex64), rf, fs, gen=True)
    kf = [M.kf32(dev, fs), M.kf32(dev, fs), M.kf32(3e3, fs), M.kf32(dev, fs), M.kf32(7e3, fs)]
    g = [1.0, 1.0, 0.5, 0.5, 1.7]
    e = M.fm_e_ref(oracle, x, fs, dev, rf)
    y = M.fm_engine_model(x, lens, kf, g, r)
    M.check_fm(f"fm engine model {kind}", y, M.fm_truth(x, lens, kf, g, r), e, lens, g)
    assert M.bits_equal(y, M.fm_engine_model(x, lens, kf, g, r, passes=3))


@pytest.mark.parametrize("mistake,passes,lens", [
    ("drop_thread", 1, [8193]), ("drop_thread", 1, [1, 15, 4081, 4096, 4102]),
    ("no_carry", 1, [1, 15, 4081, 4096, 4102]), ("no_carry", 3, [4099, 8196]),
    ("per1", 3, [(1 << 20) + 4097 + 5])])
def test_fm_criterion_sees_each_mistake(oracle, mistake, passes, lens):
    """One thread's sum dropped from the prefix, the carry not applied, per forced to 1 in
    k_fm_mod_carry: each breaks the criterion at the shapes the GPU file uses (and 'per1'
    only past 256 chunks: the long three-pass case)."""
    fs, dev, rf = 48e3, 5e3, 0.0
    n = sum(lens)
    x = M.fm_input("noise", n, 19)
    r = np.ones(n, np.complex64)
    e = M.fm_e_ref(oracle, x, fs, dev, rf)
    t = M.fm_truth(x, lens, M.kf32(dev, fs), 1.0, r)
    M.check_fm("faithful", M.fm_engine_model(x, lens, M.kf32(dev, fs), 1.0, r, passes), t, e, lens, 1.0)
    with pytest.raises(AssertionError):
        M.check_fm(mistake, M.fm_engine_model(x, lens, M.kf32(dev, fs), 1.0, r, passes, mistake), t, e, lens, 1.0)
    if mistake == "per1":  # at 256 chunks (the existing three-pass test's size) it cannot show
        m = 1 << 20
        assert M.bits_equal(M.fm_engine_model(x[:m], [m], M.kf32(dev, fs), 1.0, r[:m], 3, "per1"),
                            M.fm_engine_model(x[:m], [m], M.kf32(dev, fs), 1.0, r[:m], 3))


def test_fm_where_and_inputs():
    assert M.fm_where(0, [5]) == (0, 0, 0, 0)
    assert M.fm_where(5 + 4096 + 16 * 3 + 2, [5, 9000]) == (1, 1, 3, 2)
    for kind in M.FM_CLASSES:
        x = M.fm_input(kind, 8193, 1)
        assert x.dtype == f32 and len(x) == 8193 and np.max(np.abs(x)) <= 1.3 + 1e-6
    x = M.fm_input("impulse", 8193)
    assert all(abs(x[p] - 0.3) > 0.9 for p in (0, 15, 16, 17, 4095, 4096, 4097, 8191, 8192))
    # 5 kHz at 48 kHz: |kf x| reaches 0.65 rad, a thread's 16 angles wrap past pi
    assert float(M.kf32(5e3, 48e3)) > 0.65 and 16 * 0.65 > np.pi
