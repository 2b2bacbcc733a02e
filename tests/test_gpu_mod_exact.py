"""AmDsbMod, PmDirectPhaseMod and FmPhaseAccumMod (csrc/k_mod.hip) per sample, at the
smallest shapes at which each path of the kernels runs (tests/mod_ref.py: truths,
yardsticks, and the numpy model on which tests/test_mod_ref.py shows that these criteria
see a dropped thread sum, a missing carry and per = 1 in k_fm_mod_carry).

* AM  bit for bit the oracle (its RF Rotator is the reference's own, tabulated).
* PM  truth g (cos phi, sin phi) r in f64, phi = f64(f32(kp x)); max |gpu - truth| <= MARGIN x
      e_ref, e_ref = max |oracle - truth| on the same input.
* FM  truth g e^{j Phi} r, Phi the longdouble running sum of the angles of the correctly
      rounded f32 pairs (cos, sin)(f32(kf x)), carried across calls. The kernel re-seeds every
      16-sample thread group from an exact integer phase, so max |gpu - truth| / g over the
      WHOLE run, whatever its length, is held to MARGIN x e_ref of the reference's first 4096
      samples from rest. The truth's pairs rest on sincos_cr being correctly rounded, which by
      its own error analysis (hip_common.hpp) fails about once in 10^6 values, by one ulp.

Out of scope here: non-finite inputs; |kf x| >= 2^20 (the library sincosf path of
sincos_cr); retunes past a table with ctr0 != 0.
"""
import numpy as np
import pytest

import mod_ref as M

pytestmark = pytest.mark.gpu
f32 = np.float32

MOD_NS = (1, 255, 2047, 2048, 2049, 4101)
MOD_CALLS = [1, 2047, 2053]
MOD_LONG = 2048 * 2048 + 2048 + 5      # the grid-stride loop's second iteration, a partial last tile
FM_NS = (1, 15, 16, 17, 4095, 4096, 4097, 8193)
FM_CALLS = [1, 15, 4081, 4096, 4102]
FM_TUNINGS = [(48e3, 5e3, 0.0), (48e3, 5e3, 1500.0), (10e6, 75e3, 0.0), (10e6, 75e3, -1.5e6)]


def run(blk, x, lens):
    return np.concatenate([blk.process(np.ascontiguousarray(c)) for c in M.split(x, lens)])


def am_input(n, seed):
    """Noise of amplitude 3 (so the clamp acts), with values that put cl + mi x exactly on
    +1 and -1 for (cl, mi) = (0.5, 0.5), and just beyond either side."""
    x = (3.0 * M.fm_input("noise", n, seed)).astype(f32)
    for i, v in enumerate((1.0, -3.0, np.nextafter(f32(1.0), f32(2.0)), np.nextafter(f32(-3.0), f32(-4.0)), 1.5, -3.5)):
        x[i * 7 % n::97][:3] = v
    return x


# --------------------------------------------------------------------------------- AM ==
@pytest.mark.parametrize("rf,cl,mi,g,clamp", [(12e3, 0.5, 0.5, 1.3, True), (-5e3, 0.5, 0.5, 0.7, False),
                                              (0.0, 1.0, 0.8, 1.0, True)])
def test_am_small_shapes(gpu_lib, oracle, rf, cl, mi, g, clamp):
    """mod_tiles at one thread, a partial tile, the tile edge +-1 and two tiles and a bit, in
    one call each and streamed: bit for bit the oracle."""
    fs = 48e3

    def mk():
        m = gpu_lib.AmDsbMod(fs, rf, cl, mi)
        m.set_gain(g)
        m.set_clamp(clamp)
        return m
    x = am_input(max(MOD_NS), 21)
    if (cl, mi) == (0.5, 0.5):
        v = f32(cl) + f32(mi) * x
        assert np.any(v == 1.0) and np.any(v == -1.0) and np.any(v > 1.0) and np.any(v < -1.0)
    ref = oracle.am_mod(x, fs, rf, cl, mi, g, clamp)
    for n in MOD_NS:
        got = mk().process(x[:n].copy())
        assert M.bits_equal(got, ref[:n]), f"n = {n}: max abs {float(np.max(np.abs(got - ref[:n]))):.3e}"
    got = run(mk(), x[:sum(MOD_CALLS)], MOD_CALLS)
    assert M.bits_equal(got, ref[:sum(MOD_CALLS)])
    assert M.bits_equal(M.am_restate(x, M.osc_E(gpu_lib, rf, fs, len(x))[0], cl, mi, g, clamp), ref)
    print(f"[parity] am rf={rf} clamp={clamp} g={g}: n in {MOD_NS} and calls {MOD_CALLS} bit-exact (max|err| 0 "
          f"against the oracle, tol 0)")


def test_am_pm_grid_stride(gpu_lib, oracle):
    """n = 2048 x 2048 + 2048 + 5: grid_for caps the grid at 2048 workgroups, so workgroups
    0 and 1 take a second tile, the last one partial. (-1.5 MHz, 10 MHz) closes a cycle: AM is
    bit for bit the oracle at any length; PM by its criterion."""
    fs, rf, n = 10e6, -1.5e6, MOD_LONG
    x = am_input(n, 23)
    am = gpu_lib.AmDsbMod(fs, rf, 0.5, 0.5)
    am.set_gain(1.3)
    am.set_clamp(True)
    got, ref = am.process(x), oracle.am_mod(x, fs, rf, 0.5, 0.5, 1.3, True)
    bad = np.nonzero(got != ref)[0]
    assert M.bits_equal(got, ref), f"first difference at {int(bad[0]) if len(bad) else -1} (tile {int(bad[0]) // 2048 if len(bad) else -1})"
    print(f"[parity] am grid-stride n={n}: bit-exact (max|err| 0 against the oracle, tol 0)")
    kp, g = 1.2, 0.7
    pm = gpu_lib.PmDirectPhaseMod(fs, kp, rf)
    pm.set_gain(g)
    xs = M.fm_input("noise", n, 25)
    r = M.osc_E(gpu_lib, rf, fs, n)[0]
    M.check_pm(f"pm grid-stride n={n}", pm.process(xs), M.pm_truth(xs, kp, g, r), M.pm_e_ref(oracle, xs, fs, kp, g, rf), g)


@pytest.mark.parametrize("passes", [1, 3])
def test_modulators_past_the_table(gpu_lib, oracle, passes):
    """The three modulators with nco_table = 5001 (mid-tile for mod_tiles and for the FM
    chunk) over 3 x 4096 + 7 samples in calls [4099, 8196]: inside the table as above, past it
    the oscillator's OSC_TOL on top (tests/test_gpu_osc_seam.py has every tuning, budget and
    split; this is the one case that makes this file see a slip at the table's end)."""
    fs, rf, b, lens = 48e3, 1500.0, 5001, [4099, 8196]
    n = sum(lens)
    e, _, cl_, nt = M.osc_E(gpu_lib, rf, fs, n, b)
    assert cl_ == 0 and nt == b
    x = M.fm_input("noise", n, 37)
    am = gpu_lib.AmDsbMod(fs, rf, 0.5, 0.5).configure_option("nco_table", b)
    am.set_gain(1.3)
    w = M.check_osc_product("am past the table", run(am, x, lens), M.am_restate(x, e, 0.5, 0.5, 1.3, False),
                            np.abs(M.am_base(x, 0.5, 0.5, 1.3, False)), nt)
    print(f"[parity] am budget {b}: bit-exact inside the table, max |y - restatement| / |m| past it {w:.3e} (tol {M.OSC_TOL:.1e} + 2u)")
    kp, g = 1.2, 0.7
    pm = gpu_lib.PmDirectPhaseMod(fs, kp, rf).configure_option("nco_table", b)
    pm.set_gain(g)
    M.check_pm(f"pm budget {b}", run(pm, x, lens), M.pm_truth(x, kp, g, e), M.pm_e_ref(oracle, x, fs, kp, g, rf), g, nt)
    fm = fm_mk(gpu_lib, fs, 5e3, rf, passes, g).configure_option("nco_table", b)
    M.check_fm(f"fm budget {b} passes={passes}", run(fm, x, lens), M.fm_truth(x, lens, M.kf32(5e3, fs), g, e),
               M.fm_e_ref(oracle, x, fs, 5e3, rf), lens, g, nt)


# --------------------------------------------------------------------------------- PM ==
@pytest.mark.parametrize("kind", M.FM_CLASSES)
@pytest.mark.parametrize("fs,kp,g,rf", [(48e3, 0.9, 1.0, 0.0), (48e3, 2.5, 0.7, 12e3), (10e6, 1.2, 1.0, -1.5e6)])
def test_pm_small_shapes(gpu_lib, oracle, fs, kp, g, rf, kind):
    def mk():
        m = gpu_lib.PmDirectPhaseMod(fs, kp, rf)
        m.set_gain(g)
        assert m.taps()[0] == f32(kp)
        return m
    x = M.fm_input(kind, max(MOD_NS), 27)
    r = M.osc_E(gpu_lib, rf, fs, len(x))[0]
    truth = M.pm_truth(x, kp, g, r)
    for n in MOD_NS:
        M.check_pm(f"pm {fs:g}/{kp}/{g}/{rf:g} {kind} n={n}", mk().process(x[:n].copy()), truth[:n],
                   M.pm_e_ref(oracle, x[:n], fs, kp, g, rf), g)
    n = sum(MOD_CALLS)
    M.check_pm(f"pm {fs:g}/{kp}/{g}/{rf:g} {kind} calls {MOD_CALLS}", run(mk(), x[:n], MOD_CALLS), truth[:n],
               M.pm_e_ref(oracle, x[:n], fs, kp, g, rf), g)


# --------------------------------------------------------------------------------- FM ==
def fm_mk(lib, fs, dev, rf, passes=1, g=1.0):
    m = lib.FmPhaseAccumMod(fs, dev, rf)
    if passes == 3:
        m.configure_option("mod_passes", 3)
    if g != 1.0:
        m.set_gain(g)
    assert m.taps()[0] == M.kf32(dev, fs)
    return m


@pytest.mark.parametrize("kind", M.FM_CLASSES)
@pytest.mark.parametrize("fs,dev,rf", FM_TUNINGS)
def test_fm_small_shapes(gpu_lib, oracle, fs, dev, rf, kind):
    """One thread with a partial group (n < 16), n = 1, the group edge, the last / fast split
    of k_fm_mod_sp at 4095 / 4096 / 4097, two chunks and one sample; then ragged streamed
    calls (the phase carries). Single pass and the three passes, each by the criterion."""
    x = M.fm_input(kind, sum(FM_CALLS), 29)
    kf = M.kf32(dev, fs)
    r = M.osc_E(gpu_lib, rf, fs, len(x))[0]
    for passes in (1, 3):
        for n in FM_NS:
            M.check_fm(f"fm {fs:g}/{dev:g}/{rf:g} {kind} passes={passes} n={n}",
                       fm_mk(gpu_lib, fs, dev, rf, passes).process(x[:n].copy()), M.fm_truth(x[:n], [n], kf, 1.0, r[:n]),
                       M.fm_e_ref(oracle, x[:n], fs, dev, rf), [n], 1.0)
        M.check_fm(f"fm {fs:g}/{dev:g}/{rf:g} {kind} passes={passes} calls {FM_CALLS}",
                   run(fm_mk(gpu_lib, fs, dev, rf, passes), x, FM_CALLS), M.fm_truth(x, FM_CALLS, kf, 1.0, r),
                   M.fm_e_ref(oracle, x, fs, dev, rf), FM_CALLS, 1.0)


@pytest.mark.parametrize("passes", [1, 3])
def test_fm_half_turn(gpu_lib, oracle, passes):
    """A thread group whose 16 angles sum to within 1e-7 rad of -pi, and the next to +pi: the
    f64 atan2 at its branch cut, the half-turn count doubled into the top bit of the Q0.64
    phase. One sample with f32(kf x) = f32(pi) (the pair (-1, -8.7e-8)) among zeros, then its
    negative in the next group; the groups after them inherit the half turns."""
    fs, dev, n = 48e3, 5e3, 4097
    kf = M.kf32(dev, fs)
    v = f32(np.pi) / kf
    for _ in range(64):  # the f32 neighbour of pi / kf whose product rounds to f32(pi)
        if f32(kf * v) == f32(np.pi):
            break
        v = np.nextafter(v, f32(np.inf) if f32(kf * v) < f32(np.pi) else f32(-np.inf))
    assert f32(kf * v) == f32(np.pi)
    x = np.zeros(n, f32)
    x[3], x[16 + 5], x[40 * 16 + 15] = v, -v, v
    dc, ds = M.fm_pairs(x[3:4], kf)
    assert dc[0] == -1.0 and -1e-7 < ds[0] < 0.0
    r = np.ones(n, np.complex64)
    # the yardstick on zeros and half turns is tiny (the reference multiplies by (1, 0) and
    # (-1, -8.7e-8)): taken from the noise class at the same tuning, as the other cases have it
    e_ref = M.fm_e_ref(oracle, M.fm_input("noise", n, 29), fs, dev, 0.0)
    got = fm_mk(gpu_lib, fs, dev, 0.0, passes).process(x)
    M.check_fm(f"fm half turn passes={passes}", got, M.fm_truth(x, [n], kf, 1.0, r), e_ref, [n], 1.0)
    assert np.all(got.real[3:16 + 5] < -0.999) and np.all(got.real[16 + 5:40 * 16 + 15] > 0.999) and got.real[-1] < -0.999


@pytest.mark.parametrize("fs,dev,rf,g", [(48e3, 5e3, 1500.0, 0.6), (10e6, 75e3, 0.0, 1.0)])
def test_fm_setters_between_calls(gpu_lib, oracle, fs, dev, rf, g):
    """set_deviation and set_gain between calls: the phase carries, the truth takes each
    call's kf and gain."""
    x = M.fm_input("noise", sum(FM_CALLS), 31)
    devs = [dev, dev, 0.6 * dev, dev, 1.4 * dev]
    gs = [g, g, 0.5, 0.5, 1.7]
    r = M.osc_E(gpu_lib, rf, fs, len(x))[0]
    for passes in (1, 3):
        m = fm_mk(gpu_lib, fs, dev, rf, passes, g)
        out = []
        for xc, d, gg in zip(M.split(x, FM_CALLS), devs, gs):
            m.set_deviation(d)
            m.set_gain(gg)
            assert m.taps()[0] == M.kf32(d, fs)
            out.append(m.process(xc.copy()))
        kfs = [M.kf32(d, fs) for d in devs]
        M.check_fm(f"fm {fs:g}/{dev:g}/{rf:g} set_deviation/set_gain passes={passes}", np.concatenate(out),
                   M.fm_truth(x, FM_CALLS, kfs, gs, r), M.fm_e_ref(oracle, x, fs, dev, rf), FM_CALLS, gs)


@pytest.mark.parametrize("kind,n,fs,dev,rf", [("noise", 65 * 4096 + 17, 48e3, 5e3, 1500.0),
                                              ("impulse", 65 * 4096 + 17, 10e6, 75e3, -1.5e6),
                                              ("noise", (1 << 20) + 4097 + 5, 48e3, 5e3, 0.0)])
def test_fm_long(gpu_lib, oracle, kind, n, fs, dev, rf):
    """65 chunks and 17 samples: the look-back walks past one 64-record step. 2^20 + 4097 + 5
    samples are 258 chunks: per = 2 in k_fm_mod_carry. On top of the criterion, the single
    pass, the three passes and the same input streamed in calls that are multiples of 4096
    give the same bits (the chunks and thread groups coincide, the phases are integers)."""
    x = M.fm_input(kind, n, 33)
    r = M.osc_E(gpu_lib, rf, fs, n)[0]
    one = fm_mk(gpu_lib, fs, dev, rf).process(x)
    M.check_fm(f"fm long {kind} n={n} {fs:g}/{dev:g}/{rf:g}", one, M.fm_truth(x, [n], M.kf32(dev, fs), 1.0, r),
               M.fm_e_ref(oracle, x, fs, dev, rf), [n], 1.0)
    three = fm_mk(gpu_lib, fs, dev, rf, 3).process(x)
    assert M.bits_equal(three, one), f"three passes differ first at {M.fm_where(int(np.nonzero(three != one)[0][0]), [n])}"
    lens = [3 * 4096, 4096, 60 * 4096]
    lens.append(n - sum(lens))
    for passes in (1, 3):
        got = run(fm_mk(gpu_lib, fs, dev, rf, passes), x, lens)
        assert M.bits_equal(got, one), f"streamed {lens} passes={passes} differ first at {int(np.nonzero(got != one)[0][0])}"


def test_fm_record_reuse_and_reset(gpu_lib, oracle):
    """Calls of 70, 1 and 70 chunks on one handle: during the third, the records beyond the
    first carry the first call's launch tag, not the second's. Then reset(): the output
    equals a fresh handle's bit for bit."""
    fs, dev, rf = 48e3, 5e3, 1500.0
    lens = [70 * 4096 - 5, 4096 - 9, 70 * 4096 + 3]
    x = M.fm_input("noise", sum(lens), 35)
    r = M.osc_E(gpu_lib, rf, fs, len(x))[0]
    m = fm_mk(gpu_lib, fs, dev, rf)
    M.check_fm("fm calls of 70, 1, 70 chunks", run(m, x, lens), M.fm_truth(x, lens, M.kf32(dev, fs), 1.0, r),
               M.fm_e_ref(oracle, x, fs, dev, rf), lens, 1.0)
    m.status()
    m.reset()
    n = 2 * 4096 + 11
    assert M.bits_equal(m.process(x[:n].copy()), fm_mk(gpu_lib, fs, dev, rf).process(x[:n].copy()))
