"""Every consumer of the oscillator (hip_common.hpp OscDev / osc_run) across the end of
its table, and across the wrap of a cyclic table inside a run.

nco_table = B straight after construction tabulates B outputs of the reference's
recurrence; output B and later come from the drift model. With B = 5001 (odd, mid-tile
for the 2048 and 4096 tiles), 6144 (a k_mod tile boundary, mid-tile for 4096), 1, and
one budget inside each single-pass scan's warm-up overlap, the call splits of
mod_ref.seam_calls put the seam inside a tile (a mixed run, kind 2), on a call boundary,
and alone in a one-sample call. The yardstick is E = orion_osc_table_phasors(f, fs, n, B),
the host's long-double evaluation of the same table and model (tests/mod_ref.py):

* inside the table every product kernel (the four k_rotator modes, AmDsbMod, CwKeyedMod)
  equals the oracle's f32 op order with E bit for bit; past it |y - restatement| <=
  OSC_TOL amp + 2 u amp. An indexing slip is of the order of the step angle (0.196 rad at
  1500 Hz / 48 kHz), five orders above OSC_TOL = 1e-6;
* PM and FM: their criteria (tests/test_gpu_mod_exact.py) with E in the truth, plus
  OSC_TOL g past the table;
* the scan consumers (SsbPhasingMod, SsbProductDemod, FmQuadratureDemod.with_translate):
  tests/iir_ref.py's truths with E as the oscillator (mod_ref.OscAdapter), per sample
  |y - truth| <= MARGIN rho(oracle) B[n], plus past the table the oscillator's share:
  a phasor error of OSC_TOL in the front product, through the filters' l1 gain sum|h|
  (iir_ref.henv of the stages):
    SsbProductDemod    OSC_TOL max|x| sum|h_lp4| sum|h_dc|;
    SsbPhasingMod      per part, OSC_TOL (2 max|a| sum|h_lp4| + |I[n]| + |Q[n]|): the audio
                       oscillator's error through each LP4 into both parts, and the RF
                       oscillator's on (I, side Q);
    with_translate     2 OSC_TOL k sum|h_lp4|: z conj(p) moves by OSC_TOL |x|, the angle of
                       each of the two samples in z conj(prev) by OSC_TOL (|x| cancels: the
                       inputs have |x| >= 0.5 so that roundings stay relative), atan2_approx
                       has slope <= 1 in the angle away from its octant ties (test_mod_ref.py),
                       and k = 1 / dev scales it. The input is checked to keep 1e-4 rad off
                       those ties, where atan2_approx jumps.
  rho(oracle) is the oracle's own run against the truth with ITS oscillator.

The input is noise (a tone at the oscillator's frequency would hide a one-sample slip).
Cyclic tunings at the default budget are the reference at any length: bit for bit.
"""
import numpy as np
import pytest

import iir_ref as R
import mod_ref as M

pytestmark = pytest.mark.gpu
f32 = np.float32
N = M.N_SEAM
SEAM = [(f, fs, b) for f, fs in M.ACYCLIC for b in M.BUDGETS]
CYC = [(-1.5e6, 10e6, M.N_CYC, [[M.N_CYC], [4099, 61444]]), (100e3, 10e6, 80000, [[80000]])]


def ids(v):
    return f"{v:g}" if isinstance(v, float) else None


def cnoise(n, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    return (amp * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))).astype(np.complex64)


def with_budget(blk, b):
    return blk.configure_option("nco_table", b) if b is not None else blk


def run(fn, x, lens):
    """fn(chunk) per call (chunk: the call's samples, or its length for a generator)."""
    return np.concatenate([fn(np.ascontiguousarray(c)) for c in M.split(x, lens)])


def table(lib, f, fs, n, b):
    e, cs, cl, nt = M.osc_E(lib, f, fs, n, b if b is not None else 1 << 20)
    if b is not None:
        assert cl == 0 and nt == b, (f, fs, b, cl, nt)
        return e, nt
    assert cl > 0
    return e, n  # a cycle: the table serves every output


def product_consumers(lib, oracle, f, fs, b, x, key):
    """(name, handle factory, call, restatement, amplitude) of every product kernel."""
    e, nt = table(lib, f, fs, len(x), b)
    env = M.cw_env(oracle, key, fs, 2.0, 8.0)
    am = (1.0, 0.8, 1.3, False)

    def mk_am():
        m = lib.AmDsbMod(fs, f, am[0], am[1])
        m.set_gain(am[2])
        return m
    xr = x.real.astype(f32).copy()
    pairs = lambda z: np.ascontiguousarray(z).view(f32)  # noqa: E731  (per component)
    return nt, [
        ("Rotator.process", lambda: lib.Rotator(f, fs), lambda h, c: h.process(c), x, M.rot_rotate(x, e), np.abs(x)),
        ("Rotator.mix_usb_block", lambda: lib.Rotator(f, fs), lambda h, c: h.mix_usb_block(c), x, M.rot_mix_usb(x, e),
         np.abs(x)),
        ("Nco.process", lambda: lib.Nco(f, fs), lambda h, c: h.process(c), x, M.nco_mix(x, e), np.abs(x)),
        ("Nco.next_cs_block", lambda: lib.Nco(f, fs), lambda h, c: pairs(h.next_cs_block(len(c) // 2)), pairs(e),
         pairs(e), np.ones(2 * len(x))),
        ("Rotator.next_cs_block", lambda: lib.Rotator(f, fs), lambda h, c: pairs(h.next_cs_block(len(c) // 2)), pairs(e),
         pairs(e), np.ones(2 * len(x))),
        ("AmDsbMod", mk_am, lambda h, c: h.process(c), xr, M.am_restate(xr, e, *am), np.abs(M.am_base(xr, *am))),
        ("CwKeyedMod", lambda: lib.CwKeyedMod(fs, f, 2.0, 8.0), lambda h, c: h.process(c), key, M.cw_restate(env, e), env),
    ]


def keying(n):
    k = np.repeat(np.tile(np.array([1.0, 0.0, 0.6, 1.4, -0.2, 1.0], f32), 1 + n // 2400), 400)[:n]
    return (k + 0.01 * np.random.default_rng(5).standard_normal(n) * (np.arange(n) % 3 == 0)).astype(f32)


def check_products(lib, oracle, f, fs, b, n, splits):
    x = cnoise(n, 41)
    nt, cons = product_consumers(lib, oracle, f, fs, b, x, keying(n))
    for name, mk, call, inp, rest, amp in cons:
        per = 2 if "next_cs" in name else 1  # the generators are checked per component
        worst = 0.0
        for lens in splits:
            h = with_budget(mk(), b)
            got = run(lambda c: call(h, c), inp, [per * v for v in lens])
            worst = max(worst, M.check_osc_product(f"{name} {f:g}/{fs:g} budget {b} calls {lens}", got, rest, amp, per * nt))
        print(f"[parity] seam {name} {f:g}/{fs:g} budget {b}: bit-exact inside the table, max |y - restatement| / amp "
              f"past it {worst:.3e} (tol {M.OSC_TOL:.1e} + 2u) over calls {splits}")


@pytest.mark.parametrize("f,fs,b", SEAM, ids=ids)
def test_seam_products(gpu_lib, oracle, f, fs, b):
    """The four k_rotator modes, AmDsbMod (mod_tiles) and CwKeyedMod (osc_at: the control
    without runs) across the seam, every call split."""
    check_products(gpu_lib, oracle, f, fs, b, N, M.seam_calls(N, b))


@pytest.mark.parametrize("f,fs,n,splits", CYC, ids=ids)
def test_cycle_wrap_products(gpu_lib, oracle, f, fs, n, splits):
    """A cyclic table whose wrap falls inside a run: every output is the reference's, so the
    restatement with E is the oracle itself (asserted), bit for bit at any split."""
    x = cnoise(n, 41)
    e = M.osc_E(gpu_lib, f, fs, n)[0]
    assert M.bits_equal(M.rot_rotate(x, e), oracle.rotator(x, f, fs)) and M.bits_equal(M.nco_mix(x, e), oracle.nco(x, f, fs))
    check_products(gpu_lib, oracle, f, fs, None, n, splits)


# ---------------------------------------------------------------------------- PM / FM ==
def check_pm_fm(lib, oracle, f, fs, b, n, splits):
    e, nt = table(lib, f, fs, n, b)
    x = M.fm_input("noise", n, 43)
    kp, g = 1.2, 0.7
    e_pm = M.pm_e_ref(oracle, x, fs, kp, g, f)
    dev = 5e3 if fs < 1e6 else 75e3
    e_fm = M.fm_e_ref(oracle, x, fs, dev, f)
    for lens in splits:
        pm = with_budget(lib.PmDirectPhaseMod(fs, kp, f), b)
        pm.set_gain(g)
        M.check_pm(f"seam pm {f:g}/{fs:g} budget {b} calls {lens}", run(pm.process, x, lens), M.pm_truth(x, kp, g, e),
                   e_pm, g, nt)
        for passes in (1, 3):
            fm = with_budget(lib.FmPhaseAccumMod(fs, dev, f), b)
            if passes == 3:
                fm.configure_option("mod_passes", 3)
            fm.set_gain(g)
            M.check_fm(f"seam fm {f:g}/{fs:g} budget {b} passes={passes} calls {lens}", run(fm.process, x, lens),
                       M.fm_truth(x, lens, M.kf32(dev, fs), g, e), e_fm, lens, g, nt)


@pytest.mark.parametrize("f,fs,b", SEAM, ids=ids)
def test_seam_pm_fm(gpu_lib, oracle, f, fs, b):
    check_pm_fm(gpu_lib, oracle, f, fs, b, N, M.seam_calls(N, b))


@pytest.mark.parametrize("f,fs,n,splits", CYC, ids=ids)
def test_cycle_wrap_pm_fm(gpu_lib, oracle, f, fs, n, splits):
    check_pm_fm(gpu_lib, oracle, f, fs, None, n, splits)


# ------------------------------------------------------------------ the scan consumers ==
def sum_h(rec, coef):
    return float(np.sum(R.henv(rec, coef)))


def check_scan(name, got, truth, bnd, rho_o, extra, nt):
    """|y - truth| <= MARGIN rho(oracle) B[n] (+ extra[n] from output nt on). Returns the
    largest ratio to that limit and where."""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), f"{name}: non-finite output"
    lim = M.MARGIN * rho_o * bnd
    lim[nt:] += np.broadcast_to(extra, lim.shape)[nt:]
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(q))
    assert q[i] <= 1.0, f"{name}: |y - truth| = {err[i]:.3e} > {lim[i]:.3e} at output {i} (table {nt})"
    return float(q[i]), i


def demod_case(lib, oracle, spec, path, f, fs, b, n, splits, x, extra):
    ad = M.OscAdapter(oracle, lib, b if b is not None else 1 << 20)
    nt = table(lib, f, fs, n, b)[1]
    truth, bnd = spec.truth_bound(ad, x)
    rho_o = R.rho(spec.ref(oracle, x), *spec.truth_bound(oracle, x))[0]
    worst = (0.0, 0)
    for lens in splits:
        blk = with_budget(spec.mk(lib), b)
        if path:
            blk.configure_option("scan_path", path)
        got = run(blk.process, x, lens)
        blk.status()
        worst = max(worst, check_scan(f"{spec} budget {b} path {path} calls {lens}", got, truth, bnd, rho_o, extra, nt))
    print(f"[parity] seam {spec} budget {b} scan_path {path}: max |y - truth| / limit {worst[0]:.3g} at {worst[1]} "
          f"(rho oracle {rho_o:.3g}, oscillator share {float(np.max(extra)):.3e}) over calls {splits}")


def ssb_demod_case(lib, oracle, f, fs, b, n, splits, path):
    spec = R.ssb_spec(fs, f, 2800.0)
    x = cnoise(n, 45)
    c6 = oracle.lpdc_coeffs(fs, R.audio_lp_fc(2800.0), 2.0)
    extra = M.OSC_TOL * float(np.max(np.abs(x))) * sum_h("lp4", c6[:5]) * sum_h("dc", c6[5])
    demod_case(lib, oracle, spec, path, f, fs, b, n, splits, x, extra)


def fm_translate_case(lib, oracle, f, fs, b, n, splits, path):
    dev, bw = (2500.0, 5000.0) if fs < 1e6 else (75e3, 15e3)
    spec = R.fm_spec(fs, dev, bw, translate=f)
    rng = np.random.default_rng(47)
    x = ((0.5 + 0.5 * rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(np.complex64)
    # The discriminator's argument keeps 1e-4 rad off atan2_approx's octant edges (|re| = |im|
    # and the axes, where it jumps): samples that land nearer are drawn again.
    p = np.conj(M.osc_E(lib, f, fs, n, b if b is not None else 1 << 20)[0].astype(np.complex128))
    for _ in range(20):
        z = x.astype(np.complex128) * p
        ang = np.angle(z * np.conj(np.concatenate([[1.0], z[:-1]])))
        off = np.abs((ang + np.pi / 8) % (np.pi / 4) - np.pi / 8)
        bad = np.nonzero(off <= 1e-4)[0]
        if not len(bad):
            break
        x[bad] = ((0.5 + 0.5 * rng.uniform(0, 1, len(bad))) * np.exp(2j * np.pi * rng.uniform(0, 1, len(bad)))).astype(np.complex64)
    assert not len(bad) and np.min(np.abs(x)) >= 0.5 - 1e-6
    k = 1.0 / max(dev, 1.0)
    extra = 2.0 * M.OSC_TOL * k * sum_h("lp4", oracle.lp_cascade_coeffs(fs, R.audio_lp_fc(bw)))
    demod_case(lib, oracle, spec, path, f, fs, b, n, splits, x, extra)


def ssb_mod_case(lib, oracle, f, rf, fs, b, n, splits, passes):
    a = M.fm_input("noise", n, 49) * f32(0.5)
    ad = M.OscAdapter(oracle, lib, b if b is not None else 1 << 20)
    nt = table(lib, f, fs, n, b)[1]
    assert table(lib, rf, fs, n, b)[1] == nt
    bw, usb = 2800.0, True

    def mk():
        m = with_budget(lib.SsbPhasingMod(fs, bw, f, rf, usb), b)
        return m.configure_option("mod_passes", passes) if passes else m
    c5 = np.asarray(mk().taps()[:5], f32)
    assert np.array_equal(c5, oracle.lp_cascade_coeffs(fs, R.audio_lp_fc(bw)))
    truth, bnd = R.ssb_mod_truth_bound(ad, a, c5, fs, f, rf, usb)
    t_o, b_o = R.ssb_mod_truth_bound(oracle, a, c5, fs, f, rf, usb)
    ref = oracle.ssb_mod(a, fs, bw, f, rf, usb)
    rho_o = max(R.rho(ref.real, t_o.real, b_o)[0], R.rho(ref.imag, t_o.imag, b_o)[0])
    # |I[n]| + |Q[n]| <= sqrt(2) |truth[n]| (|r| = 1)
    extra = M.OSC_TOL * (2.0 * float(np.max(np.abs(a))) * sum_h("lp4", c5) + np.sqrt(2.0) * np.abs(truth))
    worst = (0.0, 0)
    for lens in splits:
        m = mk()
        got = run(m.process, a, lens)
        m.status()
        assert np.all(np.isfinite(got.view(f32)))
        for part, t in ((got.real, truth.real), (got.imag, truth.imag)):
            worst = max(worst, check_scan(f"SsbPhasingMod {f:g}+{rf:g}/{fs:g} budget {b} passes {passes} calls {lens}",
                                          part, t, bnd, rho_o, extra, nt))
    print(f"[parity] seam SsbPhasingMod if {f:g} rf {rf:g} / {fs:g} budget {b} mod_passes {passes}: max |y - truth| / limit "
          f"{worst[0]:.3g} at {worst[1]} (rho oracle {rho_o:.3g}) over calls {splits}")


RF_OF = {1500.0: 700.0, 700.0: -5000.0, -5000.0: 1500.0, 1.234e6: 1.234e6}  # the RF oscillator beside the audio one


@pytest.mark.parametrize("passes", [0, 3])
@pytest.mark.parametrize("f,fs,b", SEAM + [(f, fs, 3900) for f, fs in M.ACYCLIC], ids=ids)
def test_seam_ssb_phasing_mod(gpu_lib, oracle, f, fs, b, passes):
    """Both cursors of k_ssb_mod_sp (audio and RF oscillator, one budget) and the front /
    back kernels of the three-pass form. 3900: inside chunk 1's warm-up, which starts at 3840."""
    ssb_mod_case(gpu_lib, oracle, f, RF_OF[f], fs, b, N, M.seam_calls(N, b), passes)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("f,fs,b", SEAM + [(f, fs, 8000) for f, fs in M.ACYCLIC], ids=ids)
def test_seam_ssb_product_demod(gpu_lib, oracle, f, fs, b, path):
    """Pre::Ssb's cursor in k_lpdc_sp (8000: inside chunk 1's warm-up, which starts at 7936)
    and in the three-kernel scan."""
    ssb_demod_case(gpu_lib, oracle, f, fs, b, N, M.seam_calls(N, b), path)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("f,fs,b", SEAM + [(f, fs, 8000) for f, fs in M.ACYCLIC], ids=ids)
def test_seam_fm_translate(gpu_lib, oracle, f, fs, b, path):
    fm_translate_case(gpu_lib, oracle, f, fs, b, N, M.seam_calls(N, b), path)


@pytest.mark.parametrize("f,fs,n,splits", CYC, ids=ids)
def test_cycle_wrap_scans(gpu_lib, oracle, f, fs, n, splits):
    for v in (0, 1):
        ssb_demod_case(gpu_lib, oracle, f, fs, None, n, splits, v)
        fm_translate_case(gpu_lib, oracle, f, fs, None, n, splits, v)
    for passes in (0, 3):
        ssb_mod_case(gpu_lib, oracle, f, f, fs, None, n, splits, passes)
