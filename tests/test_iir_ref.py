"""tests/iir_ref.py (the float64 reference of the IIR scan tests) checked against the C
oracle, on the CPU: for every block and input class the oracle's own rho (its worst
per-sample distance from the f64 truth in units of the bound B) is finite and printed,
and its whole-record nrmse against the truth is within the tolerance test_gpu_parity.py
uses for that block. The front ends restated in iir_ref are checked bit for bit (the
oracle's real-input recurrence on the restated d[n] is the oracle's demodulator), the
restated criteria against the designs test_gpu_parity.py documents, and two mutations of
the oracle's output show that rho sees what the nrmse does not."""
import numpy as np
import pytest

import iir_ref as R

FS = 48e3
N = 3 * R.K_SP_CH + 5
EDGES = (R.K_SP_CH, 2 * R.K_SP_CH)

SPECS = [
    R.lp_cascade_spec(48e3, 4500.0), R.lp_cascade_spec(1.25e6, 13.5e3), R.lp_cascade_spec(48e3, 300.0),
    R.biquad_spec(R.resonator(0.99, 1234.0, 48e3), "resonator r=0.99"),
    R.biquad_spec(R.resonator(0.9999, 1234.0, 48e3), "resonator r=0.9999"),
    R.dc_spec(48e3, 2.0), R.dc_spec(48e3, 0.1), R.dc_spec(48e3, 10e3),
    R.lpdc_spec(48e3, 2520.0, 2.0, None), R.lpdc_spec(48e3, 2520.0, 2.0, "identity"),
    R.lpdc_spec(48e3, 2520.0, 2.0, "sqrt"), R.lpdc_spec(48e3, 2520.0, 2.0, "abs"),
    R.lpdc_spec(48e3, 2520.0, 0.1, None), R.lpdc_spec(48e3, 2520.0, 10e3, None),
    R.fm_spec(48e3, 2500.0, 5000.0), R.fm_spec(48e3, 2500.0, 5000.0, translate=3000.0),
    R.pm_spec(48e3, 0.9, 5000.0), R.ssb_spec(48e3, 1500.0, 2800.0),
    R.am_spec(48e3, 5000.0, False), R.am_spec(48e3, 5000.0, True),
    R.cw_spec(48e3, 700.0, 300.0), R.cw_spec(48e3, 700.0, 300.0, gain=2.0),
]


def ulp_floor(fn, x):
    """test_gpu_parity.py's floor, the reference's own sensitivity to a last-bit scaling of
    its input: nrmse between fn(x s) / s and fn(x). There s = 1 + 2^-23 alone; here the
    largest over four such scalings, because on a constant input the f32 recurrence settles
    on a fixed point of its rounding and a single scaling samples one such point."""
    y = fn(x)
    return max(R.nrmse(fn((x * s).astype(x.dtype)) / s, y)
               for s in (np.float32(1.0 + 2.0 ** -23), np.float32(1.0 - 2.0 ** -24), np.float32(1.0 + 2.0 ** -22),
                         np.float32(1.0 - 2.0 ** -23)))


def block_tol(oracle, spec, x=None):
    """test_gpu_parity.py's floor_tol for the block: max(base, 2 x the 1-ulp floor), the
    floor taken on the dense normal input (where test_gpu_parity.py takes it) and on x."""
    fn = lambda v: spec.ref(oracle, v)  # noqa: E731
    f = ulp_floor(fn, R.spec_input(spec, "dense", N, 1000, EDGES))
    return max(spec.tol, 2.0 * f, 2.0 * ulp_floor(fn, x) if x is not None else 0.0)


def constant_input_bias(c5):
    """On a constant input the TDF-II states settle at about the output's size and every
    step rounds both of them the same way: an offset of up to 2 u |y| per biquad enters
    the state at every sample and is amplified by the DC gain of the state-to-output path,
    1 / (1 + a1 + a2) (650 at 48 kHz / 300 Hz). Two biquads: 4 u / (1 + a1 + a2) of the
    output, relative. The 1-ulp floor does not see it (it is a bias, not a sensitivity):
    the oracle measures 2.8e-5 at 1.25 MHz / 13.5 kHz and 6.0e-5 at 48 kHz / 300 Hz on
    the step, against floors of 1.9e-5 and 1.8e-5 and this bound of 5.4e-5 and 1.6e-4."""
    _, _, _, a1, a2 = (float(v) for v in c5)
    return 4.0 * R.U / (1.0 + a1 + a2)


@pytest.mark.parametrize("spec", SPECS, ids=repr)
def test_oracle_rho_and_nrmse(oracle, spec):
    """The oracle against the f64 truth, every input class: rho finite (printed with its
    index), nrmse within the block's tolerance in test_gpu_parity.py (1e-6 for the real
    filters, 1e-5 for the demodulators and the DC-pole cascades; both as there no tighter
    than twice the reference's own 1-ulp sensitivity, which is taken once per block on the
    dense normal input, the input test_gpu_parity.py takes it on: on a burst or a step a
    single scaled run is too noisy an estimate of it; on the step also no tighter than
    constant_input_bias). Leading zeros stay exactly zero."""
    for k, cls in enumerate(R.CLASSES):
        x = R.spec_input(spec, cls, N, 1000 + k, EDGES)
        tol = block_tol(oracle, spec, x)
        if cls == "step" and spec.coef is not None and spec.kind != "onepole":
            tol = max(tol, constant_input_bias(spec.coef(oracle)))
        truth, b = spec.truth_bound(oracle, x)
        ref = spec.ref(oracle, x)
        rho, i = R.rho(ref, truth, b)
        e = R.nrmse(ref, truth)
        print(f"[parity] {spec} {cls}: oracle rho {rho:.3g} at {i}, nrmse vs f64 {e:.3e} (tol {tol:.1e})")
        assert np.isfinite(rho) and np.all(np.isfinite(truth)) and np.all(b >= 0), (spec, cls)
        assert e <= tol, f"{spec} {cls}: nrmse {e:.3e} > {tol:.1e}"
        nz = np.nonzero(x)[0]
        if spec.zero_preserving and len(nz) and nz[0] > 0:
            assert not np.any(ref[:nz[0]]) and not np.any(truth[:nz[0]]) and not np.any(b[:nz[0]])


def test_fronts_are_the_oracles(oracle):
    """The restated f32 front ends, bit for bit: the oracle's real-input recurrence on
    iir_ref's d[n] equals the oracle's demodulator on the IQ input."""
    x = R.input_class("dense", 5000, 7, (), complex_=True)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    fc = R.audio_lp_fc(5000.0)
    assert same(oracle.lp_cascade(R.front_fm(oracle, x, FS, 2500.0), FS, fc), oracle.fm_demod(x, FS, 2500.0, 5000.0))
    assert same(oracle.lp_cascade(R.front_fm(oracle, x, FS, 2500.0, 3000.0), FS, fc),
                oracle.fm_demod(x, FS, 2500.0, 5000.0, translate_hz=3000.0))
    assert same(oracle.lp_cascade(R.front_pm(x, 0.9), FS, fc), oracle.pm_demod(x, FS, 0.9, 5000.0))
    assert same(oracle.lp_dc_cascade(R.front_ssb(oracle, x, FS, 1500.0), FS, R.audio_lp_fc(2800.0), 2.0),
                oracle.ssb_demod(x, FS, 1500.0, 2800.0))
    xa = (x + np.complex64(3.0)).astype(np.complex64)
    assert same(oracle.lp_dc_cascade(R.front_am_power(xa), FS, fc, 2.0, map="sqrt"), oracle.am_demod(xa, FS, 5000.0))
    assert same(oracle.lp_dc_cascade(R.front_am_abs(x), FS, fc, 2.0), oracle.am_demod(x, FS, 5000.0, abs_approx=(0.9482, 0.3920)))
    # the CW one-pole has no real-input oracle entry: the f64 truth within a few u instead
    # (a magnitude off by one ulp would by itself be 1 u |d| of the bound's u henv * |d|)
    t, b = R.truth_bound(R.front_cw(x), rec="onepole", coef=R.cw_alpha(FS, 300.0))
    assert R.rho(oracle.cw_demod(x, FS, 700.0, 300.0), t, b)[0] < 16.0
    assert np.array_equal(np.array(R.NR.lp_cascade_coeffs(FS, fc), np.float32), oracle.lp_cascade_coeffs(FS, fc))


def test_ssb_mod_truth(oracle):
    """SsbPhasingMod's truth (two f64 LP4s with the oracle's oscillators): the oracle's rho
    on the real and imaginary parts is finite and small, every input class."""
    c5 = oracle.lp_cascade_coeffs(FS, R.audio_lp_fc(2800.0))
    for k, cls in enumerate(R.CLASSES):
        a = R.input_class(cls, N, 2000 + k, (R.K_SCAN_CH, 2 * R.K_SCAN_CH - R.K_SP_WARM))
        t, b = R.ssb_mod_truth_bound(oracle, a, c5, FS, 1500.0, 9000.0, True)
        ref = oracle.ssb_mod(a, FS, 2800.0, 1500.0, 9000.0, True)
        rr, ir = R.rho(ref.real, t.real, b), R.rho(ref.imag, t.imag, b)
        print(f"[parity] SsbPhasingMod {cls}: oracle rho re {rr[0]:.3g} at {rr[1]}, im {ir[0]:.3g} at {ir[1]}")
        assert np.isfinite(rr[0]) and np.isfinite(ir[0])
        assert max(R.nrmse(ref.real, t.real), R.nrmse(ref.imag, t.imag)) <= 1e-5


def test_criteria_restated(oracle):
    """scan_blocks.cpp's criteria on the designs whose kernels test_gpu_parity.py names:
    the resonator at r = 0.9999 does not forget within a chunk (three-kernel scan), r =
    0.99 and LpCascade 1.25M/13.5k do (k_scan_sp); SsbProductDemod at 48 kHz / 2800 Hz has
    ||A_lp^256|| far below 1e-10 (k_lpdc_sp); the bisected designs sit where they were asked to."""
    assert R.scan_sp_choice(R.biquad_ss(R.resonator(0.9999, 1234.0, FS))[0]) == ("three", None)
    assert R.scan_sp_choice(R.biquad_ss(R.resonator(0.99, 1234.0, FS))[0])[0] == "k_scan_sp"
    assert R.scan_sp_choice(R.lp4_ss(oracle.lp_cascade_coeffs(1.25e6, 13.5e3))[0])[0] == "k_scan_sp"
    c = oracle.lpdc_coeffs(FS, R.audio_lp_fc(2800.0), 2.0)[:5]
    assert R.lpdc_single_pass(c) and R.fro(R.lp4_ss(c)[0], R.K_SP_WARM) < 1e-18
    # the state space is the recurrence: A^k B is the state k steps after a unit impulse
    A, B = R.lp4_ss(c)
    h = R.lp4_64(np.r_[1.0, np.zeros(40)], c)
    s = B.copy()
    for k in range(1, 41):  # x = 0: y0 = z0_1, y = b0 y0 + z1_1
        assert abs(float(c[0]) * s[0] + s[2] - h[k]) <= 1e-14
        s = A @ s
    for H in (R.K_SP_WARM, 512, 1024, R.K_SP_CH):
        for target in (0.5e-10, 2e-10):
            r = R.resonator_at(H, target)
            got = R.fro(R.biquad_ss(R.resonator(r, 1234.0, FS))[0], H)
            fc = R.lp_cutoff_at(H, target, FS, oracle.lp_cascade_coeffs)
            gl = R.fro(R.lp4_ss(oracle.lp_cascade_coeffs(FS, fc))[0], H)
            print(f"[parity] horizon {H} target {target:.1e}: resonator r {r:.7f} -> {got:.3e}; LP cutoff {fc:.3f} Hz -> {gl:.3e}")
            assert 0.8 * target < got < 1.25 * target and 0.8 * target < gl < 1.25 * target
    assert R.dc_lookback_chunks(np.float32(0.9999), R.K_SP_CH) == 57 and R.dc_lookback_chunks(0.0, R.K_SP_CH) == 1


def _mutation_case(oracle, spec, seed):
    x = R.spec_input(spec, "dense", N, seed, EDGES)
    truth, b = spec.truth_bound(oracle, x)
    ref = spec.ref(oracle, x)
    return x, truth, b, ref, R.rho(ref, truth, b)[0], block_tol(oracle, spec)


@pytest.mark.parametrize("spec", [R.lp_cascade_spec(48e3, 4500.0), R.dc_spec(48e3, 2.0), R.lpdc_spec(48e3, 2520.0, 2.0, None)],
                         ids=repr)
def test_mutation_one_sample(oracle, spec):
    """One sample of the oracle's output, at index 8192, moved by 16 rho_oracle B[n]: the rho
    criterion (rho <= 5 rho_oracle) fails; the whole-record nrmse stays within tolerance."""
    x, truth, b, ref, rho_o, tol = _mutation_case(oracle, spec, 31)
    mut = ref.copy()
    mut[R.K_SP_CH] = np.float32(truth[R.K_SP_CH] + 16.0 * rho_o * b[R.K_SP_CH])
    rho_m, i = R.rho(mut, truth, b)
    e = R.nrmse(mut, ref)
    print(f"[parity] {spec} one sample moved: rho {rho_m:.3g} at {i} (oracle {rho_o:.3g}), nrmse vs oracle {e:.3e}")
    assert i == R.K_SP_CH and rho_m > 5.0 * rho_o
    assert e <= tol


def test_mutation_short_warm_up(oracle):
    """A design with ||A^256|| = 1e-5 (five orders outside the criterion) run the way the
    warm-up kernels would run it if the criterion let it through, on the input that shows
    it: a burst of amplitude 1e3 ending where the warm-up of the chunk at 8192 begins (the
    state entering the warm-up is 1e6 times the signal after it), and the outputs from
    8192 on computed from a zero state at 8192 - 256. rho fails; the nrmse passes. (At
    ||A^256|| = 1e-6 the same mutation measures rho 24 at sample 8192, a 5 % error of the
    signal there, against the oracle's own 26 in the quiet stretch before the burst: the
    bound's 1e-10 term after a burst of 1e3 hides it from a margin of 5.)"""
    fc = R.lp_cutoff_at(R.K_SP_WARM, 1e-5, FS, oracle.lp_cascade_coeffs)
    spec = R.lp_cascade_spec(FS, fc)
    assert not R.lpdc_single_pass(spec.coef(oracle))
    e0 = R.K_SP_CH
    x = R.spec_input(spec, "burst", N, 32, (e0 - R.K_SP_WARM,))
    truth, b = spec.truth_bound(oracle, x)
    ref = spec.ref(oracle, x)
    rho_o = R.rho(ref, truth, b)[0]
    mut = ref.copy()
    mut[e0:] = spec.ref(oracle, x[e0 - R.K_SP_WARM:])[R.K_SP_WARM:]
    rho_m, i = R.rho(mut, truth, b)
    e = R.nrmse(mut, ref)
    print(f"[parity] {spec} zero state at {e0 - R.K_SP_WARM}: rho {rho_m:.3g} at {i} (oracle {rho_o:.3g}), nrmse vs oracle {e:.3e}")
    assert rho_m > 5.0 * rho_o and e0 <= i < e0 + 256
    assert e <= block_tol(oracle, spec)
