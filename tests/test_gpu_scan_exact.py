"""Per-sample tests of the IIR scan kernels (csrc/k_scan.hip), every kernel and path.

Each block is compared, sample for sample, with the float64 truth of tests/iir_ref.py
(validated against the C oracle in tests/test_iir_ref.py) through one figure,

    rho(y) = max_n |y[n] - truth[n]| / B[n],

B the a-priori bound u henv * |d| + 1e-10 sum(henv) max |d| of iir_ref.truth_bound. What
is asserted is rho(gpu) <= MARGIN rho(oracle): the oracle's own f32 run of the same
stream, against the same truth and B. MARGIN = 5 is ssb_tol's margin (two correct f32
results of these cascades differ by at most ~3.5 x the reference's own distance from
exact arithmetic). Every case prints `[parity] ... rho gpu / oracle` with the sample
index of each. One stream per input class is run as one call at every length around
the chunk edges of the kernel it reaches and in ragged calls that carry the f32 state;
the oracle's figure is the one of the whole stream. Where one f32 answer exists the
assertion is exact (leading zeros, the integer DC blocker at r = 0, reset, run-to-run
bits, batched rows).

Which kernel a design reaches is computed from scan_blocks.cpp's criteria restated in
iir_ref (scan_sp_choice, lpdc_single_pass) on the coefficients the library reports,
asserted against the side of the threshold the design was bisected for, and named in
each docstring: scan_path 0 is single pass where valid, 1 the three-kernel scan
(k_scan_agg / k_scan_carry / k_scan_apply).
"""
import numpy as np
import pytest

import iir_ref as R

pytestmark = pytest.mark.gpu

K_SCAN_C = 16        # scan.hpp:25 kScanC: samples per lane, three-kernel scan and k_ssb_mod_sp
K_SCAN_NT = 256      # scan.hpp:26 kScanNT: lanes per workgroup
K_SCAN_CH = 4096     # scan.hpp:27 kScanCH: the three-kernel scan's and k_ssb_mod_sp's chunk
K_SP_WARM = 256      # scan.hpp:88 kSpWarm: LP4 warm-up samples of k_lpdc_sp / k_ssb_mod_sp
K_SP_C = 32          # scan.hpp:93 kSpC: samples per lane of k_scan_sp
K_SP_CH = 8192       # scan.hpp:94 kSpCH: k_scan_sp's chunk
K_LPDC_SC = 32       # scan.hpp:95 kLpdcSC: samples per lane of k_lpdc_sp (chunk kLpdcSC * kScanNT)
assert (K_SCAN_C, K_SCAN_NT, K_SCAN_CH, K_SP_WARM, K_SP_C, K_SP_CH, K_LPDC_SC) == (
    R.K_SCAN_C, R.K_SCAN_NT, R.K_SCAN_CH, R.K_SP_WARM, R.K_SP_C, R.K_SP_CH, R.K_LPDC_SC)

FS = 48e3
MARGIN = 5.0
# (block name prefix, kernel label, input class) -> margin, each justified in DESIGN.md §3.3
MARGINS = {
    # After a burst of 1e3 the DC blocker's y (|y| ~ 500) has taken u |y| of rounding per
    # step, carried on at r^k ~ 1, in the reference (192 sequential steps) and in the kernel
    # (6 lane pairs of 32 steps, f32 entering states) alike: per lane both inject up to 3e-4.
    # What is left when the burst ends is the end point of that walk, and B (which passes
    # input errors through h_dc = delta - (1 - r) r^k only) has by then fallen to 7e-6. On
    # this stream the oracle's end point is 5e-5 (rho 7), the kernel's 1.9e-4 in one call
    # and 4.0e-4 in the ragged calls (rho 33 and 57): measured 8.13 x, margin 12.
    ("LpDcCascade 48000/2520/2 map=None", "k_lpdc_sp", "burst"): 12.0,
}

# kernel label -> (chunk, stride, warm-up): chunk c > 0 puts out [chunk + (c - 1) stride, chunk + c stride)
GEOMETRY = {
    "three": (K_SCAN_CH, K_SCAN_CH, 0),                                  # k_scan.hip run3: n / kScanCH workgroups
    "k_scan_sp": (K_SP_CH, K_SP_CH, 0),                                  # scan_sp_chunks
    "k_lpdc_sp dc": (K_LPDC_SC * K_SCAN_NT, K_LPDC_SC * K_SCAN_NT, 0),   # lpdc_sp_demod_chunks(n, kLpdcSC, 0)
    "k_lpdc_sp": (K_LPDC_SC * K_SCAN_NT, K_LPDC_SC * K_SCAN_NT - K_SP_WARM, K_SP_WARM),  # (.., kSpWarm)
    "k_ssb_mod_sp": (K_SCAN_CH, K_SCAN_CH - K_SP_WARM, K_SP_WARM),       # lpdc_sp_chunks
}


def geometry(kernels):
    """Chunk edges (with the warm-up starts), one-call lengths and call splits for a run
    that passes through the given kernels (two for the LP4 scan + DC scan forms)."""
    edges, lens, splits = set(), {1}, []
    n = 0
    for k in kernels:
        chunk, stride, warm = GEOMETRY[k.split("<")[0].strip()]
        n = max(n, 3 * chunk + 5)
        edges |= {chunk, chunk + stride}
        if warm:
            edges |= {chunk - warm, chunk + stride - warm}
        lens |= {chunk - 1, chunk, chunk + 1, chunk + stride + 1, 3 * chunk + 5}
        splits += [[1, 7, chunk, 1, stride + 1], [chunk], [chunk + 1]]
    return n, sorted(edges), sorted(v for v in lens if v <= n), [s + [n - sum(s)] for s in splits]


class _NoOracle:
    """spec.chain() without coefficients: only the map is read from it."""

    @staticmethod
    def lpdc_coeffs(*a):
        return [0.0] * 6

    @staticmethod
    def lp_cascade_coeffs(*a):
        return [0.0] * 5


def reach(spec, coef, path):
    """The kernels spec's block launches with scan_path = path, from ScanStage's
    constructor and run, AmBlock::run and LpDcBlock::run (scan_blocks.cpp) on the
    coefficients coef: a list of labels, the GEOMETRY key first in each."""
    if spec.kind in ("bq", "lp4", "onepole"):
        A = {"bq": R.biquad_ss, "lp4": R.lp4_ss, "onepole": R.onepole_ss}[spec.kind](coef)[0]
        k, trs = R.scan_sp_choice(A)
        return ["three"] if path == 1 or k == "three" else [f"k_scan_sp<trs={trs}>"]
    if spec.kind == "dc":
        return ["three"] if path == 1 else ["k_lpdc_sp dc <Pre::Real>"]
    sp = R.lpdc_single_pass(coef)
    mapped = spec.kind == "am_sqrt" or spec.chain(_NoOracle).get("map") in ("sqrt", "abs")
    if sp and path == 0:
        return ["k_lpdc_sp"]
    if not mapped:
        return ["three"]  # RecK::LPDC with Pre::Real / Ssb / AmAbs
    # LP4 scan with the map as its post-stage, then a DC scan through a temporary
    if spec.kind == "am_sqrt":  # <LP4, AmSqrt, Sqrt> is scan_sp_supported
        k, trs = R.scan_sp_choice(R.lp4_ss(coef)[0])
        lp = "three" if path == 1 or k == "three" else f"k_scan_sp<trs={trs}>"
    else:  # <LP4, Real, Sqrt | Abs>: the three-kernel scan only
        lp = "three"
    return [lp, "three" if path == 1 else "k_lpdc_sp dc <Pre::Real>"]


def make(lib, spec, path):
    blk = spec.mk(lib)
    if path:
        blk.configure_option("scan_path", path)
    return blk


def chain_of(spec, blk, oracle):
    """truth_bound's keywords with the coefficients the library reports (asserted equal to
    the oracle's; the CW pole, an expf, is taken from the block)."""
    ch = dict(spec.chain(oracle))
    t = blk.taps()
    if spec.kind == "onepole":
        assert abs(float(t[0]) - float(ch["coef"])) <= 2.0 ** -23, (t, ch)
        ch["coef"] = np.float32(t[0])
    elif spec.kind == "dc":
        assert np.float32(t[0]) == np.float32(ch["r"]), (t, ch)
    else:
        assert np.array_equal(np.asarray(t[:5], np.float32), np.asarray(ch["coef"], np.float32)), (spec, t, ch)
        if ch.get("r") is not None:
            assert np.float32(t[5]) == np.float32(ch["r"]), (t, ch)
    return ch


def coef_of(spec, blk):
    t = blk.taps()
    return np.float32(t[0]) if spec.kind in ("onepole", "dc") else np.asarray(t[:5], np.float32)


def run_calls(blk, x, lens):
    outs = []
    for c in R.split_calls(x, lens):
        outs.append(blk.process(np.ascontiguousarray(c)))
        blk.status()
    return np.concatenate(outs, axis=-1)


def check_stream(lib, oracle, spec, path, classes=R.CLASSES, expect=None):
    """Every input class through spec's block on scan_path path: one call at every length
    of the reached kernels' geometry and the ragged splits, rho(gpu) <= margin rho(oracle)."""
    probe = make(lib, spec, path)
    kernels = reach(spec, coef_of(spec, probe), path)
    if expect is not None:
        assert kernels == expect, f"{spec} path {path}: reaches {kernels}, the design was made for {expect}"
    ch = chain_of(spec, probe, oracle)
    n, edges, lens, splits = geometry(kernels)
    for k, cls in enumerate(classes):
        x = R.spec_input(spec, cls, n, 4000 + 10 * k + path, edges)
        truth, b = R.truth_bound(spec.front(oracle, x), **ch)
        assert np.all(np.isfinite(truth)), f"{spec} {cls}: the truth is not finite (input outside the map's domain)"
        rho_o, i_o = R.rho(spec.ref(oracle, x), truth, b)
        worst = (0.0, 0, "")
        for m in lens:
            got = run_calls(make(lib, spec, path), x[:m], [m])
            assert np.all(np.isfinite(got)), f"{spec} {cls} n={m}"
            r, i = R.rho(got, truth[:m], b[:m])
            worst = max(worst, (r, i, f"n={m}"))
        for s in splits:
            got = run_calls(make(lib, spec, path), x, s)
            assert np.all(np.isfinite(got)), f"{spec} {cls} calls {s}"
            r, i = R.rho(got, truth, b)
            worst = max(worst, (r, i, f"calls {s}"))
        margin = max([MARGIN] + [v for (nm, kn, c), v in MARGINS.items()
                                 if spec.name.startswith(nm) and kn in " ".join(kernels) and c == cls])
        print(f"[parity] {spec} path {path} {'+'.join(kernels)} {cls}: rho gpu {worst[0]:.3g} at {worst[1]} ({worst[2]}) "
              f"/ oracle {rho_o:.3g} at {i_o} = {worst[0] / rho_o if rho_o > 0 else float(worst[0] > 0):.2f}")
        assert worst[0] <= margin * rho_o, (f"{spec} path {path} {kernels} {cls}: rho gpu {worst[0]:.4g} at sample {worst[1]} "
                                            f"({worst[2]}) > {margin} x oracle {rho_o:.4g}")


# ========================================== Biquad, LpCascade: k_scan_sp's four horizons ==
HORIZONS = [(K_SP_WARM, "inside", "k_scan_sp<trs=3>"), (K_SP_WARM, "outside", "k_scan_sp<trs=4>"),
            (2 * K_SP_WARM, "inside", "k_scan_sp<trs=4>"), (2 * K_SP_WARM, "outside", "k_scan_sp<trs=5>"),
            (4 * K_SP_WARM, "inside", "k_scan_sp<trs=5>"), (4 * K_SP_WARM, "outside", "k_scan_sp<trs=0>"),
            (K_SP_CH, "inside", "k_scan_sp<trs=0>"), (K_SP_CH, "outside", "three")]
assert [h for h, _, _ in HORIZONS[:6:2]] == [K_SP_C << t for t in (3, 4, 5)]  # scan_blocks.cpp:37-38
TARGET = {"inside": 0.5e-10, "outside": 2e-10}
HIDS = [f"{h}_{s}" for h, s, _ in HORIZONS]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("horizon,side,kernel", HORIZONS, ids=HIDS)
def test_biquad_at_each_horizon(gpu_lib, oracle, horizon, side, kernel, path):
    """Biquad resonators (poles r e^{+-j w0}, 1234 Hz / 48 kHz) whose ||A^h||_F is 0.5e-10
    (inside) and 2e-10 (outside) at h = 256, 512, 1024 (the lane-scan horizons 2^trs kSpC,
    trs = 3, 4, 5) and 8192 (kSpCH). scan_path 0: k_scan_sp<BQ, Real, Id, trs> with the trs
    the criterion gives (inside h: that horizon's; outside: the next, trs = 0 the full lane
    scan), and outside 8192 the three-kernel scan; scan_path 1: k_scan_agg / k_scan_carry /
    k_scan_apply <BQ, Real, Id>."""
    r = R.resonator_at(horizon, TARGET[side])
    spec = R.biquad_spec(R.resonator(r, 1234.0, FS), f"resonator {horizon} {side}")
    f = R.fro(R.biquad_ss(spec.coef(oracle))[0], horizon)
    assert (f < R.TRUNC) == (side == "inside"), (horizon, side, f)
    check_stream(gpu_lib, oracle, spec, path, expect=["three"] if path else [kernel])


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("horizon,side,kernel", HORIZONS, ids=HIDS)
def test_lp_cascade_at_each_horizon(gpu_lib, oracle, horizon, side, kernel, path):
    """LpCascade cutoffs at 48 kHz (1233 Hz down to 42 Hz) bisected to the same norms at the
    same horizons: k_scan_sp<LP4, Real, Id, trs>, the three-kernel scan <LP4, Real, Id>
    outside 8192 and on scan_path 1."""
    fc = float(np.float32(R.lp_cutoff_at(horizon, TARGET[side], FS, oracle.lp_cascade_coeffs)))
    spec = R.lp_cascade_spec(FS, fc)
    f = R.fro(R.lp4_ss(spec.coef(oracle))[0], horizon)
    assert (f < R.TRUNC) == (side == "inside"), (horizon, side, f)
    check_stream(gpu_lib, oracle, spec, path, expect=["three"] if path else [kernel])


# ================================ the LPDC family at the warm-up threshold ||A_lp^256|| ==
def warm_cutoff(oracle, side):
    return float(np.float32(R.lp_cutoff_at(K_SP_WARM, TARGET[side], FS, oracle.lp_cascade_coeffs)))


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("side", ["inside", "outside"])
@pytest.mark.parametrize("mp", [None, "identity", "sqrt", "abs"])
def test_lp_dc_cascade_at_the_warm_up(gpu_lib, oracle, mp, side, path):
    """LpDcCascade (2 Hz DC pole) with the LP cutoff bisected to ||A_lp^256||_F = 0.5e-10 /
    2e-10. Inside, scan_path 0: k_lpdc_sp<RealLp | RealLp | RealLpSqrt | RealLpAbs> for map
    None / identity / sqrt / abs (8192-sample chunks after a 256-sample LP4 warm-up).
    Outside, or scan_path 1: the three-kernel scan <LPDC, Real, Id> without a map; with
    one, the three-kernel scan <LP4, Real, Sqrt | Abs> then a DC scan (k_lpdc_sp<Real>,
    DC-only, on scan_path 0; the three-kernel scan <DC, Real, Id> on 1). The sqrt map's
    inputs are offset to keep the LP4 output above 1 (below zero the reference is NaN)."""
    spec = R.lpdc_spec(FS, warm_cutoff(oracle, side), 2.0, mp)
    assert R.lpdc_single_pass(spec.coef(oracle)) == (side == "inside")
    if side == "inside" and path == 0:
        expect = ["k_lpdc_sp"]
    elif mp in ("sqrt", "abs"):
        expect = ["three", "three" if path else "k_lpdc_sp dc <Pre::Real>"]
    else:
        expect = ["three"]
    check_stream(gpu_lib, oracle, spec, path, expect=expect)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_ssb_demod_at_the_warm_up(gpu_lib, oracle, side, path):
    """SsbProductDemod with the audio bandwidth that puts its LP (0.9 bw) at the same two
    norms: k_lpdc_sp<Pre::Ssb> inside on scan_path 0, the three-kernel scan <LPDC, Ssb, Id>
    outside and on scan_path 1."""
    fc = warm_cutoff(oracle, side)
    bw = float(np.float32(fc / 0.9))  # the LP is designed at f32(bw) * f32(0.9): within an ulp of fc
    spec = R.ssb_spec(FS, 1500.0, bw)
    assert R.lpdc_single_pass(spec.coef(oracle)) == (side == "inside")
    check_stream(gpu_lib, oracle, spec, path, expect=["k_lpdc_sp"] if side == "inside" and path == 0 else ["three"])


# ==================================================================== the DC pole's range ==
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("cut", [2.0, 0.1, 10e3], ids=["2Hz", "clamp_0.9999", "r0"])
def test_dc_blocker_poles(gpu_lib, oracle, cut, path):
    """DcBlocker at 2 Hz / 48 kHz, at the 0.9999 clamp (0.1 Hz) and at r = 0 (cut >= fs / 2
    pi). scan_path 0: k_lpdc_sp<Pre::Real> (DC-only: abutting 8192-sample chunks, the DC
    look-back without an LP4); scan_path 1: the three-kernel scan <DC, Real, Id>."""
    spec = R.dc_spec(FS, cut)
    r = float(make(gpu_lib, spec, 0).taps()[0])
    assert cut == 2.0 or r == {0.1: float(np.float32(0.9999)), 10e3: 0.0}[cut]
    check_stream(gpu_lib, oracle, spec, path, expect=["three"] if path else ["k_lpdc_sp dc <Pre::Real>"])


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("cut", [2.0, 0.1, 10e3], ids=["2Hz", "clamp_0.9999", "r0"])
def test_lp_dc_cascade_poles(gpu_lib, oracle, cut, path):
    """LpDcCascade 48 kHz / 2520 Hz with the same three DC poles: k_lpdc_sp<Pre::RealLp>
    (scan_path 0), the three-kernel scan <LPDC, Real, Id> (1)."""
    check_stream(gpu_lib, oracle, R.lpdc_spec(FS, 2520.0, cut, None), path, expect=["three"] if path else ["k_lpdc_sp"])


# ============================================================================ demodulators ==
DEMODS = [
    (R.fm_spec(FS, 2500.0, 5000.0), "k_scan_sp<trs=3>"),
    (R.fm_spec(FS, 2500.0, 5000.0, translate=3000.0), "k_scan_sp<trs=3>"),
    (R.pm_spec(FS, 0.9, 5000.0), "k_scan_sp<trs=3>"),
    (R.ssb_spec(FS, 1500.0, 2800.0), "k_lpdc_sp"),
    (R.am_spec(FS, 5000.0, False), "k_lpdc_sp"),
    (R.am_spec(FS, 5000.0, True), "k_lpdc_sp"),
    (R.cw_spec(FS, 700.0, 300.0, gain=2.0), "k_scan_sp<trs=5>"),
]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("spec,kernel", DEMODS, ids=["fm", "fm_translate", "pm", "ssb", "am_sqrt", "am_abs", "cw"])
def test_demodulators(gpu_lib, oracle, spec, kernel, path):
    """The demodulators at their usual designs, truth on the reference's own f32 front-end
    value (iir_ref fronts: the scan is measured, not atan2_approx). scan_path 0:
    FmQuadratureDemod, with and without with_translate, k_scan_sp<LP4, Fm, Id, 3>;
    PmQuadratureDemod k_scan_sp<LP4, Pm, Id, 3>; SsbProductDemod k_lpdc_sp<Pre::Ssb>;
    AmEnvelopeDemod PowerSqrt k_lpdc_sp<Pre::AmSqrt>, AbsApprox k_lpdc_sp<Pre::AmAbs>;
    CwEnvelopeDemod with set_gain(2) k_scan_sp<ONEPOLE, Cw, Gain, 5> (a^1024 < 1e-10 <
    a^512 at 300 Hz). scan_path 1: the three-kernel scan <LP4, Fm | Pm, Id>, <LPDC, Ssb |
    AmAbs, Id>, <ONEPOLE, Cw, Gain>, and for PowerSqrt <LP4, AmSqrt, Sqrt> then <DC, Real,
    Id>. PowerSqrt's inputs carry an offset that keeps the LP4 output above 1."""
    if path:
        expect = ["three", "three"] if spec.kind == "am_sqrt" else ["three"]
    else:
        expect = [kernel]
    check_stream(gpu_lib, oracle, spec, path, expect=expect)


@pytest.mark.parametrize("path", [0, 1])
def test_am_power_sqrt_outside_the_warm_up(gpu_lib, oracle, path):
    """AmEnvelopeDemod PowerSqrt with a bandwidth whose LP4 does not forget within the
    warm-up (||A_lp^256|| = 2e-10): the two-scan form, k_scan_sp<LP4, AmSqrt, Sqrt, 4> then
    k_lpdc_sp<Pre::Real> (scan_path 0), the three-kernel scans <LP4, AmSqrt, Sqrt> and <DC,
    Real, Id> (1)."""
    bw = float(np.float32(warm_cutoff(oracle, "outside") / 0.9 * 0.999))
    spec = R.am_spec(FS, bw, False)
    assert not R.lpdc_single_pass(spec.coef(oracle))
    check_stream(gpu_lib, oracle, spec, path,
                 expect=["three", "three"] if path else ["k_scan_sp<trs=4>", "k_lpdc_sp dc <Pre::Real>"])


# =========================================================================== SsbPhasingMod ==
@pytest.mark.parametrize("passes", [0, 3])
@pytest.mark.parametrize("side", ["usual", "inside", "outside"])
def test_ssb_phasing_mod(gpu_lib, oracle, side, passes):
    """SsbPhasingMod, rho on the real and the imaginary part against two f64 LP4 cascades
    with the oracle's oscillators. mod_passes 0 with ||A_lp^256|| < 1e-10 (2800 Hz, and the
    bandwidth bisected to 0.5e-10): k_ssb_mod_sp (4096-sample chunks after a 256-sample
    warm-up); at 2e-10, or mod_passes 3: k_ssb_mod_front, the three-kernel scan <LP4, Real,
    Id> on two channels, k_ssb_mod_back."""
    bw = 2800.0 if side == "usual" else float(np.float32(warm_cutoff(oracle, side) / 0.9 * (1.001 if side == "inside" else 0.999)))
    if_hz, rf_hz, usb = 1500.0, 9000.0, side != "outside"

    def mk():
        M = gpu_lib.SsbPhasingMod(FS, bw, if_hz, rf_hz, usb)
        return M.configure_option("mod_passes", passes) if passes else M

    c5 = np.asarray(mk().taps()[:5], np.float32)
    assert np.array_equal(c5, oracle.lp_cascade_coeffs(FS, R.audio_lp_fc(bw)))
    assert R.lpdc_single_pass(c5) == (side != "outside")
    kernel = "k_ssb_mod_sp" if passes == 0 and side != "outside" else "three"
    n, edges, lens, splits = geometry([kernel])
    for k, cls in enumerate(R.CLASSES):
        a = R.input_class(cls, n, 6000 + k, edges)
        truth, b = R.ssb_mod_truth_bound(oracle, a, c5, FS, if_hz, rf_hz, usb)
        ref = oracle.ssb_mod(a, FS, bw, if_hz, rf_hz, usb)
        rho_o = max(R.rho(ref.real, truth.real, b), R.rho(ref.imag, truth.imag, b))
        worst = (0.0, 0, "")
        for s in [[m] for m in lens] + splits:
            m = sum(s)
            got = run_calls(mk(), a[:m], s)
            assert np.all(np.isfinite(got.view(np.float32))), (cls, s)
            for part, t in ((got.real, truth[:m].real), (got.imag, truth[:m].imag)):
                r, i = R.rho(part, t, b[:m])
                worst = max(worst, (r, i, f"calls {s}"))
        print(f"[parity] SsbPhasingMod {side} bw={bw:.6g} mod_passes {passes} {kernel} {cls}: rho gpu {worst[0]:.3g} at "
              f"{worst[1]} ({worst[2]}) / oracle {rho_o[0]:.3g} at {rho_o[1]} = {worst[0] / rho_o[0]:.2f}")
        assert worst[0] <= MARGIN * rho_o[0], (side, passes, cls, worst, rho_o)
        nz = np.nonzero(a)[0]
        if len(nz) and nz[0] > 0:
            assert not np.any(mk().process(a).view(np.float32)[:2 * nz[0]])


# ======================================================================== exact assertions ==
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


ZERO_PRESERVING = [R.lp_cascade_spec(FS, 4500.0), R.biquad_spec(R.resonator(0.9999, 1234.0, FS), "resonator r=0.9999"),
                   R.biquad_spec(R.resonator(0.99, 1234.0, FS), "resonator r=0.99"), R.dc_spec(FS, 2.0), R.dc_spec(FS, 10e3),
                   R.lpdc_spec(FS, 2520.0, 2.0, None), R.lpdc_spec(FS, 2520.0, 2.0, "abs"), R.ssb_spec(FS, 1500.0, 2800.0),
                   R.am_spec(FS, 5000.0, True), R.am_spec(FS, 5000.0, False), R.cw_spec(FS, 700.0, 300.0, gain=2.0)]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("spec", ZERO_PRESERVING, ids=repr)
def test_leading_zeros_are_exact(gpu_lib, oracle, spec, path):
    """Outputs before the first non-zero input sample are exactly zero, for every block with
    a linear or zero-preserving front end (real input, SSB, AM: sqrt(0) = 0, CW, the DC
    blocker), with the first sample one past a chunk edge, mid-chunk and in a second call:
    a zero-state aggregate, warm-up or look-back that leaks anything shows here. Kernels as
    in the tests above (k_scan_sp, k_lpdc_sp per front end and DC-only; the three-kernel
    scan on scan_path 1)."""
    n = 3 * K_SP_CH + 5
    for first in (K_SP_CH + 1, K_SP_CH + K_SP_CH - K_SP_WARM + 77, 2 * K_SP_CH):
        x = R.input_class("dense", n, first, (), complex_=spec.complex_in)
        x[first:] += np.float32(spec.offset)  # PowerSqrt: a positive LP4 output after the zeros
        x[:first] = 0
        got = run_calls(make(gpu_lib, spec, path), x, [n])
        assert not np.any(got[:first]), f"{spec} path {path}: non-zero at {np.nonzero(got[:first])[0][:4]} before {first}"
        assert np.any(got[first:first + 4])
        got = run_calls(make(gpu_lib, spec, path), x, [K_SP_CH - 3, n - K_SP_CH + 3])
        assert not np.any(got[:first]), f"{spec} path {path} two calls: non-zero before {first}"


@pytest.mark.parametrize("path", [0, 1])
def test_integer_dc_blocker_r0(gpu_lib, oracle, path):
    """DcBlocker with r = 0 (cut >= fs / 2 pi) on integer samples in [-2^20, 2^20]: got ==
    x[n] - x[n-1] bit for bit (every difference is an integer below 2^22), in one call at
    every DC-only chunk-edge length and streamed. k_lpdc_sp<Pre::Real>, whose look-back
    must not divide by r (scan_path 0); the three-kernel scan <DC, Real, Id> (1)."""
    n = 3 * K_SP_CH + 5
    x = np.random.default_rng(20).integers(-2 ** 20, 2 ** 20 + 1, n).astype(np.float32)
    want = (x - np.concatenate([[np.float32(0)], x[:-1]])).astype(np.float32)
    mk = lambda: make(gpu_lib, R.dc_spec(FS, 10e3), path)  # noqa: E731
    assert float(mk().taps()[0]) == 0.0
    for m in (1, 2, K_SCAN_CH, K_SCAN_CH + 1, K_SP_CH - 1, K_SP_CH, K_SP_CH + 1, 2 * K_SP_CH + 1, n):
        got = run_calls(mk(), x[:m], [m])
        assert same_bits(got, want[:m]), f"n={m}: first difference at {np.nonzero(got != want[:m])[0][:4]}"
    for lens in ([1, 7, K_SP_CH, 1, K_SP_CH + 1], [K_SP_CH], [K_SP_CH + 1], [3001] * 8):
        lens = lens + [n - sum(lens)]
        got = run_calls(mk(), x, lens)
        assert same_bits(got, want), f"calls {lens}: first difference at {np.nonzero(got != want)[0][:4]}"


BITS = [R.lp_cascade_spec(FS, 4500.0), R.biquad_spec(R.resonator(0.9999, 1234.0, FS), "resonator r=0.9999"),
        R.fm_spec(FS, 2500.0, 5000.0, translate=3000.0), R.cw_spec(FS, 700.0, 300.0, gain=2.0), R.dc_spec(FS, 2.0),
        R.lpdc_spec(FS, 2520.0, 2.0, None), R.ssb_spec(FS, 1500.0, 2800.0)]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("spec", BITS, ids=repr)
def test_reset_and_run_to_run_bits(gpu_lib, oracle, spec, path):
    """A handle after reset() equals a fresh handle, and two runs of the same calls on fresh
    handles equal each other, bit for bit, where the combination order is fixed: the
    three-kernel scan (scan_path 1, every block) and k_scan_sp (LpCascade, FM with
    with_translate, CW; the r = 0.9999 resonator takes the three-kernel scan on both paths).
    k_lpdc_sp (DcBlocker, LpDcCascade, SsbProductDemod on scan_path 0) is NOT asserted
    bit-reproducible: its DC look-back closes at whichever predecessor has published an
    inclusive prefix, so the order in which the f64 entering state is summed depends on
    timing. Its repeated and reset runs are held to the rho bound instead."""
    n = 3 * K_SP_CH + 5
    lens = [K_SP_CH + 1, 7, n - K_SP_CH - 8]
    x = R.spec_input(spec, "dense", n, 77, ())
    y = R.spec_input(spec, "dense", 5000, 78, ())
    blk = make(gpu_lib, spec, path)
    kernels = reach(spec, coef_of(spec, blk), path)
    first = run_calls(blk, x, lens)
    run_calls(blk, y, [len(y)])
    blk.reset()
    again = run_calls(blk, x, lens)
    fresh = run_calls(make(gpu_lib, spec, path), x, lens)
    if not any(k.startswith("k_lpdc_sp") for k in kernels):
        assert same_bits(first, fresh), f"{spec} {kernels}: two fresh runs differ at {np.nonzero(first != fresh)[0][:4]}"
        assert same_bits(again, fresh), f"{spec} {kernels}: after reset differs at {np.nonzero(again != fresh)[0][:4]}"
    else:
        truth, b = R.truth_bound(spec.front(oracle, x), **chain_of(spec, blk, oracle))
        rho_o = R.rho(spec.ref(oracle, x), truth, b)[0]
        for name, got in (("first", first), ("after reset", again), ("fresh", fresh)):
            r, i = R.rho(got, truth, b)
            print(f"[parity] {spec} path {path} {kernels} {name}: rho gpu {r:.3g} at {i} / oracle {rho_o:.3g}")
            assert r <= MARGIN * rho_o, (spec, name, r, i, rho_o)


@pytest.mark.parametrize("path", [0, 1])
def test_ssb_batched_rows(gpu_lib, oracle, path):
    """SsbProductDemod(channels = 5): row c against the single-channel block on that row.
    scan_path 1, the three-kernel scan <LPDC, Ssb, Id> with one k_scan_carry workgroup per
    channel (blockIdx.y in agg / apply): the same arithmetic in the same order, bit for bit.
    scan_path 0, k_lpdc_sp<Pre::Ssb> with chunks * channels workgroups: the same instance,
    but the look-back is timing dependent (test_reset_and_run_to_run_bits), so each row
    is held to the rho bound against its own truth."""
    nch, n = 5, 2 * K_SP_CH + K_SP_CH - K_SP_WARM + 9
    spec1, specn = R.ssb_spec(FS, 1500.0, 2800.0), R.ssb_spec(FS, 1500.0, 2800.0, channels=nch)
    x = np.stack([R.input_class(("dense", "burst", "impulse", "step", "burst_silence")[c], n, 90 + c,
                                (K_SP_CH, K_SP_CH - K_SP_WARM), complex_=True) for c in range(nch)])
    blk = make(gpu_lib, specn, path)
    got = blk.process(np.ascontiguousarray(x))
    blk.status()
    assert got.shape == (nch, n) and np.all(np.isfinite(got))
    ch = chain_of(spec1, make(gpu_lib, spec1, path), oracle)
    for c in range(nch):
        one = run_calls(make(gpu_lib, spec1, path), x[c], [n])
        if path == 1:
            assert same_bits(got[c], one), f"row {c} differs from the single-channel call at {np.nonzero(got[c] != one)[0][:4]}"
        truth, b = R.truth_bound(spec1.front(oracle, x[c]), **ch)
        rho_o = R.rho(spec1.ref(oracle, x[c]), truth, b)[0]
        r, i = R.rho(got[c], truth, b)
        print(f"[parity] SsbProductDemod 5 channels path {path} row {c}: rho gpu {r:.3g} at {i} / oracle {rho_o:.3g}")
        assert r <= MARGIN * rho_o, (c, r, i, rho_o)


# ======================================================================= one long DC case ==
@pytest.mark.parametrize("cut", [0.1, 2.0], ids=["clamp_0.9999", "2Hz"])
@pytest.mark.parametrize("block", ["DcBlocker", "LpDcCascade"])
def test_dc_look_back_past_its_horizon(gpu_lib, oracle, block, cut):
    """70 chunks (573,440 samples, the largest input of this file) of standard-normal noise
    on a 0.25 offset through the DC look-back of k_lpdc_sp (<Pre::Real> DC-only with
    8192-sample chunks, <Pre::RealLp> with 7936-sample strides): more predecessors than
    the 64 a wave walks at a time, and more than the K after which r^(K len) < 1e-20 lets
    the walk end (57 and 59 chunks at the 0.9999 clamp, 22 and 23 at 2 Hz). rho as everywhere,
    and again over the last 10 chunks alone, where every walk has ended at its horizon."""
    n = 70 * K_SP_CH
    spec = R.dc_spec(FS, cut) if block == "DcBlocker" else R.lpdc_spec(FS, 2520.0, cut, None)
    blk = make(gpu_lib, spec, 0)
    assert reach(spec, coef_of(spec, blk), 0)[0].startswith("k_lpdc_sp")
    ch = chain_of(spec, blk, oracle)
    stride = K_SP_CH if block == "DcBlocker" else K_SP_CH - K_SP_WARM
    K = R.dc_lookback_chunks(ch["r"], stride)
    assert n // stride > 65 and K <= n // stride - 10, (K, n // stride)
    x = (np.random.default_rng(70).standard_normal(n) + 0.25).astype(np.float32)
    truth, b = R.truth_bound(x, **ch)
    ref = spec.ref(oracle, x)
    got = run_calls(blk, x, [n])
    assert np.all(np.isfinite(got))
    tail = n - 10 * K_SP_CH
    for name, sl in (("whole", slice(0, n)), ("last 10 chunks", slice(tail, n))):
        rho_o, i_o = R.rho(ref[sl], truth[sl], b[sl])
        r, i = R.rho(got[sl], truth[sl], b[sl])
        print(f"[parity] {spec} 70 chunks K={K} {name}: rho gpu {r:.3g} at {i + sl.start} / oracle {rho_o:.3g} at "
              f"{i_o + sl.start} = {r / rho_o:.2f}")
        assert r <= MARGIN * rho_o, (spec, name, r, i, rho_o)
