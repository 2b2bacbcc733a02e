"""TEST INFRASTRUCTURE: a plain float64 reference for the IIR scan kernels
(csrc/k_scan.hip), numpy / scipy only, validated against the C oracle in
tests/test_iir_ref.py and used per sample by tests/test_gpu_scan_exact.py.

* truth     the reference's recurrence in float64 with the f32 coefficients the
            library reports, applied to the f32 recurrence input d[n] (the sample
            itself, or a demodulator's f32 front-end value: fronts below);
* bound     B[n] = u (henv * |d|)[n] + 1e-10 sum(henv) max_{m<=n} |d[m]|, u = 2^-24,
            henv[k] = max_{j>=k} |h[j]| the monotone envelope of the f64 impulse
            response (cut where |h| < 1e-30). The second term is the truncation the
            single-pass kernels allow themselves (scan_blocks.cpp: 1e-10);
* rho       max_n |y[n] - truth[n]| / B[n] and where it occurs. B has the right
            shape, not the right constant: tests compare rho(gpu) with rho(oracle);
* criteria  scan_blocks.cpp's kernel choice restated (TDF-II state space as iir.hpp,
            mat_pow, the Frobenius tests), and bisection for designs that sit at a
            chosen norm at a chosen horizon.
"""
import functools

import numpy as np
import scipy.signal as sg

import np_ref as NR

f32 = np.float32
U = 2.0 ** -24
TRUNC = 1e-10        # scan_blocks.cpp:35, 41, 58, 403: ||A^k||_F < 1e-10
H_CUT = 1e-30        # the impulse response is cut where |h| falls below this
H_MAX = 1 << 20      # impulse-response samples computed (0.9999^k < 1e-30 at k = 690,742)

# scan.hpp:25-27, 88, 93-95
K_SCAN_C = 16
K_SCAN_NT = 256
K_SCAN_CH = K_SCAN_C * K_SCAN_NT
K_SP_WARM = 256
K_SP_C = 2 * K_SCAN_C
K_SP_CH = K_SP_C * K_SCAN_NT
K_LPDC_SC = 32
DC_HORIZON = 1e-20   # k_scan.hip:757-762, 795: the DC look-back ends once r^(K len) < 1e-20


# ------------------------------------------------------------------ recurrences (f64) ==
def _c64(c):
    return tuple(float(f32(v)) for v in c)


def biquad64(d, c):
    """iir.rs:34-40 in f64 with the f32 coefficients c = (b0, b1, b2, a1, a2)."""
    b0, b1, b2, a1, a2 = _c64(c)
    return sg.lfilter([b0, b1, b2], [1.0, a1, a2], np.asarray(d, np.float64))


def lp4_64(d, c):
    """iir.rs:79-83 LpCascade: the biquad twice."""
    return biquad64(biquad64(d, c), c)


def dc64(v, r):
    """dc.rs:47-51 / iir.rs:160-163: y = v - v1 + r y1."""
    return sg.lfilter([1.0, -1.0], [1.0, -float(f32(r))], np.asarray(v, np.float64))


def onepole64(d, a):
    """cw.rs:40: y = a y + (1 - a) d, (1 - a) rounded to f32 as the reference has it."""
    a = f32(a)
    return sg.lfilter([float(f32(f32(1.0) - a))], [1.0, -float(a)], np.asarray(d, np.float64))


_REC = {"bq": biquad64, "lp4": lp4_64, "onepole": onepole64}


def _rec(rec, coef, d):
    return _REC[rec](d, coef)


@functools.lru_cache(maxsize=None)
def _henv_cached(rec, coef):
    imp = np.zeros(H_MAX)
    imp[0] = 1.0
    h = np.abs(dc64(imp, coef) if rec == "dc" else _rec(rec, coef, imp))
    keep = np.nonzero(h >= H_CUT)[0]
    h = h[:keep[-1] + 1] if len(keep) else h[:1]
    return np.maximum.accumulate(h[::-1])[::-1].copy()


def henv(rec, coef):
    """The monotone envelope of stage rec's f64 impulse response ('dc': coef = r, 'onepole': a)."""
    scalar = rec in ("dc", "onepole")
    return _henv_cached(rec, float(f32(coef)) if scalar else tuple(float(f32(v)) for v in coef))


def _runmax(a):
    return np.maximum.accumulate(a) if len(a) else a


def stage_bound(he, a, e=None):
    """One stage's bound: input magnitude a[n], input error e[n] (None: exact):
    henv * (u a + e) + 1e-10 sum(henv) max_{m<=n} a[m]; exactly zero until a or e is not."""
    a = np.abs(np.asarray(a, np.float64))
    src = U * a if e is None else U * a + e
    n = len(a)
    k = he[:n]
    b = np.maximum(sg.fftconvolve(k, src)[:n] if n * len(k) > 1 << 16 else np.convolve(k, src)[:n], 0.0)
    b = b + TRUNC * he.sum() * _runmax(a)
    b[_runmax(src) == 0.0] = 0.0
    return b


def truth_bound(d, rec=None, coef=None, map=None, r=None, gain=1.0):
    """Truth and bound of [rec stage] -> [map] -> [DC blocker with pole r] -> [gain] on the
    f32 recurrence input d. rec: None, 'bq', 'lp4' or 'onepole'; map: None, 'identity',
    'sqrt' or 'abs' (applied in f64; the sqrt also rounds, u |v|, and passes the LP4's bound
    through its slope 1 / (2 sqrt v), as e / max(sqrt v, sqrt e) so that it stays finite
    while the LP4 output rises from zero); r: None for no DC stage."""
    d = np.asarray(d, f32).astype(np.float64)
    v, b = d, None
    if rec is not None:
        v = _rec(rec, coef, d)
        b = stage_bound(henv(rec, coef), d)
    if map == "sqrt":
        assert rec is not None
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.sqrt(v)
            den = np.maximum(s, np.sqrt(b))
            b = np.where(den > 0, b / np.where(den > 0, den, 1.0), 0.0) + U * np.abs(s)
        v = s
    elif map == "abs":
        v = np.abs(v)
    if r is not None:
        b = stage_bound(henv("dc", r), v, b)
        v = dc64(v, r)
    if gain != 1.0:
        g = float(f32(gain))
        v = v * g
        b = b * abs(g) + U * np.abs(v)
    return v, b


def rho(y, truth, b):
    """(max_n |y - truth| / B, its index). Where B is exactly zero the output must be too."""
    y = np.asarray(y, np.float64)
    assert y.shape == truth.shape == b.shape, (y.shape, truth.shape, b.shape)
    if y.size == 0:
        return 0.0, 0
    err = np.abs(y - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    q = np.where(np.isfinite(y), q, np.inf)
    i = int(np.argmax(q))
    return float(q[i]), i


def nrmse(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    den = np.sqrt(np.mean(ref ** 2))
    return float(np.sqrt(np.mean((got - ref) ** 2)) / (den if den > 0 else 1.0))


# --------------------------------------------------- f32 front ends (recurrence inputs) ==
def _ri(x):
    x = np.asarray(x, np.complex64)
    return x.real.astype(f32), x.imag.astype(f32)


def phasors(oracle, n, freq_hz, fs):
    """The reference's own oscillator outputs (its f32 recurrence, from the oracle)."""
    return oracle.rotator(np.ones(n, np.complex64), freq_hz, fs)


def front_fm(oracle, x, fs, dev_hz, translate_hz=None):
    """fm.rs:48-68: [z conj(p)], z conj(prev) (prev = 1 at first), atan2_approx, k = 1 / max(dev, 1)."""
    a, b = _ri(x)
    if translate_hz is not None:
        c, dd = _ri(phasors(oracle, len(a), translate_hz, fs))
        dd = -dd
        a, b = ((a * c).astype(f32) - (b * dd).astype(f32)).astype(f32), ((a * dd).astype(f32) + (b * c).astype(f32)).astype(f32)
    pr_, pi_ = np.concatenate([[f32(1)], a[:-1]]).astype(f32), np.concatenate([[f32(0)], b[:-1]]).astype(f32)
    qr = ((a * pr_).astype(f32) + (b * pi_).astype(f32)).astype(f32)
    qi = ((b * pr_).astype(f32) - (a * pi_).astype(f32)).astype(f32)
    k = f32(f32(1.0) / max(f32(dev_hz), f32(1.0)))
    return (NR.atan2_approx(qi, qr) * k).astype(f32)


def front_pm(x, k):
    """pm.rs:54-58: w = z conj(prev) in num-complex's order, k atan2_approx(w.im, w.re)."""
    a, b = _ri(x)
    c = np.concatenate([[f32(1)], a[:-1]]).astype(f32)
    nd = (-np.concatenate([[f32(0)], b[:-1]])).astype(f32)
    wr = ((a * c).astype(f32) - (b * nd).astype(f32)).astype(f32)
    wi = ((a * nd).astype(f32) + (b * c).astype(f32)).astype(f32)
    return (f32(k) * NR.atan2_approx(wi, wr)).astype(f32)


def front_ssb(oracle, x, fs, bfo_hz):
    """ssb.rs:33-38 / rotator.rs:88-94: fma(I, p.re, Q p.im) with the BFO's phasors."""
    a, b = _ri(x)
    pr_, pi_ = _ri(phasors(oracle, len(a), bfo_hz, fs))
    return NR._fma(a, pr_, (b * pi_).astype(f32)) if len(a) else a


def front_am_power(x):
    """am.rs:201-205: fma(I, I, Q Q)."""
    a, b = _ri(x)
    return NR._fma(a, a, (b * b).astype(f32)) if len(a) else a


def front_am_abs(x, k1=0.9482, k2=0.3920):
    """am.rs:232-239: fma(k1, |I|, k2 |Q|)."""
    a, b = _ri(x)
    return NR._fma(np.full(len(a), f32(k1), f32), np.abs(a), (f32(k2) * np.abs(b)).astype(f32)) if len(a) else a


def front_cw(x):
    """cw.rs:38-39: sqrtf(I I + Q Q), no FMA."""
    a, b = _ri(x)
    return np.sqrt(((a * a).astype(f32) + (b * b).astype(f32)).astype(f32)).astype(f32)


def audio_lp_fc(bw):
    """The demodulators' LP cutoff: bw * 0.9 in f32 (fm.rs:24, pm.rs:27, ssb.rs:17, am.rs:27)."""
    return f32(f32(bw) * f32(0.9))


def ssb_truth(oracle, x, fs=48e3, bfo=1500.0, bw=2800.0, f32_front=False):
    """SsbProductDemod (ssb.rs:28-71) in f64: the reference's own BFO phasors, the product
    I p.re + Q p.im (in f64, or the reference's f32 fma with f32_front), then the
    LpDcCascade (iir.rs:151-165) with the reference's f32 coefficients, all in f64."""
    x = np.asarray(x, np.complex64)
    if f32_front:
        d = front_ssb(oracle, x, fs, bfo).astype(np.float64)
    else:
        p = phasors(oracle, len(x), bfo, fs).astype(np.complex128)
        d = x.real.astype(np.float64) * p.real + x.imag.astype(np.float64) * p.imag
    c = oracle.lpdc_coeffs(fs, audio_lp_fc(bw), 2.0)
    return lpdc64(d, c)


def lpdc64(d, c6, map=None):
    """iir.rs:151-186 LpDcCascade in f64 with c6 = (b0, b1, b2, a1, a2, r) on an f64 input."""
    y = np.asarray(d, np.float64)
    for _ in range(2):
        y = biquad64(y, c6[:5])
    if map == "sqrt":
        y = np.sqrt(y)
    elif map == "abs":
        y = np.abs(y)
    return dc64(y, c6[5])


def ssb_mod_truth_bound(oracle, a, c5, fs, if_hz, rf_hz, usb):
    """SsbPhasingMod (modulate/ssb.rs:43-114): the f32 products a p.re, a p.im with the
    audio oscillator, one f64 LP4 each, z = (I, side Q) times the RF oscillator in f64.
    Returns (truth complex128, B) with B = B_I + B_Q + u (|I| + |Q|) for both parts
    (|r| <= 1 up to the oscillator's own rounding)."""
    a = np.asarray(a, f32)
    p = phasors(oracle, len(a), if_hz, fs)
    r = phasors(oracle, len(a), rf_hz, fs).astype(np.complex128)
    di, dq = (a * p.real.astype(f32)).astype(f32), (a * p.imag.astype(f32)).astype(f32)
    ti, bi = truth_bound(di, "lp4", c5)
    tq, bq = truth_bound(dq, "lp4", c5)
    tq = tq * (1.0 if usb else -1.0)
    t = (ti * r.real - tq * r.imag) + 1j * (tq * r.real + ti * r.imag)
    return t, bi + bq + U * (np.abs(ti) + np.abs(tq))


# ------------------------------------------------------------ scan_blocks.cpp's criteria ==
def resonator(r, f0, fs):
    """A two-pole resonator (poles r e^{+-j w0}) with zeros at +-1: b = (1 - r)(1, 0, -1)."""
    w = 2 * np.pi * f0 / fs
    g = 1.0 - r
    return (f32(g), f32(0.0), f32(-g), f32(-2 * r * np.cos(w)), f32(r * r))


def biquad_ss(c):
    """design.cpp biquad_ss (iir.hpp BiquadK, state (z1, z2)): y = b0 x + z1,
    z1' = b1 x + z2 - a1 y, z2' = b2 x - a2 y, with the f32 coefficients in f64."""
    b0, b1, b2, a1, a2 = _c64(c)
    return np.array([[-a1, 1.0], [-a2, 0.0]]), np.array([b1 - a1 * b0, b2 - a2 * b0])


def lp4_ss(c):
    """design.cpp lp_cascade_ss: state (z0_1, z0_2, z1_1, z1_2); the second biquad's input
    is the first one's output y0 = b0 x + z0_1."""
    A1, B1 = biquad_ss(c)
    A = np.zeros((4, 4))
    A[:2, :2] = A1
    A[2:, 2:] = A1
    A[2:, 0] = B1
    return A, np.concatenate([B1, B1 * float(f32(c[0]))])


def onepole_ss(a):
    return np.array([[float(f32(a))]]), np.array([float(f32(f32(1.0) - f32(a)))])


def mat_pow(A, k):
    """design.cpp mat_pow: binary powering in f64."""
    R = np.eye(len(A))
    P = np.array(A, np.float64)
    k = int(k)
    while k:
        if k & 1:
            R = R @ P
        P = P @ P
        k >>= 1
    return R


def fro(A, k):
    """||A^k||_F."""
    return float(np.sqrt(np.sum(mat_pow(A, k) ** 2)))


def scan_sp_choice(A):
    """ScanStage's constructor (scan_blocks.cpp:31-46) for a scan_sp_supported stage:
    ('k_scan_sp', trs) when ||A^kSpCH|| < 1e-10, trs the first of 3, 4, 5 with
    ||A^(kSpC 2^trs)|| < 1e-10, else 0 (the full lane scan); ('three', None) otherwise."""
    if not fro(A, K_SP_CH) < TRUNC:
        return "three", None
    for trs in (3, 4, 5):
        if fro(A, K_SP_C << trs) < TRUNC:
            return "k_scan_sp", trs
    return "k_scan_sp", 0


def lpdc_single_pass(c5):
    """scan_blocks.cpp:52-58, 400-403: k_lpdc_sp / k_ssb_mod_sp when ||A_lp^kSpWarm|| < 1e-10."""
    return fro(lp4_ss(c5)[0], K_SP_WARM) < TRUNC


def dc_lookback_chunks(r, length):
    """k_scan.hip:757-762: the K with r^(K length) < 1e-20 (None for r = 0: one chunk)."""
    r = float(f32(r))
    if r <= 0.0:
        return 1
    return int(np.floor(np.log(DC_HORIZON) / (length * np.log(r)))) + 1


def bisect_design(coefs_of, ss_of, horizon, target, lo, hi):
    """The parameter p in [lo, hi] at which ||A(coefs_of(p))^horizon||_F = target, by
    bisection on log ||.|| (monotone in a pole radius or a cutoff over these ranges)."""
    f = lambda p: np.log(max(fro(ss_of(coefs_of(p))[0], horizon), 1e-300)) - np.log(target)  # noqa: E731
    flo, fhi = f(lo), f(hi)
    assert flo * fhi < 0, f"no sign change over [{lo}, {hi}]: {flo:.3g}, {fhi:.3g}"
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        fm = f(mid)
        if fm * flo > 0:
            lo, flo = mid, fm
        else:
            hi = mid
    return 0.5 * (lo + hi)


def resonator_at(horizon, target, f0=1234.0, fs=48e3):
    """The resonator pole radius with ||A^horizon||_F = target."""
    return bisect_design(lambda r: resonator(r, f0, fs), biquad_ss, horizon, target, 0.5, 0.999999)


def lp_cutoff_at(horizon, target, fs=48e3, coeffs=NR.lp_cascade_coeffs):
    """The LpCascade cutoff (Hz) whose LP4 has ||A^horizon||_F = target."""
    return bisect_design(lambda fc: coeffs(fs, f32(fc)), lp4_ss, horizon, target, fs * 2e-5, fs * 0.2)


# --------------------------------------------------------------------- input classes ==
def split_calls(x, lens):
    out, i = [], 0
    for n in lens:
        out.append(x[..., i:i + n])
        i += n
    assert i == x.shape[-1], (i, x.shape)
    return out


def impulse_positions(n, chunk_edges):
    """Where the scans' geometry changes: 0, 1, lane-run edges (kScanC, kSpC), wave edges
    (64 lanes of kScanC / kSpC samples), and every chunk edge -1, +0, +1."""
    pos = {0, 1, K_SCAN_C - 1, K_SCAN_C, K_SP_C - 1, K_SP_C, 64 * K_SCAN_C - 1, 64 * K_SCAN_C,
           64 * K_SP_C - 1, 64 * K_SP_C}
    for e in chunk_edges:
        pos |= {e - 1, e, e + 1}
    return np.array(sorted(p for p in pos if 0 <= p < n), np.int64)


def input_class(kind, n, seed, edges, complex_=False, offset=0.0, burst=1e3):
    """The seeded input classes. edges: chunk boundaries of the kernel under test (the
    burst ends at each, impulses sit at each -1, +0, +1). offset: added to every sample
    (the sqrt maps need a positive LP4 output); burst: the burst amplitude."""
    rng = np.random.default_rng(seed)

    def noise(m):
        return rng.standard_normal(m) + 1j * rng.standard_normal(m) if complex_ else rng.standard_normal(m)

    if kind == "dense":
        x = noise(n)
    elif kind in ("burst", "burst_silence"):
        env = np.full(n, 0.0 if kind == "burst_silence" else 1e-3)
        for e in edges:
            env[max(0, e - 192):e] = burst
        x = noise(n) * env
    elif kind == "step":
        x = np.zeros(n, np.complex128 if complex_ else np.float64)
        x[100:] = 3.0
    elif kind == "impulse":
        x = np.zeros(n, np.complex128 if complex_ else np.float64)
        pos = impulse_positions(n, edges)
        amp = np.ldexp(rng.choice([-1.0, 1.0], len(pos)), rng.integers(-3, 4, len(pos)))
        x[pos] = amp * (1 + 0.5j) if complex_ else amp
    else:
        raise ValueError(kind)
    if offset:
        x = x + offset
    return x.astype(np.complex64 if complex_ else f32)


CLASSES = ("dense", "burst", "burst_silence", "step", "impulse")


# ------------------------------------------------------------------------ the blocks ==
class Spec:
    """One block under test: how to build it (mk(lib)), the oracle's output (ref(oracle,
    x)), the f32 recurrence input (front(oracle, x)), the f64 chain after it (chain(oracle)
    -> truth_bound's keywords), the LP stage's coefficients (coef(oracle): what the
    criteria are evaluated on), and what the inputs must look like."""

    def __init__(self, name, mk, ref, front, chain, kind, coef=None, complex_in=False, offset=0.0, burst=1e3,
                 zero_preserving=True, tol=1e-6):
        self.name, self.mk, self.ref, self.front, self.chain = name, mk, ref, front, chain
        self.kind, self.coef, self.complex_in, self.offset, self.burst = kind, coef, complex_in, offset, burst
        self.zero_preserving, self.tol = zero_preserving, tol

    def truth_bound(self, oracle, x):
        return truth_bound(self.front(oracle, x), **self.chain(oracle))

    def __repr__(self):
        return self.name


def _real(oracle, x):
    return np.asarray(x, f32)


def lp_cascade_spec(fs, fc):
    return Spec(f"LpCascade {fs:g}/{fc:.6g}", lambda lib: lib.LpCascade(fs, fc), lambda o, x: o.lp_cascade(x, fs, fc),
                _real, lambda o: dict(rec="lp4", coef=o.lp_cascade_coeffs(fs, fc)), "lp4",
                coef=lambda o: o.lp_cascade_coeffs(fs, fc))


def biquad_spec(c, name):
    c = tuple(f32(v) for v in c)
    return Spec(f"Biquad {name}", lambda lib: lib.Biquad(*c), lambda o, x: o.biquad(x, *c), _real,
                lambda o: dict(rec="bq", coef=c), "bq", coef=lambda o: c)


def dc_spec(fs, cut):
    return Spec(f"DcBlocker {fs:g}/{cut:g}", lambda lib: lib.DcBlocker(fs, cut), lambda o, x: o.dc_blocker(x, fs, cut),
                _real, lambda o: dict(r=o.lpdc_coeffs(fs, 1000.0, cut)[5]), "dc")


def lpdc_spec(fs, lp, dc, map):
    sq = map == "sqrt"
    return Spec(f"LpDcCascade {fs:g}/{lp:.6g}/{dc:g} map={map}", lambda lib: lib.LpDcCascade(fs, lp, dc, map=map),
                lambda o, x: o.lp_dc_cascade(x, fs, lp, dc, map=map), _real,
                lambda o: dict(rec="lp4", coef=o.lpdc_coeffs(fs, lp, dc)[:5], map=map, r=o.lpdc_coeffs(fs, lp, dc)[5]),
                "lpdc", coef=lambda o: o.lpdc_coeffs(fs, lp, dc)[:5], offset=4.0 if sq else 0.0, burst=2.0 if sq else 1e3,
                zero_preserving=not sq, tol=1e-5)


def fm_spec(fs, dev, bw, translate=None):
    def mk(lib):
        D = lib.FmQuadratureDemod(fs, dev, bw)
        return D.with_translate(translate) if translate is not None else D
    return Spec(f"FmQuadratureDemod {fs:g}/{dev:g}/{bw:g} translate={translate}", mk,
                lambda o, x: o.fm_demod(x, fs, dev, bw, translate_hz=translate),
                lambda o, x: front_fm(o, x, fs, dev, translate),
                lambda o: dict(rec="lp4", coef=o.lp_cascade_coeffs(fs, audio_lp_fc(bw))), "lp4",
                coef=lambda o: o.lp_cascade_coeffs(fs, audio_lp_fc(bw)), complex_in=True, zero_preserving=False, tol=1e-5)


def pm_spec(fs, k, bw):
    return Spec(f"PmQuadratureDemod {fs:g}/{k:g}/{bw:g}", lambda lib: lib.PmQuadratureDemod(fs, k, bw),
                lambda o, x: o.pm_demod(x, fs, k, bw), lambda o, x: front_pm(x, k),
                lambda o: dict(rec="lp4", coef=o.lp_cascade_coeffs(fs, audio_lp_fc(bw))), "lp4",
                coef=lambda o: o.lp_cascade_coeffs(fs, audio_lp_fc(bw)), complex_in=True, zero_preserving=False, tol=1e-5)


def _demod_lpdc(o, fs, bw):
    return o.lpdc_coeffs(fs, audio_lp_fc(bw), 2.0)


def ssb_spec(fs, bfo, bw, channels=1):
    return Spec(f"SsbProductDemod {fs:g}/{bfo:g}/{bw:.6g}", lambda lib: lib.SsbProductDemod(fs, bfo, bw, channels=channels),
                lambda o, x: o.ssb_demod(x, fs, bfo, bw), lambda o, x: front_ssb(o, x, fs, bfo),
                lambda o: dict(rec="lp4", coef=_demod_lpdc(o, fs, bw)[:5], r=_demod_lpdc(o, fs, bw)[5]), "lpdc",
                coef=lambda o: _demod_lpdc(o, fs, bw)[:5], complex_in=True, tol=1e-5)


def am_spec(fs, bw, abs_approx):
    if abs_approx:
        return Spec(f"AmEnvelopeDemod AbsApprox {fs:g}/{bw:g}", lambda lib: lib.AmEnvelopeDemod(fs, bw, abs_approx=True),
                    lambda o, x: o.am_demod(x, fs, bw, abs_approx=(0.9482, 0.3920)), lambda o, x: front_am_abs(x),
                    lambda o: dict(rec="lp4", coef=_demod_lpdc(o, fs, bw)[:5], r=_demod_lpdc(o, fs, bw)[5]), "lpdc",
                    coef=lambda o: _demod_lpdc(o, fs, bw)[:5], complex_in=True, tol=1e-5)
    return Spec(f"AmEnvelopeDemod PowerSqrt {fs:g}/{bw:g}", lambda lib: lib.AmEnvelopeDemod(fs, bw),
                lambda o, x: o.am_demod(x, fs, bw), lambda o, x: front_am_power(x),
                lambda o: dict(rec="lp4", coef=_demod_lpdc(o, fs, bw)[:5], map="sqrt", r=_demod_lpdc(o, fs, bw)[5]),
                "am_sqrt", coef=lambda o: _demod_lpdc(o, fs, bw)[:5], complex_in=True, offset=2.0, burst=1.0, tol=1e-5)


def cw_alpha(fs, bw):
    """cw.rs:17-18: exp(-TAU max(bw, 1) / fs) in f32."""
    return NR.expf(f32(f32(-NR.TAU * max(f32(bw), f32(1.0))) / f32(fs)))


def cw_spec(fs, tone, bw, gain=1.0):
    def mk(lib):
        C = lib.CwEnvelopeDemod(fs, tone, bw)
        if gain != 1.0:
            C.set_gain(gain)
        return C
    return Spec(f"CwEnvelopeDemod {fs:g}/{bw:g} gain={gain:g}", mk, lambda o, x: o.cw_demod(x, fs, tone, bw, gain=gain),
                lambda o, x: front_cw(x), lambda o: dict(rec="onepole", coef=cw_alpha(fs, bw), gain=gain), "onepole",
                coef=lambda o: cw_alpha(fs, bw), complex_in=True, tol=1e-5)


def spec_input(spec, cls, n, seed, edges):
    return input_class(cls, n, seed, edges, complex_=spec.complex_in, offset=spec.offset, burst=spec.burst)
