"""TEST INFRASTRUCTURE: truths and yardsticks for the analog modulators (csrc/k_mod.hip)
and for every consumer of the oscillator (hip_common.hpp OscDev) across the end of its
table. Plain numpy, f64 / longdouble. Validated against the C oracle in
tests/test_mod_ref.py; used per sample by tests/test_gpu_mod_exact.py and
tests/test_gpu_osc_seam.py.

* E            osc_E(lib, f, fs, n, B): the host's definition of the engine's oscillator at
               table budget B (orion_osc_table_phasors: rec_table, then rec_state_after in
               long double). Inside the table it is the reference bit for bit; past it the
               device evaluates the same drift model in f32 (hip_common.hpp osc_model).
* OSC_TOL      the bound on |device - E| per component past the table.
* restatements the oracle's f32 op order with E as the phasors (rot_rotate, rot_mix_usb,
               nco_mix, am_restate, cw_restate): what a kernel must give bit for bit inside
               the table.
* truths       pm_truth, fm_truth (f64 / longdouble), with their criteria (check_*).
* models       fm_engine_model and seam_phasors restate, in numpy, HOW the kernels index
               (16-sample groups with Q0.64 phases; table / model runs per tile), each with
               switches for the indexing mistakes the GPU tests must catch. test_mod_ref.py
               runs every criterion on the faithful model (passes) and on each mistake
               (fails), so the GPU files are known to see them before they reach a GPU.
"""
import numpy as np

import np_ref as NR

f32 = np.float32
U = 2.0 ** -24
MARGIN = 5.0

# |device oscillator - E| per component past the table. The project's own bound for the
# osc_model code at nco_table = 0 (test_rotator, test_nco_block). Roundings of osc_model
# past a table (hip_common.hpp:153-155), each on a value of magnitude <= 1: phasor_at twice
# (S and mtab[off]: sincospif < 1 ulp on each component, the f32 turn count exact, the
# first-order correction 2 roundings: <= 3u each), cmul (a product and an fma per
# component: 2u), the magnitude (fma: u, on ~1) and its product (u): 3u + 3u + 2u + 2u =
# 10u = 6e-7 in the worst case, inside 1e-6.
OSC_TOL = 1e-6

# k_mod.hip / k_fir.hip / kernels.hpp geometry
MOD_TILE = 2048
ROT_TILE = 4096
FM_C = 16
FM_NT = 256
FM_CH = FM_C * FM_NT
TWO_PI_L = np.longdouble(2) * np.arctan2(np.longdouble(0), np.longdouble(-1))

ACYCLIC = ((1500.0, 48e3), (700.0, 48e3), (-5000.0, 48e3), (1.234e6, 10e6))
CYCLIC = ((-1.5e6, 10e6), (100e3, 10e6))
BUDGETS = (5001, 6144, 1)
N_SEAM = 3 * 4096 + 7
N_CYC = 65543


def seam_calls(n, b):
    """The call splits of a seam case (n outputs, table budget b)."""
    out = [[n], [4099, n - 4099]]
    if 0 < b < n:
        out.append([b, n - b])
    if 1 < b < n - 1:
        out.append([b - 1, 1, 1, n - b - 1])
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------- the oscillator ==
_E = {}


def osc_E(lib, f, fs, n, b=1 << 20):
    """(E[0:n] complex64, cyc_start, cyc_len, n_tab) of Rotator / Nco (f, fs) at budget b."""
    key = (float(f), float(fs), int(b))
    if key not in _E or len(_E[key][0]) < n:
        _E[key] = lib.osc_table_phasors(f, fs, max(int(n), 1), int(b))
    e, cs, cl, nt = _E[key]
    return e[:n], cs, cl, nt


class OscAdapter:
    """The oracle with E as its Rotator: what tests/iir_ref.py's truths take their phasors
    from (iir_ref.phasors calls .rotator(ones, f, fs)). Everything else is the oracle's."""

    def __init__(self, oracle, lib, budget):
        self._o, self._lib, self._b = oracle, lib, budget

    def rotator(self, x, freq_hz, fs, chunk=0):
        x = np.asarray(x, np.complex64)
        return rot_rotate(x, osc_E(self._lib, freq_hz, fs, len(x), self._b)[0])

    def __getattr__(self, name):
        return getattr(self._o, name)


def _fma(a, b, c):
    """np_ref._fma on arrays of any length (one element included)."""
    a, b, c = (np.atleast_1d(np.asarray(v, f32)) for v in (a, b, c))
    if a.size == 1:
        return NR._fma(np.repeat(a, 2), np.repeat(b, 2), np.repeat(c, 2))[:1]
    return NR._fma(a, b, c)


def _ri(z):
    z = np.asarray(z, np.complex64)
    return z.real.astype(f32), z.imag.astype(f32)


def _cplx(re, im):
    out = np.empty(len(re), np.complex64)
    out.real, out.imag = re, im
    return out


def rot_rotate(x, p):
    """rotator.rs:80-83: (fma(a, c, -(b s)), fma(b, c, a s))."""
    (a, b), (c, s) = _ri(x), _ri(p)
    if not len(a):
        return np.zeros(0, np.complex64)
    return _cplx(_fma(a, c, -((b * s).astype(f32))), _fma(b, c, (a * s).astype(f32)))


def rot_mix_usb(x, p):
    """rotator.rs:88-94: fma(I, c, Q s)."""
    (a, b), (c, s) = _ri(x), _ri(p)
    return _fma(a, c, (b * s).astype(f32)) if len(a) else a


def nco_mix(x, p):
    """nco.rs:63-66: (a c - b s, a s + b c), no FMA."""
    (a, b), (c, s) = _ri(x), _ri(p)
    return _cplx(((a * c).astype(f32) - (b * s).astype(f32)).astype(f32),
                 ((a * s).astype(f32) + (b * c).astype(f32)).astype(f32))


def am_base(x, cl, mi, g, clamp):
    """am.rs:87-89: m = (cl + mi x) [clamped to +-1] * g, in f32."""
    v = (f32(cl) + (f32(mi) * np.asarray(x, f32)).astype(f32)).astype(f32)
    if clamp:
        v = np.minimum(np.maximum(v, f32(-1.0)), f32(1.0))
    return (v * f32(g)).astype(f32)


def am_restate(x, p, cl, mi, g, clamp):
    m = am_base(x, cl, mi, g, clamp)
    c, s = _ri(p)
    return _cplx((m * c).astype(f32), (m * s).astype(f32))


def cw_env(oracle, key, fs, rise, fall):
    """CwKeyedMod's envelope from the oracle: its output with a 0 Hz tone (w = 1: the
    oscillator stays 1 + 0j, the mix returns (env, 0))."""
    return oracle.cw_mod(key, fs, 0.0, rise, fall).real.astype(f32)


def cw_restate(env, p):
    """cw.rs:80-85: base = (env gain, 0) through mix_with_nco."""
    return nco_mix(_cplx(np.asarray(env, f32), np.zeros(len(env), f32)), p)


def seam_phasors(e, n_tab, lens, tile, mistake=None):
    """The phasors a kernel with tiles of `tile` outputs (from each call's first) serves for
    the calls `lens` when its runs are indexed as osc_run / osc_in_tab index them, from E (e,
    len >= sum(lens) + 1). mistake: None (faithful: e), or
      'exponent'  the model exponent k + 1 - n_tab one too large (every model output is the next one's);
      'rem+'      rem one too large (the first model output of a mixed run read from the table's padding);
      'table'     a mixed run treated as table-only (its model outputs read from the padding).
    The padding of an acyclic table is its last entry at best (osc.cpp uploads nothing there)."""
    n = int(sum(lens))
    out = np.array(e[:n], np.complex64)
    if mistake is None or n_tab >= n:
        return out
    pad = e[n_tab - 1] if n_tab else np.complex64(0)
    if mistake == "exponent":
        out[n_tab:] = e[n_tab + 1:n + 1]
        return out
    k0 = 0
    for ln in lens:
        for t0 in range(k0, k0 + ln, tile):
            t1 = min(t0 + tile, k0 + ln)
            if t0 < n_tab < t0 + tile and n_tab < t1:  # kind 2 (osc_run looks at the whole tile)
                if mistake == "rem+":
                    out[n_tab] = pad
                elif mistake == "table":
                    out[n_tab:t1] = pad
        k0 += ln
    return out


def check_osc_product(name, y, rest, amp, n_tab):
    """A k_rotator mode / AmDsbMod / CwKeyedMod: bit for bit the restatement inside the table;
    past it |y - rest| <= OSC_TOL amp + 2 u amp (amp: |x|, or the base amplitude). Returns
    the measured max of |y - rest| / amp past the table."""
    y, rest = np.asarray(y), np.asarray(rest)
    assert y.shape == rest.shape and y.dtype == rest.dtype, (name, y.shape, rest.shape, y.dtype, rest.dtype)
    assert np.all(np.isfinite(y.view(f32))), f"{name}: non-finite output"
    nt = min(int(n_tab), len(y))
    if not bits_equal(y[:nt], rest[:nt]):
        bad = np.nonzero(y[:nt] != rest[:nt])[0]
        raise AssertionError(f"{name}: differs from the restatement inside the table, first at output "
                             f"{int(bad[0]) if len(bad) else 'a signed zero'} of {nt}")
    if nt == len(y):
        return 0.0
    amp = np.asarray(amp, np.float64)[nt:]
    err = np.abs(y[nt:].astype(np.complex128 if np.iscomplexobj(y) else np.float64) - rest[nt:])
    lim = OSC_TOL * amp + 2 * U * amp
    i = int(np.argmax(err - lim))
    assert err[i] <= lim[i], f"{name}: |y - restatement| = {err[i]:.3e} > {lim[i]:.3e} at output {nt + i} (table {nt})"
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(amp > 0, err / np.where(amp > 0, amp, 1.0), 0.0)))


# --------------------------------------------------------------------------- PM / FM ==
def kf32(dev_hz, fs):
    """fm.rs:48 / blocks.cpp: kf = TAU * dev / fs in f32, left to right."""
    return f32(f32(NR.TAU * f32(dev_hz)) / f32(fs))


def split(x, lens):
    out, i = [], 0
    for n in lens:
        out.append(x[i:i + n])
        i += n
    assert i == len(x), (i, len(x))
    return out


def _per_sample(v, lens):
    v = np.atleast_1d(np.asarray(v))
    if len(v) == 1:
        v = np.repeat(v, len(lens))
    assert len(v) == len(lens)
    return np.repeat(v, lens)


def pm_truth(x, kp, g, r):
    """g (cos phi, sin phi) r with phi = f64(f32(kp x)), r the oscillator, all in f64."""
    phi = (f32(kp) * np.asarray(x, f32)).astype(f32).astype(np.float64)
    return float(f32(g)) * np.exp(1j * phi) * np.asarray(r, np.complex128)


def fm_pairs(x, kf):
    """The correctly rounded f32 (cos, sin) of f32(kf x) (f64 cos / sin, one more rounding:
    correct but for f64 results within 2^-53 relative of an f32 tie). The kernel's sincos_cr
    gives the same pair but for about one value in 10^6 (its own error analysis,
    hip_common.hpp): the truth's pairs rest on that."""
    ph = (np.asarray(kf, f32) * np.asarray(x, f32)).astype(f32).astype(np.float64)
    return np.cos(ph).astype(f32), np.sin(ph).astype(f32)


def fm_truth(x, lens, kf, g, r):
    """y = g e^{j Phi} r: Phi the longdouble running sum (mod 2 pi) of alpha = atan2(ds, dc)
    over the pairs, carried across the calls `lens`; kf and g one value or one per call."""
    x = np.asarray(x, f32)
    dc, ds = fm_pairs(x, _per_sample(kf, lens).astype(f32))
    alpha = np.arctan2(ds.astype(np.longdouble), dc.astype(np.longdouble))
    phi = np.fmod(np.cumsum(alpha), TWO_PI_L).astype(np.float64)
    gs = _per_sample(g, lens).astype(f32).astype(np.float64)
    return gs * np.exp(1j * phi) * np.asarray(r, np.complex128)


def fm_where(i, lens):
    """(call, chunk, thread, k) of output i of the calls `lens`."""
    c = 0
    for c, n in enumerate(lens):
        if i < n:
            break
        i -= n
    return c, i // FM_CH, (i % FM_CH) // FM_C, i % FM_C


def fm_e_ref(oracle, x, fs, dev, rf):
    """FM yardstick: max |oracle - truth| over the first 4096 samples of the oracle's run
    from rest on x, gain 1, truth with the reference's own RF phasors. (The kernel re-seeds
    every 16-sample group from an exact phase: its error must not grow with n, so it is held
    to the reference before that has drifted.)"""
    n = min(len(x), FM_CH)
    xs = np.asarray(x[:n], f32)
    r = oracle.nco(np.zeros(n, np.complex64), rf, fs, gen=True)
    return float(np.max(np.abs(oracle.fm_mod(xs, fs, dev, rf) - fm_truth(xs, [n], kf32(dev, fs), 1.0, r))))


def pm_e_ref(oracle, x, fs, kp, g, rf):
    """PM yardstick: max |oracle - truth| on the same input. The oracle's runner has gain 1;
    the gain scales reference and truth alike, so the yardstick at gain g is |g| times the
    one at gain 1 (without the gain's own rounding: the tighter of the two readings)."""
    x = np.asarray(x, f32)
    r = oracle.nco(np.zeros(len(x), np.complex64), rf, fs, gen=True)
    return abs(float(f32(g))) * float(np.max(np.abs(oracle.pm_mod(x, fs, kp, rf) - pm_truth(x, kp, 1.0, r))))


def check_pm(name, y, truth, e_ref, g, n_tab=None):
    """max |y - truth| <= MARGIN e_ref (+ OSC_TOL g past the table)."""
    assert np.all(np.isfinite(np.asarray(y).view(f32))), f"{name}: non-finite output"
    err = np.abs(np.asarray(y, np.complex128) - truth)
    lim = np.full(len(err), MARGIN * e_ref)
    if n_tab is not None:
        lim[min(int(n_tab), len(err)):] += OSC_TOL * abs(float(f32(g)))
    i = int(np.argmax(err - lim))
    print(f"[parity] {name}: max|gpu - truth| {float(err.max()):.3e} at {int(np.argmax(err))} (tile "
          f"{int(np.argmax(err)) // MOD_TILE}), yardstick e_ref {e_ref:.3e} x {MARGIN:g}")
    assert err[i] <= lim[i], f"{name}: |y - truth| = {err[i]:.3e} > {lim[i]:.3e} at output {i}"
    return float(err.max())


def check_fm(name, y, truth, e_ref, lens, g, n_tab=None):
    """max_n |y - truth| / g <= MARGIN e_ref over the whole run (+ OSC_TOL past the table)."""
    assert np.all(np.isfinite(np.asarray(y).view(f32))), f"{name}: non-finite output"
    gs = np.abs(_per_sample(g, lens).astype(f32).astype(np.float64))
    err = np.abs(np.asarray(y, np.complex128) - truth) / gs
    lim = np.full(len(err), MARGIN * e_ref)
    if n_tab is not None:
        lim[min(int(n_tab), len(err)):] += OSC_TOL
    j = int(np.argmax(err))
    print(f"[parity] {name}: max|gpu - truth|/g {float(err[j]):.3e} at (call, chunk, thread, k) = "
          f"{fm_where(j, lens)}, yardstick e_ref {e_ref:.3e} x {MARGIN:g}")
    i = int(np.argmax(err - lim))
    assert err[i] <= lim[i], (f"{name}: |y - truth|/g = {err[i]:.3e} > {lim[i]:.3e} at (call, chunk, thread, k) = "
                              f"{fm_where(i, lens)}")
    return float(err[j])


def fm_input(kind, n, seed=1):
    """The FM / PM input classes: 'noise' uniform in [-1, 1); 'tones' two tones (0.5 and 0.3
    of amplitude, incommensurate with the chunk); 'impulse' +-1 impulses at the chunk, wave
    and thread-group edges (-1, +0, +1) over a DC offset of 0.3."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-1.0, 1.0, n).astype(f32)
    if kind == "tones":
        k = np.arange(n)
        return (0.5 * np.sin(2 * np.pi * 0.0213 * k) + 0.3 * np.sin(2 * np.pi * 0.1471 * k + 1.0)).astype(f32)
    if kind == "impulse":
        x = np.full(n, 0.3)
        pos = {0, 1}
        for e in list(range(FM_CH, n + FM_CH, FM_CH)) + [FM_C, 2 * FM_C, 64 * FM_C, 128 * FM_C, FM_CH + 64 * FM_C]:
            pos |= {e - 1, e, e + 1}
        pos = np.array(sorted(p for p in pos if 0 <= p < n))
        x[pos] += rng.choice([-1.0, 1.0], len(pos))
        return x.astype(f32)
    raise ValueError(kind)


FM_CLASSES = ("noise", "tones", "impulse")
K_TURNS_PER_RAD = 2.9358905032820014e18  # k_mod.hip: 2^64 / (2 pi)


def _phasor_at(ph):
    """hip_common.hpp phasor_at on uint64 phases (sincospif as the correctly rounded f32)."""
    hi = (ph >> np.uint64(40)).astype(np.float64) * (1.0 / 8388608.0)
    lo = (ph & np.uint64((1 << 40) - 1)).astype(f32)
    s, c = np.sin(np.pi * hi).astype(f32), np.cos(np.pi * hi).astype(f32)
    d = ((lo * f32(6.28318530717958647692 / 1099511627776.0)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    return _fma(-s, d, c), _fma(c, d, s)


def fm_engine_model(x, lens, kf, g, r, passes=1, mistake=None):
    """k_mod.hip's FM kernels restated in numpy (how they index, not their bits: sincospif
    and sincos_cr taken as correctly rounded): per call, threads of 16 samples (pairs (1, 0)
    past the call's end), each thread's pairs multiplied in f64 and one atan2 as a Q0.64 turn
    count (half turns doubled), the exclusive prefix of those counts (wrapping uint64) from
    the carried phase, phasor_at of it, the reference's f32 recurrence over the 16 pairs, the
    gain, the non-FMA mix with r. passes 3: the chunk offsets through k_fm_mod_carry's
    per-thread runs of `per` chunks. mistake: None, or
      'drop_thread'  one thread's sum (thread 77 of each call's first chunk) left out of the prefix;
      'no_carry'     the carried phase of the previous call not applied;
      'per1'         per forced to 1 in k_fm_mod_carry (chunks from 256 on keep their own sum
                     as their offset and are missing from the carried phase)."""
    x = np.asarray(x, f32)
    kfs, gs = _per_sample(kf, [1] * len(lens)).astype(f32), _per_sample(g, [1] * len(lens)).astype(f32)
    out, carry, k0 = [], np.uint64(0), 0
    for ci, (xc, n) in enumerate(zip(split(x, lens), lens)):
        ng = -(-n // FM_C)
        c = np.ones(ng * FM_C, f32)
        s = np.zeros(ng * FM_C, f32)
        c[:n], s[:n] = fm_pairs(xc, kfs[ci])
        c, s = c.reshape(ng, FM_C), s.reshape(ng, FM_C)
        pr, pi = np.ones(ng), np.zeros(ng)
        for k in range(FM_C):
            cc, ss = c[:, k].astype(np.float64), s[:, k].astype(np.float64)
            pr, pi = pr * cc - pi * ss, pr * ss + pi * cc
        q = np.rint(np.arctan2(pi, pr) * K_TURNS_PER_RAD * 0.5).astype(np.int64).astype(np.uint64) * np.uint64(2)
        if mistake == "drop_thread":
            t = 77 if ng > 78 else ng // 2
            if t < ng - 1:
                q = q.copy()
                q[t] = 0
        with np.errstate(over="ignore"):
            cin = np.uint64(0) if mistake == "no_carry" else carry
            excl = np.cumsum(q, dtype=np.uint64) - q
            tot = excl[-1] + q[-1]
            if passes == 3 and mistake == "per1":
                nch = -(-ng // FM_NT)
                sums = np.add.reduceat(q, np.arange(0, ng, FM_NT), dtype=np.uint64)
                offs = np.cumsum(sums, dtype=np.uint64) - sums
                offs[FM_NT:] = sums[FM_NT:]  # never rewritten: still the chunk's own sum
                tot = np.sum(sums[:FM_NT], dtype=np.uint64) if nch > FM_NT else tot
                within = excl - np.repeat(excl[::FM_NT], FM_NT)[:ng]
                excl = np.repeat(offs, FM_NT)[:ng] + within
            ph = cin + excl
            carry = cin + tot
        zr, zi = _phasor_at(ph)
        yr, yi = np.empty((ng, FM_C), f32), np.empty((ng, FM_C), f32)
        for k in range(FM_C):
            zr, zi = (_fma(zr, c[:, k], -((zi * s[:, k]).astype(f32))),
                      _fma(zi, c[:, k], (zr * s[:, k]).astype(f32)))
            yr[:, k], yi[:, k] = (zr * gs[ci]).astype(f32), (zi * gs[ci]).astype(f32)
        out.append(nco_mix(_cplx(yr.reshape(-1)[:n], yi.reshape(-1)[:n]), r[k0:k0 + n]))
        k0 += n
    return np.concatenate(out)
