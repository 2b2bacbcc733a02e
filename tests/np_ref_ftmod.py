"""TEST INFRASTRUCTURE — numpy float32 restatement of the reference's FT8 / FT4 modulators
and hard demodulators (src/modulate/ft8.rs, ft4.rs, src/demodulate/ft8.rs, ft4.rs) in the
reference's own operation order, and the f64 closed form the device modulator is measured
against. `_fma`, `cosf`, `sinf` and `f32` come from np_ref; the RF stage runs through the C
oracle's Rotator (oracle.rotator: a fresh Rotator, rotate_block).

The modulator's phasor recurrence is one serial chain over the frame: the restatement
loops over the 151,680 (60,480) samples in Python, vectorised over the cases asked for
at once (a few seconds per call), and caches the phasors per (mode, fs, base_hz, data):
gain and the RF stage are applied to the cached phasors.
"""

import numpy as np

import np_ref_sync as S
from np_ref import TAU, _fma, cosf, f32, sinf

FT8, FT4 = S.FT8, S.FT4
MODES = {"ft8": FT8, "ft4": FT4}
# pi to long-double precision: the double nearest pi plus its residual
PI_LD = np.longdouble(3.141592653589793) + np.longdouble(1.2246467991473532e-16)


def frame_len(mode):
    return mode["sps"] * mode["total"]


def symbol_sequence(mode, data):
    """build_symbol_sequence (ft8.rs:65-85, ft4.rs:73-103), by position flags as the reference."""
    reserved = np.zeros(mode["total"], bool)
    syms = np.zeros(mode["total"], np.uint8)
    if mode["name"] == "ft4":
        reserved[[0, 104]] = True
    for blk, p in enumerate(mode["pos"]):
        c = mode["costas"][blk]
        reserved[p:p + len(c)] = True
        syms[p:p + len(c)] = c
    data = np.asarray(data, np.uint8)
    assert len(data) == mode["data"] == int((~reserved).sum())
    syms[~reserved] = data
    return syms


def data_positions(mode):
    return np.flatnonzero(symbol_sequence(mode, np.full(mode["data"], 255, np.uint8)) == 255)


def tone_steps(mode, fs, base_hz, sign=1.0):
    """w_k = (cos phi, sin phi), phi = f32(sign TAU * f / fs), f = base + f32(k) * spacing
    (ft8.rs:98-101; sign -1: the demodulator's, demodulate/ft8.rs:39-44)."""
    nt = mode["tones"]
    wr, wi = np.empty(nt, f32), np.empty(nt, f32)
    for k in range(nt):
        f = f32(f32(base_hz) + f32(f32(k) * mode["spacing"]))
        phi = f32(f32(f32(sign) * TAU * f) / f32(fs))
        wr[k], wi[k] = cosf(phi), sinf(phi)
    return wr, wi


# ------------------------------------------------------------------ modulator --
_PHASORS = {}


def recurrence_phasors(mode, fs, cases):
    """The running phasor z after every sample's step (ft8.rs:94-147) for each case
    (base_hz, data tuple): a list of complex64 [frame_len]. All uncached cases run in one
    pass over the samples."""
    keys = [(mode["name"], float(fs), float(b), tuple(int(t) for t in d)) for b, d in cases]
    todo = [k for k in dict.fromkeys(keys) if k not in _PHASORS]
    if todo:
        c = max(2, len(todo))  # np_ref._fma wants arrays: carry a copy when one case is asked for
        run = todo + [todo[-1]] * (c - len(todo))
        sps, total = mode["sps"], mode["total"]
        syms = np.stack([symbol_sequence(mode, k[3]) for k in run])
        steps = [tone_steps(mode, fs, k[2]) for k in run]
        out = np.empty((2, c, sps * total), f32)
        z = np.stack([np.ones(c, f32), np.zeros(c, f32)])  # (re, im) rows
        ctr = 0
        idx = 0
        rows = np.arange(c)
        for s in range(total):
            wr = np.array([steps[j][0][syms[j, s]] for j in rows], f32)
            wi = np.array([steps[j][1][syms[j, s]] for j in rows], f32)
            for i in range(sps):
                # zr' = fma(zr, wr, -(zi wi)); zi' = fma(zi, wr, zr wi)
                cross = z[::-1] * wi
                cross[0] = -cross[0]
                z = _fma(z, wr[None, :], cross)
                out[:, :, idx] = z
                idx += 1
                if i % 4 == 3 and i < (sps & ~3):
                    ctr += 4
                    if (ctr & 0x3FF) < 4:
                        r2 = z[0] * z[0] + z[1] * z[1]
                        inv = f32(1.0) / np.sqrt(r2)
                        z = z * inv[None, :]
                elif i >= (sps & ~3):
                    ctr += 1
        for j, k in enumerate(todo):
            zc = (out[0, j] + 1j * out[1, j]).astype(np.complex64)
            zc.setflags(write=False)
            _PHASORS[k] = zc
    return [_PHASORS[k] for k in keys]


def modulate(mode, fs, base_hz, rf_hz, gain, data):
    """Ft8Mod / Ft4Mod::modulate (ft8.rs:88-156): complex64 [frame_len]."""
    z = recurrence_phasors(mode, fs, [(base_hz, data)])[0]
    g = f32(gain)
    out = (g * z.real + 1j * (g * z.imag)).astype(np.complex64)
    if f32(rf_hz) != 0:
        import oracle

        out = oracle.rotator(out, float(rf_hz), float(fs))
    return out


# ---------------------------------------------------------------- closed form --
def q_steps(mode, fs, base_hz):
    """Each tone step's angle as a Q0.64 fraction of a turn, in long double: Python ints."""
    wr, wi = tone_steps(mode, fs, base_hz)
    out = []
    for k in range(mode["tones"]):
        rev = np.arctan2(np.longdouble(wi[k]), np.longdouble(wr[k])) / (2 * PI_LD)
        if rev < 0:
            rev += np.longdouble(1.0)
        out.append(int(np.rint(rev * np.longdouble(2.0) ** 64)) % (1 << 64))
    return out


def enter_phases(mode, syms, steps):
    """The phase entering each symbol: wrapping sums of sps * step[tone] (Python ints)."""
    out, ph = [], 0
    for s in syms:
        out.append(ph)
        ph = (ph + mode["sps"] * int(steps[int(s)])) % (1 << 64)
    return out


def closed_form(mode, fs, base_hz, data, steps=None):
    """e^{j 2 pi ph / 2^64}, ph = enter[s] + (i + 1) step[tone_s], as complex128 [frame_len]:
    the f64 phasor of the Q-steps (steps: the library's, or q_steps)."""
    steps = q_steps(mode, fs, base_hz) if steps is None else [int(v) for v in steps]
    syms = symbol_sequence(mode, data)
    enter = np.array(enter_phases(mode, syms, steps), np.uint64)
    st = np.array([steps[int(s)] for s in syms], np.uint64)
    i1 = np.arange(1, mode["sps"] + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ph = (enter[:, None] + st[:, None] * i1[None, :]).ravel()  # wraps modulo 2^64
    a = ph.astype(np.float64) * (2.0 * np.pi / 2.0 ** 64)
    return np.cos(a) + 1j * np.sin(a)


def d0(z_rec, z_cf):
    """max |dz| between the recurrence's phasors and the closed form's."""
    return float(np.max(np.abs(np.asarray(z_rec, np.complex128) - z_cf)))


# ---------------------------------------------------------------- demodulator --
def demod_energies(mode, fs, base_hz, iq):
    """detect_tone's correlator energy (demodulate/ft8.rs:74-126) of every (symbol, tone) of
    the first frame length of iq: float32 [total][tones]. Vectorised over the cells."""
    sps, total, nt = mode["sps"], mode["total"], mode["tones"]
    x = np.asarray(iq, np.complex64)[:sps * total].reshape(total, sps)
    xr, xi = x.real.astype(f32), x.imag.astype(f32)
    wr, wi = tone_steps(mode, fs, base_hz, -1.0)
    ar, ai = np.zeros((total, nt), f32), np.zeros((total, nt), f32)
    pr, pi = np.ones(nt, f32), np.zeros(nt, f32)
    with np.errstate(invalid="ignore"):
        for i in range(sps):
            a, b = xr[:, i][:, None], xi[:, i][:, None]
            # num-complex Mul (no FMA), AddAssign
            ar = ar + (a * pr[None, :] - b * pi[None, :])
            ai = ai + (a * pi[None, :] + b * pr[None, :])
            pr, pi = _fma(pr, wr, -(pi * wi)), _fma(pi, wr, pr * wi)
        return (ar * ar + ai * ai).astype(f32)


def pick_tones(mode, energies):
    """The strict > argmax from -1.0 in tone order (a NaN never wins), sync positions dropped."""
    e = np.asarray(energies, f32)
    best = np.full(e.shape[0], f32(-1.0))
    tone = np.zeros(e.shape[0], np.uint8)
    with np.errstate(invalid="ignore"):
        for k in range(e.shape[1]):
            better = e[:, k] > best
            best = np.where(better, e[:, k], best)
            tone = np.where(better, np.uint8(k), tone)
    return tone[data_positions(mode)].astype(np.uint8)


def demodulate(mode, fs, base_hz, iq):
    e = demod_energies(mode, fs, base_hz, iq)
    return pick_tones(mode, e), e


def frame_data(mode, seed):
    return np.random.default_rng(seed).integers(0, mode["tones"], mode["data"]).astype(np.uint8)
