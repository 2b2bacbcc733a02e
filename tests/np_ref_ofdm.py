"""An independent numpy restatement of the OFDM symbol layer (reference src/multicarrier,
modulate/ofdm.rs, demodulate/ofdm.rs, modulate/qam.rs, demodulate/qam.rs, sync/ofdm_sync.rs:
270-352), f32 operation for operation, for tests/test_ofdm_oracle.py, tests/test_gpu_ofdm.py and
tests/test_gpu_ofdm_exact.py (whose comparison rule, input sets and deliberate departures are at the end).

The transform is an f32 radix-2 decimation in time of its own (the twiddles computed in
f64 by libm and rounded once), and truth for it is numpy.fft in complex128.
"""
import functools
import math

import numpy as np

from np_ref import _fma, cosf, sinf  # glibc's cosf / sinf and the exactly rounded f32 fma

F = np.float32
BITS = {"bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6, "qam256": 8}
ORDERS = list(BITS)
FRAC_1_SQRT_2 = F(0.70710678118654752440)
SQRT_2 = F(1.41421356237309504880)
PI = F(math.pi)
TAU = F(2.0 * math.pi)
EQUALIZER_FLOOR = F(1e-6)


def cplx(re, im):
    """complex64 from its parts with no arithmetic (re + 1j * im loses the sign of a zero)."""
    re, im = np.asarray(re, F), np.asarray(im, F)
    out = np.empty(np.broadcast(re, im).shape, np.complex64)
    out.real, out.imag = re, im
    return out


# ---- constellations -------------------------------------------------------------------------
def axis_scale(bits):  # modulate/qam.rs:27-31
    m = 1 << (bits // 2)
    return F(1.0 / math.sqrt(2.0 * float(m * m - 1) / 3.0))


def axis_table(bits):  # modulate/qam.rs:45-57
    m, t, s = 1 << (bits // 2), np.zeros(16, F), axis_scale(bits)
    for g in range(m):
        t[g ^ (g >> 1)] = F(F(2 * g + 1) - F(m)) * s
    return t


def threshold_table(bits):  # demodulate/qam.rs:28-41
    m, t, s = 1 << (bits // 2), np.zeros(15, F), axis_scale(bits)
    for j in range(m - 1):
        t[j] = F(F(2 * j) - F(m - 2)) * s
    return t


def map_bits(order, bits):
    b = np.asarray(bits, np.uint8) & 1
    nb = BITS[order]
    b = b[: b.size // nb * nb].reshape(-1, nb)
    if order == "bpsk":
        return cplx(np.where(b[:, 0] == 0, F(1), F(-1)), np.zeros(len(b), F))
    if order == "qpsk":
        return cplx(np.where(b[:, 0] == 0, FRAC_1_SQRT_2, -FRAC_1_SQRT_2),
                    np.where(b[:, 1] == 0, FRAC_1_SQRT_2, -FRAC_1_SQRT_2))
    k, t = nb // 2, axis_table(nb)
    w = 1 << np.arange(k - 1, -1, -1)
    return cplx(t[b[:, :k] @ w], t[b[:, k:] @ w])


def decide(order, syms):
    s = np.asarray(syms, np.complex64)
    if order == "bpsk":
        return (s.real < 0).astype(np.uint8)
    if order == "qpsk":
        return np.stack([s.real < 0, s.imag < 0], 1).astype(np.uint8).reshape(-1)
    nb = BITS[order]
    k, thr = nb // 2, threshold_table(nb)[: (1 << (nb // 2)) - 1]
    out = np.zeros((s.size, nb), np.uint8)
    for col, v in ((0, s.real), (k, s.imag)):
        nat = (v[:, None] > thr[None, :]).sum(1)  # NaN exceeds nothing
        gray = nat ^ (nat >> 1)
        for b in range(k):
            out[:, col + b] = (gray >> (k - 1 - b)) & 1
    return out.reshape(-1)


def soft_llr(order, syms):
    s = np.asarray(syms, np.complex64)
    if order == "bpsk":
        return (F(4.0) * s.real).astype(F)
    if order == "qpsk":
        sc = F(F(4.0) * SQRT_2)
        return np.stack([sc * s.real, sc * s.imag], 1).astype(F).reshape(-1)
    nb = BITS[order]
    k, m, t = nb // 2, 1 << (nb // 2), axis_table(nb)
    out = np.zeros((s.size, nb), F)
    g = np.arange(m)
    with np.errstate(invalid="ignore", over="ignore"):
        for col, v in ((0, s.real.astype(F)), (k, s.imag.astype(F))):
            d = v[:, None] - t[None, :m]
            d = (d * d).astype(F)
            for b in range(k):
                one = ((g >> (k - 1 - b)) & 1) == 1
                d0 = np.fmin.reduce(np.concatenate([np.full((s.size, 1), np.inf, F), d[:, ~one]], 1), axis=1)
                d1 = np.fmin.reduce(np.concatenate([np.full((s.size, 1), np.inf, F), d[:, one]], 1), axis=1)
                out[:, col + b] = d1 - d0
    return out.reshape(-1)


# ---- CarrierPlan / CarrierGrid --------------------------------------------------------------
def index_bounds(n_fft):
    return -(n_fft // 2), (n_fft - 1) // 2


def validate(n_fft, data, pilots):
    """config.rs:223-252 -> (code, index): 0 ok, 1 out of range, 2 overlap, 3 empty data."""
    if len(data) == 0:
        return 3, 0
    lo, hi = index_bounds(n_fft)
    for i in list(data) + list(pilots):
        if i < lo or i > hi:
            return 1, int(i)
    seen = set()
    for i in list(data) + list(pilots):
        if int(i) in seen:
            return 2, int(i)
        seen.add(int(i))
    return 0, 0


def validate_edge_guard(n_fft, data, pilots, g):  # config.rs:262-278
    rc = validate(n_fft, data, pilots)
    if rc[0]:
        return rc
    lo, hi = index_bounds(n_fft)
    for i in list(data) + list(pilots):
        if i < lo + g or i > hi - g:
            return 4, int(i)
    return 0, 0


def contiguous_data(n_fft, pilots, edge_guard, include_dc):  # config.rs:128-149
    lo, hi = index_bounds(n_fft)
    ps = set(int(p) for p in pilots)
    return np.array([i for i in range(lo + 1 + edge_guard, hi - edge_guard + 1)
                     if (i != 0 or include_dc) and i not in ps], np.int32)


def bins_of(idx, n_fft):  # grid.rs:48: rem_euclid
    return (np.asarray(idx, np.int64) % n_fft).astype(np.uint32)


def occupied_bins(n_fft, data, pilots):
    return np.unique(np.concatenate([bins_of(data, n_fft), bins_of(pilots, n_fft)])).astype(np.uint32)


def occupied_half_carriers(data, pilots):
    a = np.concatenate([np.asarray(data, np.int64), np.asarray(pilots, np.int64)])
    return int(np.abs(a).max()) if a.size else 0


# ---- the transform --------------------------------------------------------------------------
TINY = np.finfo(F).tiny
FFT_VARIANTS = ("fma", "w0", "f32tw", "ftz", "tw_rot", "tw_rot_fused")  # departures from the host arithmetic, for the tests' own proof
EQ_VARIANTS = ("recip", "interp_fma", "floor_strict")


def ftz(v):
    """Subnormals flushed to a zero of their sign."""
    v = np.asarray(v, F)
    return np.where(np.abs(v) < TINY, np.copysign(F(0), v), v).astype(F)


@functools.lru_cache(maxsize=None)
def _twiddles(n, f32):
    if f32:  # the f32tw departure: the angle and cos / sin in f32
        return np.array([complex(cosf(F(F(TAU * F(k)) / F(n))), -sinf(F(F(TAU * F(k)) / F(n)))) for k in range(n // 2)],
                        np.complex64)
    return np.array([complex(F(math.cos(2.0 * math.pi * k / n)), F(-math.sin(2.0 * math.pi * k / n)))
                     for k in range(n // 2)], np.complex64)


def twiddles(n, f32=False):
    return _twiddles(int(n), bool(f32)).copy()


@functools.lru_cache(maxsize=None)
def _bitrev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def bitrev(n):
    return _bitrev(int(n)).copy()


def fused_second_stages(n):
    """The stage sizes that come second in a pass of two fused stages (a leading radix-2 pass where log2 n is odd)."""
    cur, out = (2 if (n.bit_length() - 1) & 1 else 1), set()
    while cur < n:
        out.add(4 * cur)
        cur <<= 2
    return out


def fft_radix2(x, inverse=False, variant=None):
    """Rows of x (..., n): f32 radix-2 decimation in time: the bit reversal, then stages of size
    2, 4, .. n, every one multiplying by its twiddle (W^0 included) as t.re = b.re w.re - b.im
    w.im, t.im = b.re w.im + b.im w.re, then a + t and a - t; the inverse conjugates the
    twiddles and multiplies by f32(1 / n) at the end.

    variant names one departure from that arithmetic (none of them is the library's): "fma" t.re
    = fma(b.re, w.re, -(b.im w.im)), t.im = fma(b.re, w.im, b.im w.re); "w0" t = b where the
    twiddle index is 0; "f32tw" the twiddles from f32 cos / sin of an f32 angle; "ftz" subnormal
    inputs and results flushed to zero; "tw_rot" the twiddles of the upper half of every stage
    of size >= 4 taken as -i times those a quarter stage below instead of read from the table;
    "tw_rot_fused" the same in the second stage of each fused pair only (sizes 4, 16, 64 .. where
    log2 n is even, 8, 32, 128 .. where it is odd), which is where a kernel that does two stages
    per pass would make that saving."""
    assert variant is None or variant in FFT_VARIANTS, variant
    x = np.array(x, np.complex64)
    n = x.shape[-1]
    tw = twiddles(n, variant == "f32tw")
    p = bitrev(n)
    z = ftz if variant == "ftz" else (lambda v: v)
    re, im = z(x.real.astype(F).reshape(-1, n)[:, p]).copy(), z(x.imag.astype(F).reshape(-1, n)[:, p]).copy()
    ln = 2
    with np.errstate(all="ignore"):
        while ln <= n:
            half, step = ln // 2, n // ln
            wr = tw.real[::step][:half].astype(F)
            wi = tw.imag[::step][:half].astype(F)
            if half >= 2 and (variant == "tw_rot" or (variant == "tw_rot_fused" and ln in fused_second_stages(n))):
                # -i (a + i b) = b - i a
                q = half // 2
                wr, wi = np.concatenate([wr[:q], wi[:q]]), np.concatenate([wi[:q], -wr[:q]])
            if inverse:
                wi = -wi
            r, i = re.reshape(len(re), -1, ln), im.reshape(len(im), -1, ln)
            ar, ai, br, bi = r[..., :half].copy(), i[..., :half].copy(), r[..., half:].copy(), i[..., half:].copy()
            if variant == "fma":
                wrb, wib = np.broadcast_to(wr, br.shape), np.broadcast_to(wi, br.shape)
                tr = _fma(br, wrb, -(bi * wi).astype(F))
                ti = _fma(br, wib, (bi * wr).astype(F))
            else:
                tr = z(z((br * wr).astype(F)) - z((bi * wi).astype(F)))
                ti = z(z((br * wi).astype(F)) + z((bi * wr).astype(F)))
            if variant == "w0":
                tr[..., 0], ti[..., 0] = br[..., 0], bi[..., 0]
            r[..., :half], i[..., :half] = z(ar + tr), z(ai + ti)
            r[..., half:], i[..., half:] = z(ar - tr), z(ai - ti)
            ln *= 2
        if inverse:
            g = F(1.0) / F(n)
            re, im = z(re * g), z(im * g)
    return cplx(re, im).reshape(x.shape)


def fft_truth(x, inverse=False):
    x = np.asarray(x, np.complex64).astype(np.complex128)
    return np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1)


def nrmse(got, want):
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return float(np.sqrt(np.sum(np.abs(got - want) ** 2) / np.sum(np.abs(want) ** 2)))


# ---- window, prefix, rotator ----------------------------------------------------------------
def window_ramp(symbol_len, roll_off):  # symbol_window.rs:47-59
    l = min(roll_off, symbol_len // 2)
    return np.array([F(0.5) * F(F(1.0) - cosf(F(F(PI * F(F(i) + F(0.5))) / F(l)))) for i in range(l)], F)


def window_apply(sym, ramp):  # symbol_window.rs:80-98, rows of (..., symbol_len)
    y = np.array(sym, np.complex64)
    l = len(ramp)
    if l:
        w = np.ones(y.shape[-1], F)
        w[:l] = ramp
        edge = np.zeros(y.shape[-1], bool)
        edge[:l] = True
        edge[-l:] = True
        w[-l:] = ramp[::-1]
        re = np.where(edge, (y.real * w).astype(F), y.real)
        im = np.where(edge, (y.imag * w).astype(F), y.imag)
        y = cplx(re, im)
    return y


def rotator(freq_hz, fs, n):  # dsp/rotator.rs:16-61
    phi = F(F(TAU * F(freq_hz)) / F(fs))
    wr, wi = cosf(phi), sinf(phi)
    zr, zi, out = F(1), F(0), np.zeros(n, np.complex64)
    for k in range(n):
        zr, zi = _fma(zr, wr, -F(zi * wi)), _fma(zi, wr, F(zr * wi))
        if ((k + 1) & 0x3FF) == 0:
            inv = F(1.0) / np.sqrt(F(F(zr * zr) + F(zi * zi)))
            zr, zi = F(zr * inv), F(zi * inv)
        out[k] = complex(zr, zi)
    return out


def rotate_gain(s, r, g):  # modulate/ofdm.rs:525-532
    s, r, g = np.asarray(s, np.complex64), np.asarray(r, np.complex64), F(g)
    sr, si, rr, ri = s.real.astype(F), s.imag.astype(F), r.real.astype(F), r.imag.astype(F)
    re = g * _fma(sr, rr, -(si * ri).astype(F))
    im = g * _fma(si, rr, (sr * ri).astype(F))
    return cplx(re, im)


def gain(s, g):
    s = np.asarray(s, np.complex64)
    return cplx(F(g) * s.real, F(g) * s.imag)


# ---- OfdmMod / OfdmDemod --------------------------------------------------------------------
class Config:
    def __init__(self, n_fft, cp_len, data, pilot_idx, pilot_val, fs=1e6, rf_hz=0.0, gain=1.0, order="qpsk",
                 backoff=0, roll_off=0):
        self.n_fft, self.cp_len, self.order = n_fft, cp_len, order
        self.data, self.pilot_idx = np.asarray(data, np.int32), np.asarray(pilot_idx, np.int32)
        self.pilot_val = np.asarray(pilot_val, np.complex64)
        self.fs, self.rf_hz, self.gain, self.backoff, self.roll_off = fs, rf_hz, gain, backoff, roll_off
        self.data_bins, self.pilot_bins = bins_of(self.data, n_fft), bins_of(self.pilot_idx, n_fft)
        self.bps = len(self.data) * BITS[order]
        self.sym_len = n_fft + cp_len


def modulate(cfg, bits, rot=None):
    """OfdmMod::modulate (modulate/ofdm.rs:469-543): baseband at cfg.gain (the symbol window
    before the gain); with rot (the rotator's phasors for these samples) the RF form."""
    bits = np.asarray(bits, np.uint8)
    nsym = -(-bits.size // cfg.bps)
    padded = np.zeros(nsym * cfg.bps, np.uint8)
    padded[: bits.size] = bits
    syms = map_bits(cfg.order, padded).reshape(nsym, -1)
    freq = np.zeros((nsym, cfg.n_fft), np.complex64)
    freq[:, cfg.data_bins] = syms
    freq[:, cfg.pilot_bins] = cfg.pilot_val
    t = fft_radix2(freq, True)
    y = np.concatenate([t[:, cfg.n_fft - cfg.cp_len:], t], 1) if cfg.cp_len else t
    y = window_apply(y, window_ramp(cfg.sym_len, cfg.roll_off)).reshape(-1)
    return rotate_gain(y, rot, cfg.gain) if rot is not None else gain(y, cfg.gain)


def symbol_freq(cfg, iq, transform=fft_radix2):
    """SymbolFft::demod_symbol (symbol_fft.rs:112-126) of every whole symbol: (nsym, n_fft)."""
    iq = np.asarray(iq, np.complex64)
    nsym = iq.size // cfg.sym_len
    start = cfg.cp_len - min(cfg.backoff, cfg.cp_len)
    w = iq[: nsym * cfg.sym_len].reshape(nsym, cfg.sym_len)[:, start: start + cfg.n_fft]
    return transform(w)


def demodulate(cfg, iq, g=1.0, eq=None, transform=fft_radix2):
    """OfdmDemod::process (demodulate/ofdm.rs:67-94), eq (an Equalizer) between the transform
    and the gather."""
    f = symbol_freq(cfg, iq, transform)
    if eq is not None:
        f = np.stack([eq.process(row) for row in f]) if len(f) else f
    s = f[:, cfg.data_bins].reshape(-1).astype(np.complex64)
    return gain(s, g) if abs(F(g) - F(1.0)) > np.finfo(F).eps else s


# ---- OfdmEqualizer --------------------------------------------------------------------------
def training_pattern(n_fft):  # sync/ofdm_sync.rs:270-272, :335-352
    state, mask, out = 0x4F46444D54524E31, (1 << 64) - 1, np.zeros(n_fft, np.complex64)

    def nxt():
        nonlocal state
        state ^= (state << 13) & mask
        state ^= state >> 7
        state ^= (state << 17) & mask
        return F(F(np.uint64(state)) / F(2.0 ** 64)) - F(0.5)

    for i in range(n_fft):
        re = FRAC_1_SQRT_2 if nxt() >= 0 else -FRAC_1_SQRT_2
        im = FRAC_1_SQRT_2 if nxt() >= 0 else -FRAC_1_SQRT_2
        out[i] = complex(re, im)
    return out


def cdiv(a, b, variant=None):
    """num-complex Complex / Complex: ((a.re b.re + a.im b.im) / |b|^2, (a.im b.re - a.re b.im) / |b|^2).
    variant "recip" (a departure, not the library's): times f32(1 / |b|^2) instead."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    ar, ai, br, bi = a.real.astype(F), a.imag.astype(F), b.real.astype(F), b.imag.astype(F)
    with np.errstate(all="ignore"):
        ns = (br * br).astype(F) + (bi * bi).astype(F)
        if variant == "recip":
            inv = (F(1.0) / ns).astype(F)
            re = ((ar * br).astype(F) + (ai * bi).astype(F)) * inv
            im = ((ai * br).astype(F) - (ar * bi).astype(F)) * inv
        else:
            re = ((ar * br).astype(F) + (ai * bi).astype(F)) / ns
            im = ((ai * br).astype(F) - (ar * bi).astype(F)) / ns
    return cplx(re, im)


def cmul(a, b):
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    ar, ai, br, bi = a.real.astype(F), a.imag.astype(F), b.real.astype(F), b.imag.astype(F)
    with np.errstate(all="ignore"):
        re = (ar * br).astype(F) - (ai * bi).astype(F)
        im = (ar * bi).astype(F) + (ai * br).astype(F)
    return cplx(re, im)


def equalizer_weight(h, variant=None):  # demodulate/ofdm.rs:495-502; "floor_strict" (a departure): m > floor
    h = np.atleast_1d(np.asarray(h, np.complex64))
    hr, hi = h.real.astype(F), h.imag.astype(F)
    with np.errstate(all="ignore"):
        m = (hr * hr).astype(F) + (hi * hi).astype(F)
        ok = m > EQUALIZER_FLOOR if variant == "floor_strict" else m >= EQUALIZER_FLOOR
        re = np.where(ok, hr / m, F(0)).astype(F)
        im = np.where(ok, -hi / m, F(0)).astype(F)
    return cplx(re, im)


def interpolate_at(pbins, ratios, b, variant=None):  # demodulate/ofdm.rs:514-537; "interp_fma" (a departure): one fma
    pbins = [int(p) for p in pbins]
    if len(pbins) == 1:
        return np.complex64(ratios[0])
    hi = sum(1 for p in pbins if p < b)
    if hi == 0:
        return np.complex64(ratios[0])
    if hi == len(pbins):
        return np.complex64(ratios[-1])
    if pbins[hi] == b:
        return np.complex64(ratios[hi])
    t = F(F(b - pbins[hi - 1]) / F(pbins[hi] - pbins[hi - 1]))
    lr, ur = np.complex64(ratios[hi - 1]), np.complex64(ratios[hi])
    with np.errstate(all="ignore"):
        if variant == "interp_fma":
            re = _fma(F(F(ur.real) - F(lr.real)), t, F(lr.real))
            im = _fma(F(F(ur.imag) - F(lr.imag)), t, F(lr.imag))
        else:
            re = F(lr.real) + F(F(F(ur.real) - F(lr.real)) * t)
            im = F(lr.imag) + F(F(F(ur.imag) - F(lr.imag)) * t)
    return cplx(re, im)[()]


def interpolate_bins(pbins, ratios, bins, variant=None):
    """interpolate_at at many bins in one pass, the same operations elementwise (the tests hold
    the two to the same bytes); what Equalizer.process uses."""
    pb, bins = np.asarray(pbins, np.int64), np.asarray(bins, np.int64)
    ratios = np.asarray(ratios, np.complex64)
    if len(pb) == 1:
        return np.full(len(bins), ratios[0], np.complex64)
    hi = np.searchsorted(pb, bins, side="left")  # how many pilots lie below the bin
    out = ratios[np.clip(hi, 0, len(pb) - 1)].copy()  # held past the ends, a pilot's own ratio on its bin
    between = (hi > 0) & (hi < len(pb)) & (pb[np.clip(hi, 0, len(pb) - 1)] != bins)
    h = hi[between]
    t = ((bins[between] - pb[h - 1]).astype(F) / (pb[h] - pb[h - 1]).astype(F)).astype(F)
    lr, ur = ratios[h - 1], ratios[h]
    with np.errstate(all="ignore"):
        dr, di = (ur.real - lr.real).astype(F), (ur.imag - lr.imag).astype(F)
        if variant == "interp_fma":
            re, im = _fma(dr, t, lr.real.astype(F)), _fma(di, t, lr.imag.astype(F))
        else:
            re, im = lr.real + (dr * t).astype(F), lr.imag + (di * t).astype(F)
    if h.size:
        out[between] = cplx(re, im)
    return out


class Equalizer:
    def __init__(self, cfg, method, variant=None):
        assert variant is None or variant in EQ_VARIANTS, variant
        self.method, self.n, self.variant = method, cfg.n_fft, variant
        order = np.argsort(cfg.pilot_bins, kind="stable")
        self.pbins, self.pvals = cfg.pilot_bins[order], cfg.pilot_val[order]
        self.dbins = cfg.data_bins.copy()
        self.est = np.ones(self.n, np.complex64)
        self.weight = np.ones(self.n, np.complex64)

    def estimate_from_training_symbol(self, rx):
        if self.method == "training_symbol" and len(rx) >= self.n:
            self.weight = equalizer_weight(cdiv(np.asarray(rx, np.complex64)[: self.n], training_pattern(self.n),
                                                self.variant), self.variant)

    def process(self, x):
        x = np.asarray(x, np.complex64)[: self.n]
        if self.method == "pilot_interp":
            if len(self.pbins):
                ratios = cdiv(x[self.pbins], self.pvals, self.variant)
                self.est[self.dbins] = interpolate_bins(self.pbins, ratios, self.dbins, self.variant)
                self.est[self.pbins] = ratios
            return cmul(x, equalizer_weight(self.est, self.variant))
        return cmul(x, self.weight)


def evm_db(order, soft, bits):  # demodulate/ofdm.rs:263-293
    soft = np.asarray(soft, np.complex64)
    ideal = map_bits(order, bits)
    if soft.size == 0 or ideal.size != soft.size:
        return None
    er, ei = (soft.real - ideal.real).astype(F), (soft.imag - ideal.imag).astype(F)
    err = ref = 0.0  # sequential f64 sums, as the reference's loop
    for v in ((er * er).astype(F) + (ei * ei).astype(F)).tolist():
        err += v
    for v in ((ideal.real * ideal.real).astype(F) + (ideal.imag * ideal.imag).astype(F)).tolist():
        ref += v
    if ref <= 0:
        return None
    return F(10.0 * math.log10(err / ref)) if err > 0 else F(-np.inf)


# ---- shared test inputs ---------------------------------------------------------------------
def edge_values(order, rng, n=4099):
    """Random normal soft symbols, then on both axes the exact thresholds, +-0 and the values
    one ulp either side of each threshold."""
    v = (0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    thr = threshold_table(BITS[order])[: (1 << (BITS[order] // 2)) - 1] if BITS[order] >= 4 else np.zeros(1, np.float32)
    sp = np.concatenate([thr, np.nextafter(thr, np.float32(np.inf)), np.nextafter(thr, np.float32(-np.inf)),
                         np.array([0.0, -0.0], np.float32)]).astype(np.float32)
    k = sp.size
    v[:k] = cplx(sp, v[:k].imag)
    v[k: 2 * k] = cplx(v[k: 2 * k].real, sp)
    v[2 * k: 3 * k] = cplx(sp, sp[::-1])
    assert np.signbit(v[:k].real).sum() > np.sum(sp < 0)  # the -0.0 is in
    return v


def channel3(iq):
    """A static 3-tap channel, applied per channel stream (the prefix absorbs it)."""
    taps = np.array([1.0, 0.35 - 0.2j, -0.15 + 0.1j], np.complex128)
    return np.convolve(iq.astype(np.complex128), taps)[: iq.size].astype(np.complex64)


def training_symbol(r):
    """The training pattern on the plan's occupied bins (sync/ofdm_sync.rs:286-332)."""
    f = np.zeros(r.n_fft, np.complex64)
    occ = occupied_bins(r.n_fft, r.data, r.pilot_idx)
    f[occ] = training_pattern(r.n_fft)[occ]
    t = fft_radix2(f, True)
    return np.concatenate([t[r.n_fft - r.cp_len:], t])


# ---- exact comparison and the exact tests' inputs -------------------------------------------
def _words(a):
    """The real words of a float or complex array as unsigned integers (other dtypes: as they are)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(np.float32 if a.dtype == np.complex64 else np.float64)
    if a.dtype.kind == "f":
        return a, a.view(np.dtype(f"u{a.dtype.itemsize}"))
    return None, a


def diff_words(a, b):
    """How many words of two arrays of one shape and dtype differ: a NaN against a NaN is no
    difference (the host's default NaN and the device's have other payloads and signs), every
    other word counts unless it is byte-equal, the sign of a zero or an inf included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    fa, wa = _words(a)
    fb, wb = _words(b)
    if fa is None:
        return int(np.count_nonzero(wa != wb))
    na, nb = np.isnan(fa), np.isnan(fb)
    return int(np.count_nonzero((na != nb) | (~na & ~nb & (wa != wb))))


def same_bits(a, b):
    """Equal shapes and dtypes, NaN in the same words of both, every other word byte-equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and diff_words(a, b) == 0


FFT_SIZES = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
# default_rng([seed, n]). The scaled seed is the first from 7104 up whose rows meet the overflow condition at every
# size (7104 draws one quiet row at n = 8 that stays finite at three times the top scale).
SET_SEEDS = {"normal": 7101, "integers": 7102, "negzero": 7103, "scaled": 7106}
SUBNORMAL_SCALE = 2e-41  # every output word of the restatement subnormal or zero, n = 8 .. 4096
OVERFLOW_OVER_TOP = 3.0  # overflow rows = top rows x 3: an inf in every row, under half the words NaN (found on the CPU)


def top_scale(n):
    return 3e38 / math.sqrt(n) / 4.0


def input_sets(n):
    """The transform's seeded input sets for size n: {name: (rows, n) complex64}.
    normal: complex normal rows. integers: Gaussian integers, |re|, |im| <= 8 (exact sums, equal
    magnitudes cancelling). negzero: a row of -0.0 - 0.0j and a row of +0.0 with a single -0.0.
    impulse: unit impulses 1 at index 1, i at n - 1, -1 at 3 and 1 at n / 2 + 1: half of every butterfly
    is an exact zero, so the output is the twiddle products themselves, to the last bit.
    subnormal / top / overflow: the same three normal rows at 2e-41, at 3e38 / sqrt(n) / 4 and
    at three times that (tests/test_ofdm_oracle.py holds the restatement's outputs to: subnormal
    or zero; all finite; an inf in every row and at most half the words NaN)."""
    def rng(name):
        return np.random.default_rng([SET_SEEDS[name], n])

    def normal(g, rows):
        return g.standard_normal((rows, n)) + 1j * g.standard_normal((rows, n))

    sets = {"normal": normal(rng("normal"), 4).astype(np.complex64)}
    g = rng("integers")
    sets["integers"] = cplx(g.integers(-8, 9, (4, n)).astype(F), g.integers(-8, 9, (4, n)).astype(F))
    z = np.zeros((2, 2 * n), F)
    z[0] = F(-0.0)
    z[1, int(rng("negzero").integers(0, 2 * n))] = F(-0.0)
    sets["negzero"] = z.view(np.complex64)
    sets["impulse"] = np.zeros((4, n), np.complex64)
    for row, (at, v) in enumerate(((1, 1), (n - 1, 1j), (3, -1), (n // 2 + 1, 1))):
        sets["impulse"][row, at] = v
    base = normal(rng("scaled"), 3)
    for name, scale in (("subnormal", SUBNORMAL_SCALE), ("top", top_scale(n)), ("overflow", OVERFLOW_OVER_TOP * top_scale(n))):
        with np.errstate(over="ignore"):
            sets[name] = (base * scale).astype(np.complex64)
        assert np.all(np.isfinite(sets[name].view(F))), (name, n)  # one inf going in is NaN everywhere coming out
    return sets


def cycle_rows(x, k):
    """k rows drawn from x's in turn."""
    return np.ascontiguousarray(x[np.arange(k) % len(x)])


def pilot_layout(n, boost=False):
    """(edge guard, pilot indices, pilot values) of the exact tests: n >= 32 the four pilots
    -21, -7, 7, 21 of n_fft 64 scaled by n / 64 (out of bin order), n = 16 two pilots, n = 8
    one; boost: the values times 4/3 (so that a division by |pilot|^2 is no division by 1)."""
    if n >= 32:
        idx = np.array([-(21 * n // 64), -(7 * n // 64), 7 * n // 64, 21 * n // 64], np.int32)
        val = np.array([1, -1, 1j, 1], np.complex64)
    elif n == 16:
        idx, val = np.array([-3, 3], np.int32), np.array([1, -1], np.complex64)
    else:
        idx, val = np.array([2], np.int32), np.array([1j], np.complex64)
    if boost:
        val = gain(val, F(4.0) / F(3.0))
    return n // 16, idx, val


def floor_triplet(pval, variant=None):
    """Three received pilot values whose estimate rx / pval has |h|^2 one ulp below
    kEqualizerFloor, exactly on it and one ulp above it, found by search on cdiv itself."""
    lo, hi = np.nextafter(EQUALIZER_FLOOR, F(0)), np.nextafter(EQUALIZER_FLOOR, F(1))
    root = np.sqrt(EQUALIZER_FLOOR).astype(F)
    hr = root
    for _ in range(40):
        hr = np.nextafter(hr, F(0))
    cand_r = [hr]
    for _ in range(80):
        cand_r.append(np.nextafter(cand_r[-1], F(1)))
    cand_i = np.sqrt(np.arange(0, 400) * 0.125 * float(hi - EQUALIZER_FLOOR)).astype(F)
    h = cplx(np.repeat(np.array(cand_r, F), len(cand_i)), np.tile(cand_i, len(cand_r)))
    rx = cmul(h, np.full(h.shape, pval, np.complex64))
    est = cdiv(rx, np.full(h.shape, pval, np.complex64), variant)
    m = (est.real * est.real).astype(F) + (est.imag * est.imag).astype(F)
    out = []
    for target in (lo, EQUALIZER_FLOOR, hi):
        hit = np.flatnonzero(m == target)
        assert hit.size, f"no received pilot gives |h|^2 == {target!r}"
        out.append(rx[hit[0]])
    return np.array(out, np.complex64)


EQ_ROWS = {"plain": 0, "pilot_zero": 1, "crossing": 2, "floor_below": 3, "floor_on": 4, "floor_above": 5, "last": 6}
EQ_SEED = 7201


def equalizer_case(n, boost=False):
    """(Config, x (7, n) complex64) for the pilot-interpolating equalizer: normal rows (std 0.7)
    with, by EQ_ROWS: the second bin-sorted pilot (the only one at n = 8) received as exactly 0;
    the first and second received as -0.003 and +0.004 times their values, so that the estimate
    between them passes through 0 and |h|^2 crosses the floor twice among the data bins;
    the first pilot's estimate with |h|^2 one ulp below the floor, on it and one ulp above it
    (the data bins below the first pilot hold that estimate). Rows 0 and 6 are left as drawn."""
    guard, idx, val = pilot_layout(n, boost)
    cfg = Config(n, n // 4, contiguous_data(n, idx, guard, False), idx, val, order="qam16")
    g = np.random.default_rng([EQ_SEED, n])
    x = (0.7 * (g.standard_normal((7, n)) + 1j * g.standard_normal((7, n)))).astype(np.complex64)
    order = np.argsort(cfg.pilot_bins, kind="stable")
    pb, pv = cfg.pilot_bins[order], cfg.pilot_val[order]
    second = min(1, len(pb) - 1)
    x[EQ_ROWS["pilot_zero"], pb[second]] = 0
    if len(pb) >= 2:
        x[EQ_ROWS["crossing"], pb[0]] = gain(pv[0], F(-0.003))
        x[EQ_ROWS["crossing"], pb[1]] = gain(pv[1], F(0.004))
    x[[EQ_ROWS["floor_below"], EQ_ROWS["floor_on"], EQ_ROWS["floor_above"]], pb[0]] = floor_triplet(pv[0])
    return cfg, x


def equalizer_run(cfg, x, variant=None):
    """The pilot-interpolating Equalizer over the rows of x on one handle: (outputs, erased),
    erased[r, b] where row r's coefficient at bin b is 0."""
    eq = Equalizer(cfg, "pilot_interp", variant)
    out, erased = [], []
    for row in x:
        out.append(eq.process(row))
        erased.append(equalizer_weight(eq.est, variant) == 0)
    return np.stack(out), np.stack(erased)


def check_equalizer_erasures(cfg, erased):
    """What equalizer_case builds, asserted on the restatement's own erasures."""
    pb = np.sort(cfg.pilot_bins)
    held = cfg.data_bins if len(pb) == 1 else cfg.data_bins[cfg.data_bins < pb[0]]
    first = np.concatenate([held, pb[:1]]).astype(np.int64)  # the bins that carry the first pilot's estimate
    assert held.size > 0
    assert not erased[EQ_ROWS["plain"]].any() and not erased[EQ_ROWS["last"]].any()
    assert erased[EQ_ROWS["pilot_zero"], pb[min(1, len(pb) - 1)]]
    assert erased[EQ_ROWS["floor_below"]][first].all()
    assert not erased[EQ_ROWS["floor_on"]][first].any() and not erased[EQ_ROWS["floor_above"]][first].any()
    if len(pb) >= 2:
        between = np.sort(cfg.data_bins[(cfg.data_bins > pb[0]) & (cfg.data_bins < pb[1])]).astype(np.int64)
        e = erased[EQ_ROWS["crossing"]][between]
        assert e.any() and not e[0] and not e[-1]  # kept, erased, kept: the floor is crossed twice among data bins
        assert not erased[EQ_ROWS["crossing"]][first].any()
