"""An independent restatement of the reference's PSK31 (test infrastructure): Varicode
(src/codec/varicode.rs), QPSK31's rate 1/2, K = 5 convolutional code with its Viterbi
decoders (src/codec/psk31.rs), and further down the modulators and demodulators
(src/modulate/psk31.rs, src/demodulate/psk31.rs), in plain Python over numpy float32
scalars and vectors, so that every * and + rounds once to f32 as the reference's do. The library's host layer
(csrc/psk31.cpp) is held to this file byte for byte by tests/test_psk31_oracle.py.

Nothing here is shared with the library: the alphabet is stated again below, the trellis is
walked predecessor by predecessor as psk31.rs:110-136 does, and the survivor table stores
previous states (the kernel stores two bits per state instead)."""
import numpy as np

F = np.float32
VARICODE_MAX_BITS = 10
TRACEBACK_DEPTH = 32
PATHMEM = 128

# G3PLX Varicode, ASCII 0..127, codewords as transmitted (varicode.rs:27-156)
_ALPHABET = """
1010101011 1011011011 1011101101 1101110111 1011101011 1101011111 1011101111 1011111101
1011111111 11101111 11101 1101101111 1011011101 11111 1101110101 1110101011
1011110111 1011110101 1110101101 1110101111 1101011011 1101101011 1101101101 1101010111
1101111011 1101111101 1110110111 1101010101 1101011101 1110111011 1011111011 1101111111
1 111111111 101011111 111110101 111011011 1011010101 1010111011 101111111
11111011 11110111 101101111 111011111 1110101 110101 1010111 110101111
10110111 10111101 11101101 11111111 101110111 101011011 101101011 110101101
110101011 110110111 11110101 110111101 111101101 1010101 111010111 1010101111
1010111101 1111101 11101011 10101101 10110101 1110111 11011011 11111101
101010101 1111111 111111101 101111101 11010111 10111011 11011101 10101011
11010101 111011101 10101111 1101111 1101101 101010111 110110101 101011101
101110101 101111011 1010101101 111110111 111101111 111111011 1010111111 101101101
1011011111 1011 1011111 101111 101101 11 111101 1011011
101011 1101 111101011 10111111 11011 111011 1111 111
111111 110111111 10101 10111 101 110111 1111011 1101011
11011111 1011101 111010101 1010110111 110111011 1010110101 1011010111 1110110101
""".split()
assert len(_ALPHABET) == 128
VARICODE = [(int(w, 2), len(w)) for w in _ALPHABET]


def varicode_encode(byte):
    """varicode.rs:163-169"""
    return VARICODE[0] if byte >= 128 else VARICODE[byte]


def varicode_decode(bits, length):
    """varicode.rs:176-183"""
    for i, (cw, n) in enumerate(VARICODE):
        if n == length and cw == bits:
            return i
    return None


class VaricodeEncoder:
    """varicode.rs:192-267"""

    def __init__(self):
        self.pending = []
        self.first = True

    def push_preamble(self, n):
        self.pending += [0] * n
        self.first = True

    def push_byte(self, b):
        if not self.first:
            self.pending += [0, 0]
        self.first = False
        cw, n = varicode_encode(b)
        self.pending += [(cw >> i) & 1 for i in range(n - 1, -1, -1)]

    def push_postamble(self, n):
        if not self.first:
            self.pending += [0, 0]
        self.pending += [1] * n

    def drain_bits(self):
        out, self.pending = np.array(self.pending, np.uint8), []
        return out


class VaricodeDecoder:
    """varicode.rs:277-320; shift is a u16 and len stops at VARICODE_MAX_BITS + 1."""

    def __init__(self):
        self.shift, self.len, self.prev_zero, self.chars = 0, 0, False, []

    def push_bit(self, bit):
        is_zero = bit == 0
        if is_zero and self.prev_zero:
            cw = self.shift >> 1 if self.len > 0 else 0
            cw_len = max(self.len - 1, 0)
            if cw_len > 0:
                ch = varicode_decode(cw, cw_len)
                if ch is not None:
                    self.chars.append(ch)
            self.shift, self.len, self.prev_zero = 0, 0, False
        else:
            self.shift = ((self.shift << 1) | (bit & 1)) & 0xFFFF
            if self.len < VARICODE_MAX_BITS + 1:
                self.len += 1
            self.prev_zero = is_zero

    def pop_bytes(self):
        out, self.chars = bytes(self.chars), []
        return out


def text_bits(text, preamble, postamble):
    """The bit stream modulate_text builds (modulate/psk31.rs): preamble, bytes, postamble."""
    e = VaricodeEncoder()
    e.push_preamble(preamble)
    for b in text:
        e.push_byte(b)
    e.push_postamble(postamble)
    return e.drain_bits()


# ---- convolutional code (psk31.rs:29-160) ------------------------------------------------
def _parity(x):
    return bin(x).count("1") & 1


def conv_encode(bits):
    out, sr = [], 0
    for b in bits:
        b = int(b) & 1
        window = (b << 4) | sr
        out += [_parity(window & 0b10101), _parity(window & 0b10011)]
        sr = (sr >> 1) | (b << 3)
    return np.array(out, np.uint8)


DQPSK_EXP = [(F(1.0), F(0.0)), (F(0.0), F(-1.0)), (F(0.0), F(1.0)), (F(-1.0), F(0.0))]
INF = F(np.finfo(np.float32).max) / F(2.0)


def _acs(pm, s0, s1, prev_row):
    """psk31.rs:113-135 (= :296-316): prev_row keeps what it held where nothing wins."""
    new_pm = [INF] * 16
    for prev in range(16):
        pm_prev = pm[prev]
        if pm_prev >= INF:
            continue
        for bit in (0, 1):
            window = (bit << 4) | prev
            e0, e1 = DQPSK_EXP[_parity(window & 0b10101) * 2 + _parity(window & 0b10011)]
            bm = F(F(s0 - e0) * F(s0 - e0)) + F(F(s1 - e1) * F(s1 - e1))
            ns = (prev >> 1) | (bit << 3)
            cand = F(pm_prev + bm)
            if cand < new_pm[ns]:
                new_pm[ns] = cand
                prev_row[ns] = prev
    return new_pm


def _best(pm):
    """min_by(partial_cmp.unwrap_or(Equal)): the first of equal minima."""
    best = 0
    for i in range(1, 16):
        if pm[best] > pm[i]:
            best = i
    return best


def viterbi_decode(soft):
    soft = np.asarray(soft, np.float32)
    n = len(soft) // 2
    if n == 0:
        return np.zeros(0, np.uint8)
    pm = [INF] * 16
    pm[0] = F(0.0)
    table = [[0] * 16 for _ in range(n)]
    with np.errstate(all="ignore"):
        for t in range(n):
            pm = _acs(pm, soft[2 * t], soft[2 * t + 1], table[t])
    state = _best(pm)
    out = np.zeros(n, np.uint8)
    for t in range(n - 1, -1, -1):
        out[t] = (state >> 3) & 1
        state = table[t][state]
    return out


def viterbi_decode_hard(coded):
    soft = []
    for i in range(len(coded) // 2):
        soft += list(DQPSK_EXP[(int(coded[2 * i]) & 1) * 2 + (int(coded[2 * i + 1]) & 1)])
    return viterbi_decode(np.array(soft, np.float32))


class StreamingViterbi:
    """psk31.rs:257-377"""

    def __init__(self):
        self.pm = [INF] * 16
        self.pm[0] = F(0.0)
        self.history = [[0] * 16 for _ in range(PATHMEM)]
        self.ptr = 0
        self.count = 0

    def feed_symbol(self, s_re, s_im):
        self.pm = _acs(self.pm, F(s_re), F(s_im), self.history[self.ptr])
        if self.count % 256 == 255:
            finite = [v for v in self.pm if v < INF]
            min_pm = min(finite) if finite else INF
            if min_pm > 0:
                self.pm = [F(v - min_pm) if v < INF else v for v in self.pm]
        self.ptr = (self.ptr + 1) % PATHMEM
        self.count += 1
        if self.count <= TRACEBACK_DEPTH:
            return None
        state = _best(self.pm)
        p = (self.ptr + PATHMEM - 1) % PATHMEM
        for _ in range(TRACEBACK_DEPTH):
            state = self.history[p][state]
            p = (p + PATHMEM - 1) % PATHMEM
        return (state >> 3) & 1

    def feed(self, soft):
        out = []
        for i in range(len(soft) // 2):
            b = self.feed_symbol(soft[2 * i], soft[2 * i + 1])
            if b is not None:
                out.append(b)
        return np.array(out, np.uint8)

    def flush(self):
        return self.feed(np.zeros(2 * TRACEBACK_DEPTH, np.float32))


# ---- shared test inputs ------------------------------------------------------------------
def dqpsk_soft(bits, sigma, seed):
    """The differential symbols a clean QPSK31 demodulator gives for these data bits (the
    DQPSK_EXP phasor of each coded dibit) plus Gaussian noise of deviation sigma, float32."""
    coded = conv_encode(bits)
    soft = np.array([v for i in range(len(bits)) for v in DQPSK_EXP[coded[2 * i] * 2 + coded[2 * i + 1]]], np.float32)
    if sigma > 0:
        soft = (soft + np.random.default_rng(seed).normal(0.0, sigma, soft.shape)).astype(np.float32)
    return soft


VITERBI_LENGTHS = (1, 2, 5, 33, 300)
VITERBI_KINDS = ("clean", "noisy", "zero")
_cases = {}


def viterbi_case(n_syms, kind, k=0):
    """-> (soft float32 (2 n_syms,), the restatement's bits); computed once. kind: clean,
    noisy (sigma 0.5) or zero (all-zero input: every comparison ties). k: which of the seeded
    streams of this length and kind."""
    key = (n_syms, kind, k)
    if key not in _cases:
        bits = np.random.default_rng(1000 * n_syms + k).integers(0, 2, n_syms).astype(np.uint8)
        if kind == "zero":
            soft = np.zeros(2 * n_syms, np.float32)
        else:
            soft = dqpsk_soft(bits, 0.5 if kind == "noisy" else 0.0, 77 * n_syms + k)
        _cases[key] = (soft, viterbi_decode(soft))
    return _cases[key]


# ---- modulators and demodulators (src/modulate/psk31.rs, src/demodulate/psk31.rs) ---------
# f32 throughout; glibc's sinf / cosf and the exactly rounded fma come from np_ref.py, which
# already restates dsp/rotator.rs for the analog blocks.
from np_ref import PI, TAU, cosf, sinf, rotator  # noqa: E402



def _fma_v(a, b, c):
    """np_ref._fma for float32 vectors of any length (one stream included): a * b is exact in
    f64, s = fl64(a * b + c) with its TwoSum error e; rounding s to f32 is the fused result
    unless s lies exactly on an f32 midpoint with e != 0, where the sign of e decides."""
    p = a.astype(np.float64) * b.astype(np.float64)
    cc = c.astype(np.float64)
    s = p + cc
    bb = s - p
    e = (p - (s - bb)) + (cc - bb)
    r = s.astype(np.float32)
    rd = r.astype(np.float64)
    toward = np.nextafter(r, np.where(s > rd, F(np.inf), F(-np.inf)).astype(np.float32))
    tie = (e != 0.0) & (rd != s) & (s == (rd + toward.astype(np.float64)) * 0.5)
    if tie.any():
        r = np.where(tie & ((toward.astype(np.float64) - s) * e > 0), toward, r).astype(np.float32)
    return r


BPSK, QPSK = 0, 1
BAUD = F(31.25)
LOOP_GAIN = F(0.05)


def psk31_sps(fs):
    """modulate/psk31.rs:42-44 (round: half away from zero)."""
    q = F(F(fs) / BAUD)
    return int(np.floor(float(q) + 0.5)) if q >= 0 else 0


def make_hann(sps):
    """modulate/psk31.rs:53-67"""
    if sps == 1:
        return np.ones(1, np.float32)
    denom = F(sps - 1)
    return np.array([F(0.5) - F(0.5) * cosf(F(F(PI * F(i)) / denom)) for i in range(sps)], np.float32)


class Mod:
    """Bpsk31Mod / Qpsk31Mod (modulate/psk31.rs:110-216, :248-362)."""

    def __init__(self, mode, fs, rf_hz, gain):
        self.mode, self.fs, self.rf_hz, self.gain = mode, F(fs), F(rf_hz), F(gain)
        self.sps = psk31_sps(fs)
        self.hann = make_hann(self.sps)
        self.reset()

    def reset(self):
        self.cur = (F(1.0), F(0.0))
        self.sr = 0

    def modulate_bits(self, bits):
        out = np.zeros((len(bits) * self.sps, 2), np.float32)
        p0 = self.cur
        for k, b in enumerate(bits):
            b = int(b)
            if self.mode == BPSK:
                if b == 0:
                    self.cur = (F(-self.cur[0]), F(0.0))
            else:
                window = ((b & 1) << 4) | self.sr
                self.sr = (self.sr >> 1) | ((b & 1) << 3)
                st = DQPSK_EXP[_parity(window & 0b10101) * 2 + _parity(window & 0b10011)]
                c = self.cur
                self.cur = (F(F(c[0] * st[0]) - F(c[1] * st[1])), F(F(c[1] * st[0]) + F(c[0] * st[1])))
            dr, di = F(self.cur[0] - p0[0]), F(self.cur[1] - p0[1])
            seg = out[k * self.sps:(k + 1) * self.sps]
            seg[:, 0] = self.gain * (p0[0] + self.hann * dr)
            seg[:, 1] = self.gain * (p0[1] + self.hann * di)
            p0 = self.cur
        iq = out.view(np.complex64).reshape(-1)
        if self.rf_hz != 0:
            iq = rotator(iq, self.rf_hz, self.fs)
        return iq


def stream_record(mode, channel=0, rf_hz=0.0, gain=1.0, start=0, offset=0, out_cap=1 << 20):
    return dict(mode=mode, channel=channel, rf_hz=rf_hz, gain=gain, start=start, offset=offset, out_cap=out_cap)


class DemodBank:
    """Bpsk31Demod / Qpsk31Demod::process (demodulate/psk31.rs:151-219, :329-396) for a list of
    independent streams at once: the state of every stream is one numpy float32 vector, a step
    of the loop advances all streams still inside their loop by one sample (elementwise f32
    operations round exactly as the scalars would), and the symbol dump, where sinf / cosf are
    needed, is scalar. One stream is the reference's demodulator itself.

    perturb (a numpy Generator): every sine and cosine is moved one ulp in a random direction;
    the distance between the two runs' soft values is the tolerance scale of the device
    demodulator, whose sine and cosine differ from glibc's in rare near-ties."""

    def __init__(self, fs, records, perturb=None):
        self.rec = records
        self.sps = sps = psk31_sps(fs)
        self.hann = make_hann(sps)
        hsq = F(0.0)
        for h in self.hann:
            hsq = F(hsq + F(h * h))
        self.hsq = hsq
        S = len(records)
        self.mode = np.array([r["mode"] for r in records])
        self.ch = np.array([r["channel"] for r in records])
        self.start = np.array([r["start"] for r in records], np.int64)
        self.cap = np.array([r["out_cap"] for r in records], np.int64)
        self.gain = [F(r["gain"]) for r in records]
        self.rot = np.array([F(r["rf_hz"]) != 0 for r in records])
        w = []
        for r in records:
            phi = F(F(TAU * F(-F(r["rf_hz"]))) / F(fs))
            w.append((cosf(phi), sinf(phi)))
        self.w_re = np.array([a for a, _ in w], np.float32)
        self.w_im = np.array([b for _, b in w], np.float32)
        self.offset = [r["offset"] for r in records]
        self.perturb = perturb
        self.S = S
        self.reset()

    def reset(self):
        S, sps = self.S, self.sps
        self.count = np.array([0 if o % sps == 0 else sps - o % sps for o in self.offset], np.int64)
        self.ctr = np.zeros(S, np.int64)
        self.acc_re, self.acc_im = np.zeros(S, np.float32), np.zeros(S, np.float32)
        self.prev_re, self.prev_im = np.ones(S, np.float32), np.zeros(S, np.float32)
        self.pa = np.zeros(S, np.float32)
        self.z_re, self.z_im = np.ones(S, np.float32), np.zeros(S, np.float32)
        self.base = 0

    def _sincos(self, x):
        s, c = sinf(x), cosf(x)
        if self.perturb is not None:
            s = np.nextafter(s, F(np.inf) if self.perturb.integers(2) else F(-np.inf))
            c = np.nextafter(c, F(np.inf) if self.perturb.integers(2) else F(-np.inf))
        return s, c

    def _dump(self, k, outs):
        scale = F(self.gain[k] / self.hsq)
        sr, si = F(self.acc_re[k] * scale), F(self.acc_im[k] * scale)
        self.acc_re[k] = self.acc_im[k] = 0.0
        self.count[k] = 0
        sin_pa, cos_pa = self._sincos(self.pa[k])
        pr, pi = self.prev_re[k], self.prev_im[k]
        sym_re = F(F(sr * cos_pa) + F(si * sin_pa))
        sym_im = F(F(si * cos_pa) - F(sr * sin_pa))
        d_re = F(F(sym_re * pr) + F(sym_im * pi))
        d_im = F(F(sym_im * pr) - F(sym_re * pi))
        if self.mode[k] == BPSK:
            outs[k].append(d_re)
            dec_re = F(1.0) if d_re >= 0 else F(-1.0)
            cross_im = F(d_im * dec_re)
        else:
            outs[k] += [d_re, d_im]
            if abs(d_re) >= abs(d_im):
                dec_re, dec_im = (F(1.0) if d_re >= 0 else F(-1.0)), F(0.0)
            else:
                dec_re, dec_im = F(0.0), (F(1.0) if d_im >= 0 else F(-1.0))
            cross_im = F(F(d_im * dec_re) - F(d_re * dec_im))
        mag_sq = F(F(d_re * d_re) + F(d_im * d_im))
        phase_err = F(cross_im / np.sqrt(mag_sq)) if mag_sq > F(1e-6) else F(0.0)
        pa = F(self.pa[k] + F(LOOP_GAIN * phase_err))
        if pa > PI:
            pa = F(pa - TAU)
        if pa < -PI:
            pa = F(pa + TAU)
        self.pa[k] = pa
        self.prev_re[k], self.prev_im[k] = sym_re, sym_im

    def process(self, x):
        """x complex64 (nch, n): the channels' next n samples. -> (soft: a float32 array per
        stream, in_read and out_written per stream)."""
        x = np.asarray(x, np.complex64)
        n = x.shape[1]
        xr_all, xi_all = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
        i = np.clip(self.start - self.base, 0, n)
        first = i.copy()
        need = np.where(self.mode == QPSK, 2, 1)
        outs = [[] for _ in range(self.S)]
        out_pos = np.zeros(self.S, np.int64)
        one = F(1.0)
        with np.errstate(all="ignore"):
            while True:
                a = (i < n) & (out_pos + need <= self.cap)
                if not a.any():
                    break
                idx = np.where(a, i, 0)
                xr, xi = xr_all[self.ch, idx], xi_all[self.ch, idx]
                m = a & self.rot
                if m.any():
                    zr = _fma_v(self.z_re, self.w_re, -(self.z_im * self.w_im))
                    zi = _fma_v(self.z_im, self.w_re, self.z_re * self.w_im)
                    self.z_re, self.z_im = np.where(m, zr, self.z_re), np.where(m, zi, self.z_im)
                    self.ctr = np.where(m, self.ctr + 1, self.ctr)
                    rn = m & ((self.ctr & 0x3FF) == 0)
                    if rn.any():
                        inv = one / np.sqrt(self.z_re * self.z_re + self.z_im * self.z_im)
                        self.z_re = np.where(rn, self.z_re * inv, self.z_re)
                        self.z_im = np.where(rn, self.z_im * inv, self.z_im)
                    re = xr * self.z_re - xi * self.z_im
                    im = xi * self.z_re + xr * self.z_im
                    xr, xi = np.where(m, re, xr), np.where(m, im, xi)
                h = self.hann[self.count]
                omh = one - h
                self.acc_re = np.where(a, self.acc_re + h * (xr - self.prev_re * omh), self.acc_re)
                self.acc_im = np.where(a, self.acc_im + h * (xi - self.prev_im * omh), self.acc_im)
                self.count = np.where(a, self.count + 1, self.count)
                i = np.where(a, i + 1, i)
                for k in np.flatnonzero(a & (self.count == self.sps)):
                    self._dump(k, outs)
                    out_pos[k] = len(outs[k])
        self.base += n
        return [np.array(o, np.float32) for o in outs], i - first, out_pos


# ---- carrier search (src/sync/psk31_sync.rs:82-203, :242-253) and Psk31Stream ----------------
LN_2 = F(0.6931471805599453)


def median_f32(v):
    v = np.sort(np.asarray(v, np.float32))
    if v.size == 0:
        return F(0.0)
    mid = v.size // 2
    return F(F(v[mid - 1] + v[mid]) * F(0.5)) if v.size % 2 == 0 else v[mid]


def find_carriers(wf, min_carrier_syms, peak_margin_db, max_cand):
    """-> [(time_sym, freq_bin, score)], score descending, equal scores by freq_bin then
    time_sym. Stated per symbol as masks over the whole waterfall, then runs are read off each
    bin's mask; the run sum is added symbol by symbol in f32."""
    wf = np.asarray(wf, np.float32)
    num_syms, num_bins = wf.shape
    ln_margin = F(F(F(peak_margin_db) * LN_2) / F(3.0))
    min_run = max(int(min_carrier_syms), 1)
    med = np.array([median_f32(wf[:, b]) for b in range(num_bins)], np.float32)
    glob = F(median_f32(med) + ln_margin)
    pad = np.full((num_syms, 1), -np.inf, np.float32)
    left = np.concatenate([pad, wf[:, :-1]], axis=1)
    right = np.concatenate([wf[:, 1:], pad], axis=1)
    peak = ((wf > (med + ln_margin)[None, :]) | (med > glob)[None, :]) & (wf >= left) & (wf >= right)
    runs = []
    for b in range(num_bins):
        col = np.concatenate([[False], peak[:, b], [False]])
        edges = np.flatnonzero(col[1:] != col[:-1])
        for a, e in zip(edges[::2], edges[1::2]):
            if e - a >= min_run:
                total = F(0.0)
                for v in wf[a:e, b]:
                    total = F(total + v)
                runs.append((int(a), b, F(total / F(e - a))))
    runs.sort(key=lambda r: -float(r[2]) if r[2] == r[2] else 0.0)  # stable: ties keep (bin, time) order
    return runs[:max_cand]


class Psk31Stream:
    """codec/psk31.rs:416-572 over the restated demodulator, decoder and Varicode."""

    def __init__(self, mode, fs, carrier_hz, gain=1.0):
        self.qpsk = mode == "qpsk"
        self.bank = DemodBank(fs, [stream_record(QPSK if self.qpsk else BPSK, 0, carrier_hz, gain)])
        self.vit = StreamingViterbi()
        self.vdec = VaricodeDecoder()

    def _text(self, bits):
        for b in bits:
            self.vdec.push_bit(int(b))
        return "".join(chr(c) for c in self.vdec.pop_bytes() if 0x20 <= c < 0x7F)

    def feed(self, iq):
        if len(iq) == 0:
            return ""
        soft = self.bank.process(np.asarray(iq, np.complex64)[None, :])[0][0]
        if not self.qpsk:
            return self._text(soft >= 0)
        bits = []
        for i in range(len(soft) // 2):
            d_re, d_im = soft[2 * i], soft[2 * i + 1]
            if F(F(d_re * d_re) + F(d_im * d_im)) < F(0.01):
                continue
            b = self.vit.feed_symbol(d_re, d_im)
            if b is not None:
                bits.append(b)
        return self._text(bits)

    def flush(self):
        text = self._text(self.vit.flush()) if self.qpsk else ""
        return text + self._text([0, 0])
