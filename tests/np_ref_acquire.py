"""An independent numpy restatement of the reference's OFDM burst acquisition and burst receiver
(test infrastructure): ofdm_sync, earliest_accepted, estimate_integer_cfo_bins and
correlate_segment (src/sync/ofdm_sync.rs:354-589); the equalizer branch of soft_demap,
remove_common_phase_error, decode_frame_body with a channel estimate, try_one_frame,
estimate_channel and the stream demodulator's feed / flush / drain
(src/demodulate/ofdm_frame.rs:55-274, :862-1090, :1280-1592). Written from those files over
np_ref_ofdm and np_ref_frame (preamble, training pattern, transform, LLRs, coding chain), not
from csrc/acquire.cpp.

Every function takes dtype. np.float32 is the reference operation for operation (the Schmidl &
Cox sums are vectorised over the candidate offsets and stay sequential over the samples of a
segment and over the segments: the same f32 operations in the same order; numpy contracts
nothing). np.float64 is the same algorithm in double precision, the accuracy yardstick of the
device tests; there the hard decisions inside the phase tracker are taken on the symbols rounded
to float32, everything else is complex128.

A preamble is (num_repeats, repeat_len, training) with training None or (n_fft, cp_len); a sync
result is the tuple (start_sample, cfo_hz, integer_cfo_bins, score)."""
import ctypes
import math

import numpy as np

import np_ref_frame as RFm
import np_ref_ofdm as RO
from np_ref import _fma, cosf, sinf

F = np.float32
D = np.float64
_libm = ctypes.CDLL("libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
TOP_N = 5
CPE_MIN_SYMBOLS, ALPHA, BETA = 4, 0.5, 0.05
RX = {"malformed_header": 2, "header_crc_mismatch": 3, "crc_mismatch": 4}


def _atan2(y, x, dt):
    return F(_libm.atan2f(float(y), float(x))) if dt is F else D(math.atan2(float(y), float(x)))


def _sincos(x, dt):
    return (sinf(x), cosf(x)) if dt is F else (D(math.sin(float(x))), D(math.cos(float(x))))


def _tau(dt):
    return RO.TAU if dt is F else D(2.0 * math.pi)


def _parts(x, dt):
    x = np.asarray(x)
    return x.real.astype(dt), x.imag.astype(dt)


def _cplx(re, im, dt):
    if dt is F:
        return RO.cplx(re, im)
    out = np.empty(np.broadcast(re, im).shape, np.complex128)
    out.real, out.imag = re, im
    return out


def total_len(pre):
    num, rl, tr = pre
    return num * rl + (sum(tr) if tr else 0)


# ---- sync/ofdm_sync.rs ----------------------------------------------------------------------
def sc_sums(iq, pre, start, end, dtype=F):
    """p (complex) and r per offset of [start, end): correlate_segment per adjacent pair, each
    from zero, added to p and r in segment order."""
    num, rl, _ = pre
    re, im = _parts(iq, dtype)
    d = np.arange(start, end)
    pr, pi, rr = (np.zeros(len(d), dtype) for _ in range(3))
    for seg in range(num - 1):
        sr, si, se = (np.zeros(len(d), dtype) for _ in range(3))
        for i in range(rl):
            a = d + seg * rl + i
            b = a + rl
            ar, ai, br, bi = re[a], -im[a], re[b], im[b]  # conj(a) * b, num-complex's product
            sr = sr + (ar * br - ai * bi)
            si = si + (ar * bi + ai * br)
            se = se + (br * br + bi * bi)
        pr, pi, rr = pr + sr, pi + si, rr + se
    return _cplx(pr, pi, dtype), rr


def search_end(n, pre, end):
    return min(end, max(n - total_len(pre), 0))


def ofdm_sync(iq, fs, pre, search_start, search_end_, dtype=F, detail=False):
    """The ranked results; with detail also (p, r, kept, r_peak) over the offsets of the range."""
    num, rl, tr = pre
    empty = ([], None) if detail else []
    if rl == 0 or num < 2 or fs <= 0:
        return empty
    end = search_end(len(iq), pre, search_end_)
    if search_start >= end:
        return empty
    p, r = sc_sums(iq, pre, search_start, end, dtype)
    kept = ~(r <= 0)
    den = dtype(dtype(_tau(dtype) * dtype(rl)) / dtype(fs))
    r_peak, rows = dtype(0), []
    for k in np.flatnonzero(kept):
        r_peak = max(r_peak, r[k])
        with np.errstate(all="ignore"):
            score = dtype((p[k].real * p[k].real + p[k].imag * p[k].imag) / (r[k] * r[k]))
        score = min(max(score, dtype(0)), dtype(1))
        rows.append((r[k], search_start + int(k), dtype(_atan2(p[k].imag, p[k].real, dtype) / den), score))
    if not rows or r_peak <= 0:
        return empty
    key = np.array([dtype(sc * dtype(rk / r_peak)) for rk, _, _, sc in rows], dtype)
    order = np.argsort(-key, kind="stable")
    out = [(rows[j][1], rows[j][2], 0, rows[j][3]) for j in order]
    if tr:
        for j in range(min(TOP_N, len(out))):
            s, cfo, _, sc = out[j]
            out[j] = (s, cfo, integer_cfo_bins(iq, fs, tr, s + num * rl, cfo, dtype), sc)
    return (out, (p, r, kept, r_peak)) if detail else out


def earliest_accepted(results, threshold, cluster_len):
    acc = [r for r in results if r[3] >= threshold]
    if not acc:
        return None
    first = min(r[0] for r in acc)
    for r in acc:
        if r[0] - first < max(cluster_len, 1):
            return r
    return None


def rotator(freq_hz, fs, n, dtype=F):
    """Rotator::new(freq_hz, fs).next() n times (dsp/rotator.rs:16-61)."""
    if dtype is F:
        return RO.rotator(freq_hz, fs, n)
    phi = D(D(_tau(D) * D(freq_hz)) / D(fs))
    return np.exp(1j * phi * np.arange(1, n + 1))


def rotate_block(x, freq_hz, fs, dtype=F):
    """Rotator::rotate_block (dsp/rotator.rs:74-84) from a fresh oscillator."""
    p = rotator(freq_hz, fs, len(x), dtype)
    if dtype is D:
        return np.asarray(x, np.complex128) * p
    a, b = _parts(x, F)
    pr, pi = _parts(p, F)
    return RO.cplx(_fma(a, pr, -(b * pi)), _fma(b, pr, a * pi))


def _fft(x, dtype):
    return RO.fft_radix2(x) if dtype is F else np.fft.fft(np.asarray(x, np.complex128), axis=-1)


def integer_cfo_bins(iq, fs, training, training_start, frac_hz, dtype=F, corr=False):
    n_fft, cp = training
    total = n_fft + cp
    if training_start + total > len(iq):
        return (0, None) if corr else 0
    cor = rotate_block(np.asarray(iq)[training_start:training_start + total], -frac_hz, fs, dtype)
    fr, fi = _parts(_fft(cor[None, cp:cp + n_fft], dtype)[0], dtype)
    kr, ki = _parts(RO.training_pattern(n_fft), dtype)
    ki = -ki  # conj(known) * freq, num-complex's product
    shifts = np.arange(-(n_fft // 2), n_fft // 2 + 1)
    cr, ci = np.zeros(len(shifts), dtype), np.zeros(len(shifts), dtype)
    for b in range(n_fft):
        src = (b + shifts) % n_fft
        cr = cr + (kr[b] * fr[src] - ki[b] * fi[src])
        ci = ci + (kr[b] * fi[src] + ki[b] * fr[src])
    mag = cr * cr + ci * ci
    best, best_shift = dtype(-1), 0
    for s, m in zip(shifts, mag):
        if m > best:
            best, best_shift = m, int(s)
    return (best_shift, mag) if corr else best_shift


# ---- demodulate/ofdm_frame.rs: the equalized body -------------------------------------------
def _cmul(a, b, dtype):
    return RO.cmul(a, b) if dtype is F else np.asarray(a, np.complex128) * np.asarray(b, np.complex128)


def estimate_channel(link, corrected, dtype=F):
    """The training symbol's transform at the data window, or None without a training symbol."""
    if not link.training:
        return None
    n_fft, cp = link.training
    start = link.preamble[0] * link.preamble[1]
    if len(corrected) < start + n_fft + cp:
        return None
    w0 = cp - min(getattr(link, "backoff", 0), cp)
    return _fft(np.asarray(corrected)[None, start + w0:start + w0 + n_fft], dtype)[0]


def equalizer_weights(est, dtype=F):
    """estimate_from_training_symbol -> equalizer_weight (demodulate/ofdm.rs:440-502)."""
    pat = RO.training_pattern(len(est))
    if dtype is F:
        return RO.equalizer_weight(RO.cdiv(est, pat))
    h = np.asarray(est, np.complex128) / pat.astype(np.complex128)
    m = h.real * h.real + h.imag * h.imag
    with np.errstate(all="ignore"):
        return np.where(m >= D(RO.EQUALIZER_FLOOR), np.conj(h) / m, 0)


def equalized_symbols(link, order, iq, n_sym, weight, dtype=F):
    """(n_sym, n_data): SymbolFft -> weight -> the data bins, before the phase tracker."""
    cfg = link.symcfg(order)
    w0 = link.cp_len - min(getattr(link, "backoff", 0), link.cp_len)
    x = np.asarray(iq)[:n_sym * link.sps].reshape(n_sym, link.sps)[:, w0:w0 + link.n_fft]
    f = _fft(x, dtype)
    return _cmul(f, weight[None, :], dtype)[:, cfg.data_bins]


def remove_common_phase_error(order, syms, dtype=F):
    """remove_common_phase_error (demodulate/ofdm_frame.rs:200-274) over (n_sym, n_data)."""
    syms = np.array(syms, np.complex64 if dtype is F else np.complex128)
    n_sym, n_data = syms.shape
    if n_sym < CPE_MIN_SYMBOLS or n_data == 0:
        return syms
    al, be = dtype(ALPHA), dtype(BETA)
    measured = np.zeros(n_sym, dtype)
    phase, freq = dtype(0), dtype(0)
    for k in range(n_sym):
        s, c = _sincos(-phase, dtype)
        rot = _cmul(syms[k], _cplx(c, s, dtype), dtype)
        llr = RO.soft_llr(order, rot.astype(np.complex64))
        ideal = RO.map_bits(order, (llr <= 0).astype(np.uint8))
        yr, yi = _parts(rot, dtype)
        ir, ii = _parts(ideal, dtype)
        ii = -ii  # y * conj(ideal), num-complex's product
        ar = np.cumsum(yr * ir - yi * ii, dtype=dtype)[-1]  # sequential, in carrier order
        ai = np.cumsum(yr * ii + yi * ir, dtype=dtype)[-1]
        err = dtype(0) if (ar == 0 and ai == 0) else _atan2(ai, ar, dtype)
        measured[k] = phase + err
        phase = dtype(phase + dtype(freq + dtype(al * err)))
        freq = dtype(freq + dtype(be * err))
    n = dtype(n_sym)
    sum_k = dtype(dtype(n * dtype(n - dtype(1))) / dtype(2))
    sum_k2 = dtype(dtype(dtype(dtype(n - dtype(1)) * n) * dtype(dtype(dtype(2) * n) - dtype(1))) / dtype(6))
    sum_y, sum_ky = dtype(0), dtype(0)
    for k in range(n_sym):
        sum_y = dtype(sum_y + measured[k])
        sum_ky = dtype(sum_ky + dtype(dtype(k) * measured[k]))
    denom = dtype(dtype(n * sum_k2) - dtype(sum_k * sum_k))
    if abs(denom) <= np.finfo(F).eps:
        return syms
    slope = dtype(dtype(dtype(n * sum_ky) - dtype(sum_k * sum_y)) / denom)
    intercept = dtype(dtype(sum_y - dtype(slope * sum_k)) / n)
    out = syms.copy()
    for k in range(n_sym):
        s, c = _sincos(-dtype(intercept + dtype(slope * dtype(k))), dtype)
        out[k] = _cmul(syms[k], _cplx(c, s, dtype), dtype)
    return out


def soft_demap_eq(link, order, iq, n_sym, weight, dtype=F):
    """(llrs, symbols after the phase tracker) or None when iq is short of n_sym symbols."""
    if len(iq) < n_sym * link.sps:
        return None
    syms = remove_common_phase_error(order, equalized_symbols(link, order, iq, n_sym, weight, dtype), dtype)
    return RO.soft_llr(order, syms.reshape(-1).astype(np.complex64)), syms


def decode_frame_body(link, body, est, dtype=F):
    """decode_frame_body (demodulate/ofdm_frame.rs:862-1090): "incomplete", an RxError code, or a
    dict (mcs_index, sequence_num, flags, payload, consumed, inner_ok, outer_ok, crc_ok, symbols).
    est None is the flat path of the known-start demodulator."""
    weight = None if est is None else equalizer_weights(est, dtype)

    def demap(order, iq, n_sym):
        if weight is None:
            llr = RFm.soft_demap(link, order, iq, n_sym)
            return None if llr is None else (llr, None)
        return soft_demap_eq(link, order, iq, n_sym, weight, dtype)

    hs = link.header_scheme()
    hplan = RFm.block_plan(RFm.HEADER_FIELD_BYTES, hs)
    nh = link.symbols("bpsk", hplan[5])
    got = demap("bpsk", body, nh)
    if got is None:
        return "incomplete"
    h = RFm.decode_chain(got[0], hplan, hs, 0, "sum_product")
    if isinstance(h, int):
        return h
    if not h["valid"]:
        return RX["header_crc_mismatch"]
    b = bytes(h["bytes"])
    mcs_index, plen, seq, flags, seed = b[0], int.from_bytes(b[1:5], "big"), int.from_bytes(b[5:9], "big"), b[9], \
        int.from_bytes(b[10:14], "big")
    if mcs_index >= len(link.mcs):
        return RX["malformed_header"]
    m = link.mcs[mcs_index]
    ps = link.payload_scheme(m)
    plan = RFm.block_plan(plen, ps)
    n_sym = link.symbols(m[0], plan[5])
    got = demap(m[0], body[nh * link.sps:], n_sym)
    if got is None:
        return "incomplete"
    out = RFm.decode_chain(got[0], plan, ps, seed, link.frame["ldpc_decode_rule"])
    if isinstance(out, int):
        return out
    if not out["valid"]:
        return RX["crc_mismatch"]
    return dict(mcs_index=mcs_index, sequence_num=seq, flags=flags, payload=out["bytes"][:plen],
                consumed=(nh + n_sym) * link.sps, inner_ok=out["inner_ok"], outer_ok=out["outer_ok"], crc_ok=out["crc_ok"],
                symbols=got[1])


def receive(link, iq, fs=1e6, threshold=0.5, dtype=F):
    """try_one_frame (demodulate/ofdm_frame.rs:1463-1571): None for "need more", else a dict with
    error (0 or the RxError code), consume_to, start_sample, cfo_hz, sync_score and, decoded,
    decode_frame_body's fields."""
    iq = np.asarray(iq, np.complex64)
    pre = (link.preamble[0], link.preamble[1], link.training)
    pre_len = total_len(pre)
    if len(iq) < pre_len + link.n_fft + link.cp_len:
        return None
    best = earliest_accepted(ofdm_sync(iq, fs, pre, 0, len(iq), dtype), threshold, pre_len)
    if best is None:
        return None
    start, cfo, bins, score = best
    total = dtype(cfo + dtype(dtype(bins) * dtype(dtype(fs) / dtype(link.n_fft))))
    corrected = rotate_block(iq[start:], -total, fs, dtype)
    est = estimate_channel(link, corrected, dtype)
    if len(corrected) < pre_len:
        return None
    body = decode_frame_body(link, corrected[pre_len:], est, dtype)
    if isinstance(body, str):
        return None
    step = dict(start_sample=start, cfo_hz=total, sync_score=score)
    if isinstance(body, int):
        step.update(error=body, consume_to=min(start + pre_len, len(iq)))
        return step
    consume_to = start + pre_len + body.pop("consumed")
    if consume_to > len(iq):
        return None
    step.update(body, error=0, consume_to=consume_to)
    return step


class StreamDemod:
    """OfdmFrameStreamDemod's buffer and drain loop (demodulate/ofdm_frame.rs:1395-1460)."""

    def __init__(self, link, fs=1e6, threshold=0.5):
        self.link, self.fs, self.threshold, self.buf = link, fs, threshold, np.zeros(0, np.complex64)

    def feed(self, iq):
        self.buf = np.concatenate([self.buf, np.asarray(iq, np.complex64)])
        return self.flush()

    def flush(self):
        out = []
        while True:
            step = receive(self.link, self.buf, self.fs, self.threshold)
            if step is None:
                return out
            self.buf = self.buf[step["consume_to"]:]
            out.append(step)


# ---- the captures the CPU and GPU acquisition tests share -------------------------------------
SIGMA = 0.004  # per part: the level at which every decisive case decodes on the restatement alone
OFFSETS = ((5, -28300.0, 2.0), (101, 2300.0, 1.0), (200, 42875.0, 0.5))  # (start, carrier offset Hz, phase rad)


def impair(frame, offset, cfo_hz, phase, sigma, seed, total=None, fs=1e6, amp=1.0):
    """frame at offset inside a capture of total samples (default: 50 past the frame), turned by
    a carrier offset and phase (in double precision, rounded once), then AWGN of sigma per part
    over the whole capture from a seeded generator."""
    frame = np.asarray(frame, np.complex64)
    total = offset + len(frame) + 50 if total is None else total
    k = np.arange(len(frame))
    turned = frame.astype(np.complex128) * (amp * np.exp(1j * (2.0 * np.pi * cfo_hz * k / fs + phase)))
    x = np.zeros(total, np.complex128)
    m = min(len(frame), total - offset)
    x[offset:offset + m] = turned[:m]
    rng = np.random.default_rng(seed)
    noise = (rng.standard_normal(total) + 1j * rng.standard_normal(total)) * sigma
    return (x + noise).astype(np.complex64)


def two_frame_capture(frame_a, frame_b, fs=1e6):
    """Two frames in one capture, both at +17000 Hz: the first at 50, the second, at twice the
    amplitude, 120 samples after the first ends. The second frame's plateau outranks the first's,
    so the earliest accepted candidate (50) is not among the five the integer search visits."""
    gap = 120
    total = 50 + len(frame_a) + gap + len(frame_b) + 60
    x = impair(frame_a, 50, 17000.0, 0.7, 0.0, 0, total=total, fs=fs).astype(np.complex128)
    x += impair(frame_b, 50 + len(frame_a) + gap, 17000.0, 1.9, 0.0, 0, total=total, fs=fs, amp=2.0)
    rng = np.random.default_rng(77)
    return (x + (rng.standard_normal(total) + 1j * rng.standard_normal(total)) * SIGMA).astype(np.complex64)


def receive_cases(frame_of, total, pre_len, sps):
    """The captures of the receive tests, each of total samples: name -> (capture, what it holds).
    frame_of(mcs_index, sequence_num, payload, longer_table=False) gives a frame's IQ.
    decisive: MCS entries 0-2 of the default table with 4 and 40 payload bytes at OFFSETS in turn
    (what: (mcs_index, sequence_num, payload, offset)); structural: noise alone, a frame that
    runs past the capture's end inside its payload, a frame with one header symbol turned over
    and one erased, a frame modulated under a longer table than the receiver's."""
    cases = {}
    k = 0
    for mi in range(3):
        for nbytes in (4, 40):
            off, cfo, ph = OFFSETS[k % 3]
            data = RFm.payload(nbytes, 40 + k)
            cases[f"mcs{mi}_{nbytes}"] = (impair(frame_of(mi, k, data), off, cfo, ph, SIGMA, 500 + k, total=total),
                                          (mi, k, data, off))
            k += 1
    cases["noise"] = (impair(np.zeros(0, np.complex64), 0, 0.0, 0.0, SIGMA, 600, total=total), None)
    f = frame_of(1, 9, RFm.payload(40, 90))
    cases["cut"] = (impair(f, total - len(f) + 150, -5100.0, 0.2, SIGMA, 601, total=total), None)
    bad = np.array(frame_of(1, 10, RFm.payload(40, 91)))
    bad[pre_len + sps:pre_len + 2 * sps] = -bad[pre_len + sps:pre_len + 2 * sps]
    bad[pre_len + 2 * sps:pre_len + 3 * sps] = 0
    cases["header"] = (impair(bad, 33, 12000.0, 2.9, SIGMA, 602, total=total), 33)
    cases["longer"] = (impair(frame_of(4, 11, RFm.payload(40, 92), True), 60, 8000.0, 1.1, SIGMA, 603, total=total), None)
    return cases


# ---- exact-arithmetic captures: every Schmidl & Cox product and partial sum an integer ---------
def int_pattern():
    """32 Gaussian integers with parts in -3..3, the repeat of the crafted captures."""
    rng = np.random.default_rng(3)
    return (rng.integers(-3, 4, 32) + 1j * rng.integers(-3, 4, 32)).astype(np.complex64)


def int_noise(n, seed):
    """n Gaussian integers with parts in -9..9 from a seeded generator: no structure, no ties to speak of."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-9, 10, n) + 1j * rng.integers(-9, 10, n)).astype(np.complex64)


def _z(n):
    return np.zeros(n, np.complex64)


def sc_sums_exact(iq, pre, start, end):
    """(p_re, p_im, r, bound) in int64 per offset of [start, end) for a capture of Gaussian
    integers, by differences of running sums (not sc_sums' walk). bound is the energy of the
    whole window of an offset, which no partial sum of p or r exceeds in magnitude; below 2^24
    every f32 product and partial sum of the walk is exact, in any order."""
    num, rl, _ = pre
    iq = np.asarray(iq)
    re, im = np.rint(iq.real).astype(np.int64), np.rint(iq.imag).astype(np.int64)
    assert np.array_equal(re, iq.real) and np.array_equal(im, iq.imag), "integer parts only"
    span = (num - 1) * rl

    def run(v):
        return np.concatenate([[0], np.cumsum(v, dtype=np.int64)])

    a_re, a_im, b_re, b_im = re[:-rl], im[:-rl], re[rl:], im[rl:]
    pr, pi, en = run(a_re * b_re + a_im * b_im), run(a_re * b_im - a_im * b_re), run(re * re + im * im)
    d = np.arange(start, end)
    return pr[d + span] - pr[d], pi[d + span] - pi[d], en[d + rl + span] - en[d + rl], int((en[d + rl + span] - en[d]).max())


def plateau_capture():
    """Silence, ten repeats of the pattern, twelve at twice the amplitude, silence: 814 samples."""
    pat = int_pattern()
    return np.concatenate([_z(70), np.tile(pat, 10), np.tile(2 * pat, 12), _z(40)]).astype(np.complex64)


def threshold_capture():
    """The pattern, then the pattern doubled, at 40: the score there is exactly 1/4."""
    pat = int_pattern()
    return np.concatenate([_z(40), pat, 2 * pat, _z(300)]).astype(np.complex64)


def cluster_capture(gap, total=700):
    """The quarter-score pair at 40 and a full-score pair (3 pat | 3 pat) at 40 + gap."""
    pat = int_pattern()
    x = _z(total)
    x[40:104] = np.concatenate([pat, 2 * pat])
    x[40 + gap:40 + gap + 64] = np.concatenate([3 * pat, 3 * pat])
    return x


def one_sample_capture():
    """One non-zero sample in 300: under the preamble (2, 2) exactly two offsets hold energy."""
    x = _z(300)
    x[100] = 3 - 2j
    return x


def half_band(x):
    """x times (-1)^n, exact in f32: a carrier offset of half the sample rate."""
    s = np.where(np.arange(len(x)) % 2 == 0, np.float32(1), np.float32(-1))
    out = np.empty(len(x), np.complex64)
    out.real, out.imag = np.asarray(x).real * s, np.asarray(x).imag * s
    return out


def crafted_cases():
    """name -> (preamble, capture, score threshold, the facts the capture was built for). The
    facts are asserted on the restatement (crafted_facts) before anything is held to them."""
    p, pt, p2 = (2, 32, None), (2, 32, (64, 8)), (2, 2, None)
    above = float(np.nextafter(F(0.25), F(1)))
    return {
        # the top five are the first offsets wholly inside the louder plateau; 390 .. 710 tie at key 1, so the
        # winners (lanes 134 .. 138 of a 256-wide sweep) tie with offsets in lower lanes, 512 and up
        "plateau": (p, plateau_capture(), 0.5, dict(nd=750, kept=735, top=[390, 391, 392, 393, 394], top_keys=[1.0] * 5,
                                                    accepted=70, accepted_rank=374, tied_at_best=321)),
        "threshold_met": (p, threshold_capture(), 0.25, dict(accepted=40, accepted_score=0.25)),
        "threshold_missed": (p, threshold_capture(), above, dict(accepted=None, score_at={40: 0.25})),
        # the second burst starts 135 / 136 past the earliest accepted offset (40), the cluster is 136 long
        "cluster_inside": (pt, cluster_capture(135), 0.25, dict(accepted=175, accepted_score=1.0, score_at={40: 0.25})),
        "cluster_edge": (pt, cluster_capture(136), 0.25, dict(accepted=175, score_at={40: 0.25, 176: 1.0}, top=[176, 177, 178, 179, 180])),
        "two_kept": (p2, one_sample_capture(), 0.5, dict(kept=2, top=[97, 98, -1, -1, -1], accepted=None, r_peak=13.0,
                                                        score_at={97: 0.0, 98: 0.0})),
        "two_kept_threshold_0": (p2, one_sample_capture(), 0.0, dict(kept=2, accepted=97, accepted_score=0.0)),
        "all_zero": (p2, _z(300), 0.5, dict(kept=0, top=[-1] * 5, accepted=None, r_peak=0.0)),
    }


def crafted_facts(x, pre, thr, start=0, end=None, fs=1e6):
    """What the restatement alone says of capture x: nd, kept, r_peak, top (five starts, -1
    padded), top_keys, tied_at_best (how many offsets share the best key), accepted (start or
    None), accepted_score, accepted_rank, score_at (start -> score)."""
    end = len(x) if end is None else end
    res, det = ofdm_sync(x, fs, pre, start, end, detail=True)
    nd = search_end(len(x), pre, end) - start
    if det is None:
        return dict(nd=nd, kept=0, r_peak=0.0, top=[-1] * TOP_N, top_keys=[], tied_at_best=0, accepted=None,
                    accepted_score=None, accepted_rank=None, score_at={})
    _, r, kept, r_peak = det
    score = {q[0]: float(q[3]) for q in res}
    keys = [float(F(q[3] * F(r[q[0] - start] / r_peak))) for q in res]
    best = earliest_accepted(res, thr, total_len(pre))
    starts = [q[0] for q in res]
    return dict(nd=nd, kept=int(kept.sum()), r_peak=float(r_peak), top=starts[:TOP_N] + [-1] * (TOP_N - min(TOP_N, len(res))),
                top_keys=keys[:TOP_N], tied_at_best=keys.count(keys[0]), accepted=None if best is None else best[0],
                accepted_score=None if best is None else float(best[3]),
                accepted_rank=None if best is None else starts.index(best[0]), score_at=score)


# All ones, 900 samples, preamble (2, 32): (search_start, search_end, nd). 836 offsets exist.
ONES_RANGES = ((10, 11, 1), (0, 4, 4), (831, 2000, 5), (0, 6, 6), (3, 258, 255), (0, 256, 256), (7, 264, 257), (0, 513, 513))


def ones_facts(start, nd):
    """Every offset has p = r = 32, score 1 and key 1: the ranking is the offsets in order."""
    top = list(range(start, start + min(nd, TOP_N))) + [-1] * (TOP_N - min(nd, TOP_N))
    return dict(nd=nd, kept=nd, r_peak=32.0, top=top, top_keys=[1.0] * min(nd, TOP_N), tied_at_best=nd, accepted=start,
                accepted_score=1.0, accepted_rank=0)


# Preambles (num_repeats, repeat_len) for the metric's walk: a walk of one sample; 256 + R L = 4096
# staged samples twice (the last launch that stages in LDS); 4099, odd repeat_len (the first that does not).
WALKS = ((2, 1), (5, 1), (30, 128), (2, 1920), (3, 1281))


def walk_captures(num, rl):
    """Two captures of num rl + 301 samples (301 offsets; an odd row length where num rl is
    even): seeded Gaussian noise, and the integer pattern tiled."""
    n = num * rl + 301
    rng = np.random.default_rng(1000 + num * rl)
    noise = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    return {"noise": noise, "integers": np.tile(int_pattern(), n // 32 + 1)[:n].copy()}


def assert_facts(facts, want):
    for k, v in want.items():
        if k == "score_at":
            assert all(facts[k][d] == s for d, s in v.items()), (k, v, {d: facts[k].get(d) for d in v})
        else:
            assert facts[k] == v, (k, facts[k], v)


# ---- two more link geometries -------------------------------------------------------------------
GEOMETRIES = {  # name -> n_fft, cp_len, data carriers, preamble; (mcs_index, payload bytes, payload symbols) per frame
    "128_9": (dict(n_fft=128, cp_len=9, data=np.array([i for i in range(-33, 34) if i != 0], np.int32), preamble=(2, 64)),
              ((0, 4, 8), (2, 40, 6), (3, 300, 21))),
    "256_16": (dict(n_fft=256, cp_len=16, data=np.array([i for i in range(-100, 101) if i != 0], np.int32), preamble=(2, 128)),
               ((2, 40, 2), (3, 300, 7))),
}


def geometry_captures(frame_of, frames, total=None):
    """One capture per (mcs_index, payload bytes, ...) of frames: name -> (capture, (mcs_index,
    sequence_num, payload)); the frame at 77, +1234 Hz, 0.4 rad, in a capture 300 samples longer
    than the frame, or of total samples."""
    out = {}
    for k, (mi, nbytes, _) in enumerate(frames):
        data = RFm.payload(nbytes, 70 + k)
        f = frame_of(mi, k, data)
        out[f"mcs{mi}_{nbytes}"] = (impair(f, 77, 1234.0, 0.4, SIGMA, 12, total=total or len(f) + 300), (mi, k, data))
    return out
