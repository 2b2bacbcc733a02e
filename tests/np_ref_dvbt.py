"""An independent numpy restatement of the DVB-T 2K frame (reference src/waveform/dvb_t.rs:112-718,
:862-953, src/waveform/dvb_t_tps.rs, src/sync/dvb_t_gi_sync.rs, src/modulate/dvb_t_frame.rs,
src/demodulate/dvb_t_frame.rs), written from the reference's text, f32 operation for operation,
for tests/test_dvbt_oracle.py and tests/test_gpu_dvbt.py.

The transform, window, equalizer arithmetic, coding chain and TS layer are the restatements the
other oracle files already hold to the library (np_ref_ofdm, np_ref_frame, np_ref_rs). Sums are
f32 in the reference's order: the guard-interval search is vectorised over offsets and loops
over k. |gamma| is the stated definition (the f32 rounding of the f64 square root of the f64 sum
of the two exact f64 squares), not libm's hypotf; atan2 is libm's atan2f.
"""
import ctypes
import ctypes.util

import numpy as np

import np_ref_frame as RFM
import np_ref_ofdm as RO
import np_ref_rs as RR

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]

N_FFT, KMAX, ACTIVE, DATA = 2048, 1704, 1705, 1512
CENTER = KMAX // 2
CONTINUAL = [0, 48, 54, 87, 141, 156, 192, 201, 255, 279, 282, 333, 432, 450, 483, 525, 531, 618, 636, 714, 759, 765,
             780, 804, 873, 888, 918, 939, 942, 969, 984, 1050, 1101, 1107, 1110, 1137, 1140, 1146, 1206, 1269, 1323,
             1377, 1491, 1683, 1704]
TPS_CARRIERS = [34, 50, 209, 346, 413, 569, 595, 688, 790, 901, 1073, 1219, 1262, 1286, 1469, 1594, 1687]
MAX_RX_WINDOW_BACKOFF = N_FFT // (2 * 12)
GUARD_CP = {"1/32": N_FFT // 32, "1/16": N_FFT // 16, "1/8": N_FFT // 8, "1/4": N_FFT // 4}
GUARD_CODE = {"1/32": 0, "1/16": 1, "1/8": 2, "1/4": 3}
CONST_CODE = {"qpsk": 0, "qam16": 1, "qam64": 2}
RATE_CODE = {"1/2": 0, "2/3": 1, "3/4": 2, "5/6": 3, "7/8": 4}
VBITS = {"qpsk": 2, "qam16": 4, "qam64": 6}
AXIS = {2: [1, -1], 4: [3, 1, -3, -1], 6: [7, 5, 1, 3, -7, -5, -1, -3]}
ERRORS = ("acquisition", "incomplete", "tps_decode", "payload_decode")


# ---- dvb_t.rs:383-521 -----------------------------------------------------------------------
def wk_prbs(n):
    reg, out = 0x7FF, []
    for _ in range(n):
        out.append((reg >> 10) & 1)
        reg = ((reg << 1) | (((reg >> 10) ^ (reg >> 1)) & 1)) & 0x7FF
    return np.array(out, np.uint8)


def boosted_pilot_value(wk):
    return np.complex64(F(F(F(F(4.0) / F(3.0)) * F(2.0)) * F(F(0.5) - F(wk))))


def to_bin(a):
    return (int(a) - CENTER) % N_FFT


def scattered_pilot_indices(phase):
    return list(range(3 * (phase % 4), KMAX + 1, 12))


def tps_carrier_bins():
    return [to_bin(a) for a in TPS_CARRIERS]


def continual_pilot_bins():
    return [to_bin(a) for a in CONTINUAL]


def plans():
    """Per phase: data_bins (active order), pilot_bins / pilot_values (active order), ref_bins /
    ref_values (the pilots minus the TPS bins, sorted by bin)."""
    wk, out = wk_prbs(ACTIVE), []
    for phase in range(4):
        reserved = sorted(set(CONTINUAL) | set(scattered_pilot_indices(phase)) | set(TPS_CARRIERS))
        data = [a for a in range(KMAX + 1) if a not in set(reserved)]
        assert len(data) == DATA
        pil = [(to_bin(a), boosted_pilot_value(wk[a])) for a in reserved]
        ref = sorted((b, v) for b, v in pil if b not in set(tps_carrier_bins()))
        out.append(dict(data_bins=np.array([to_bin(a) for a in data]), pilot_bins=np.array([b for b, _ in pil]),
                        pilot_values=np.array([v for _, v in pil], np.complex64), ref_bins=np.array([b for b, _ in ref]),
                        ref_values=np.array([v for _, v in ref], np.complex64)))
    return out


PLANS = plans()


# ---- Figure 9a, dvb_t.rs:138-266 ------------------------------------------------------------
def map_symbols(bits, v):
    """bits (n, v) -> complex64 (n,): even bits the I label, odd the Q label, MSB first."""
    b = np.asarray(bits, np.uint8).reshape(-1, v) & 1
    lv = (np.array(AXIS[v]).astype(F) * RO.axis_scale(v)).astype(F)
    ii = np.zeros(len(b), np.int64)
    qi = np.zeros(len(b), np.int64)
    for j in range(v):
        if j % 2 == 0:
            ii = (ii << 1) | b[:, j]
        else:
            qi = (qi << 1) | b[:, j]
    return RO.cplx(lv[ii], lv[qi])


def demap_symbols(syms, v):
    s = np.asarray(syms, np.complex64).reshape(-1)
    k = v // 2
    lv = (np.array(AXIS[v]).astype(F) * RO.axis_scale(v)).astype(F)

    def nearest(c):  # the first of equal distances
        return np.argmin(np.abs((c[:, None] - lv[None, :]).astype(F)), axis=1)

    ii, qi = nearest(s.real.astype(F)), nearest(s.imag.astype(F))
    out = np.zeros((len(s), v), np.uint8)
    for j in range(k):
        out[:, 2 * j] = (ii >> (k - 1 - j)) & 1
        out[:, 2 * j + 1] = (qi >> (k - 1 - j)) & 1
    return out


def soft_llrs(syms, v):
    s = np.asarray(syms, np.complex64).reshape(-1)
    k = v // 2
    lv = (np.array(AXIS[v]).astype(F) * RO.axis_scale(v)).astype(F)
    out = np.zeros((len(s), v), F)
    with np.errstate(all="ignore"):
        for axis, c in ((0, s.real.astype(F)), (1, s.imag.astype(F))):
            d = (c[:, None] - lv[None, :]).astype(F)
            dsq = (d * d).astype(F)
            for b in range(k):
                sel = np.array([(idx >> (k - 1 - b)) & 1 for idx in range(1 << k)], bool)
                d0 = np.fmin.reduce(np.concatenate([np.full((len(s), 1), np.inf, F), dsq[:, ~sel]], axis=1), axis=1)
                d1 = np.fmin.reduce(np.concatenate([np.full((len(s), 1), np.inf, F), dsq[:, sel]], axis=1), axis=1)
                out[:, 2 * b + axis] = (d1 - d0).astype(F)
    return out


# ---- dvb_t_tps.rs ---------------------------------------------------------------------------
GF_PRIM, GF_ORDER, BCH_GEN = 0x89, 127, 0x4377


def _gf():
    exp, log, x = [0] * (2 * GF_ORDER), [0] * (GF_ORDER + 1), 1
    for i in range(GF_ORDER):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x80:
            x ^= GF_PRIM
    for i in range(GF_ORDER, 2 * GF_ORDER):
        exp[i] = exp[i - GF_ORDER]
    return exp, log


GF_EXP, GF_LOG = _gf()


def gf_mul(a, b):
    return 0 if a == 0 or b == 0 else GF_EXP[GF_LOG[a] + GF_LOG[b]]


def tps_bch_parity(info):
    reg = 0
    for b in list(info) + [0] * 14:
        reg = (reg << 1) | (int(b) & 1)
        if reg & (1 << 14):
            reg ^= BCH_GEN
    return reg & ((1 << 14) - 1)


def tps_bch_encode(info):
    info = [int(b) for b in info]
    assert len(info) == 53
    p = tps_bch_parity(info)
    return np.array(info + [(p >> (13 - i)) & 1 for i in range(14)], np.uint8)


def tps_bch_decode(cw):
    cw = [int(b) for b in cw]
    if len(cw) != 67:
        return None
    shift = GF_ORDER - 67
    synd = []
    for i in range(1, 5):
        acc = 0
        for pos, bit in enumerate(cw):
            if bit & 1:
                acc ^= GF_EXP[(i * (66 - pos + shift)) % GF_ORDER]
        synd.append(acc)
    if not any(synd):
        return np.array(cw[:53], np.uint8)
    s1, s3 = synd[0], synd[2]
    if s1 == 0:
        return None
    num = s3 ^ gf_mul(gf_mul(s1, s1), s1)
    sig2 = 0 if num == 0 else GF_EXP[(GF_LOG[num] + GF_ORDER - GF_LOG[s1]) % GF_ORDER]
    err = []
    for pos in range(67):
        deg = 66 - pos + shift
        x = GF_EXP[(GF_ORDER - deg % GF_ORDER) % GF_ORDER]
        err.append(1 if (1 ^ gf_mul(s1, x) ^ gf_mul(sig2, gf_mul(x, x))) == 0 else 0)
    if sum(err) != (1 if sig2 == 0 else 2):
        return None
    fixed = [c ^ e for c, e in zip(cw, err)]
    if list(tps_bch_encode(fixed[:53])) != fixed:
        return None
    return np.array(fixed[:53], np.uint8)


def tps_pack(frame_number, constellation, code_rate, guard, cell_id):
    info = [0] * 53

    def put(a, b, value):
        for j, idx in enumerate(range(a, b)):
            info[idx] = (value >> (b - a - 1 - j)) & 1

    put(0, 16, 0b0011_0101_1110_1110 if frame_number % 2 == 0 else 0b1100_1010_0001_0001)
    put(16, 22, 0b011111)
    put(22, 24, frame_number & 3)
    put(24, 26, CONST_CODE[constellation])
    put(26, 29, 0)
    put(29, 32, RATE_CODE[code_rate])
    put(32, 35, RATE_CODE[code_rate])
    put(35, 37, GUARD_CODE[guard])
    put(37, 39, 0)
    put(39, 47, cell_id & 0xff)
    return np.concatenate([[0], tps_bch_encode(info)]).astype(np.uint8)


def tps_unpack(bits):
    """(frame_number, constellation, code_rate, guard, cell_id) or None."""
    if len(bits) != 68:
        return None
    info = tps_bch_decode(bits[1:])
    if info is None:
        return None

    def get(a, b):
        v = 0
        for idx in range(a, b):
            v = (v << 1) | int(info[idx])
        return v

    con = {v: k for k, v in CONST_CODE.items()}.get(get(24, 26))
    rate = {v: k for k, v in RATE_CODE.items()}.get(get(29, 32))
    if con is None or rate is None:
        return None
    return get(22, 24), con, rate, {v: k for k, v in GUARD_CODE.items()}[get(35, 37)], get(39, 47)


def tps_reference_signs():
    wk = wk_prbs(ACTIVE)
    return np.array([F(F(2.0) * F(F(0.5) - F(wk[k]))) for k in TPS_CARRIERS], F)


def tps_encode(bits68, n_symbols):
    """TpsEncoder over n_symbols, reset after every 68th: cells (n_symbols, 17)."""
    out, signs, symbol = [], tps_reference_signs(), 0
    for s in range(n_symbols):
        if symbol > 0 and (int(bits68[s % 68]) & 1):
            signs = -signs
        out.append(RO.cplx(signs, np.zeros(17, F)))
        symbol += 1
        if (s + 1) % 68 == 0:
            signs, symbol = tps_reference_signs(), 0
    return np.array(out, np.complex64).reshape(n_symbols, 17)


def tps_decide(cells):
    """TpsDecoder::feed_symbol over the rows of cells (n, 17): bit l = (sum over the carriers, in
    order, of re(cell conj(prev))) < 0."""
    cells = np.asarray(cells, np.complex64)
    bits = []
    for l in range(min(len(cells), 68)):
        if l == 0:
            bits.append(0)
            continue
        c, p = cells[l], cells[l - 1]
        acc = F(0)
        with np.errstate(all="ignore"):
            for j in range(17):
                pim = -F(p[j].imag)
                acc = F(acc + F(F(F(c[j].real) * F(p[j].real)) - F(F(c[j].imag) * pim)))
        bits.append(1 if acc < 0 else 0)
    return np.array(bits, np.uint8)


def tps_word(cells):
    bits = tps_decide(cells)
    return tps_unpack(bits) if len(bits) >= 68 else None


# ---- dvb_t_gi_sync.rs -----------------------------------------------------------------------
def norm32(re, im):
    """The stated |z|: f32(sqrt_f64(f64(re)^2 + f64(im)^2)), each square exact in f64."""
    re, im = np.asarray(re, F).astype(np.float64), np.asarray(im, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im).astype(F)


def gi_sums(iq, n_fft, cp, ds, max_syms):
    """gamma (re, im) and Phi (halved) at the offsets ds, the sequential sums vectorised over ds."""
    iq = np.asarray(iq, np.complex64)
    re, im = iq.real.astype(F), iq.imag.astype(F)
    ds = np.asarray(ds, np.int64)
    gr, gi, phi = np.zeros(len(ds), F), np.zeros(len(ds), F), np.zeros(len(ds), F)
    period = n_fft + cp
    with np.errstate(all="ignore"):
        for u in range(max_syms):
            base = ds + u * period
            fit = base + n_fft + cp <= len(iq)  # once false it stays false: the while loop has ended
            if not fit.any():
                break
            bs = np.where(fit, base, 0)
            for k in range(cp):
                ar, ai, br, bi = re[bs + k], im[bs + k], re[bs + n_fft + k], im[bs + n_fft + k]
                nbi = -bi
                pr = ((ar * br).astype(F) - (ai * nbi).astype(F)).astype(F)
                pi = ((ar * nbi).astype(F) + (ai * br).astype(F)).astype(F)
                e = (((ar * ar).astype(F) + (ai * ai).astype(F)).astype(F) +
                     ((br * br).astype(F) + (bi * bi).astype(F)).astype(F)).astype(F)
                gr = np.where(fit, (gr + pr).astype(F), gr)
                gi = np.where(fit, (gi + pi).astype(F), gi)
                phi = np.where(fit, (phi + e).astype(F), phi)
        phi = (phi * F(0.5)).astype(F)
    return gr, gi, phi


def total_key(v):
    b = np.asarray(v, F).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def gi_sync(iq, n_fft, cp, fs, search_len, rho=0.95, max_symbols=4, origin_score_ratio=0.5, detail=False):
    """dvb_t_gi_sync_with: dict(start, cfo_hz, score, gamma, phi[, metric]) or None."""
    iq = np.asarray(iq, np.complex64)
    if cp == 0 or n_fft == 0:
        return None
    need = max(search_len - 1, 0) + n_fft + cp
    if len(iq) < need or search_len == 0:
        return None
    period = n_fft + cp
    gr, gi, phi = gi_sums(iq, n_fft, cp, np.arange(search_len), max(max_symbols, 1))
    with np.errstate(all="ignore"):
        metric = (norm32(gr, gi) - (F(rho) * phi).astype(F)).astype(F)
    keys = total_key(metric)
    argmax = int(search_len - 1 - np.argmax(keys[::-1]))  # max_by: the last of equal maxima

    def single(d):
        if d + n_fft + cp > len(iq):
            return F(0)
        r, i, p = gi_sums(iq, n_fft, cp, [d], 1)
        with np.errstate(all="ignore"):
            return F(min(F(norm32(r, i)[0] / p[0]), F(1.0))) if p[0] > 0 else F(0)

    phase = argmax % period
    origin = argmax - phase
    best = argmax
    if origin_score_ratio > 0.0 and phase != 0 and period - phase <= -(-cp // 2):
        ratio = F(min(max(F(origin_score_ratio), F(0.0)), F(1.0)))
        if single(origin) >= F(ratio * single(argmax)):
            best = origin
    g_re, g_im, p = gr[best], gi[best], phi[best]
    with np.errstate(all="ignore"):
        score = F(min(F(norm32(g_re, g_im) / p), F(1.0))) if p > 0 else F(0)
        ang = F(_libm.atan2f(float(g_im), float(g_re)))
        cfo = F(F(-ang * F(fs)) / F(F(2.0 * np.pi) * F(n_fft)))
    out = dict(start=best, cfo_hz=cfo, score=score, gamma=RO.cplx(g_re, g_im)[()], phi=F(p))
    if detail:
        out.update(metric=metric, gamma_all=RO.cplx(gr, gi), phi_all=phi)
    return out


def gi_refine(iq, n_fft, cp, fs, coarse, radius, rho=0.95, max_symbols=4):
    start = max(coarse - radius, 0)
    if start > len(iq):
        return None
    sub = np.asarray(iq, np.complex64)[start:]
    r = gi_sync(sub, n_fft, cp, fs, min(2 * radius + 1, len(sub)), rho, max_symbols, 0.0)
    if r is not None:
        r["start"] += start
    return r


def integer_cfo(freq, n_fft, max_bins):
    """(bins, confidence) or None; energies summed in pilot order, the first of equal maxima."""
    freq = np.asarray(freq, np.complex64)
    if len(freq) < n_fft or n_fft == 0 or max_bins <= 0:
        return None
    pb = continual_pilot_bins()
    best_k, best_e, total, count = 0, F(-np.inf), F(0), 0
    with np.errstate(all="ignore"):
        for k in range(-max_bins, max_bins + 1):
            e = F(0)
            for b in pb:
                x = freq[(b + k) % n_fft]
                e = F(e + F(F(F(x.real) * F(x.real)) + F(F(x.imag) * F(x.imag))))
            total = F(total + e)
            count += 1
            if e > best_e:
                best_e, best_k = e, k
        mean = F(total / F(count))
        conf = F(best_e / mean) if mean > 0 else F(0)
    return best_k, conf


# ---- the frame, modulate/dvb_t_frame.rs and demodulate/dvb_t_frame.rs -----------------------
def scheme(code_rate):
    return RFM.scheme(crc="none", outer=("rs", 204, 16), inner=("conv", code_rate, "dvb_k7"),
                      outer_interleaver=("forney", 12, 17), scrambler=None)


def fs_1mhz():
    return F(F(F(1_000_000.0) * F(N_FFT)) / F(ACTIVE))


def coded_bits_for_packets(n_pkt, code_rate):
    return RFM.block_plan(n_pkt * 188, scheme(code_rate))[5]


def frame_plan(payload_len, constellation, code_rate):
    """(n_symbols, target_packets) of DvbTFrameMod::modulate."""
    per_sym = DATA * VBITS[constellation]
    n_real = max(1, -(-payload_len // 187))
    n_symbols = max(-(-coded_bits_for_packets(n_real, code_rate) // per_sym), 68)
    target = n_real
    while coded_bits_for_packets(target, code_rate) < n_symbols * per_sym:
        target += 1
    return n_symbols, target


def mod_symbols(coded, v, cp, tps_bits, n_symbols, roll_off=0):
    coded = np.asarray(coded, np.uint8)
    per_sym = DATA * v
    cells = tps_encode(tps_bits, n_symbols)
    freq = np.zeros((n_symbols, N_FFT), np.complex64)
    for s in range(n_symbols):
        pl = PLANS[s % 4]
        seg = coded[s * per_sym:(s + 1) * per_sym]
        whole = len(seg) // v  # a carrier needs all its v bits inside the coded stream
        syms = np.zeros(DATA, np.complex64)
        if whole:
            syms[:whole] = map_symbols(seg[:whole * v], v)
        freq[s, pl["data_bins"]] = syms
        freq[s, pl["pilot_bins"]] = pl["pilot_values"]
        freq[s, tps_carrier_bins()] = cells[s]
    time = RO.fft_radix2(freq, inverse=True)
    iq = np.concatenate([time[:, N_FFT - cp:], time], axis=1)
    if roll_off > 0:
        iq = RO.window_apply(iq, RO.window_ramp(N_FFT + cp, roll_off))
    return np.ascontiguousarray(iq.reshape(-1)).astype(np.complex64)


def modulate(payload, guard, constellation, code_rate, frame_number, cell_id, roll_off=0):
    """(iq, n_symbols, samples_per_symbol); no TX low-pass (that is the library's device filter)."""
    payload = np.asarray(payload, np.uint8)
    cp, v = GUARD_CP[guard], VBITS[constellation]
    n_symbols, target = frame_plan(len(payload), constellation, code_rate)
    ts = RR.ts_energy_disperse(RR.ts_stuff_null_packets(RR.ts_packetize(payload), target))
    coded = RFM.encode_chain(ts, scheme(code_rate))
    assert len(coded) >= n_symbols * DATA * v
    iq = mod_symbols(coded, v, cp, tps_pack(frame_number, constellation, code_rate, guard, cell_id), n_symbols, roll_off)
    return iq, n_symbols, N_FFT + cp


def demod_symbols(iq, n_symbols, cp, backoff, v):
    """(llr (n_symbols, 1512 v), cells (n_symbols, 17), equalized data symbols (n_symbols, 1512))."""
    iq = np.asarray(iq, np.complex64)
    sps, start = N_FFT + cp, cp - min(backoff, cp)
    win = np.stack([iq[s * sps + start:s * sps + start + N_FFT] for s in range(n_symbols)])
    freq = RO.fft_radix2(win)
    llr, cells, syms = np.zeros((n_symbols, DATA * v), F), freq[:, tps_carrier_bins()], np.zeros((n_symbols, DATA), np.complex64)
    for s in range(n_symbols):
        pl = PLANS[s % 4]
        ratios = RO.cdiv(freq[s, pl["ref_bins"]], pl["ref_values"])
        est = RO.interpolate_bins(pl["ref_bins"], ratios, pl["data_bins"])
        syms[s] = RO.cmul(freq[s, pl["data_bins"]], RO.equalizer_weight(est))
        llr[s] = soft_llrs(syms[s], v).reshape(-1)
    return llr, np.ascontiguousarray(cells), syms


def rotate(iq, freq_hz, fs):
    r = RO.rotator(freq_hz, fs, len(iq))
    iq = np.asarray(iq, np.complex64)
    a, b, pr, pi = iq.real.astype(F), iq.imag.astype(F), r.real.astype(F), r.imag.astype(F)
    return RO.cplx(RO._fma(a, pr, -(b * pi).astype(F)), RO._fma(b, pr, (a * pi).astype(F)))


def integer_cfo_correct(iq, cp, fs):
    """(rotated or None, bins or None) of DvbTFrameDemod::integer_cfo_correct."""
    sps = N_FFT + cp
    acq = gi_sync(iq, N_FFT, cp, fs, sps)
    if acq is None:
        return None, None
    accum = np.zeros(N_FFT, F)
    for s in range(8):
        off = acq["start"] + s * sps
        if off + sps > len(iq):
            break
        f = RO.fft_radix2(iq[off + cp:off + sps])
        accum = (accum + ((f.real * f.real).astype(F) + (f.imag * f.imag).astype(F)).astype(F)).astype(F)
    est = integer_cfo(RO.cplx(accum, np.zeros(N_FFT, F)), N_FFT, 32)
    if est is None:
        return None, None
    if est[0] == 0:
        return None, 0
    return rotate(iq, F(F(-F(est[0]) * F(fs)) / F(N_FFT)), fs), est[0]


def decode(iq, n_symbols, payload_len, guard, constellation, code_rate, backoff=0, integer_cfo_on=False):
    """A dict (payload, tps, cfo_hz, sync_score, timing_offset_samples, integer_cfo_bins,
    outer_fec_ok, rs_corrected_bytes) or the error's name."""
    iq = np.asarray(iq, np.complex64)
    cp, v, fs = GUARD_CP[guard], VBITS[constellation], fs_1mhz()
    sps = N_FFT + cp
    bins = None
    if integer_cfo_on:
        rot, bins = integer_cfo_correct(iq, cp, fs)
        iq = rot if rot is not None else iq
    acq = gi_sync(iq, N_FFT, cp, fs, sps)
    if acq is None:
        return "acquisition"
    start = acq["start"]
    if len(iq) < start + n_symbols * sps:
        return "incomplete"
    out = dict(cfo_hz=F(acq["cfo_hz"] + F(F(bins or 0) * F(fs / F(N_FFT)))), sync_score=acq["score"],
               timing_offset_samples=start, integer_cfo_bins=bins)
    llr, cells, _ = demod_symbols(iq[start:], n_symbols, cp, backoff, v)
    tps = tps_word(cells)
    if tps is None:
        return "tps_decode"
    packets = max(1, -(-payload_len // 187))
    sch = scheme(code_rate)
    plan = RFM.block_plan(packets * 188, sch)
    if llr.size < plan[5]:
        return "payload_decode"
    res = RFM.decode_chain(llr.reshape(-1), plan, sch)
    if not isinstance(res, dict) or not res["valid"] or len(res["bytes"]) < packets * 188:
        return "payload_decode"
    payload = RR.ts_depacketize(RR.ts_energy_disperse(res["bytes"][:packets * 188]))
    if payload is None:
        return "payload_decode"
    out.update(payload=np.asarray(payload[:payload_len], np.uint8), tps=tps, outer_fec_ok=res["outer_ok"],
               rs_corrected_bytes=res["outer_corrected_bytes"])
    return out


# ---- the inputs the CPU and GPU tests share -------------------------------------------------
def sample_payload(n):
    return ((np.arange(n) * 37 + 11) & 0xff).astype(np.uint8)


def awgn(iq, sigma, seed):
    r = np.random.default_rng(seed)
    n = (r.standard_normal(len(iq)) + 1j * r.standard_normal(len(iq))) * (sigma / np.sqrt(2.0))
    return (np.asarray(iq, np.complex64) + n.astype(np.complex64)).astype(np.complex64)


def two_tap(iq):
    """apply_fir_channel with the reference tests' two taps (0.8, 0.7 - 0.35j), in complex64."""
    iq = np.asarray(iq, np.complex64)
    out = (iq * np.complex64(0.8)).astype(np.complex64)
    out[1:] += (iq[:-1] * np.complex64(0.7 - 0.35j)).astype(np.complex64)
    return out


def place(iq, lead, tail):
    return np.concatenate([np.zeros(lead, np.complex64), np.asarray(iq, np.complex64), np.zeros(tail, np.complex64)])


def rms(iq):
    return float(np.sqrt(np.mean(np.abs(np.asarray(iq, np.complex64).astype(np.complex128)) ** 2)))


CAPTURE_PARAMS = ("1/32", "qpsk", "1/2", 2, 0x5A)  # the reference tests' capstone link
CAPTURE_PAYLOAD_LEN = 184
# name -> (lead, noise over the frame's rms, seed); chosen on the host path so that the set holds
# every outcome (test_dvbt_oracle.py asserts it): the noise levels sit well inside their class
CAPTURE_NOISE = {"clean": (200, 0.0, 0), "noisy": (37, 0.5, 11), "multipath": (150, 0.05, 12),
                 "payload_fails": (200, 1.0, 13), "tps_fails": (200, 0.0, 0), "truncated": (400, 0.0, 0)}


def capture_set(frame_iq, n_symbols, sps):
    """The noisy capture set the CPU and GPU tests share, from one modulated frame (the capstone
    link, payload sample_payload(184)): rows of one length L = n_symbols sps + 300 and their
    names, plus `short`, a capture one sample too short to search. tps_fails negates three runs
    of symbols (six differential errors: past BCH's two); truncated starts 400 samples in, so
    its frame does not fit."""
    frame_iq = np.asarray(frame_iq, np.complex64)
    L, r = n_symbols * sps + 300, rms(frame_iq)
    rows, names = [], []
    for name, (lead, noise, seed) in CAPTURE_NOISE.items():
        x = frame_iq.copy()
        if name == "multipath":
            x = two_tap(x)
        if name == "tps_fails":
            for a, b in ((5, 9), (20, 31), (40, 41)):
                x[a * sps:b * sps] = -x[a * sps:b * sps]
        row = place(x, lead, max(L - lead - len(x), 0))[:L]
        if noise:
            row = awgn(row, noise * r, seed)
        rows.append(np.ascontiguousarray(row))
        names.append(name)
    short = np.ascontiguousarray(frame_iq[:2 * sps - 2])
    return np.stack(rows), names, short
