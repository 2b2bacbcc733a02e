"""TEST INFRASTRUCTURE — numpy float32 restatement of the reference's FT8 / FT4 sync
front end (src/sync/waterfall.rs, costas.rs, ft8_sync.rs, ft4_sync.rs), in the
reference's own operation order, plus deterministic FT8 / FT4 test frames.

Two restatements, as elsewhere in this suite: a vectorised one (over waterfall cells /
score-map cells, with a Python loop over the sample index) and a plain scalar one of
goertzel_energy and costas_score; tests/test_sync_oracle.py holds them to each other
bit for bit. `_fma`, `sinf` and `cosf` come from np_ref. The frames' noise is np_ref.add_awgn's
sequence, drawn through the C oracle's add_awgn (the same generator, held equal to
np_ref's bit for bit by test_oracle.py and again on these buffers by test_sync_oracle.py):
np_ref's Python loop would take 20 s on the two buffers.
"""
import ctypes
import functools

import numpy as np

from np_ref import TAU, _fma, cosf, f32, sinf

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]

N_LLR = 174  # codec/ldpc.rs N
NEG_INF = f32(-np.inf)

# modulate/ft8.rs:9-18, sync/ft8_sync.rs:44-63; modulate/ft4.rs:9-24, sync/ft4_sync.rs:44-50
FT8 = dict(name="ft8", sps=1920, spacing=f32(6.25), tones=8, total=79, data=58,
           costas=[[3, 1, 4, 0, 6, 5, 2]] * 3, pos=[0, 36, 72])
FT4 = dict(name="ft4", sps=576, spacing=f32(20.833334), tones=4, total=105, data=87,
           costas=[[0, 1, 3, 2], [1, 0, 2, 3], [2, 3, 1, 0], [3, 2, 0, 1]], pos=[1, 34, 67, 100])
FT8_GRAY8 = [0, 1, 3, 2, 5, 6, 4, 7]
FT4_GRAY4 = [0, 1, 3, 2]


def logf(x):
    return f32(_libm.logf(float(x)))


def _vlogf(a):
    a = np.asarray(a, f32)
    return np.array([_libm.logf(float(v)) for v in a.ravel()], f32).reshape(a.shape)


# ---------------------------------------------------------------- waterfall --
def steps(fs, base_hz, spacing, num_tones):
    """waterfall.rs:84-91: w_k = (cos phi, sin phi), phi = -TAU * f / fs, f = base + k * spacing (f32)."""
    wr = np.empty(num_tones, f32)
    wi = np.empty(num_tones, f32)
    for k in range(num_tones):
        f = f32(f32(base_hz) + f32(f32(k) * f32(spacing)))
        phi = f32(f32(f32(-TAU) * f) / f32(fs))
        wr[k] = cosf(phi)
        wi[k] = sinf(phi)
    return wr, wi


def waterfall_energy(iq, fs, base_hz, spacing, sps, num_syms, num_tones, time_offset=0):
    """goertzel_energy (waterfall.rs:126-151) of every cell, vectorised over (row, tone).
    Returns (e, present): e[row, tone] f32 (0 where the row has no sample), present[row]
    false for rows that start at or past the end of the buffer (waterfall.rs:99-102)."""
    iq = np.asarray(iq, np.complex64)
    n = len(iq)
    wr, wi = steps(fs, base_hz, spacing, num_tones)
    if num_tones == 1:  # np_ref._fma takes one-element arrays for scalars: carry a second copy
        e, present = waterfall_energy(iq, fs, base_hz, 0.0, sps, num_syms, 2, time_offset)
        return e[:, :1].copy(), present
    start = time_offset + np.arange(num_syms, dtype=np.int64) * sps
    length = np.clip(n - start, 0, sps)
    xr = np.zeros((num_syms, sps), f32)
    xi = np.zeros((num_syms, sps), f32)
    for r in range(num_syms):
        seg = iq[start[r]:start[r] + length[r]] if length[r] else iq[:0]
        xr[r, :length[r]] = seg.real
        xi[r, :length[r]] = seg.imag
    ar = np.zeros((num_syms, num_tones), f32)
    ai = np.zeros((num_syms, num_tones), f32)
    pr = np.ones(num_tones, f32)
    pi = np.zeros(num_tones, f32)
    for i in range(int(length.max()) if num_syms else 0):
        live = (i < length)[:, None]
        a, b = xr[:, i][:, None], xi[:, i][:, None]
        # num-complex Mul: (a c - b d, a d + b c), no FMA; AddAssign: two adds
        mr = a * pr[None, :] - b * pi[None, :]
        mi = a * pi[None, :] + b * pr[None, :]
        ar = np.where(live, ar + mr, ar)
        ai = np.where(live, ai + mi, ai)
        # waterfall.rs:155-160 mul(phasor, w)
        pr, pi = _fma(pr, wr, -(pi * wi)), _fma(pi, wr, pr * wi)
    return (ar * ar + ai * ai).astype(f32), length > 0


def compute_waterfall(iq, fs, base_hz, spacing, sps, num_syms, num_tones, time_offset=0):
    """waterfall.rs:73-119: ln(e + 1e-12) per cell; rows past the end of the buffer stay 0.0."""
    e, present = waterfall_energy(iq, fs, base_hz, spacing, sps, num_syms, num_tones, time_offset)
    mag = _vlogf(e + f32(1e-12))
    mag[~present, :] = f32(0.0)
    return mag


def goertzel_energy_scalar(seg, w):
    """waterfall.rs:126-151, one sample at a time in Python scalars (w = (re, im))."""
    wr, wi = f32(w[0]), f32(w[1])
    ar = ai = f32(0.0)
    pr, pi = f32(1.0), f32(0.0)
    for z in seg:
        a, b = f32(z.real), f32(z.imag)
        ar = f32(ar + f32(f32(a * pr) - f32(b * pi)))
        ai = f32(ai + f32(f32(a * pi) + f32(b * pr)))
        pr, pi = _fma(pr, wr, f32(-f32(pi * wi))), _fma(pi, wr, f32(pr * wi))
    return f32(f32(ar * ar) + f32(ai * ai))


# ------------------------------------------------------------------- Costas --
def costas_score_scalar(wf, costas, pos, time_sym, freq_bin):
    """costas.rs:48-111 / ft4_sync.rs:166-219 (costas: one tone list per block)."""
    num_syms, num_tones = wf.shape
    total = f32(0.0)
    for blk, block_start in enumerate(pos):
        for ci, tone in enumerate(costas[blk]):
            sym = time_sym + block_start + ci
            if sym < 0 or sym >= num_syms:
                continue
            b = freq_bin + tone
            if b >= num_tones:
                continue
            left = wf[sym, b - 1] if b > 0 else NEG_INF
            right = wf[sym, b + 1] if b + 1 < num_tones else NEG_INF
            prev = wf[sym - 1, b] if sym > 0 else NEG_INF
            nxt = wf[sym + 1, b] if sym + 1 < num_syms else NEG_INF
            diff = f32(wf[sym, b] - max(max(left, right), max(prev, nxt)))
            total = f32(total + max(diff, f32(0.0)))
    return total


def costas_score_map(wf, mode, t_min, t_max):
    """Every (time_sym, freq_bin) score of a search, [t_max - t_min + 1][max_freq_bin + 1];
    None when the waterfall is no wider than a frame (costas.rs:138-142)."""
    wf = np.asarray(wf, f32)
    num_syms, num_tones = wf.shape
    if num_tones <= mode["tones"] or t_max < t_min:
        return None if num_tones <= mode["tones"] else np.zeros((0, num_tones - mode["tones"] + 1), f32)
    nfb = num_tones - mode["tones"] + 1
    wp = np.full((num_syms + 2, num_tones + 2), NEG_INF, f32)
    wp[1:-1, 1:-1] = wf
    t = np.arange(t_min, t_max + 1, dtype=np.int64)
    fb = np.arange(nfb, dtype=np.int64)
    total = np.zeros((len(t), nfb), f32)
    with np.errstate(invalid="ignore"):
        for blk, block_start in enumerate(mode["pos"]):
            for ci, tone in enumerate(mode["costas"][blk]):
                sym = t + block_start + ci
                b = fb + tone
                ok = ((sym >= 0) & (sym < num_syms))[:, None] & (b < num_tones)[None, :]
                s = np.clip(sym, 0, num_syms - 1)[:, None] + 1
                c = np.clip(b, 0, num_tones - 1)[None, :] + 1
                e_freq = np.maximum(wp[s, c - 1], wp[s, c + 1])
                e_time = np.maximum(wp[s - 1, c], wp[s + 1, c])
                diff = wp[s, c] - np.maximum(e_freq, e_time)
                total = np.where(ok, total + np.maximum(diff, f32(0.0)), total).astype(f32)
    return total


def top_n(score_map, t_min, max_cand):
    """costas.rs:136-173: the reference's keep-N scan, replayed literally (Python's sort
    is stable, like slice::sort_by). Returns [(time_sym, freq_bin, score)], best first."""
    if score_map is None:
        return []
    if max_cand == 0:
        raise IndexError("max_candidates == 0: the reference indexes an empty heap")
    heap = []
    for ti in range(score_map.shape[0]):
        for fb in range(score_map.shape[1]):
            score = score_map[ti, fb]
            if len(heap) < max_cand:
                heap.append((t_min + ti, fb, score))
                if len(heap) == max_cand:
                    heap.sort(key=lambda c: c[2])
            elif score > heap[0][2]:
                heap[0] = (t_min + ti, fb, score)
                heap.sort(key=lambda c: c[2])
    heap.sort(key=lambda c: c[2], reverse=True)  # reverse=True keeps equal scores in their order
    return heap


def find_candidates(wf, mode, t_min, t_max, max_cand):
    """costas.rs:125-174 (FT8) / ft4_sync.rs:122-163 (FT4)."""
    return top_n(costas_score_map(wf, mode, t_min, t_max), t_min, max_cand)


# --------------------------------------------------------------------- LLRs --
def _max4(a, b, c, d):
    return max(max(a, b), max(c, d))


def extract_llr(wf, mode, time_sym, freq_bin):
    """ft8_sync.rs:170-231 / ft4_sync.rs:227-278: 174 raw max-log LLRs of one candidate."""
    wf = np.asarray(wf, f32)
    num_syms, num_tones = wf.shape
    llr = np.zeros(N_LLR, f32)
    ft8 = mode["name"] == "ft8"
    if ft8:
        frame_syms = list(range(7, 36)) + list(range(43, 72))
    else:
        frame_syms = [k + 5 if k < 29 else k + 9 if k < 58 else k + 13 for k in range(87)]
    bits = 3 if ft8 else 2
    for k, fsym in enumerate(frame_syms):
        r = time_sym + fsym
        if r < 0 or r >= num_syms:
            continue
        s = [wf[r, freq_bin + j] if freq_bin + j < num_tones else NEG_INF for j in range(mode["tones"])]
        if ft8:
            s2 = [s[g] for g in FT8_GRAY8]
            llr[3 * k] = -f32(_max4(s2[4], s2[5], s2[6], s2[7]) - _max4(s2[0], s2[1], s2[2], s2[3]))
            llr[3 * k + 1] = -f32(_max4(s2[2], s2[3], s2[6], s2[7]) - _max4(s2[0], s2[1], s2[4], s2[5]))
            llr[3 * k + 2] = -f32(_max4(s2[1], s2[3], s2[5], s2[7]) - _max4(s2[0], s2[2], s2[4], s2[6]))
        else:
            s2 = [s[g] for g in FT4_GRAY4]
            llr[bits * k] = -f32(max(s2[2], s2[3]) - max(s2[0], s2[1]))
            llr[bits * k + 1] = -f32(max(s2[1], s2[3]) - max(s2[0], s2[2]))
    return llr


def normalise_llr(llr):
    """ft8_sync.rs:237-246: variance = (sequential f32 sum of x*x) / 174; scaled when > 1e-10."""
    llr = np.array(llr, f32)
    acc = f32(0.0)
    for v in llr:
        acc = f32(acc + f32(v * v))
    variance = f32(acc / f32(N_LLR))
    if variance > f32(1e-10):
        scale = f32(np.sqrt(f32(f32(24.0) / variance)))
        llr = (llr * scale).astype(f32)
    return llr


# ---------------------------------------------------------------- top level --
def sync_geometry(mode, base_hz, max_hz, t_min, t_max):
    """ft8_sync.rs:99-131: (num_bins, wf_syms, wf_sample_start, sym_offset_adj, wf_t_max)."""
    freq_range = max(f32(f32(max_hz) - f32(base_hz)), f32(0.0))
    num_bins = int(np.ceil(f32(freq_range / mode["spacing"]))) + mode["tones"] + 1
    wf_syms = max(t_max + mode["total"] - t_min, 1)
    start = t_min * mode["sps"] if t_min >= 0 else 0
    adj = -t_min if t_min < 0 else 0
    return num_bins, wf_syms, start, adj, max(wf_syms - mode["total"], 0)


def sync(iq, mode, fs, base_hz, max_hz, t_min, t_max, max_cand, wf=None):
    """ft8_sync (ft8_sync.rs:90-159) / ft4_sync (ft4_sync.rs:65-117): list of dicts, best
    first. wf: a waterfall to search instead of the restatement's own (same geometry)."""
    num_bins, wf_syms, start, adj, wf_t_max = sync_geometry(mode, base_hz, max_hz, t_min, t_max)
    if wf is None:
        wf = compute_waterfall(iq, fs, base_hz, mode["spacing"], mode["sps"], wf_syms, num_bins, start)
    out = []
    for (ts, fb, score) in find_candidates(wf, mode, 0, wf_t_max, max_cand):
        out.append({"time_sym": int(ts - adj), "freq_bin": int(fb), "score": f32(score),
                    "llr": normalise_llr(extract_llr(wf, mode, ts, fb))})
    return out


def ft8_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return sync(iq, FT8, fs, base_hz, max_hz, t_min, t_max, max_cand)


def ft4_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return sync(iq, FT4, fs, base_hz, max_hz, t_min, t_max, max_cand)


# -------------------------------------------------------------- test frames --
def symbol_sequence(mode, data):
    """Ft8Mod / Ft4Mod::build_symbol_sequence (ft8.rs:65-85, ft4.rs:73-103): the Costas
    blocks (and FT4's two tone-0 ramp symbols) inserted around the data tones."""
    data = list(data)
    assert len(data) == mode["data"]
    syms = [None] * mode["total"]
    if mode["name"] == "ft4":
        syms[0] = syms[104] = 0
    for blk, p in enumerate(mode["pos"]):
        for ci, tone in enumerate(mode["costas"][blk]):
            syms[p + ci] = tone
    it = iter(data)
    return [s if s is not None else next(it) for s in syms]


def frame_samples(mode, data, base_idx):
    """A CPFSK frame whose tone k sits at (base_idx + k) * spacing with fs = sps * spacing
    (12 kHz): every tone is a whole number of cycles per symbol, so the phase is an
    integer index modulo sps that steps by base_idx + tone per sample and looks up a
    cosf / sinf table. base_idx 160 (FT8) / 48 (FT4) is tone 0 at 1000 Hz."""
    sps = mode["sps"]
    tab = np.array([complex(cosf(f32(TAU * f32(j) / f32(sps))), sinf(f32(TAU * f32(j) / f32(sps)))) for j in range(sps)],
                   np.complex64)
    idx = np.empty(mode["total"] * sps, np.int64)
    ph = 0
    for s, tone in enumerate(symbol_sequence(mode, data)):
        step = base_idx + tone
        idx[s * sps:(s + 1) * sps] = (ph + step * np.arange(1, sps + 1)) % sps
        ph = int(idx[(s + 1) * sps - 1])
    return tab[idx]


def frame_data(mode, seed):
    return np.random.default_rng(seed).integers(0, mode["tones"], mode["data"]).tolist()


def data_bits(mode, data):
    """The bits the LLR signs carry: tone -> binary index through the Gray map (the
    inverse of FT8_GRAY8 / FT4_GRAY4), MSB first."""
    gray = FT8_GRAY8 if mode["name"] == "ft8" else FT4_GRAY4
    nb = 3 if mode["name"] == "ft8" else 2
    out = []
    for tone in data:
        j = gray.index(tone)
        out += [(j >> (nb - 1 - b)) & 1 for b in range(nb)]
    return np.array(out, np.int64)


FS = 12000.0
BASE_HZ = 1000.0
LATE_SYMS, UP_BINS = 2, 5
T_MIN, T_MAX, MAX_CAND = 0, 4, 5
NOISE_SEED = {"ft8": 1234, "ft4": 4321}


@functools.lru_cache(maxsize=None)
def test_frame(name):
    """The suite's search case: a frame placed LATE_SYMS symbols late and UP_BINS bins
    above BASE_HZ in a buffer of T_MAX + total symbols, noise power 0.5 (add_awgn).
    Returns (mode, iq, data, max_hz); the search over [BASE_HZ, max_hz] has 19 bins (FT8)."""
    mode = FT8 if name == "ft8" else FT4
    data = frame_data(mode, 8 if name == "ft8" else 4)
    frame = frame_samples(mode, data, (160 if name == "ft8" else 48) + UP_BINS)
    n = (T_MAX - T_MIN + mode["total"]) * mode["sps"]
    iq = np.zeros(n, np.complex64)
    iq[LATE_SYMS * mode["sps"]:LATE_SYMS * mode["sps"] + len(frame)] = frame
    import oracle

    iq = oracle.add_awgn(iq, 0.5, NOISE_SEED[name])
    iq.setflags(write=False)
    max_hz = float(f32(BASE_HZ) + f32(10.0) * mode["spacing"])
    return mode, iq, data, max_hz


test_frame.__test__ = False  # a fixture builder, not a pytest test
