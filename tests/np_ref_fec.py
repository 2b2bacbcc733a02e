"""Independent numpy restatement of the reference's inner code (test infrastructure): the
punctured, zero-tail-terminated convolutional code and its soft Viterbi decoder
(src/fec/conv.rs), the block interleaver (src/fec/interleaver.rs:53-120) and the two chain
drivers that use it (interleave_bits, modulate/ofdm_frame.rs; deinterleave_llrs,
demodulate/ofdm_frame.rs). Written from those files, in the decoder's own visit order
(states ascending, bit 0 then bit 1), not from csrc/fec.cpp. Every metric operation is one
f32 operation."""
import functools

import numpy as np

CODES = {"k5": (5, 0b10101, 0b10011), "dvb_k7": (7, 0b1111001, 0b1011011)}  # conv.rs:89-94
MATRICES = {  # conv.rs:112-120
    "1/2": ((1,), (1,)),
    "2/3": ((1, 1), (1, 0)),
    "3/4": ((1, 1, 0), (1, 0, 1)),
    "5/6": ((1, 1, 0, 1, 0), (1, 0, 1, 0, 1)),
    "7/8": ((1, 1, 1, 1, 0, 1, 0), (1, 0, 0, 0, 1, 0, 1)),
}
RATES = tuple(MATRICES)
F32 = np.float32


def _parity(x):
    return bin(x).count("1") & 1


def reg_bits(code):
    return CODES[code][0] - 1


def branch_bits(code, s, b):
    k, g0, g1 = CODES[code]
    window = ((b & 1) << (k - 1)) | (s & ((1 << (k - 1)) - 1))
    return _parity(window & g0), _parity(window & g1)


def next_state(code, s, b):
    return (s >> 1) | ((b & 1) << (reg_bits(code) - 1))


def conv_encode_mother(code, bits):
    """conv_encode_code: [g0_0, g1_0, g0_1, g1_1, ...] from a zero register."""
    out, state = [], 0
    for b in bits:
        c0, c1 = branch_bits(code, state, int(b))
        out += [c0, c1]
        state = next_state(code, state, int(b))
    return np.array(out, np.uint8)


def puncture(coded, rate):
    g0, g1 = MATRICES[rate]
    out = []
    for t in range(len(coded) // 2):
        col = t % len(g0)
        if g0[col]:
            out.append(coded[2 * t])
        if g1[col]:
            out.append(coded[2 * t + 1])
    return np.array(out, np.uint8)


def conv_encode_punctured(code, info, rate):
    padded = list(np.asarray(info, np.uint8) & 1) + [0] * reg_bits(code)
    return puncture(conv_encode_mother(code, padded), rate)


def punctured_coded_len(code, info_bits, rate):
    g0, g1 = MATRICES[rate]
    n_steps = info_bits + reg_bits(code)
    full, rem = divmod(n_steps, len(g0))
    return full * (sum(g0) + sum(g1)) + sum(g0[c] + g1[c] for c in range(rem))


@functools.lru_cache(maxsize=None)
def _table(code):
    n = 1 << reg_bits(code)
    return [[((c0 << 1) | c1, next_state(code, s, b)) for b in range(2) for c0, c1 in [branch_bits(code, s, b)]]
            for s in range(n)]


def viterbi_decode_soft(code, llr, info_bits, rate):
    """viterbi_decode_soft_with, conv.rs:304-398."""
    llr = np.asarray(llr, F32)
    rb = reg_bits(code)
    n_steps, num_states = info_bits + rb, 1 << rb
    g0, g1 = MATRICES[rate]
    full = np.zeros(2 * n_steps, F32)
    src = 0
    for t in range(n_steps):
        col = t % len(g0)
        for j, g in enumerate((g0, g1)):
            if g[col]:
                if src < len(llr):
                    full[2 * t + j] = llr[src]
                src += 1
    neg_inf = F32(np.finfo(F32).min) / F32(2.0)
    table = _table(code)
    pm = [neg_inf] * num_states
    pm[0] = F32(0.0)
    prev_state = np.zeros((n_steps, num_states), np.int64)
    with np.errstate(all="ignore"):
        for t in range(n_steps):
            l0, l1 = full[2 * t], full[2 * t + 1]
            corr = (l0 + l1, l0 - l1, -l0 + l1, -l0 - l1)
            new_pm = [neg_inf] * num_states
            row = prev_state[t]
            for prev in range(num_states):
                pm_prev = pm[prev]
                if pm_prev <= neg_inf:
                    continue
                for sym, ns in table[prev]:
                    cand = pm_prev + corr[sym]
                    if cand > new_pm[ns]:
                        new_pm[ns] = cand
                        row[ns] = prev
            pm = new_pm
    state = 0
    bits = np.zeros(n_steps, np.uint8)
    for t in range(n_steps - 1, -1, -1):
        bits[t] = (state >> (rb - 1)) & 1
        state = int(prev_state[t, state])
    return bits[:info_bits]


def interleave(rows, cols, x):
    x = np.asarray(x)
    out = np.empty_like(x)
    for r in range(rows):
        for c in range(cols):
            out[c * rows + r] = x[r * cols + c]
    return out


def deinterleave(rows, cols, x):
    x = np.asarray(x)
    out = np.empty_like(x)
    for r in range(rows):
        for c in range(cols):
            out[r * cols + c] = x[c * rows + r]
    return out


def interleave_bits(rows, cols, bits):
    bits = np.asarray(bits, np.uint8)
    block = rows * cols
    out = []
    for at in range(0, len(bits), block):
        padded = np.zeros(block, np.uint8)
        chunk = bits[at:at + block]
        padded[:len(chunk)] = chunk
        out.append(interleave(rows, cols, padded))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def deinterleave_llrs(rows, cols, llr):
    llr = np.asarray(llr, F32)
    block = rows * cols
    out = []
    for at in range(0, len(llr), block):
        chunk = llr[at:at + block]
        out.append(chunk.copy() if len(chunk) < block else deinterleave(rows, cols, chunk))
    return np.concatenate(out) if out else np.zeros(0, F32)


# ---- the inputs the CPU and GPU tests share ------------------------------------------------
INPUT_KINDS = ("clean", "noisy", "zeros", "short", "huge")


@functools.lru_cache(maxsize=None)
def frame(code, rate, info_bits, seed=0):
    """(info bits, coded bits) of one seeded frame."""
    rng = np.random.default_rng([CODES[code][0], RATES.index(rate), info_bits, seed])
    info = rng.integers(0, 2, info_bits).astype(np.uint8)
    coded = conv_encode_punctured(code, info, rate)
    info.setflags(write=False)
    coded.setflags(write=False)
    return info, coded


def noisy_llrs(coded, seed):
    """+-1 from the coded bits plus Gaussian noise of deviation 1, rounded to half-integers:
    equal path metrics (ties) occur."""
    rng = np.random.default_rng([7, seed])
    x = 1.0 - 2.0 * np.asarray(coded, np.float64) + rng.normal(0.0, 1.0, len(coded))
    return (np.round(x * 2.0) / 2.0).astype(F32)


def llr_input(kind, coded, seed=0):
    """The decode inputs: clean +-4; noisy half-integers; all zeros; the noisy input cut to
    half the coded length; the noisy input scaled by 1e38 (metrics overflow to +-inf, NaN)."""
    if kind == "clean":
        return (4.0 - 8.0 * np.asarray(coded, np.float32)).astype(F32)
    if kind == "zeros":
        return np.zeros(len(coded), F32)
    x = noisy_llrs(coded, seed)
    if kind == "noisy":
        return x
    if kind == "short":
        return x[:len(coded) // 2].copy()
    if kind == "huge":
        with np.errstate(over="ignore"):
            return (x * F32(1e38)).astype(F32)
    raise ValueError(kind)
