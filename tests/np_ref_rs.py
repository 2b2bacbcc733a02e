"""A numpy / plain Python restatement of the reference's outer code, written from
src/fec/{gf,reed_solomon,interleaver,scrambler}.rs, src/waveform/dvb_t.rs:30-110 and
src/waveform/dvb_t_ts.rs, independently of csrc/rs.cpp: what tests/test_rs_oracle.py holds the
library's host layer to, byte for byte.

The decoder also says which way a word went:
  zero           all syndromes zero
  fixed          corrected, the residual syndromes zero
  roots          the number of Chien roots is not the locator's degree
  degt           the locator's degree is above t (whatever the root count)
  deriv          a root at which the locator's derivative vanishes (no input is known to get here)
  resid_outside  a root on a degree that is never transmitted, then the residual check fails
  resid          the residual check fails otherwise
"""
import numpy as np

# ---- GF(2^8), 0x11D, generator 2 (gf.rs) ----------------------------------------------------
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
for _i in range(255, 512):
    EXP[_i] = EXP[_i - 255]


def gf_mul(a, b):
    return 0 if a == 0 or b == 0 else int(EXP[LOG[a] + LOG[b]])


def gf_div(a, b):
    if b == 0:
        raise ZeroDivisionError("GF(2^8) division by zero")
    return 0 if a == 0 else int(EXP[LOG[a] + 255 - LOG[b]])


def gf_inv(a):
    if a == 0:
        raise ZeroDivisionError("GF(2^8) inverse of zero")
    return int(EXP[255 - LOG[a]])


def gf_pow(a, n):
    if a == 0:
        return 1 if n == 0 else 0
    return int(EXP[(int(LOG[a]) * n) % 255])


def gf_exp_of(i):
    return int(EXP[i % 255])


# ---- Reed-Solomon (reed_solomon.rs) ---------------------------------------------------------
def rs_generator(n_parity):
    g = [1]
    for i in range(n_parity):
        root = gf_exp_of(i)
        out = [0] * (len(g) + 1)
        for d, c in enumerate(g):
            out[d + 1] ^= c
            out[d] ^= gf_mul(c, root)
        g = out
    return g


def rs_check(n, n_parity):
    if n == 0 or n > 255 or n_parity >= n:
        raise ValueError("bad length")


def rs_encode(n, n_parity, message):
    rs_check(n, n_parity)
    gen = rs_generator(n_parity)
    reg = [0] * n_parity
    for m in message:
        fb = int(m) ^ reg[0]
        for i in range(n_parity - 1):
            reg[i] = reg[i + 1] ^ gf_mul(fb, gen[n_parity - 1 - i])
        reg[n_parity - 1] = gf_mul(fb, gen[0])
    return np.array(list(message) + reg, np.uint8)


def _syndromes(n, n_parity, word):
    """S_j = sum word[p] (2^j)^(n - 1 - p + 255 - n), as one table lookup per (j, p)."""
    w = np.asarray(word, np.int64)
    deg = n - 1 - np.arange(n) + (255 - n)
    nz = w != 0
    out = []
    for j in range(n_parity):
        terms = EXP[(LOG[w[nz]] + (j * deg[nz]) % 255) % 255]
        out.append(int(np.bitwise_xor.reduce(terms)) if terms.size else 0)
    return out


def _berlekamp_massey(s, t):
    sigma, b, l, m = [1], [1], 0, 1

    def correct(sig, b, coef, shift):
        if len(sig) < len(b) + shift:
            sig = sig + [0] * (len(b) + shift - len(sig))
        for i, bi in enumerate(b):
            if bi:
                sig[i + shift] ^= gf_mul(coef, bi)
        return sig

    for n in range(2 * t):
        delta = s[n]
        for i in range(1, l + 1):
            if i < len(sigma):
                delta ^= gf_mul(sigma[i], s[n - i])
        if delta == 0:
            m += 1
        elif 2 * l <= n:
            t_sigma = list(sigma)
            sigma = correct(list(sigma), b, delta, m)
            l = n + 1 - l
            inv = gf_inv(delta)
            b = [gf_mul(c, inv) for c in t_sigma]
            m = 1
        else:
            sigma = correct(list(sigma), b, delta, m)
            m += 1
    return sigma


def _poly_eval(p, x):
    acc = 0
    for c in reversed(p):
        acc = gf_mul(acc, x) ^ c
    return acc


def rs_decode(n, n_parity, received):
    """decode_counted, reed_solomon.rs:141-233 -> (message, count, path). count is -1 and the
    message received[:k] for an uncorrectable word."""
    rs_check(n, n_parity)
    r = [int(v) for v in received]
    assert len(r) == n
    k, t, shift = n - n_parity, n_parity // 2, 255 - n
    prefix = np.array(r[:k], np.uint8)
    s = _syndromes(n, n_parity, r)
    if not any(s):
        return prefix, 0, "zero"
    sigma = _berlekamp_massey(s, t)
    degrees = []
    for i in range(255):
        x = gf_exp_of((255 - (i % 255)) % 255)
        val = 0
        for d, c in enumerate(sigma):
            if c:
                val ^= gf_mul(c, gf_pow(x, d))
        if val == 0:
            degrees.append(i)
    sigma_deg = max([d for d, c in enumerate(sigma) if c], default=0)
    if len(degrees) != sigma_deg or sigma_deg > t:
        return prefix, -1, "degt" if sigma_deg > t else "roots"
    omega = [0] * n_parity
    for i, si in enumerate(s):
        for j, sj in enumerate(sigma):
            if si and sj and i + j < n_parity:
                omega[i + j] ^= gf_mul(si, sj)
    deriv = [0] if len(sigma) <= 1 else [c if kk % 2 == 1 else 0 for kk, c in enumerate(sigma)][1:]
    corrected = list(r)
    count, outside = 0, False
    for i in degrees:
        x = gf_exp_of(i % 255)
        x_inv = gf_inv(x)
        ov, dv = _poly_eval(omega, x_inv), _poly_eval(deriv, x_inv)
        if dv == 0:
            return prefix, -1, "deriv"
        mag = gf_mul(x, gf_div(ov, dv))
        if shift <= i <= n - 1 + shift:
            p = n - 1 + shift - i
            if p < n and mag != 0:
                corrected[p] ^= mag
                count += 1
        else:
            outside = True
    if any(_syndromes(n, n_parity, corrected)):
        return prefix, -1, "resid_outside" if outside else "resid"
    return np.array(corrected[:k], np.uint8), count, "fixed"


# ---- the Forney interleaver (interleaver.rs:122-305) ----------------------------------------
class ConvInterleaver:
    inverse = False

    def __init__(self, branches, depth):
        assert branches > 0 and depth > 0
        self.branches, self.depth = branches, depth
        self.reset()

    def _cells(self, j):
        return (self.branches - 1 - j if self.inverse else j) * self.depth

    def reset(self):
        self.fifos = [[0] * self._cells(j) for j in range(self.branches)]
        self.pos = 0

    @property
    def roundtrip_delay(self):
        return self.branches * (self.branches - 1) * self.depth

    def feed(self, data):
        out = []
        for b in data:
            j = self.pos % self.branches
            if self._cells(j) == 0:
                out.append(int(b))
            else:
                self.fifos[j].append(int(b))
                out.append(self.fifos[j].pop(0))
            self.pos += 1
        return np.array(out, np.uint8)

    def flush(self):
        return self.feed([0] * self.roundtrip_delay)


class ConvDeinterleaver(ConvInterleaver):
    inverse = True


def bytes_to_bits(b):
    return np.unpackbits(np.asarray(b, np.uint8))  # MSB first


def bits_to_bytes(bits):
    bits = np.asarray(bits, np.uint8) & 1
    assert bits.size % 8 == 0
    return np.packbits(bits)


def frame_interleave(data, branches, depth):
    """interleave_bits' Convolutional arm in bytes, modulate/ofdm_frame.rs:464-478."""
    ci = ConvInterleaver(branches, depth)
    data = list(np.asarray(data, np.uint8))
    data += [0] * (-len(data) % branches)
    return np.concatenate([ci.feed(data), ci.flush()])


def frame_deinterleave(data, branches, depth):
    """deinterleave_bits' Convolutional arm in bytes, demodulate/ofdm_frame.rs:399-415."""
    d = branches * (branches - 1) * depth
    if len(data) <= d:
        return np.zeros(0, np.uint8)
    return ConvDeinterleaver(branches, depth).feed(data)[d:]


# ---- the PN scrambler (scrambler.rs) --------------------------------------------------------
class PnStream:
    def __init__(self, taps, width, seed):
        assert 2 <= width <= 32
        self.mask = (1 << width) - 1
        assert seed != 0 and seed & ~self.mask == 0 and taps & ~self.mask == 0
        self.taps, self.top, self.seed = taps, width - 1, seed
        self.reg = seed

    def reset(self):
        self.reg = self.seed

    def feed(self, data):
        out = []
        for byte in data:
            o = 0
            for bit in range(8):
                pn = self.reg & 1
                o |= (((int(byte) >> bit) & 1) ^ pn) << bit
                fb = bin(self.reg & self.taps).count("1") & 1
                self.reg = ((self.reg >> 1) | (fb << self.top)) & self.mask
            out.append(o)
        return np.array(out, np.uint8)


def pn_scramble(taps, width, seed, data):
    return PnStream(taps, width, seed).feed(data)


# ---- DVB-T energy dispersal and the TS layer (dvb_t.rs:30-110, dvb_t_ts.rs) -----------------
class Dispersal:
    INIT = 0b100_1010_1000_0000

    def __init__(self):
        self.reg = self.INIT

    def reset(self):
        self.reg = self.INIT

    def _bit(self):
        fb = (self.reg ^ (self.reg >> 1)) & 1
        self.reg = (self.reg >> 1) | (fb << 14)
        return fb

    def advance_byte(self):
        for _ in range(8):
            self._bit()

    def feed(self, data):
        out = []
        for byte in data:
            o = 0
            for bit in range(7, -1, -1):
                o |= (((int(byte) >> bit) & 1) ^ self._bit()) << bit
            out.append(o)
        return np.array(out, np.uint8)


def ts_energy_disperse(packets):
    p = np.array(packets, np.uint8)
    assert p.size % 188 == 0
    prbs = Dispersal()
    for i in range(p.size // 188):
        pk = p[i * 188:(i + 1) * 188]
        if i % 8 == 0:
            prbs.reset()
            pk[0] ^= 0x47 ^ 0xB8
        else:
            prbs.advance_byte()
        pk[1:] = prbs.feed(pk[1:])
    return p


def ts_packetize(payload):
    payload = np.asarray(payload, np.uint8)
    n_packets = max(-(-payload.size // 187), 1)
    out = np.zeros(n_packets * 188, np.uint8)
    for p in range(-(-payload.size // 187)):
        chunk = payload[p * 187:(p + 1) * 187]
        out[p * 188] = 0x47
        out[p * 188 + 1:p * 188 + 1 + chunk.size] = chunk
    out[0] = 0x47
    return out


def ts_depacketize(packets):
    packets = np.asarray(packets, np.uint8)
    if packets.size == 0 or packets.size % 188:
        return None
    return packets.reshape(-1, 188)[:, 1:].reshape(-1).copy()


def ts_null_packet():
    p = np.full(188, 0xFF, np.uint8)
    p[:4] = [0x47, 0x1F, 0xFF, 0x10]
    return p


def ts_stuff_null_packets(ts, target_packets):
    ts = np.asarray(ts, np.uint8)
    have = ts.size // 188
    return np.concatenate([ts] + [ts_null_packet()] * max(target_packets - have, 0))


# ---- the input sets of the tests ------------------------------------------------------------
# (n, n_parity, errors per word): the rows tests/test_rs_oracle.py and tests/test_gpu_rs.py run
ROWS = [(204, 16, 0), (204, 16, 1), (204, 16, 8), (204, 16, 9), (255, 32, 16), (255, 32, 17),
        (10, 2, 1), (10, 2, 2), (10, 2, 3), (12, 4, 2), (12, 4, 3), (12, 4, 4), (7, 3, 1), (7, 3, 2),
        (3, 2, 1), (3, 2, 2), (2, 1, 0), (2, 1, 1)]


SEED = 1  # found on the CPU with this restatement: every decoder path and a miscorrection occur


def words_per_row(n):
    return 24 if n >= 204 else 300


def make_words(n, n_parity, n_err, count, seed):
    """count received words of the row: seeded random messages, encoded, n_err distinct
    positions hit with nonzero error values. The first words place their errors at position 0,
    at position n - 1 and in the parity only (where the row leaves room); after them come the
    all-zero word and the all-0xFF word. Returns (sent messages, received words); the sent
    message of the two constant words is their own prefix."""
    rng = np.random.default_rng([seed, n, n_parity, n_err])
    k = n - n_parity
    sent, words = [], []
    for w in range(count):
        msg = rng.integers(0, 256, k, dtype=np.uint8)
        cw = rs_encode(n, n_parity, msg)
        e = min(n_err, n)
        if w == 0 and e >= 1:
            pos = np.concatenate([[0], 1 + rng.choice(n - 1, e - 1, replace=False)])
        elif w == 1 and e >= 1:
            pos = np.concatenate([[n - 1], rng.choice(n - 1, e - 1, replace=False)])
        elif w == 2 and 1 <= e <= n_parity:
            pos = k + rng.choice(n_parity, e, replace=False)
        else:
            pos = rng.choice(n, e, replace=False)
        cw[pos.astype(np.int64)] ^= rng.integers(1, 256, e, dtype=np.uint8)
        sent.append(msg)
        words.append(cw)
    for fill in (0x00, 0xFF):
        words.append(np.full(n, fill, np.uint8))
        sent.append(np.full(k, fill, np.uint8))
    return np.array(sent, np.uint8), np.array(words, np.uint8)
