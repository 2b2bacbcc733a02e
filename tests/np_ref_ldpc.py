"""TEST INFRASTRUCTURE — numpy float32 restatement of the reference's FT8 / FT4 channel
codec (src/codec/ldpc.rs, crc.rs, ft8.rs, ft4.rs, gray.rs) in the reference's own
operation order, plus the deterministic codeword batches the LDPC tests share.

Two restatements of ldpc_decode_soft, as elsewhere in this suite: `decode_batch`,
vectorised over a batch of codewords, and `decode_scalar`, which follows ldpc.rs:673-757
loop for loop (m[check][bit] and e[check][bit] arrays, the 1-based padded NM / MN tables).
Both take the check rule and return (plain, errors, iterations); test_ldpc_oracle.py holds
them to each other and to the library's host decoder bit for bit. `decode_batch` also takes
operation variants (np_ref_ldpc_family.VARIANTS: one-line departures that stand in for a
drifting device build; the default is the reference), and `knife_set` gives the words on
which such a departure changes an output.

The check rule: "reference" is ldpc.rs as written, e = -2 fast_atanh(a) for every check.
"sum_product" is e = +2 fast_atanh(a) for the checks with 7 entries and nothing else
changed (with LLR > 0 meaning 0 and tanh(-m / 2), a check with an even
number of other entries needs the opposite sign).

The parity-check matrix is stated here in the published form (WSJT-X, ft8_lib): one line
per check, the 1-based codeword bits it joins, in the published order. The library states
it as a 0-based edge list; orion_ldpc_tables is held to this statement.
"""
import functools

import numpy as np

import np_ref_ldpc_family as F

f32 = np.float32
N, K, M = 174, 91, 83
RULES = ("reference", "sum_product")
PROTOCOLS = ("ft8", "ft4")
FT4_XOR = bytes([0x4A, 0x5E, 0x89, 0xB4, 0xB0, 0x8A, 0x79, 0x55, 0xBE, 0x28])  # ft4.rs:22
GRAY = {"ft8": [0, 1, 3, 2, 5, 6, 4, 7], "ft4": [0, 1, 3, 2]}  # gray.rs:10,28
BITS = {"ft8": 3, "ft4": 2}

H_ROWS = """\
4 31 59 91 92 96 153
5 32 60 93 115 146
6 24 61 94 122 151
7 33 62 95 96 143
8 25 63 83 93 96 148
6 32 64 97 126 138
5 34 65 78 98 107 154
9 35 66 99 139 146
10 36 67 100 107 126
11 37 67 87 101 139 158
12 38 68 102 105 155
13 39 69 103 149 162
8 40 70 82 104 114 145
14 41 71 88 102 123 156
15 42 59 106 123 159
1 33 72 106 107 157
16 43 73 108 141 160
17 37 74 81 109 131 154
11 44 75 110 121 166
45 55 64 111 130 161 173
8 46 71 112 119 166
18 36 76 89 113 114 143
19 38 77 104 116 163
20 47 70 92 138 165
2 48 74 113 128 160
21 45 78 83 117 121 151
22 47 58 118 127 164
16 39 62 112 134 158
23 43 79 120 131 145
19 35 59 73 110 125 161
20 36 63 94 136 161
14 31 79 98 132 164
3 44 80 124 127 169
19 46 81 117 135 167
7 49 58 90 100 105 168
12 50 61 118 119 144
13 51 64 114 118 157
24 52 76 129 148 149
25 53 69 90 101 130 156
20 46 65 80 120 140 170
21 54 77 100 140 171
35 82 133 142 171 174
14 30 83 113 125 170
4 29 68 120 134 173
1 4 52 57 86 136 152
26 51 56 91 122 137 168
52 84 110 115 145 168
7 50 81 99 132 173
23 55 67 95 172 174
26 41 77 109 141 148
2 27 41 61 62 115 133
27 40 56 124 125 126
18 49 55 124 141 167
6 33 85 108 116 156
28 48 70 85 105 129 158
9 54 63 131 147 155
22 53 68 109 121 174
3 13 48 78 95 123
31 69 133 150 155 169
12 43 66 89 97 135 159
5 39 75 102 136 167
2 54 86 101 135 164
15 56 87 108 119 171
10 44 82 91 111 144 149
23 34 71 94 127 153
11 49 88 92 142 157
29 34 87 97 147 162
30 50 60 86 137 142 162
10 53 66 84 112 128 165
22 57 85 93 140 159
28 32 72 103 132 166
28 29 84 88 117 143 150
1 26 45 80 128 147
17 27 89 103 116 153
51 57 98 163 165 172
21 37 73 138 152 169
16 47 76 130 137 154
3 24 30 72 104 139
9 40 90 106 134 151
15 58 60 74 111 150 163
18 42 79 144 146 152
25 38 65 99 122 160
17 42 75 129 170 172
"""


# ------------------------------------------------------------------- tables --
@functools.lru_cache(maxsize=None)
def tables():
    """dict: nm (83, 7) 1-based and 0-padded, num_rows (83,), mn (174, 3) 1-based in
    ascending check order, h (83, 174) 0/1, generator (83, 12) bit-packed MSB first,
    edges (522, 2) 0-based [check, bit] in check-major order, row_start (84,)."""
    rows = [[int(v) for v in line.split()] for line in H_ROWS.strip().splitlines()]
    assert len(rows) == M
    nm = np.zeros((M, 7), np.int64)
    for j, r in enumerate(rows):
        nm[j, :len(r)] = r
    num_rows = np.array([len(r) for r in rows], np.int64)
    h = np.zeros((M, N), np.uint8)
    for j, r in enumerate(rows):
        for b in r:
            h[j, b - 1] = 1
    mn = np.array([[j + 1 for j in range(M) if h[j, i]] for i in range(N)], np.int64)  # ascending checks
    # the generator: eliminate the last 83 columns of H = [Hm | Hp] to the identity over
    # GF(2); the first 91 columns are then Hp^-1 Hm
    a = h.copy()
    for r in range(M):
        c = K + r
        piv = r + int(np.flatnonzero(a[r:, c])[0])
        if piv != r:
            a[[r, piv]] = a[[piv, r]]
        for j in np.flatnonzero(a[:, c]):
            if j != r:
                a[j] ^= a[r]
    assert (a[:, K:] == np.eye(M, dtype=np.uint8)).all()
    gen = np.packbits(np.concatenate([a[:, :K], np.zeros((M, 5), np.uint8)], axis=1), axis=1)
    edges = np.array([(j, b - 1) for j, r in enumerate(rows) for b in r], np.int64)
    row_start = np.concatenate([[0], np.cumsum(num_rows)])
    return dict(nm=nm, num_rows=num_rows, mn=mn, h=h, generator=gen, edges=edges, row_start=row_start)


# ---------------------------------------------------------------- CRC, encode --
def crc14(message, num_bits):
    """crc.rs:37-54."""
    rem = 0
    idx_byte = 0
    for idx_bit in range(num_bits):
        if idx_bit % 8 == 0:
            rem ^= message[idx_byte] << 6
            idx_byte += 1
        rem = ((rem << 1) ^ 0x2757) if rem & 0x2000 else (rem << 1)
        rem &= 0xFFFF
    return rem & 0x3FFF


def add_crc(payload):
    """crc.rs:61-76: 10-byte payload -> a91 (12 bytes)."""
    a91 = bytearray(payload[:10]) + bytearray(2)
    a91[9] &= 0xF8
    c = crc14(a91, 82)
    a91[9] |= c >> 11
    a91[10] = (c >> 3) & 0xFF
    a91[11] = (c << 5) & 0xFF
    return bytes(a91)


def extract_crc(a91):
    return (a91[9] & 7) << 11 | a91[10] << 3 | a91[11] >> 5


def ldpc_encode(a91):
    """ldpc.rs:593-617 as bits: 174 codeword bits (uint8) of a 12-byte a91."""
    msg = np.unpackbits(np.frombuffer(bytes(a91), np.uint8))[:K]
    g = np.unpackbits(tables()["generator"], axis=1)[:, :K]
    parity = (g.astype(np.int64) @ msg.astype(np.int64)) % 2
    return np.concatenate([msg, parity]).astype(np.uint8)


def codeword_bits(protocol, payload, a91_xor=None):
    """The 174 bits a frame carries (FT4 XORs the payload first, ft4.rs:30-34)."""
    p = bytes(b ^ x for b, x in zip(payload, FT4_XOR)) if protocol == "ft4" else bytes(payload)
    a91 = add_crc(p)
    if a91_xor is not None:
        a91 = bytes(b ^ x for b, x in zip(a91, a91_xor))
    return ldpc_encode(a91)


def encode(protocol, payload, a91_xor=None):
    """Ft8Codec::encode (ft8.rs:29-59) / Ft4Codec::encode (ft4.rs:29-65): Gray-coded tones."""
    bits = codeword_bits(protocol, payload, a91_xor)
    nb = BITS[protocol]
    vals = bits.reshape(-1, nb) @ (1 << np.arange(nb - 1, -1, -1))
    return np.array([GRAY[protocol][v] for v in vals], np.uint8)


def frame_to_llr_hard(protocol, tones):
    """ft8.rs:79-89 / ft4.rs:79-89."""
    nb = BITS[protocol]
    llr = np.zeros(N, f32)
    for s, tone in enumerate(tones):
        b = GRAY[protocol].index(int(tone) & ((1 << nb) - 1))
        for pos in range(nb):
            llr[s * nb + pos] = f32(-10.0) if (b >> (nb - 1 - pos)) & 1 else f32(10.0)
    return llr


def count_errors(plain):
    """ldpc.rs:625-637 for one word or a batch [..., 174]."""
    return ((np.asarray(plain, np.int64) @ tables()["h"].T.astype(np.int64)) % 2).sum(axis=-1)


# ------------------------------------------------------------- scalar decoder --
def _tanh1(x):
    if x < f32(-4.97):
        return f32(-1.0)
    if x > f32(4.97):
        return f32(1.0)
    x2 = x * x
    a = x * (f32(945.0) + x2 * (f32(105.0) + x2))
    b = f32(945.0) + x2 * (f32(420.0) + x2 * f32(15.0))
    return a / b


def _atanh1(x):
    x2 = x * x
    a = x * (f32(945.0) + x2 * (f32(-735.0) + x2 * f32(64.0)))
    b = f32(945.0) + x2 * (f32(-1050.0) + x2 * f32(225.0))
    return a / b


def decode_scalar(llr, max_iter=20, rule="reference"):
    """ldpc.rs:673-757 loop for loop (numpy float32 scalars: every op is one rounding)."""
    t = tables()
    nm, num_rows, mn = t["nm"].tolist(), t["num_rows"].tolist(), t["mn"].tolist()  # lists: plain int indexing
    llr = [f32(v) for v in np.asarray(llr, f32)]
    zero, two = f32(0.0), f32(2.0)
    plain = [int(v <= zero) for v in llr]
    init_errors = int(count_errors(plain))
    if init_errors == 0:
        return np.array(plain, np.uint8), 0, 0
    m = [list(llr) for _ in range(M)]
    e = [[zero] * N for _ in range(M)]
    min_errors, best, iterations = init_errors, list(plain), 0
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            iterations += 1
            for j in range(M):
                nr = int(num_rows[j])
                factor = f32(2.0) if (rule == "sum_product" and nr == 7) else f32(-2.0)
                for ii1 in range(nr):
                    i1 = nm[j][ii1] - 1
                    a = f32(1.0)
                    for ii2 in range(nr):
                        if ii2 != ii1:
                            i2 = nm[j][ii2] - 1
                            a = a * _tanh1(-m[j][i2] / two)
                    e[j][i1] = factor * _atanh1(a)
            for i in range(N):
                l = llr[i]
                for ji in range(3):
                    l = l + e[mn[i][ji] - 1][i]
                plain[i] = int(l <= zero)
            errors = int(count_errors(plain))
            if errors < min_errors:
                min_errors, best = errors, list(plain)
                if errors == 0:
                    break
            for i in range(N):
                for ji1 in range(3):
                    j1 = mn[i][ji1] - 1
                    l = llr[i]
                    for ji2 in range(3):
                        if ji2 != ji1:
                            l = l + e[mn[i][ji2] - 1][i]
                    m[j1][i] = l
    return np.array(best, np.uint8), min_errors, iterations


# ---------------------------------------------------------- vectorised decoder --
def _vtanh(x, variants=()):
    return F.fast_tanh(x, variants)  # the same rational function, ldpc.rs:644-653 = ldpc_codes.rs:560-570


def _vatanh(x):
    x2 = x * x
    a = x * (f32(945.0) + x2 * (f32(-735.0) + x2 * f32(64.0)))
    b = f32(945.0) + x2 * (f32(-1050.0) + x2 * f32(225.0))
    return (a / b).astype(f32)


@functools.lru_cache(maxsize=None)
def _graph():
    """bit_of [522]: the bit of each edge; bit_edge [174, 3]: the edges of each bit in ascending
    check order (the edge list is check-major); starts: per check weight the first edges."""
    t = tables()
    bit_of = t["edges"][:, 1]
    bit_edge = np.array([np.flatnonzero(bit_of == i) for i in range(N)], np.int64)
    starts = {nr: t["row_start"][:-1][t["num_rows"] == nr] for nr in (6, 7)}
    return bit_of, bit_edge, starts


def _iteration(llr, m, rule, variants=()):
    """One iteration on [L, 174] LLRs and [L, 522] bit -> check messages: the check -> bit
    messages per bit (e0, e1, e2, each [L, 174]), the decision sums [L, 174] and the next bit ->
    check messages [L, 522]. variants: np_ref_ldpc_family.VARIANTS, the default is the reference."""
    bit_of, bit_edge, starts = _graph()
    tm = _vtanh(-m / f32(2.0), variants)
    el = np.zeros_like(tm)
    for nr in (6, 7):
        idx = starts[nr][:, None] + np.arange(nr)[None, :]
        factor = f32(2.0) if (rule == "sum_product" and nr == 7) else f32(-2.0)
        tr = tm[:, idx]  # [L, rows, nr]
        for p1 in range(nr):
            a = np.ones(tr.shape[:2], f32)
            for p2 in (range(nr - 1, -1, -1) if "prod_desc" in variants else range(nr)):
                if p2 != p1:
                    a = a * tr[:, :, p2]
            el[:, idx[:, p1]] = factor * _vatanh(a)
    e0, e1, e2 = el[:, bit_edge[:, 0]], el[:, bit_edge[:, 1]], el[:, bit_edge[:, 2]]
    l = ((llr + e0) + e1) + e2
    ml = np.empty_like(tm)
    if "sum_assoc" in variants:
        ml[:, bit_edge[:, 0]] = llr + (e1 + e2)
        ml[:, bit_edge[:, 1]] = llr + (e0 + e2)
        ml[:, bit_edge[:, 2]] = llr + (e0 + e1)
    else:
        ml[:, bit_edge[:, 0]] = (llr + e1) + e2
        ml[:, bit_edge[:, 1]] = (llr + e0) + e2
        ml[:, bit_edge[:, 2]] = (llr + e0) + e1
    return (e0, e1, e2), l, ml


def decode_batch(llr, max_iter=20, rule="reference", variants=()):
    """The same arithmetic per codeword, vectorised over a batch [B, 174] and over the
    checks of equal weight; messages live on the 522 edges. Returns (plain [B, 174] uint8,
    errors [B], iterations [B])."""
    bit_of = _graph()[0]
    llr = np.ascontiguousarray(llr, f32).reshape(-1, N)
    nb = llr.shape[0]
    zero = f32(0.0)
    plain = (llr <= zero).astype(np.uint8)
    errors = count_errors(plain)
    iterations = np.zeros(nb, np.int64)
    live = np.flatnonzero(errors != 0)  # words still iterating
    m = llr[:, bit_of].copy()  # [B, 522]
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            if len(live) == 0:
                break
            iterations[live] += 1
            _, l, ml = _iteration(llr[live], m[live], rule, variants)
            cur = (l <= zero).astype(np.uint8)
            err = count_errors(cur)
            better = err < errors[live]
            idx_b = live[better]
            errors[idx_b] = err[better]
            plain[idx_b] = cur[better]
            m[live] = ml
            live = live[~(better & (err == 0))]
    return plain, errors.astype(np.int64), iterations


def trace(llr, depth, rule="reference", variants=()):
    """Iterations 1 .. depth on every word with no early exit: (errors [depth + 1, B], the
    initial decision's first; (e0, e1, e2) and the decision sums [B, 174] of iteration depth)."""
    llr = np.ascontiguousarray(llr, f32).reshape(-1, N)
    errors = [count_errors((llr <= 0).astype(np.uint8))]
    m = llr[:, _graph()[0]].copy()
    e = l = None
    with np.errstate(all="ignore"):
        for _ in range(depth):
            e, l, m = _iteration(llr, m, rule, variants)
            errors.append(count_errors((l <= 0).astype(np.uint8)))
    return np.array(errors), e, l


# ------------------------------------------------------------------ finisher --
RESULT_FIELDS = ("payload", "status", "iterations", "errors")


def finish(protocol, plain, errors, iterations):
    """ft8.rs:98-129 / ft4.rs:98-127 as the library's record: (payload bytes[10], status,
    iterations, errors); status 0 parity failed, 1 CRC mismatch, 2 decoded; the payload is
    zeros unless decoded."""
    if errors != 0:
        return bytes(10), 0, int(iterations), int(errors)
    a91 = np.packbits(np.concatenate([np.asarray(plain[:K], np.uint8), np.zeros(5, np.uint8)])).tobytes()
    buf = bytearray(a91)
    buf[9] &= 0xF8
    buf[10] = buf[11] = 0
    if extract_crc(a91) != crc14(buf, 82):
        return bytes(10), 1, int(iterations), 0
    p = bytearray(a91[:10])
    if protocol == "ft4":
        p = bytearray(b ^ x for b, x in zip(p, FT4_XOR))
    p[9] &= 0xF8
    return bytes(p), 2, int(iterations), 0


def records(protocol, plain, errors, iterations):
    return [finish(protocol, plain[k], errors[k], iterations[k]) for k in range(len(errors))]


# ------------------------------------------------------------------- batches --
SIGMAS = (0.4, 0.6, 0.8)
WORDS_PER_SIGMA = 32
BATCH_SEED = 2024


def random_payload(rng):
    p = bytearray(rng.integers(0, 256, 10, dtype=np.uint8).tobytes())
    p[9] &= 0xF8
    return bytes(p)


def noisy_llr(bits, sigma, rng):
    """BPSK (0 -> +1, 1 -> -1) plus Gaussian noise, scaled to mean square 24 in f32 as
    normalise_llr leaves its output (ft8_sync.rs:237-246)."""
    x = (1.0 - 2.0 * bits.astype(np.float64)) + sigma * rng.standard_normal(N)
    x = x.astype(f32)
    scale = f32(np.sqrt(f32(24.0) / f32(np.mean(x.astype(np.float64) ** 2))))
    return (x * scale).astype(f32)


@functools.lru_cache(maxsize=None)
def batch(protocol="ft8"):
    """The shared batch: 32 noisy words at each of sigma 0.4 / 0.6 / 0.8, then the edge
    cases. Returns (llr [B, 174] f32 read-only, names: list of labels, payloads)."""
    rng = np.random.default_rng(BATCH_SEED)
    llr, names, payloads = [], [], []
    for sigma in SIGMAS:
        for k in range(WORDS_PER_SIGMA):
            p = random_payload(rng)
            llr.append(noisy_llr(codeword_bits(protocol, p), sigma, rng))
            names.append(f"sigma{sigma}/{k}")
            payloads.append(p)
    p = random_payload(rng)
    clean = np.where(codeword_bits(protocol, p) == 1, f32(-10.0), f32(10.0)).astype(f32)
    # all-zero LLRs: every bit decides 1 (0 <= 0); 24 errors, 20 iterations under both rules
    llr.append(np.zeros(N, f32)); names.append("zeros"); payloads.append(None)
    # +-inf on a valid word
    llr.append(np.where(clean > 0, f32(np.inf), f32(-np.inf)).astype(f32)); names.append("inf"); payloads.append(p)
    # three NaN entries: NaN <= 0 is false, the bits decide 0
    x = clean.copy(); x[[3, 90, 171]] = f32(np.nan)
    llr.append(x); names.append("nan3"); payloads.append(p)
    # one wrong hard bit on otherwise confident words, the bit in a check with 7 entries:
    # the reference rule fails on these, sum_product decodes them
    for k, pos in enumerate((0, 57, 100, 152)):
        x = clean.copy(); x[pos] = -x[pos] * f32(0.3)
        llr.append(x); names.append(f"flip1/{k}"); payloads.append(p)
    # bit 173's three checks have 6 entries each, where the reference's sign is right
    x = clean.copy(); x[173] = -x[173] * f32(0.3)
    llr.append(x); names.append("flip1_w6"); payloads.append(p)
    # parity passes, the CRC does not: one CRC bit of a91 flipped before the LDPC encode
    flip = bytearray(12); flip[10] = 0x10
    bad = codeword_bits(protocol, p, bytes(flip))
    llr.append(np.where(bad == 1, f32(-10.0), f32(10.0)).astype(f32)); names.append("crc_bad"); payloads.append(None)
    # the same with one wrong hard bit: status 1 after iterations under sum_product
    x = llr[-1].copy(); x[20] = -x[20] * f32(0.3)
    llr.append(x); names.append("crc_bad_flip1"); payloads.append(None)
    out = np.array(llr, f32)
    out.setflags(write=False)
    return out, names, payloads


@functools.lru_cache(maxsize=None)
def batch_decoded(protocol, rule, max_iter=20):
    """decode_batch of the shared batch, computed once: (plain, errors, iterations)."""
    plain, errors, iterations = decode_batch(batch(protocol)[0], max_iter, rule)
    for a in (plain, errors, iterations):
        a.setflags(write=False)
    return plain, errors, iterations


# --------------------------------------------------------------- knife-edge words --
# As in np_ref_ldpc_family (which explains them): the LLR of a balanced bit is the largest
# float32 whose decision sum in iteration `depth` is still <= 0, so that bit of `plain`, decoded
# with max_iter = depth, reports the float32 sum of the messages that reach it to the last ulp.
# Any of the 174 bits may be balanced, since plain shows them all.
KNIFE_BITS = 6
KNIFE_SIGMA = 0.5
KNIFE_CASES = tuple((rule, depth) for rule in RULES for depth in (1, 2))
# (protocol, rule, depth) -> the seeds of its knife words, one word per seed: from 1 upwards the
# first six for which the restatement alone meets the conditions of tests/test_ldpc_oracle.py
# (every requested bit holds at depth 1, at least half of them at depth 2). Under the reference
# rule few noisy words lose unsatisfied checks in an iteration, so those seeds are far apart.
KNIFE_SEEDS = {
    ("ft8", "reference", 1): (2, 22, 23, 49, 53, 103), ("ft8", "reference", 2): (11, 70, 79, 147, 169, 212),
    ("ft8", "sum_product", 1): (1, 2, 3, 4, 5, 6), ("ft8", "sum_product", 2): (2, 3, 4, 5, 6, 7),
    ("ft4", "reference", 1): (17, 29, 38, 45, 46, 49), ("ft4", "reference", 2): (85, 88, 140, 183, 188, 274),
    ("ft4", "sum_product", 1): (1, 2, 3, 4, 5, 6), ("ft4", "sum_product", 2): (1, 3, 4, 5, 7, 8),
}


def knife_words(protocol, rule, depth, seed, want=KNIFE_BITS):
    """(word [1, 174] float32, balanced: [the bits that hold], requested: [the bits balanced])."""
    t = tables()
    rng = np.random.default_rng([seed, PROTOCOLS.index(protocol), depth, 78])
    x = noisy_llr(codeword_bits(protocol, random_payload(rng)), KNIFE_SIGMA, rng)
    check_sets = [set((t["mn"][b] - 1).tolist()) for b in range(N)]
    bits = F.pick_disjoint(check_sets, rng.permutation(N), want)
    for i, b in enumerate(bits):
        nbs = [[n - 1 for n in t["nm"][c, :t["num_rows"][c]].tolist() if n - 1 != b] for c in sorted(check_sets[b])]
        F.treat_neighbours(x, nbs, i % 3, i // 3)
    for _ in range(1 if depth == 1 else 8):
        _, (e0, e1, e2), _ = trace(x, depth, rule)
        new = F.balance(e0[0, bits], e1[0, bits], e2[0, bits])
        new = np.where(np.isnan(new), x[bits], new).astype(f32)
        if np.array_equal(new.view(np.uint32), x[bits].view(np.uint32)):
            break
        x[bits] = new
    rows = np.repeat(x[None], 1 + len(bits), axis=0)
    for i, b in enumerate(bits):
        rows[1 + i, b] = np.nextafter(x[b], f32(np.inf))
    errors, _, l = trace(rows, depth, rule)
    return x[None].copy(), [F.hold(errors, l, bits, depth)], [len(bits)]


@functools.lru_cache(maxsize=None)
def knife_set(protocol, rule, depth):
    """The committed knife words of (protocol, rule, depth), read-only: (words [6, 174],
    balanced: per word the bits that hold, requested: per word the number of bits balanced)."""
    parts = [knife_words(protocol, rule, depth, seed) for seed in KNIFE_SEEDS[(protocol, rule, depth)]]
    words = np.concatenate([p[0] for p in parts])
    words.setflags(write=False)
    return words, [p[1][0] for p in parts], [p[2][0] for p in parts]


# -------------------------------------------------------------- encoded frames --
def encoded_frame(protocol, payload, base_idx):
    """The CPFSK samples (np_ref_sync.frame_samples) of a frame that carries payload."""
    import np_ref_sync as S

    mode = S.FT8 if protocol == "ft8" else S.FT4
    return S.frame_samples(mode, encode(protocol, payload).tolist(), base_idx)


def search_buffer(protocol, payload, noise_power, late_syms=None, payload_seed=None, noise_seed=11):
    """An encoded frame in np_ref_sync's search buffer: LATE_SYMS symbols late (or
    late_syms), UP_BINS bins above BASE_HZ, plus complex Gaussian noise of the given power
    from default_rng(noise_seed). Returns complex64 [n]."""
    import np_ref_sync as S

    mode = S.FT8 if protocol == "ft8" else S.FT4
    late = S.LATE_SYMS if late_syms is None else late_syms
    frame = encoded_frame(protocol, payload, (160 if protocol == "ft8" else 48) + S.UP_BINS)
    n = (S.T_MAX - S.T_MIN + mode["total"]) * mode["sps"]
    iq = np.zeros(n, np.complex128)
    iq[late * mode["sps"]:late * mode["sps"] + len(frame)] = frame
    rng = np.random.default_rng(noise_seed)
    iq += np.sqrt(noise_power / 2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return iq.astype(np.complex64)


def frame_payload(seed=7):
    """77 payload bits from default_rng(seed), packed MSB first into 10 bytes."""
    bits = np.random.default_rng(seed).integers(0, 2, 77).astype(np.uint8)
    return np.packbits(np.concatenate([bits, np.zeros(3, np.uint8)])).tobytes()
