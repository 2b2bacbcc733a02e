"""A numpy / plain Python restatement of the reference's outer BCH code, written from the
behaviour of src/fec/bch.rs independently of csrc/bch.cpp: what tests/test_bch_oracle.py holds
the library's host layer to, byte for byte. The field is np_ref_rs's.

The decoder also says which way a word went:
  clean    all syndromes zero
  fixed    flipped at most t bits and the residual syndromes are zero (a miscorrection when
           the message is not the one sent)
  resid    the residual syndromes are not all zero
  count    the residual is zero but more than t roots were applied
and whether a root fell below the shortening offset (never applied, never counted), and how
many entries the locator vector had.
"""
import numpy as np

from np_ref_rs import EXP, LOG, gf_inv, gf_mul

# (n, t, errors): the frame's code on both sides of t, the perfect code of t = 1 (two errors
# always miscorrect), shortened codes, a long locator, the shortest legal word, and the largest
# t of the device on both sides of it, full length and shortened: all 62 syndromes live (the
# last packed word half used) and a locator that reaches lane 32 and beyond
ROWS = [(184, 8, 0), (184, 8, 1), (184, 8, 4), (184, 8, 8), (184, 8, 9), (184, 8, 12), (255, 1, 2), (255, 2, 2),
        (255, 2, 3), (128, 3, 3), (128, 3, 4), (255, 16, 16), (255, 16, 17), (9, 1, 0), (9, 1, 1), (9, 1, 2),
        (255, 31, 31), (255, 31, 32), (207, 31, 31), (207, 31, 33)]
SEED = 41
WORDS = 26  # no multiple of the kernel's four words per workgroup


def generator(t):
    """g(x), highest degree first: the product of (x + 2^e) over the union of the conjugacy
    classes of 2^1 .. 2^(2t)."""
    if t < 1:
        raise ValueError("t = 0")
    if t > 127:
        raise ValueError("t too large")
    roots = set()
    for i in range(1, 2 * t + 1):
        e = i % 255
        while e not in roots:
            roots.add(e)
            e = e * 2 % 255
    g = [1]  # low degree first
    for e in sorted(roots):
        a = int(EXP[e])
        out = [0] * (len(g) + 1)
        for d, c in enumerate(g):
            out[d + 1] ^= c
            out[d] ^= gf_mul(c, a)
        g = out
    if len(g) > 255:
        raise ValueError("t too large")
    assert all(c in (0, 1) for c in g) and g[-1] == 1
    return np.array(g[::-1], np.uint8)


def dims(n, t):
    """(k, parity bits); raises ValueError as the reference's constructor fails."""
    if n < 1 or n > 255:
        raise ValueError("bad length")
    pb = len(generator(t)) - 1
    if pb >= n:
        raise ValueError("bad length")
    return n - pb, pb


def encode(n, t, msgs):
    """(W, k) -> (W, n): the message as it is, then the remainder of (bit 0 of the message)
    x^parity by g(x), by long division over all words at once."""
    msgs = np.atleast_2d(msgs)
    k, pb = dims(n, t)
    g = generator(t).astype(np.uint8)
    work = np.concatenate([msgs & 1, np.zeros((len(msgs), pb), np.uint8)], axis=1)
    for p in range(k):
        lead = work[:, p].astype(bool)
        work[lead, p:p + pb + 1] ^= g
    return np.concatenate([msgs, work[:, k:]], axis=1)


def _syndromes(n, t, words):
    """(W, n) -> (W, 2t): S_j = sum over set elements of 2^(j * degree), degree 254 - p."""
    deg = 254 - np.arange(n)
    tab = EXP[(np.arange(1, 2 * t + 1)[:, None] * deg[None]) % 255]  # (2t, n)
    return np.bitwise_xor.reduce(np.where((words != 0)[:, None, :], tab[None], 0), axis=2)


def _locator(s, t):
    """Berlekamp-Massey on S_1 .. S_2t (s[0] is S_1): the locator vector, low degree first,
    grown exactly as the reference grows it."""
    sigma, b, l, m = [1], [1], 0, 1

    def add_shifted(sig, b, coef, shift):
        sig = sig + [0] * max(0, len(b) + shift - len(sig))
        for i, bi in enumerate(b):
            if bi:
                sig[i + shift] ^= gf_mul(coef, bi)
        return sig

    for n in range(1, 2 * t + 1):
        delta = int(s[n - 1])
        for i in range(1, l + 1):
            if i < len(sigma):
                delta ^= gf_mul(sigma[i], int(s[n - 1 - i]))
        if delta == 0:
            m += 1
        elif 2 * l < n:
            old = list(sigma)
            sigma = add_shifted(sigma, b, delta, m)
            l = n - l
            inv = gf_inv(delta)
            b = [gf_mul(c, inv) for c in old]
            m = 1
        else:
            sigma = add_shifted(sigma, b, delta, m)
            m += 1
    return sigma


def decode(n, t, words):
    """(W, n) -> msgs (W, k), status (W,) int32, and per word a dict path / outside /
    locator_len."""
    words = np.atleast_2d(words)
    k, _ = dims(n, t)
    shift = 255 - n
    syn = _syndromes(n, t, words)
    msgs = words[:, :k].copy()
    status = np.zeros(len(words), np.int32)
    info = []
    for w, word in enumerate(words):
        if not syn[w].any():
            info.append({"path": "clean", "outside": False, "locator_len": 0})
            continue
        sigma = _locator(syn[w], t)
        # sigma at 2^-d for every degree d
        d = np.arange(255)
        val = np.zeros(255, np.int64)
        for i, c in enumerate(sigma):
            if c:
                val ^= EXP[(int(LOG[c]) + i * ((255 - d) % 255)) % 255]
        roots = np.flatnonzero(val == 0)
        applied = roots[roots >= shift]
        fixed = word.copy()
        fixed[254 - applied] ^= 1
        residual = int(np.count_nonzero(_syndromes(n, t, fixed[None])[0]))
        n_found = int(applied.size)
        rec = {"outside": bool((roots < shift).any()), "locator_len": len(sigma)}
        if residual != 0 or n_found > t:
            status[w] = -max(residual, n_found)
            rec["path"] = "resid" if residual else "count"
        else:
            status[w] = n_found
            msgs[w] = fixed[:k]
            rec["path"] = "fixed"
        info.append(rec)
    return msgs, status, info


def make_words(n, t, errors, nwords=WORDS, seed=SEED):
    """(sent messages, received words). Errors are 1 -> 0 and 0 -> 1 flips at distinct places.
    Every second word carries other nonzero byte values on set elements (still set); every
    fifth word with errors has one of its 0 -> 1 errors arrive as 2 (set, and ^= 1 leaves it
    set: the residual check must reject it)."""
    k, _ = dims(n, t)
    rng = np.random.default_rng([seed, n, t, errors])
    msgs = rng.integers(0, 2, (nwords, k), dtype=np.uint8)
    words = encode(n, t, msgs)
    for w in range(nwords):
        pos = rng.choice(n, min(errors, n), replace=False)
        words[w, pos] ^= 1
        if w % 5 == 4 and errors:
            zero_to_one = [p for p in pos if words[w, p] == 1]
            if zero_to_one:
                words[w, zero_to_one[0]] = 2
        if w % 2:
            sel = (words[w] == 1) & (rng.random(n) < 0.3)
            sel[pos] = False  # an error position keeps its value
            words[w, sel] = rng.integers(2, 256, int(sel.sum()), dtype=np.uint8)
    return msgs, words
