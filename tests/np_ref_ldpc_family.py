"""A numpy restatement of the reference's inner LDPC family, written from the behaviour of
src/fec/ldpc_codes.rs independently of csrc/ldpc_family.cpp and vectorised over words: what
tests/test_ldpc_family_oracle.py holds the library's host layer to, equal in every output.
numpy's elementwise float32 arithmetic is one IEEE rounding per operation, as the reference's
is, so equality is the standard.

The decoder also reports, per word, the iteration whose decision became the best snapshot (0:
the initial decision), which names the word's path:
  valid      the initial decision is a codeword (0 iterations)
  decoded    unsat reached 0 in iterations >= 1
  failed     max_iter iterations, unsat > 0
  stale      failed, and the best snapshot is not the last iteration's decision
"""
import numpy as np

F = np.float32
CODES = {"n512r12": (512, 256, 0x4C44504335313200), "n576r23": (576, 384, 0x4C44504335313201),
         "n512r34": (512, 384, 0x4C44504335313202)}
NAMES = list(CODES)
COL_WEIGHT = 3
MASK64 = (1 << 64) - 1
SIGMAS = (0.3, 0.5, 0.6, 0.7, 0.9)
WORDS = 24
SEED = 31
RULES = ("sum_product", "min_sum", ("scaled_min_sum", 0.75))


class Graph:
    """The code's Tanner graph. A-block: each message column taps three rows; a row is picked
    as the least-loaded one, scanning from a pseudo-random offset, among those that are not in
    the column yet and share no row pair with an earlier column; the staircase follows."""

    def __init__(self, name):
        self.name = name
        self.n, self.k, seed = CODES[name]
        self.m = m = self.n - self.k
        load = np.zeros(m, np.int64)
        used = np.zeros((m, m), bool)  # symmetric: this pair of rows already shares a column
        state = seed
        self.relaxed = 0
        col_rows = []
        for _ in range(self.k):
            rows = []
            while len(rows) < COL_WEIGHT:
                state ^= (state << 13) & MASK64
                state ^= state >> 7
                state ^= (state << 17) & MASK64
                order = (state % m + np.arange(m)) % m
                free = np.ones(m, bool)
                free[rows] = False
                ok = free.copy()
                for q in rows:
                    ok &= ~used[q]
                cand = order[ok[order]]
                if cand.size:
                    rows.append(int(cand[np.argmin(load[cand])]))  # the first of the least loaded
                else:
                    self.relaxed += 1
                    rows.append(int(order[free[order]][0]))
            for a in rows:
                load[a] += 1
                for b in rows:
                    if a != b:
                        used[a, b] = True
            col_rows.append(sorted(rows))
        self.col_rows = np.array(col_rows)
        checks = [[] for _ in range(m)]
        for col, rows in enumerate(col_rows):
            for r in rows:
                checks[r].append(col)
        for i in range(m):
            checks[i].append(self.k + i)
            if i > 0:
                checks[i].append(self.k + i - 1)
        self.check_start = np.cumsum([0] + [len(c) for c in checks]).astype(np.uint32)
        self.check_bits = np.concatenate(checks).astype(np.uint32)
        self.n_edges = int(self.check_bits.size)
        self.degrees = np.diff(self.check_start.astype(np.int64))
        self.max_deg = int(self.degrees.max())
        # bit -> (check, edge), checks ascending: the edge list sorted by (bit, check)
        edge_check = np.repeat(np.arange(m), self.degrees)
        order = np.lexsort((edge_check, self.check_bits))
        self.bit_edges = order.astype(np.uint32)
        self.bit_checks = edge_check[order].astype(np.uint32)
        self.bit_degrees = np.bincount(self.check_bits, minlength=self.n)
        self.bit_start = np.cumsum(np.concatenate([[0], self.bit_degrees])).astype(np.uint32)
        # padded tables for the vectorised decoder
        D = self.max_deg
        self.c_idx = np.zeros((m, D), np.int64)
        self.c_on = np.zeros((m, D), bool)
        for c in range(m):
            d = int(self.degrees[c])
            self.c_idx[c, :d] = self.check_start[c] + np.arange(d)
            self.c_on[c, :d] = True
        self.b_idx = np.zeros((self.n, 3), np.int64)
        self.b_on = np.zeros((self.n, 3), bool)
        for b in range(self.n):
            d = int(self.bit_degrees[b])
            self.b_idx[b, :d] = self.bit_edges[self.bit_start[b]:self.bit_start[b] + d]
            self.b_on[b, :d] = True

    def encode(self, msgs):
        """(W, K) uint8 -> (W, N): the message as it is, then p_i = s_i ^ p_(i-1), s the row
        sums of bit 0 of the message over the A block."""
        msgs = np.atleast_2d(msgs)
        bit = (msgs & 1).astype(np.int64)
        s = np.zeros((len(msgs), self.m), np.int64)
        for j in range(COL_WEIGHT):
            np.add.at(s, (slice(None), self.col_rows[:, j]), bit)
        parity = np.cumsum(s & 1, axis=1) & 1
        return np.concatenate([msgs, parity.astype(np.uint8)], axis=1)

    def syndrome_weight(self, hard):
        """(W, N) -> (W,): checks whose bits (bit 0 of each element) have odd parity."""
        h = (np.atleast_2d(hard) & 1).astype(np.int64)
        per_edge = h[:, self.check_bits.astype(np.int64)]
        sums = np.add.reduceat(per_edge, self.check_start[:-1].astype(np.int64), axis=1)
        return (sums & 1).sum(axis=1)


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = Graph(name)
    return _GRAPHS[name]


def fast_tanh(x):
    x2 = x * x
    a = x * (F(945.0) + x2 * (F(105.0) + x2))
    b = F(945.0) + x2 * (F(420.0) + x2 * F(15.0))
    with np.errstate(all="ignore"):
        y = a / b
    return np.where(x < F(-4.97), F(-1.0), np.where(x > F(4.97), F(1.0), y)).astype(F)


def fast_atanh(x):
    x2 = x * x
    a = x * (F(945.0) + x2 * (F(-735.0) + x2 * F(64.0)))
    b = F(945.0) + x2 * (F(-1050.0) + x2 * F(225.0))
    with np.errstate(all="ignore"):
        return (a / b).astype(F)


def _check_update(g, msg, rule):
    """(W, E) bit -> check messages -> (W, E) check -> bit messages."""
    W = len(msg)
    D = g.max_deg
    out = np.zeros_like(msg)
    if rule == "sum_product":
        th = np.where(g.c_on[None], fast_tanh(msg / F(2.0))[:, g.c_idx], F(1.0)).astype(F)  # (W, M, D)
        for i1 in range(D):
            prod = np.ones((W, g.m), F)
            for i2 in range(D):
                if i2 != i1:
                    prod = prod * th[:, :, i2]  # a slot past the degree holds 1.0: x * 1.0 is x
            prod = np.where(prod < F(-1.0), F(-1.0), np.where(prod > F(1.0), F(1.0), prod)).astype(F)  # NaN passes
            e = F(2.0) * fast_atanh(prod)
            on = g.c_on[:, i1]
            out[:, g.c_idx[on, i1]] = e[:, on]
        return out
    scale = F(rule[1]) if isinstance(rule, tuple) else F(1.0)
    v = msg[:, g.c_idx]  # (W, M, D)
    min1 = np.full((W, g.m), np.inf, F)
    min2 = np.full((W, g.m), np.inf, F)
    argmin = np.zeros((W, g.m), np.int64)
    parity = np.ones((W, g.m), F)
    for j in range(D):
        on = g.c_on[None, :, j]
        vj = v[:, :, j]
        parity = np.where(on & (vj < 0), -parity, parity)
        a = np.abs(vj)
        first = on & (a < min1)
        second = on & ~first & (a < min2)
        min2 = np.where(first, min1, np.where(second, a, min2))
        argmin = np.where(first, j, argmin)
        min1 = np.where(first, a, min1)
    for i1 in range(D):
        s_other = np.where(v[:, :, i1] < 0, -parity, parity).astype(F)
        mag = np.where(argmin == i1, min2, min1).astype(F)
        with np.errstate(all="ignore"):
            e = ((scale * s_other) * mag).astype(F)
        on = g.c_on[:, i1]
        out[:, g.c_idx[on, i1]] = e[:, on]
    return out


def decode(name, llr, max_iter=50, rule="sum_product"):
    """(W, N) float32 -> bits (W, K) uint8, unsat (W,), iterations (W,), best_iter (W,) int32."""
    g = graph(name)
    llr = np.ascontiguousarray(np.atleast_2d(llr), F)
    W = len(llr)
    hard = (llr <= 0).astype(np.uint8)
    unsat = g.syndrome_weight(hard)
    best = hard.copy()
    min_unsat = unsat.copy()
    iters = np.zeros(W, np.int64)
    best_iter = np.zeros(W, np.int64)
    live = np.flatnonzero(unsat != 0)
    msg = llr[live][:, g.check_bits.astype(np.int64)]
    for it in range(1, max_iter + 1):
        if live.size == 0:
            break
        L = llr[live]
        with np.errstate(all="ignore"):
            ext = _check_update(g, msg, rule)
            e = np.where(g.b_on[None], ext[:, g.b_idx], F(0.0)).astype(F)  # (w, N, 3)
            dec = L + e[:, :, 0]
            dec = np.where(g.b_on[None, :, 1], dec + e[:, :, 1], dec)
            dec = np.where(g.b_on[None, :, 2], dec + e[:, :, 2], dec)
            total = e[:, :, 0]
            total = np.where(g.b_on[None, :, 1], total + e[:, :, 1], total)
            total = np.where(g.b_on[None, :, 2], total + e[:, :, 2], total)
            total = (L + total).astype(F)
        h = (dec <= 0).astype(np.uint8)
        u = g.syndrome_weight(h)
        iters[live] = it
        better = u < min_unsat[live]
        idx = live[better]
        min_unsat[idx] = u[better]
        best[idx] = h[better]
        best_iter[idx] = it
        with np.errstate(all="ignore"):
            new = np.zeros_like(msg)
            for j in range(3):
                on = g.b_on[:, j]
                new[:, g.b_idx[on, j]] = (total[:, on] - e[:, on, j]).astype(F)
        keep = u != 0
        live, msg = live[keep], new[keep]
    return best[:, :g.k].copy(), min_unsat.astype(np.int32), iters.astype(np.int32), best_iter.astype(np.int32)


def path(unsat, iters, best_iter, max_iter=50):
    if iters == 0 and unsat == 0:
        return "valid"
    if unsat == 0:
        return "decoded"
    return "stale" if best_iter != iters else "failed"


# ---- the input set --------------------------------------------------------------------------
def noisy_words(name, si, nwords=WORDS, seed=SEED):
    """(messages, codewords, llr): random messages as BPSK (bit 0 -> +1) plus Gaussian noise of
    SIGMAS[si], llr = 2 y / sigma^2 in float32."""
    g = graph(name)
    rng = np.random.default_rng([seed, NAMES.index(name), si])
    msgs = rng.integers(0, 2, (nwords, g.k), dtype=np.uint8)
    cws = g.encode(msgs)
    sigma = SIGMAS[si]
    y = (1.0 - 2.0 * cws) + sigma * rng.standard_normal(cws.shape)
    return msgs, cws, (2.0 * y / sigma ** 2).astype(F)


def special_words(name):
    """All-zero LLRs; a decodable word with NaN in three places; with +inf and -inf; with 1e30s."""
    g = graph(name)
    _, _, llr = noisy_words(name, 2, 4, SEED + 1)
    out = [np.zeros(g.n, F)]
    a = llr[0].copy()
    a[[3, g.k - 1, g.n - 2]] = np.nan
    b = llr[1].copy()
    b[[0, 77]] = np.inf
    b[[5, g.k + 9]] = -np.inf
    c = llr[2].copy()
    c[::7] = F(1e30)
    c[3::11] = F(-1e30)
    d = llr[3].copy()
    d[:] = np.where(d > 0, F(np.inf), F(-np.inf))  # a codeword at full confidence, but for the noise's flips
    return np.array(out + [a, b, c, d], F)


def input_set(name):
    """Every LLR word of the code's oracle set, (W, N) float32."""
    return np.concatenate([noisy_words(name, si)[2] for si in range(len(SIGMAS))] + [special_words(name)])
