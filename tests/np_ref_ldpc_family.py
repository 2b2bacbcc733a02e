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


# One-line departures from the reference's operation list, for the tests alone: each stands in
# for a way a device build drifts from a host build, so that the CPU can prove that an input set
# would notice it. The default, no variant, is the reference.
#   fma            the numerator's 945 + x2 * (105 + x2) as one fused step (f64, then rounded)
#   sat_nonstrict  fast_tanh saturates on x <= -4.97 / x >= 4.97 instead of < / >
#   flush          a subnormal argument of fast_tanh reads as zero (of its sign)
#   prod_desc      the leave-one-out product runs from the last entry down
#   sum_assoc      the update sum is ((llr + e0) + e1) + e2 instead of llr + ((e0 + e1) + e2)
VARIANTS = ("fma", "sat_nonstrict", "flush", "prod_desc", "sum_assoc")
TINY = np.finfo(F).tiny  # the smallest normal


def fast_tanh(x, variants=()):
    if "flush" in variants:
        x = np.where(np.abs(x) < TINY, np.copysign(F(0.0), x), x).astype(F)
    x2 = x * x
    inner = F(105.0) + x2
    if "fma" in variants:
        mid = (x2.astype(np.float64) * inner.astype(np.float64) + 945.0).astype(F)
    else:
        mid = F(945.0) + x2 * inner
    a = x * mid
    b = F(945.0) + x2 * (F(420.0) + x2 * F(15.0))
    with np.errstate(all="ignore"):
        y = a / b
    lo, hi = (x <= F(-4.97), x >= F(4.97)) if "sat_nonstrict" in variants else (x < F(-4.97), x > F(4.97))
    return np.where(lo, F(-1.0), np.where(hi, F(1.0), y)).astype(F)


def fast_atanh(x):
    x2 = x * x
    a = x * (F(945.0) + x2 * (F(-735.0) + x2 * F(64.0)))
    b = F(945.0) + x2 * (F(-1050.0) + x2 * F(225.0))
    with np.errstate(all="ignore"):
        return (a / b).astype(F)


def _check_update(g, msg, rule, variants=()):
    """(W, E) bit -> check messages -> (W, E) check -> bit messages."""
    W = len(msg)
    D = g.max_deg
    out = np.zeros_like(msg)
    if rule == "sum_product":
        th = np.where(g.c_on[None], fast_tanh(msg / F(2.0), variants)[:, g.c_idx], F(1.0)).astype(F)  # (W, M, D)
        for i1 in range(D):
            prod = np.ones((W, g.m), F)
            for i2 in (range(D - 1, -1, -1) if "prod_desc" in variants else range(D)):
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


def _iteration(g, L, msg, rule, variants=()):
    """One iteration on (w, N) LLRs and (w, E) bit -> check messages: the check -> bit messages
    per bit e (w, N, 3), the decision sums (w, N) and the next bit -> check messages (w, E)."""
    with np.errstate(all="ignore"):
        ext = _check_update(g, msg, rule, variants)
        e = np.where(g.b_on[None], ext[:, g.b_idx], F(0.0)).astype(F)  # (w, N, 3)
        dec = L + e[:, :, 0]
        dec = np.where(g.b_on[None, :, 1], dec + e[:, :, 1], dec)
        dec = np.where(g.b_on[None, :, 2], dec + e[:, :, 2], dec)
        if "sum_assoc" in variants:
            total = dec
        else:
            total = e[:, :, 0]
            total = np.where(g.b_on[None, :, 1], total + e[:, :, 1], total)
            total = np.where(g.b_on[None, :, 2], total + e[:, :, 2], total)
            total = (L + total).astype(F)
        new = np.zeros_like(msg)
        for j in range(3):
            on = g.b_on[:, j]
            new[:, g.b_idx[on, j]] = (total[:, on] - e[:, on, j]).astype(F)
    return e, dec.astype(F), new


def decode(name, llr, max_iter=50, rule="sum_product", variants=()):
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
        _, dec, new = _iteration(g, llr[live], msg, rule, variants)
        h = (dec <= 0).astype(np.uint8)
        u = g.syndrome_weight(h)
        iters[live] = it
        better = u < min_unsat[live]
        idx = live[better]
        min_unsat[idx] = u[better]
        best[idx] = h[better]
        best_iter[idx] = it
        keep = u != 0
        live, msg = live[keep], new[keep]
    return best[:, :g.k].copy(), min_unsat.astype(np.int32), iters.astype(np.int32), best_iter.astype(np.int32)


def trace(name, llr, depth, rule="sum_product", variants=()):
    """Iterations 1 .. depth on every word with no early exit: (unsat (depth + 1, W), the
    initial decision's first; e (W, N, 3) and the decision sums (W, N) of iteration depth)."""
    g = graph(name)
    llr = np.ascontiguousarray(np.atleast_2d(llr), F)
    unsat = [g.syndrome_weight((llr <= 0).astype(np.uint8))]
    msg = llr[:, g.check_bits.astype(np.int64)]
    e = dec = None
    for _ in range(depth):
        e, dec, msg = _iteration(g, llr, msg, rule, variants)
        unsat.append(g.syndrome_weight((dec <= 0).astype(np.uint8)))
    return np.array(unsat), e, dec


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


# ---- knife-edge words -----------------------------------------------------------------------
# A decoder returns decisions only, and on noisy words a decision does not move when a message is
# off by an ulp. A knife-edge word makes it move: the LLR of a balanced bit b is the largest
# float32 L whose decision sum ((L + e0) + e1) + e2 in iteration `depth` is still <= 0, so bit b
# of the output (decoded with max_iter = depth) reports the float32 sum of the check -> bit
# messages that reach b to the last ulp. The neighbours of the balanced bits (the other bits of
# their checks) are put where fast_tanh changes branch or leaves the normal range.
KNIFE_WORDS = 6
KNIFE_BITS = 24
SAT = F(2.0) * F(4.97)  # an LLR whose half is the saturation bound itself
SAT_VALUES = (np.nextafter(SAT, F(0.0)), SAT, np.nextafter(SAT, F(np.inf)))
SUB_VALUES = (F(1e-40), F(3e-39), F(1.4e-45), TINY, np.nextafter(TINY, F(0.0)))
# (rule, depth) -> per code the seeds of its knife words, one word per seed: from 1 upwards the
# first six for which the restatement alone meets the conditions of test_ldpc_family_oracle.py
# (every requested bit holds at depth 1, at least half of them at depth 2)
KNIFE_CASES = (("sum_product", 1), ("sum_product", 2), ("min_sum", 1), (("scaled_min_sum", 0.75), 1))
KNIFE_SEEDS = {
    ("sum_product", 1): {"n512r12": (1, 2, 3, 4, 5, 6), "n576r23": (1, 2, 3, 4, 5, 6), "n512r34": (1, 2, 3, 4, 5, 6)},
    ("sum_product", 2): {"n512r12": (2, 6, 7, 8, 9, 11), "n576r23": (1, 5, 12, 13, 17, 19),
                         "n512r34": (1, 2, 4, 5, 17, 25)},
    ("min_sum", 1): {"n512r12": (1, 2, 3, 4, 5, 6), "n576r23": (1, 2, 3, 4, 5, 6), "n512r34": (1, 2, 4, 5, 6, 7)},
    ("scaled_min_sum", 1): {"n512r12": (1, 2, 3, 4, 5, 6), "n576r23": (1, 2, 3, 4, 5, 6),
                            "n512r34": (1, 2, 3, 4, 5, 6)},
}


def rule_id(rule):
    return rule if isinstance(rule, str) else rule[0]


def _key(x):
    """float32 -> int64, ordered as the floats are (-0.0 and 0.0 both 0)."""
    i = np.asarray(x, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(F)


def balance(e0, e1, e2):
    """Elementwise the largest finite float32 L with ((L + e0) + e1) + e2 <= 0 (float32 addition
    is monotone in L, so a bisection over the ordered floats finds it); NaN where there is none."""
    e0, e1, e2 = (np.asarray(v, F) for v in (e0, e1, e2))
    big = np.finfo(F).max

    def holds(L):
        with np.errstate(all="ignore"):
            return ((L + e0) + e1) + e2 <= 0

    lo = np.broadcast_to(_key(-big), e0.shape).copy()
    hi = np.broadcast_to(_key(big), e0.shape).copy()
    ok = holds(_unkey(lo)) & ~holds(_unkey(hi))
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        h = holds(_unkey(mid))
        lo, hi = np.where(h, mid, lo), np.where(h, hi, mid)
    return np.where(ok, _unkey(lo), F(np.nan)).astype(F)


def treat_neighbours(x, neighbours, kind, count):
    """Rewrite the LLRs x[neighbours] of one balanced bit, signs kept. kind 0: untouched; 1: on
    the saturation bound and its two float32 neighbours; 2: subnormal (and the smallest normal,
    whose half is subnormal), one neighbour per check when count is even and every other
    neighbour when it is odd. neighbours: a list per check of the bit. In a check with two or
    more subnormal entries the product underflows to zero whatever the arithmetic, so only the
    one-per-check form reports how a subnormal goes through fast_tanh and the divide."""
    j = count
    for c, nb in enumerate(neighbours):
        if kind == 1:
            pick = list(nb)
        elif kind == 2:
            pick = [nb[(count // 2 + c) % len(nb)]] if count % 2 == 0 else list(nb[::2])
        else:
            pick = []
        for n in pick:
            v = (SAT_VALUES[j % 3] if kind == 1 else SUB_VALUES[j % 5])
            x[n] = np.copysign(v, x[n])
            j += 1


def pick_disjoint(check_sets, order, want):
    """Greedily, in the given order, the bits whose checks no chosen bit shares."""
    taken, out = set(), []
    for b in order:
        if len(out) == want:
            break
        if taken.isdisjoint(check_sets[b]):
            taken.update(check_sets[b])
            out.append(int(b))
    return out


def hold(unsat, dec, bits, depth):
    """The balanced bits that hold. Row 0 of the batch is the word; row 1 + i is the word with
    bit bits[i] at the next float32 above. A bit holds when its decision sum in iteration depth
    is <= 0 in the word and > 0 in its own row, and the word's unsatisfied count after
    iteration depth is below every earlier one (none of them 0), so that the snapshot the
    decoder returns is that iteration's."""
    u = unsat[:, 0]
    if not (u[depth] < u[:depth].min() and u[:depth].min() > 0):
        return []
    return [b for i, b in enumerate(bits) if dec[0, b] <= 0 and dec[1 + i, b] > 0]


def knife_words(name, rule, depth, seed, nwords=1, want=KNIFE_BITS):
    """(words (nwords, N) float32, balanced: per word the list of message bits that hold,
    requested: per word the number of bits that were balanced)."""
    g = graph(name)
    _, _, llr = noisy_words(name, 2, nwords, seed)
    rng = np.random.default_rng([seed, NAMES.index(name), depth, 77])
    check_sets = [set(g.bit_checks[g.bit_start[b]:g.bit_start[b + 1]].tolist()) for b in range(g.k)]
    words, balanced, requested = [], [], []
    for w in range(nwords):
        x = llr[w].copy()
        bits = pick_disjoint(check_sets, rng.permutation(g.k), want)
        for i, b in enumerate(bits):
            nbs = []
            for c in sorted(check_sets[b]):
                members = g.check_bits[g.check_start[c]:g.check_start[c + 1]].tolist()
                nbs.append([n for n in members if n != b])
            treat_neighbours(x, nbs, i % 3, i // 3)
        # at depth 1 the messages into b do not depend on any balanced LLR; at depth 2 they do,
        # weakly (through the neighbours' other checks, and through the rounding of total - e),
        # so the balance is repeated until no LLR moves, a few times at the most
        for _ in range(1 if depth == 1 else 8):
            _, e, _ = trace(name, x, depth, rule)
            new = balance(e[0, bits, 0], e[0, bits, 1], e[0, bits, 2])
            new = np.where(np.isnan(new), x[bits], new).astype(F)
            if np.array_equal(new.view(np.uint32), x[bits].view(np.uint32)):
                break
            x[bits] = new
        batch = np.repeat(x[None], 1 + len(bits), axis=0)
        for i, b in enumerate(bits):
            batch[1 + i, b] = np.nextafter(x[b], F(np.inf))
        unsat, _, dec = trace(name, batch, depth, rule)
        words.append(x)
        balanced.append(hold(unsat, dec, bits, depth))
        requested.append(len(bits))
    return np.array(words, F), balanced, requested


_KNIFE_SETS = {}


def knife_set(name, rule, depth):
    """The code's committed knife words for (rule, depth), built once and read-only: (words (6,
    N), balanced: per word the bits that hold, requested: per word the bits that were balanced)."""
    key = (name, rule_id(rule), depth)
    if key not in _KNIFE_SETS:
        parts = [knife_words(name, rule, depth, seed) for seed in KNIFE_SEEDS[key[1:]][name]]
        words = np.concatenate([p[0] for p in parts])
        words.setflags(write=False)
        _KNIFE_SETS[key] = (words, [p[1][0] for p in parts], [p[2][0] for p in parts])
    return _KNIFE_SETS[key]


# ---- exact words for the min-sum rules ------------------------------------------------------
# With integer LLRs of magnitude at most 3 every value the min-sum decoder forms is a small
# integer (with scale 0.5 and at most 8 iterations, a small multiple of 2^-8), exact in float32;
# so an integer decoder written from the definition is a reference that shares no operation list
# with the float32 code.
INT_SIGMAS = (0.5, 0.7, 0.9)
INT_WORDS = 16
INT_SEED = 41
INT_MAX_ITER = 20
HALF_MAX_ITER = 8
HALF_UNIT = 256  # 2^8: scale 0.5 halves once per iteration, 8 iterations


def int_words(name, minus_zero=False):
    """(48, N) float32: rint(2 y) clipped to +-3, y a BPSK codeword plus noise of INT_SIGMAS, 16
    words each; minus_zero: every second zero written as -0.0."""
    g = graph(name)
    out = []
    for si, sigma in enumerate(INT_SIGMAS):
        rng = np.random.default_rng([INT_SEED, NAMES.index(name), si])
        cws = g.encode(rng.integers(0, 2, (INT_WORDS, g.k), dtype=np.uint8))
        y = (1.0 - 2.0 * cws) + sigma * rng.standard_normal(cws.shape)
        out.append(np.clip(np.rint(2.0 * y), -3, 3).astype(F))
    x = np.concatenate(out) + F(0.0)  # no -0.0 from rint
    if minus_zero:
        flat = x.reshape(-1)
        zeros = np.flatnonzero(flat == 0)
        flat[zeros[1::2]] = F(-0.0)
    return x


def int_min_sum(name, llr, max_iter, unit=1, halve=False):
    """Min-sum in int64 from the definition, on LLRs that are whole multiples of 1 / unit: a
    check sends each of its bits the product of the other bits' signs (a zero counts as plus)
    times the smallest of the other bits' magnitudes, halved if halve (scale 0.5; the halving
    must leave no remainder); a bit sends each check its LLR plus what the other checks sent,
    and decides 1 when its LLR plus everything sent is <= 0. Decoding stops when every check
    holds; the decision returned is the first with the fewest unsatisfied checks.
    Returns (bits (W, K), unsat, iterations, the largest magnitude formed in units of 1 / unit,
    stats: ties = checks met with their two smallest magnitudes equal, zero_sums = decision sums
    that were exactly 0)."""
    g = graph(name)
    x = np.atleast_2d(llr).astype(np.float64) * unit
    assert np.array_equal(np.rint(x), x), "LLRs are whole units"
    L = x.astype(np.int64)  # (W, N)
    W, big = len(L), np.int64(1) << 60
    edge_bit = g.check_bits.astype(np.int64)

    def unsat_of(hard):
        return np.add.reduceat(hard[:, edge_bit], g.check_start[:-1].astype(np.int64), axis=1).__and__(1).sum(axis=1)

    hard = (L <= 0).astype(np.int64)
    best, fewest = hard.copy(), unsat_of(hard)
    iterations = np.zeros(W, np.int64)
    to_check = L[:, edge_bit]  # (W, E): what each edge's bit tells its check
    max_mag, stats = int(np.abs(L).max()), {"ties": 0, "zero_sums": 0}
    for _ in range(max_iter):
        run = fewest != 0  # words still decoding; the others keep what they have
        if not run.any():
            break
        iterations[run] += 1
        q = to_check[:, g.c_idx]  # (W, M, D), slots past a check's degree masked below
        sign = np.where(g.c_on[None] & (q < 0), -1, 1)
        mag = np.where(g.c_on[None], np.abs(q), big)
        two = np.sort(mag, axis=2)[:, :, :2]
        stats["ties"] += int((two[run, :, 0] == two[run, :, 1]).sum())
        others = np.where(mag == two[:, :, :1], two[:, :, 1:2], two[:, :, :1])  # the smallest of the others
        if halve:
            assert not (others[run][:, g.c_on] & 1).any(), "scale 0.5 leaves a remainder: unit too small"
            others = others // 2
        sent = sign.prod(axis=2, keepdims=True) * sign * others
        to_bit = np.zeros_like(to_check)
        to_bit[:, g.c_idx[g.c_on]] = sent[:, g.c_on]
        per_bit = np.where(g.b_on[None], to_bit[:, g.b_idx], 0)  # (W, N, 3)
        sums = L + per_bit.sum(axis=2)
        stats["zero_sums"] += int((sums[run] == 0).sum())
        hard = (sums <= 0).astype(np.int64)
        u = unsat_of(hard)
        better = run & (u < fewest)
        best[better], fewest[better] = hard[better], u[better]
        nxt = to_check.copy()
        for j in range(3):
            on = g.b_on[:, j]
            nxt[:, g.b_idx[on, j]] = sums[:, on] - per_bit[:, on, j]
        to_check = np.where(run[:, None], nxt, to_check)
        max_mag = max(max_mag, int(np.abs(sums[run]).max()), int(np.abs(to_check[run]).max()))
    return best[:, :g.k].astype(np.uint8), fewest.astype(np.int32), iterations.astype(np.int32), max_mag, stats
