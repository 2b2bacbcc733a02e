"""CPU: the library's host side of the LDPC family (csrc/ldpc_family.cpp through the C ABI and
orion_sdr.Ldpc) against tests/np_ref_ldpc_family.py, equal in every output: the three graphs
as CSR arrays, encode, the syndrome weight, and decode under all three rules on the input set
(per code and sigma 24 noisy words, then all-zero LLRs, NaN, infinities, 1e30) with max_iter
50, 1 and 0; the paths that set must hold; the knife-edge words, on which a decision reports a
float32 sum to the last ulp, with the proof that each operation variant moves one of their
outputs; the integer words against an int64 min-sum decoder; the reference's own properties
(tests/unit/fec.rs:526-653); the argument errors of every entry, the device entries' before any
launch; and the host code of both frame codes under the sanitizers as a stand-alone program."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_ldpc_family as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECT = {"n512r12": (512, 256, 1279, {4, 5}), "n576r23": (576, 384, 1535, {7, 8}), "n512r34": (512, 384, 1407, {10, 11})}


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


@pytest.fixture(scope="module")
def decoded():
    """(code, rule, max_iter) -> the restatement's (bits, unsat, iterations, best_iter) on the
    code's whole input set, computed once."""
    cache = {}

    def get(name, rule, max_iter=50):
        key = (name, rule, max_iter)
        if key not in cache:
            cache[key] = R.decode(name, R.input_set(name), max_iter, rule)
        return cache[key]

    return get


# ---- the graphs -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_graph_equals_the_restatement(lib, name):
    g, c = R.graph(name), lib.Ldpc(name)
    n, k, edges, degs = EXPECT[name]
    assert (c.n, c.k, c.m, c.n_edges, c.max_check_degree, c.relaxed_picks) == (n, k, n - k, edges, max(degs), 0)
    assert (g.n, g.k, g.n_edges, set(g.degrees.tolist()), g.relaxed) == (n, k, edges, degs, 0)
    got = c.graph()
    for key in ("check_start", "check_bits", "bit_start", "bit_checks", "bit_edges"):
        assert got[key].dtype == np.uint32 and np.array_equal(got[key], getattr(g, key)), key
    # bit degrees: 3 for message bits, 2 for parity bits, 1 for the last
    assert np.array_equal(np.diff(got["bit_start"].astype(np.int64)), [3] * k + [2] * (n - k - 1) + [1])
    # within a check: message columns ascending, then K + i, then K + i - 1
    for i in (0, 1, n - k - 1):
        bits = got["check_bits"][got["check_start"][i]:got["check_start"][i + 1]].tolist()
        tail = [k + i] if i == 0 else [k + i, k + i - 1]
        assert bits[-len(tail):] == tail and bits[:-len(tail)] == sorted(bits[:-len(tail)]) and max(bits[:-len(tail)]) < k
    # a parity bit's checks are row i, then row i + 1
    b = k + 5
    assert got["bit_checks"][got["bit_start"][b]:got["bit_start"][b + 1]].tolist() == [5, 6]
    # no two message columns share a pair of rows (the A-block 4-cycle guard held everywhere)
    pairs = collections.Counter()
    for col in range(k):
        r = got["bit_checks"][got["bit_start"][col]:got["bit_start"][col] + 3].tolist()
        pairs.update([(r[0], r[1]), (r[0], r[2]), (r[1], r[2])])
    assert max(pairs.values()) == 1
    assert lib.Ldpc(c).code == name  # a code object is accepted where a name is


# ---- encode and the syndrome ----------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_encode_and_syndrome_weight_equal_the_restatement(lib, name):
    g, c = R.graph(name), lib.Ldpc(name)
    rng = np.random.default_rng([32, R.NAMES.index(name)])
    msgs = rng.integers(0, 2, (9, g.k), dtype=np.uint8)
    msgs[1] = rng.integers(0, 256, g.k, dtype=np.uint8)  # other byte values: copied, bit 0 in the parity
    msgs[2] = 0
    msgs[3] = 1
    cws = g.encode(msgs)
    assert np.array_equal(c.encode(msgs), cws) and np.array_equal(c.encode(msgs[4]), cws[4])
    assert np.array_equal(cws[:, :g.k], msgs) and not g.syndrome_weight(cws).any()
    assert c.syndrome_weight(cws[0]) == 0 and not c.syndrome_weight(cws).any()
    hard = cws.copy()
    hard[:, ::37] ^= 1
    hard[5] = rng.integers(0, 256, g.n, dtype=np.uint8)
    want = g.syndrome_weight(hard)
    assert np.array_equal(c.syndrome_weight(hard), want) and want.min() > 0
    assert c.syndrome_weight(np.ones(g.n, np.uint8)) == int((g.degrees % 2).sum())


# ---- decode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_input_set_holds_every_path(decoded, name):
    """What binds: per code, under the default rule, the set holds a word valid at once, one
    decoded in 1 iteration, one decoded in >= 5, one failed after 50 iterations with unsat > 0,
    and a failed one whose best snapshot is not the last iteration's decision."""
    _, unsat, iters, best_iter = decoded(name, "sum_product")
    noisy = slice(0, len(R.SIGMAS) * R.WORDS)
    u, i, b = unsat[noisy], iters[noisy], best_iter[noisy]
    assert ((u == 0) & (i == 0)).any(), "valid at once"
    assert ((u == 0) & (i == 1)).any(), "decoded in 1 iteration"
    assert ((u == 0) & (i >= 5)).any(), "decoded in >= 5 iterations"
    assert ((u > 0) & (i == 50)).any(), "failed after 50 iterations"
    assert ((u > 0) & (i == 50) & (b != 50)).any(), "failed with a stale best snapshot"
    print(f"[paths] {name}: {collections.Counter(R.path(*x) for x in zip(u, i, b))}, iterations "
          f"{[int(v) for v in np.bincount(i)[:8]]} ...")


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: r if isinstance(r, str) else r[0])
@pytest.mark.parametrize("name", R.NAMES)
def test_decode_equals_the_restatement(lib, decoded, name, rule):
    c, llr = lib.Ldpc(name), R.input_set(name)
    for max_iter in (50, 1, 0):
        bits, unsat, iters, _ = decoded(name, rule, max_iter)
        hb, hu, hi = c.decode_soft(llr, max_iter, rule)
        assert hb.dtype == np.uint8 and hu.dtype == np.int32 and hi.dtype == np.int32
        assert np.array_equal(hi, iters), np.flatnonzero(hi != iters)[:8]
        assert np.array_equal(hu, unsat), np.flatnonzero(hu != unsat)[:8]
        assert np.array_equal(hb, bits)
        if max_iter == 0:
            assert not hi.any() and np.array_equal(hb, (llr[:, :c.k] <= 0).astype(np.uint8))
    one = c.decode_soft(llr[30], 50, rule)  # one word: a (K,) array and two ints
    b50, u50, i50, _ = decoded(name, rule, 50)
    assert np.array_equal(one[0], b50[30]) and one[1:] == (int(u50[30]), int(i50[30]))


def test_the_scale_of_scaled_min_sum_is_used(lib):
    c, llr = lib.Ldpc("n512r34"), R.input_set("n512r34")[48:96]
    a = c.decode_soft(llr, 50, ("scaled_min_sum", 0.75))
    b = c.decode_soft(llr, 50, ("scaled_min_sum", 0.5))
    m = c.decode_soft(llr, 50, "min_sum")
    one = c.decode_soft(llr, 50, ("scaled_min_sum", 1.0))
    assert not np.array_equal(a[2], b[2]) and not np.array_equal(a[2], m[2])
    assert all(np.array_equal(x, y) for x, y in zip(m, one))
    for i, want in enumerate(R.decode("n512r34", llr, 50, ("scaled_min_sum", 0.5))[:3]):
        assert np.array_equal(b[i], want)


# ---- knife-edge words: the arithmetic to the last bit ---------------------------------------
CASE_IDS = [f"{R.rule_id(rule)}_d{depth}" for rule, depth in R.KNIFE_CASES]


def _differing(a, b):
    """Words in which any of bits, unsat, iterations differs."""
    return int(sum(any(not np.array_equal(x[w], y[w]) for x, y in zip(a, b)) for w in range(len(a[0]))))


@pytest.mark.parametrize("case", R.KNIFE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("name", R.NAMES)
def test_knife_words_meet_their_conditions_on_the_restatement_alone(name, case):
    """Six words per code, rule and depth, 24 message bits balanced in each on pairwise disjoint
    checks. A bit holds when its decision sum in iteration depth is <= 0 at its LLR and > 0 at
    the next float32, and that iteration's decision is the snapshot the decoder returns. At
    depth 1 every bit holds; at depth 2 (where a balanced LLR feeds back into the messages that
    reach it) at least half do."""
    rule, depth = case
    g = R.graph(name)
    words, balanced, requested = R.knife_set(name, rule, depth)
    assert words.shape == (R.KNIFE_WORDS, g.n) and requested == [R.KNIFE_BITS] * R.KNIFE_WORDS
    for held in balanced:
        assert max(held) < g.k and len(set(held)) == len(held)
        assert len(held) == R.KNIFE_BITS if depth == 1 else 2 * len(held) >= R.KNIFE_BITS
        rows = [set(g.col_rows[b].tolist()) for b in held]
        assert len(set().union(*rows)) == 3 * len(held), "balanced bits share a check"
    bits, unsat, iters, best_iter = R.decode(name, words, depth, rule)
    assert (iters == depth).all() and (best_iter == depth).all() and (unsat > 0).all()
    up = words.copy()
    for w, held in enumerate(balanced):
        assert bits[w, held].all()  # a sum <= 0 decides 1
        up[w, held] = np.nextafter(words[w, held], np.float32(np.inf))
    if depth == 1:  # the messages into a bit do not depend on any balanced LLR: all at once
        dec = R.trace(name, up, 1, rule)[2]
        assert all((dec[w, held] > 0).all() for w, held in enumerate(balanced))
    print(f"[knife] {name} {CASE_IDS[R.KNIFE_CASES.index(case)]}: bits held {[len(h) for h in balanced]}, "
          f"unsat {R.trace(name, words, depth, rule)[0].T.tolist()}")


@pytest.mark.parametrize("name", R.NAMES)
def test_every_operation_variant_moves_an_output_of_the_knife_words(name):
    """Non-vacuity: each one-line departure from the reference's operation list (R.VARIANTS)
    changes bits, unsat or iterations of at least one sum-product knife word; the update sum
    only feeds the second iteration, so its variant is held to the depth-2 words. The oracle
    input set (125 words, max_iter 50) notices none of the five."""
    for depth in (1, 2):
        words = R.knife_set(name, "sum_product", depth)[0]
        base = R.decode(name, words, depth)[:3]
        counts = {v: _differing(base, R.decode(name, words, depth, "sum_product", (v,))[:3]) for v in R.VARIANTS}
        print(f"[knife] {name} sum_product depth {depth}: words of {len(words)} that differ under {counts}")
        for v in R.VARIANTS:
            if (v == "sum_assoc") == (depth == 2):
                assert counts[v] > 0, (name, depth, v)
    # the min-sum words: the scale and the choice of magnitude feed the balanced sums
    words = R.knife_set(name, ("scaled_min_sum", 0.75), 1)[0]
    base = R.decode(name, words, 1, ("scaled_min_sum", 0.75))[:3]
    assert _differing(base, R.decode(name, words, 1, "min_sum")[:3]) == len(words)
    assert _differing(base, R.decode(name, words, 1, ("scaled_min_sum", float(np.nextafter(np.float32(0.75), 1))))[:3]) > 0


@pytest.mark.parametrize("case", R.KNIFE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("name", R.NAMES)
def test_host_decoder_equals_the_restatement_on_the_knife_words(lib, name, case):
    rule, depth = case
    words = R.knife_set(name, rule, depth)[0]
    for max_iter in (depth, depth + 1):
        want = R.decode(name, words, max_iter, rule)[:3]
        got = lib.Ldpc(name).decode_soft(np.array(words), max_iter, rule)
        for g, w, what in zip(got, want, ("bits", "unsat", "iterations")):
            assert np.array_equal(g, w), (what, max_iter, np.argwhere(g != w)[:8])


# ---- exact words for the min-sum rules: an int64 decoder from the definition -----------------
@pytest.fixture(scope="module")
def int_ref():
    """(code, max_iter, half) -> R.int_min_sum on the code's integer words, computed once."""
    cache = {}

    def get(name, max_iter, half=False):
        key = (name, max_iter, half)
        if key not in cache:
            cache[key] = R.int_min_sum(name, R.int_words(name), max_iter, R.HALF_UNIT if half else 1, half)
        return cache[key]

    return get


@pytest.mark.parametrize("name", R.NAMES)
def test_integer_words_hold_what_they_must(int_ref, name):
    """On the integer reference alone: every magnitude formed stays below 2^24 (so float32 holds
    it exactly; with scale 0.5 in units of 2^-8), and the set has equal-magnitude ties, decision
    sums that are exactly 0, a word decoded in at most 2 iterations and a word that fails."""
    x = R.int_words(name)
    assert x.shape == (len(R.INT_SIGMAS) * R.INT_WORDS, R.graph(name).n) and np.abs(x).max() == 3 and (x == 0).any()
    z = R.int_words(name, minus_zero=True)
    assert np.array_equal(x, z) and np.signbit(z).sum() - np.signbit(x).sum() == (x == 0).sum() // 2
    for half, max_iter in ((False, R.INT_MAX_ITER), (True, R.HALF_MAX_ITER)):
        _, unsat, iters, max_mag, stats = int_ref(name, max_iter, half)
        print(f"[knife] {name} integer words{' scale 0.5' if half else ''}: largest magnitude {max_mag}, {stats}, "
              f"iterations {np.bincount(iters).tolist()}, failed {int((unsat > 0).sum())}")
        assert max_mag < 2 ** 24
        assert stats["ties"] > 0 and stats["zero_sums"] > 0
        assert ((unsat == 0) & (iters >= 1) & (iters <= 2)).any() and (unsat > 0).any()


@pytest.mark.parametrize("name", R.NAMES)
def test_min_sum_equals_the_integer_decoder(lib, int_ref, name):
    """The host decoder and the float32 restatement equal the int64 decoder in bits, unsat and
    iterations: min_sum at max_iter 20, 1 and 0, scale 0.5 at max_iter 8, each on the words as
    they are and with every second zero written as -0.0."""
    c = lib.Ldpc(name)
    for half, max_iter in ((False, R.INT_MAX_ITER), (False, 1), (False, 0), (True, R.HALF_MAX_ITER)):
        rule = ("scaled_min_sum", 0.5) if half else "min_sum"
        want = int_ref(name, max_iter, half)[:3]
        for minus_zero in (False, True):
            x = R.int_words(name, minus_zero)
            for what, got in (("restatement", R.decode(name, x, max_iter, rule)[:3]), ("host", c.decode_soft(x, max_iter, rule))):
                for g, w, field in zip(got, want, ("bits", "unsat", "iterations")):
                    assert np.array_equal(g, w), (what, field, max_iter, half, minus_zero, np.argwhere(g != w)[:8])


# ---- the reference's own properties (tests/unit/fec.rs:526-653) -----------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_encoded_word_satisfies_every_check_and_clean_llrs_decode_exactly(lib, name):
    c = lib.Ldpc(name)
    msg = np.random.default_rng([33, c.n]).integers(0, 2, c.k, dtype=np.uint8)
    cw = c.encode(msg)
    assert cw.shape == (c.n,) and np.array_equal(cw[:c.k], msg) and c.syndrome_weight(cw) == 0
    bits, unsat, iters = c.decode_soft(np.where(cw == 0, 8.0, -8.0).astype(np.float32))
    assert unsat == 0 and iters == 0 and np.array_equal(bits, msg)


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: r if isinstance(r, str) else r[0])
@pytest.mark.parametrize("name,n_err", [("n512r12", 5), ("n512r34", 3)])
def test_soft_errors_are_corrected_under_every_rule(lib, name, n_err, rule):
    """Strong LLRs with a few weak wrong-sign values: belief propagation converges to the
    message, under sum-product and both min-sum rules."""
    c = lib.Ldpc(name)
    rng = np.random.default_rng([34, c.n, n_err])
    msg = rng.integers(0, 2, c.k, dtype=np.uint8)
    llr = np.where(c.encode(msg) == 0, 6.0, -6.0).astype(np.float32)
    pos = rng.choice(c.n, n_err, replace=False)
    llr[pos] = -llr[pos] * np.float32(0.5)
    bits, unsat, iters = c.decode_soft(llr, 50, rule)
    assert unsat == 0 and iters >= 1 and np.array_equal(bits, msg)
    if rule == "sum_product":  # the default rule is sum-product
        d = c.decode_soft(llr)
        assert np.array_equal(d[0], bits) and d[1:] == (unsat, iters)


def test_llr_convention_positive_means_bit_zero(lib):
    c = lib.Ldpc("n512r12")
    msg = (np.arange(c.k) % 2).astype(np.uint8)
    llr = np.where(c.encode(msg) == 0, 1.5, -1.5).astype(np.float32)
    bits, unsat, _ = c.decode_soft(llr, 50)
    assert unsat == 0 and np.array_equal(bits, msg)


# ---- argument errors ------------------------------------------------------------------------
def test_host_argument_errors(lib):
    for bad in ("n512r23", "N512R12", 0, None):
        with pytest.raises(ValueError):
            lib.Ldpc(bad)
    c = lib.Ldpc("n576r23")
    llr = np.zeros(c.n, np.float32)
    for bad in (lambda: c.encode(np.zeros(c.k - 1, np.uint8)), lambda: c.encode(np.zeros(c.k, np.int32)),
                lambda: c.encode(np.zeros((2, 2, c.k), np.uint8)), lambda: c.syndrome_weight(np.zeros(c.k, np.uint8)),
                lambda: c.decode_soft(llr.astype(np.float64)), lambda: c.decode_soft(llr[:-1]),
                lambda: c.decode_soft(llr, -1), lambda: c.decode_soft(llr, 50, "sum-product"),
                lambda: c.decode_soft(llr, 50, "scaled_min_sum"), lambda: c.decode_soft(llr, 50, ("min_sum", 0.5)),
                lambda: c.decode_soft(llr, 50, ("scaled_min_sum", "x")), lambda: c.decode_soft(list(llr))):
        with pytest.raises(ValueError):
            bad()


def test_device_entries_refuse_bad_arguments_before_any_launch(lib):
    """Every check runs before anything touches a device, so this passes without one."""
    n = 512
    llr = np.zeros((2, 2 * n), np.float32)
    bits = np.zeros((2, 300), np.uint8)
    D, E = lib.ldpc_family_decode_batch, lib.ldpc_family_encode_batch
    for bad in (lambda: D(llr, "n512r13"), lambda: D(llr, "n512r12", rule="sum"), lambda: D(llr, "n512r12", rule=("scaled_min_sum",)),
                lambda: D(llr.astype(np.float64), "n512r12"), lambda: D(llr[0], "n512r12"), lambda: D(llr[:, :n - 1], "n512r12"),
                lambda: D(llr[:, :575], "n576r23"), lambda: D(llr, "n512r12", max_iter=-1),
                lambda: D(llr, "n512r12", interleaver=(7, 11)),  # 1024 is not whole blocks of 77
                lambda: D(llr, "n512r12", interleaver=(0, 4)), lambda: D(llr, "n512r12", interleaver=(1 << 13, 1 << 13)),
                lambda: D(np.zeros((2, 77 * 6), np.float32), "n512r12", interleaver=(7, 11)),  # 462: no whole codeword
                lambda: E(bits, "n512"), lambda: E(bits.astype(np.int8), "n512r12"), lambda: E(bits[0], "n512r12"),
                lambda: E(bits[:, :0], "n512r12"), lambda: E(bits, "n512r12", interleaver=(3, 0))):
        with pytest.raises(ValueError):
            bad()


# ---- the host code under the sanitizers -----------------------------------------------------
def test_host_frame_codes_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/ldpc_family.cpp, bch.cpp (with rs.cpp for the field) and tests/fec2_host/main.cpp,
    built with the host compiler alone and -fsanitize=address,undefined into a stand-alone
    binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "fec2_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src,
                    os.path.join(src, "ldpc_family.cpp"), os.path.join(src, "bch.cpp"), os.path.join(src, "rs.cpp"),
                    os.path.join(ROOT, "tests", "fec2_host", "main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "fec2_host: ok" in out.stdout, out.stdout + out.stderr
