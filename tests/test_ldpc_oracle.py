"""CPU: the FT8 / FT4 channel codec on the host (csrc/ldpc.cpp through the C ABI) against
tests/np_ref_ldpc.py, everything exact.

The batch is np_ref_ldpc.batch: 32 BPSK + noise words at each of sigma 0.4 / 0.6 / 0.8,
scaled to mean square 24, then the edge cases. The vectorised restatement and the
library's host decoder and the scalar restatement (ldpc.rs loop for loop in Python
scalars, a third of a second per word that runs 20 iterations) are all compared on every
word under both rules. The knife-edge words (np_ref_ldpc.knife_set) add what that batch cannot
see: decisions that report a float32 sum to the last ulp, with the proof that each operation
variant of the restatement moves one of their outputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_ref_ldpc as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOCOLS = ("ft8", "ft4")
N_NOISY = len(R.SIGMAS) * R.WORDS_PER_SIGMA


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def _host(lib, llr, protocol, rule, max_iter=20):
    """The library's host decoder on a batch: (records as tuples, plain)."""
    recs, plains = [], []
    for x in llr:
        r, p = lib.ldpc_decode_host(np.ascontiguousarray(x), protocol, rule, max_iter)
        recs.append((r["payload"].tobytes(), int(r["status"]), int(r["iterations"]), int(r["errors"])))
        plains.append(p)
    return recs, np.array(plains)


# ---- tables ---------------------------------------------------------------------
def test_table_structure():
    t = R.tables()
    assert t["h"].shape == (83, 174) and len(t["edges"]) == 522 and int(t["h"].sum()) == 522
    assert set(t["num_rows"].tolist()) == {6, 7} and int((t["num_rows"] == 7).sum()) == 24
    assert (t["h"].sum(axis=0) == 3).all()  # every bit in exactly 3 checks
    assert t["mn"].shape == (174, 3) and (np.diff(t["mn"], axis=1) > 0).all()


def test_library_tables_equal_the_restatement(lib):
    t = R.tables()
    edges, row_start, bit_check, gen = lib.ldpc_tables()
    assert np.array_equal(edges, t["edges"])
    assert np.array_equal(row_start, t["row_start"])
    assert np.array_equal(bit_check, t["mn"] - 1)
    assert np.array_equal(gen, t["generator"])


# ---- CRC and encoding --------------------------------------------------------------
def test_crc14(lib):
    rng = np.random.default_rng(5)
    for nbits in (1, 8, 77, 82, 96):
        msg = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        assert lib.ft_crc14(msg, nbits) == R.crc14(msg, nbits)
    assert R.crc14(bytes(12), 82) == 0


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_encoded_words_satisfy_every_check_and_equal_the_restatement(lib, protocol):
    rng = np.random.default_rng(91)
    codec = lib.Ft8Codec if protocol == "ft8" else lib.Ft4Codec
    for _ in range(64):
        p = rng.integers(0, 256, 10, dtype=np.uint8).tobytes()  # slack bits of byte 9 set in most
        bits = R.codeword_bits(protocol, p)
        assert int(R.count_errors(bits)) == 0
        tones = codec.encode(p)
        assert tones.dtype == np.uint8 and tones.shape == (58 if protocol == "ft8" else 87,)
        assert np.array_equal(tones, R.encode(protocol, p))
        llr = codec.frame_to_llr_hard(tones)
        assert np.array_equal(llr.view(np.uint32), R.frame_to_llr_hard(protocol, tones).view(np.uint32))
        assert np.array_equal((llr < 0).astype(np.uint8), bits)


# ---- the decoders --------------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_the_batch_has_the_cases_it_is_meant_to_have(protocol):
    """Asserted on the restatement alone, before anything is compared with it."""
    _, errors, iterations = R.batch_decoded(protocol, "sum_product")
    e, it = errors[:N_NOISY], iterations[:N_NOISY]
    at_once = int((it == 0).sum())
    late = int(((e == 0) & (it >= 3)).sum())
    failed = int(((e != 0) & (it == 20)).sum())
    print(f"{protocol} sum_product: {at_once} valid at once, {late} converge after >= 3 iterations, {failed} fail")
    assert at_once >= 5 and late >= 10 and failed >= 5
    # under the reference rule every noisy word that starts with an error fails
    _, e_ref, it_ref = R.batch_decoded(protocol, "reference")
    started_wrong = it_ref[:N_NOISY] != 0
    assert int(started_wrong.sum()) >= 50
    assert (e_ref[:N_NOISY][started_wrong] != 0).all() and (it_ref[:N_NOISY][started_wrong] == 20).all()
    assert np.array_equal(it_ref[:N_NOISY] == 0, it == 0)


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_host_decoder_equals_the_vectorised_restatement(lib, protocol, rule):
    llr, names, _ = R.batch(protocol)
    plain, errors, iterations = R.batch_decoded(protocol, rule)
    want = R.records(protocol, plain, errors, iterations)
    got, got_plain = _host(lib, llr, protocol, rule)
    bad = [names[k] for k in range(len(names)) if got[k] != want[k] or not np.array_equal(got_plain[k], plain[k])]
    assert not bad, bad


@pytest.mark.parametrize("group", ["sigma0.4", "sigma0.6", "sigma0.8", "edge"])
@pytest.mark.parametrize("rule", R.RULES)
def test_scalar_restatement_equals_the_vectorised_one(rule, group):
    llr, names, _ = R.batch("ft8")
    plain, errors, iterations = R.batch_decoded("ft8", rule)
    for k in [k for k, n in enumerate(names) if n.startswith(group) or (group == "edge" and k >= N_NOISY)]:
        p, e, it = R.decode_scalar(llr[k], 20, rule)
        assert (e, it) == (int(errors[k]), int(iterations[k])) and np.array_equal(p, plain[k]), names[k]


@pytest.mark.parametrize("rule", R.RULES)
def test_edge_cases(lib, rule):
    llr, names, payloads = R.batch("ft8")
    plain, errors, iterations = R.batch_decoded("ft8", rule)
    rec = dict(zip(names, R.records("ft8", plain, errors, iterations)))
    k = names.index("zeros")
    assert plain[k].all() and errors[k] == 24 and iterations[k] == 20 and rec["zeros"][1] == 0
    p = payloads[names.index("inf")]
    assert rec["inf"] == (p, 2, 0, 0)
    # NaN spreads over the whole graph in three iterations, NaN <= 0 is false for every bit,
    # and the all-zero word is a codeword whose CRC is 0: the reference "decodes" zeros
    assert rec["nan3"] == (bytes(10), 2, 3, 0)
    assert rec["crc_bad"] == (bytes(10), 1, 0, 0)
    for j in range(4):
        assert rec[f"flip1/{j}"] == ((p, 2, 1, 0) if rule == "sum_product" else (bytes(10), 0, 20, 3))
    assert rec["flip1_w6"][:2] == (p, 2)
    if rule == "sum_product":
        assert rec["crc_bad_flip1"] == (bytes(10), 1, 1, 0)
    # the library agrees on each (also covered by the batch test) and on max_iter 0 and 1
    for max_iter in (0, 1):
        pl, er, it = R.decode_batch(llr, max_iter, rule)
        assert (it <= max_iter).all() and (it[er != 0] == max_iter).all()
        got, got_plain = _host(lib, llr, "ft8", rule, max_iter)
        assert got == R.records("ft8", pl, er, it) and np.array_equal(got_plain, pl)


# ---- knife-edge words: the arithmetic to the last bit -----------------------------------
KNIFE_IDS = [f"{rule}_d{depth}" for rule, depth in R.KNIFE_CASES]


def _differing(a, b):
    """Words in which any of plain, errors, iterations differs."""
    return int(sum(any(not np.array_equal(x[w], y[w]) for x, y in zip(a, b)) for w in range(len(a[0]))))


@pytest.mark.parametrize("case", R.KNIFE_CASES, ids=KNIFE_IDS)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_knife_words_meet_their_conditions_on_the_restatement_alone(protocol, case):
    """Six words per protocol, rule and depth, 6 bits balanced in each on pairwise disjoint
    checks (with their neighbours that is most of the 174 bits). A bit holds when its decision
    sum in iteration depth is <= 0 at its LLR and > 0 at the next float32, and that iteration's
    decision is what the decoder returns. At depth 1 every bit holds, at depth 2 at least half.
    The reference rule's sign depends on the check having 7 entries: bits of both kinds of
    check are among those that hold."""
    rule, depth = case
    t = R.tables()
    words, balanced, requested = R.knife_set(protocol, rule, depth)
    assert words.shape == (6, 174) and requested == [R.KNIFE_BITS] * 6
    weights = set()
    for held in balanced:
        assert len(held) == R.KNIFE_BITS if depth == 1 else 2 * len(held) >= R.KNIFE_BITS
        checks = (t["mn"][held] - 1).ravel()
        assert len(set(checks.tolist())) == 3 * len(held), "balanced bits share a check"
        weights.update(t["num_rows"][checks].tolist())
    assert weights == {6, 7}
    plain, errors, iterations = R.decode_batch(words, depth, rule)
    history = R.trace(words, depth, rule)[0]
    assert (iterations == depth).all() and (errors > 0).all()
    assert (history[depth] < history[:depth].min(axis=0)).all() and np.array_equal(errors, history[depth])
    up = np.array(words)
    for w, held in enumerate(balanced):
        assert plain[w, held].all()  # a sum <= 0 decides 1
        up[w, held] = np.nextafter(words[w, held], np.float32(np.inf))
    if depth == 1:  # the messages into a bit do not depend on any balanced LLR: all at once
        l = R.trace(up, 1, rule)[2]
        assert all((l[w, held] > 0).all() for w, held in enumerate(balanced))
    print(f"[knife] {protocol} {rule} depth {depth}: bits held {[len(h) for h in balanced]}, errors {history.T.tolist()}")


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_every_operation_variant_moves_an_output_of_the_knife_words(protocol, rule):
    """Non-vacuity, for both protocols under both rules: each one-line departure from the
    reference's operation list (np_ref_ldpc_family.VARIANTS) changes plain, errors or iterations
    of at least one knife word. The three bit -> check sums only feed the second iteration, so
    their variant is held to the depth-2 words, the other four to the depth-1 words. The shared
    batch (105 words, 20 iterations) notices none of the five under either rule."""
    for depth in (1, 2):
        words = R.knife_set(protocol, rule, depth)[0]
        base = R.decode_batch(words, depth, rule)
        counts = {v: _differing(base, R.decode_batch(words, depth, rule, (v,))) for v in R.F.VARIANTS}
        print(f"[knife] {protocol} {rule} depth {depth}: words of {len(words)} that differ under {counts}")
        for v in R.F.VARIANTS:
            if (v == "sum_assoc") == (depth == 2):
                assert counts[v] > 0, (protocol, rule, depth, v)


@pytest.mark.parametrize("case", R.KNIFE_CASES, ids=KNIFE_IDS)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_host_decoder_and_scalar_restatement_equal_the_vectorised_one_on_the_knife_words(lib, protocol, case):
    rule, depth = case
    words = R.knife_set(protocol, rule, depth)[0]
    for max_iter in (depth, depth + 1):
        plain, errors, iterations = R.decode_batch(words, max_iter, rule)
        got, got_plain = _host(lib, words, protocol, rule, max_iter)
        assert got == R.records(protocol, plain, errors, iterations) and np.array_equal(got_plain, plain), max_iter
    plain, errors, iterations = R.decode_batch(words, depth, rule)
    for w in range(len(words)):
        p, e, it = R.decode_scalar(words[w], depth, rule)
        assert (e, it) == (int(errors[w]), int(iterations[w])) and np.array_equal(p, plain[w]), w


# ---- the codec classes -----------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_codec_round_trip(lib, protocol):
    codec = lib.Ft8Codec if protocol == "ft8" else lib.Ft4Codec
    rng = np.random.default_rng(17)
    for _ in range(8):
        p = R.random_payload(rng)
        tones = codec.encode(p)
        assert codec.decode_soft(codec.frame_to_llr_hard(tones)) == p
        assert codec.decode_hard(tones) == p
        assert codec.decode_hard(tones, rule="sum_product", max_iter=5) == p
    ones = bytes([0xFF] * 10)  # 77 ones and the slack bits set
    assert codec.decode_hard(codec.encode(ones)) == bytes([0xFF] * 9 + [0xF8])
    # a word the reference rule cannot correct: None; sum_product returns the payload
    llr = codec.frame_to_llr_hard(codec.encode(p))
    llr[0] = -llr[0] * np.float32(0.3)
    assert codec.decode_soft(llr) is None
    assert codec.decode_soft(llr, rule="sum_product") == p


def test_codec_rejects_wrong_shapes_and_types(lib):
    with pytest.raises(ValueError):
        lib.Ft8Codec.encode(bytes(9))
    with pytest.raises(ValueError):
        lib.Ft8Codec.decode_soft(np.zeros(173, np.float32))
    with pytest.raises(ValueError):
        lib.Ft8Codec.decode_soft(np.zeros(174, np.float64))
    with pytest.raises(ValueError):
        lib.Ft8Codec.decode_hard(np.zeros(87, np.uint8))
    with pytest.raises(ValueError):
        lib.Ft4Codec.decode_hard(np.zeros(87, np.int32))
    with pytest.raises(lib.OrionError, match="error -3"):
        lib.ldpc_decode_host(np.zeros(174, np.float32), "ft8", 2, 20)
    with pytest.raises(lib.OrionError, match="error -3"):
        lib.ldpc_decode_host(np.zeros(174, np.float32), "ft8", "reference", 256)


# ---- the host code under the sanitizers ---------------------------------------------------
def test_host_codec_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/ldpc.cpp and tests/ldpc_host/main.cpp, built with the host compiler alone and
    -fsanitize=address,undefined into a stand-alone binary; run as a subprocess."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "orion-sdr_amd", "csrc")
    exe = str(tmp_path / "ldpc_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-I", src, os.path.join(src, "ldpc.cpp"),
                    os.path.join(ROOT, "tests", "ldpc_host", "main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ldpc_host: ok" in out.stdout, out.stdout + out.stderr
