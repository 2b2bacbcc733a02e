"""GPU: both belief-propagation decoders (csrc/k_ldpc_family.hip, csrc/k_ldpc.hip) to the last
bit. A decoder returns decisions only, and on noisy words those do not move when a message is
off by an ulp; the words here make them move:

  knife-edge words (np_ref_ldpc_family.knife_set, np_ref_ldpc.knife_set): the LLR of each
  balanced bit is the largest float32 whose decision sum in iteration d is still <= 0, so with
  max_iter = d that bit of the output reports the float32 sum of the messages that reach it to
  the last ulp; the bits around it sit on fast_tanh's saturation bound or are subnormal. The
  CPU modules (test_ldpc_family_oracle.py, test_ldpc_oracle.py) prove on the restatement that
  a fused multiply-add, a reversed product, a reassociated sum, a non-strict comparison and a
  flushed subnormal each change an output of these words.

  integer words (np_ref_ldpc_family.int_words): LLRs in {-3 .. 3}, on which every value the
  min-sum rules form is exact, against an int64 decoder written from the definition.

Every comparison is equality, in every output: the device against the library's host decoder,
the numpy restatement and (integer words) the int64 decoder. Launches: one word, the whole
set, and the family sets once behind the fused 32 x 32 deinterleaver."""
import numpy as np
import pytest

import np_ref_ldpc as T
import np_ref_ldpc_family as R

pytestmark = pytest.mark.gpu

FAMILY_IDS = [f"{R.rule_id(rule)}_d{depth}" for rule, depth in R.KNIFE_CASES]
FT_IDS = [f"{rule}_d{depth}" for rule, depth in T.KNIFE_CASES]
IL = (32, 32)


def same(got, want, what):
    for g, w, field in zip(got, want, ("bits", "unsat", "iterations")):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape and np.array_equal(g, w), (what, field, np.flatnonzero(g != w)[:8])


def family_everywhere(lib, name, words, max_iter, rule, want, singles):
    """want (the restatement's or the integer decoder's outputs) = the host decoder = the
    device on the whole set in one launch = the device on words[singles], one word a launch."""
    c = lib.Ldpc(name)
    words = np.ascontiguousarray(words)
    same(c.decode_soft(words, max_iter, rule), want, "host")
    same(lib.ldpc_family_decode_batch(words.reshape(1, -1), name, max_iter=max_iter, rule=rule), want, "one launch")
    for w in singles:
        got = lib.ldpc_family_decode_batch(words[w:w + 1], name, max_iter=max_iter, rule=rule)
        same(got, [x[w:w + 1] for x in want], f"word {w} alone")


def behind_the_deinterleaver(lib, name, words, max_iter, rule, want):
    """The words, repeated until they fill whole 32 x 32 blocks, interleaved block by block."""
    n = words.shape[1]
    count = next(k for k in range(len(words), 64) if k * n % (IL[0] * IL[1]) == 0)
    pick = np.arange(count) % len(words)
    plain = words[pick].reshape(-1)
    block = IL[0] * IL[1]
    stream = np.concatenate([lib.BlockInterleaver(*IL).interleave(plain[b:b + block]) for b in range(0, len(plain), block)])
    got = lib.ldpc_family_decode_batch(stream[None], name, max_iter=max_iter, rule=rule, interleaver=IL)
    same(got, [x[pick] for x in want], "behind the deinterleaver")


# ---- the COFDM family --------------------------------------------------------------------
@pytest.mark.parametrize("case", R.KNIFE_CASES, ids=FAMILY_IDS)
@pytest.mark.parametrize("name", R.NAMES)
def test_family_knife_words(gpu_lib, name, case):
    rule, depth = case
    words, balanced, _ = R.knife_set(name, rule, depth)
    want = R.decode(name, words, depth, rule)[:3]
    assert all(want[0][w, held].all() for w, held in enumerate(balanced))
    family_everywhere(gpu_lib, name, words, depth, rule, want, range(len(words)))
    behind_the_deinterleaver(gpu_lib, name, words, depth, rule, want)
    # one more iteration than the balance was made for: the next update runs on the same sums
    family_everywhere(gpu_lib, name, words, depth + 1, rule, R.decode(name, words, depth + 1, rule)[:3], [0])


@pytest.mark.parametrize("minus_zero", [False, True], ids=["zeros", "minus_zeros"])
@pytest.mark.parametrize("name", R.NAMES)
def test_family_min_sum_equals_the_integer_decoder(gpu_lib, name, minus_zero):
    """min_sum at max_iter 20, 1 and 0 and scale 0.5 at max_iter 8 against the int64 decoder (and
    the restatement, and the host); every second zero written as -0.0 changes nothing."""
    words = R.int_words(name, minus_zero)
    for half, max_iter in ((False, R.INT_MAX_ITER), (False, 1), (False, 0), (True, R.HALF_MAX_ITER)):
        rule = ("scaled_min_sum", 0.5) if half else "min_sum"
        want = R.int_min_sum(name, words, max_iter, R.HALF_UNIT if half else 1, half)
        assert want[3] < 2 ** 24
        want = want[:3]
        same(R.decode(name, words, max_iter, rule)[:3], want, "restatement")
        if max_iter >= R.HALF_MAX_ITER:
            decoded, failed = int(np.flatnonzero(want[1] == 0)[0]), int(np.flatnonzero(want[1] > 0)[0])
            assert 1 <= want[2][decoded] < max_iter and want[2][failed] == max_iter
            singles = [decoded, failed]
        else:
            singles = [0]
        family_everywhere(gpu_lib, name, words, max_iter, rule, want, singles)
        if max_iter >= R.HALF_MAX_ITER:
            behind_the_deinterleaver(gpu_lib, name, words, max_iter, rule, want)


# ---- FT8 / FT4 ---------------------------------------------------------------------------
def _tuples(rec):
    return [(r["payload"].tobytes(), int(r["status"]), int(r["iterations"]), int(r["errors"])) for r in np.atleast_1d(rec).ravel()]


@pytest.mark.parametrize("case", T.KNIFE_CASES, ids=FT_IDS)
@pytest.mark.parametrize("protocol", T.PROTOCOLS)
def test_ft_knife_words(gpu_lib, protocol, case):
    """The whole record (payload, status, iterations, errors, padding) and plain: the device on
    the whole set and on every word alone = the host decoder = the restatement."""
    rule, depth = case
    words, balanced, _ = T.knife_set(protocol, rule, depth)
    words = np.array(words)
    for max_iter in (depth, depth + 1):
        plain, errors, iterations = T.decode_batch(words, max_iter, rule)
        want = T.records(protocol, plain, errors, iterations)
        if max_iter == depth:
            assert all(plain[w, held].all() for w, held in enumerate(balanced)) and (iterations == depth).all()
        host = [gpu_lib.ldpc_decode_host(x, protocol, rule, max_iter) for x in words]
        assert _tuples(np.array([h[0] for h in host])) == want and np.array_equal(np.array([h[1] for h in host]), plain)
        res, got_plain = gpu_lib.ldpc_decode_batch(words, protocol, rule, max_iter, return_plain=True)
        assert res.shape == (len(words),) and _tuples(res) == want and not res["pad"].any()
        assert got_plain.dtype == np.uint8 and np.array_equal(got_plain, plain), np.argwhere(got_plain != plain)[:8]
        assert res.tobytes() == np.array([h[0] for h in host]).tobytes()
        for w in range(len(words)) if max_iter == depth else [0]:
            one, one_plain = gpu_lib.ldpc_decode_batch(words[w:w + 1], protocol, rule, max_iter, return_plain=True)
            assert one.tobytes() == res[w:w + 1].tobytes() and np.array_equal(one_plain[0], plain[w]), w
