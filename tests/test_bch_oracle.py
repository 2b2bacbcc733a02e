"""CPU: the library's host side of the outer BCH code (csrc/bch.cpp through the C ABI and
orion_sdr.Bch) against tests/np_ref_bch.py, byte for byte: the generator, the LFSR encoder, the
decoder's messages, status words and locator lengths on every row of the input set (words that
hold byte values other than 0 and 1); the paths that set must hold; the bound on the locator
vector; the reference's own properties (tests/unit/fec.rs:428-520); and the argument errors of
every entry, the device entries' before any launch. The host code runs under the sanitizers in
tests/test_ldpc_family_oracle.py's stand-alone program."""
import numpy as np
import pytest

import np_ref_bch as R


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


@pytest.fixture(scope="module")
def decoded():
    """Every row's input set through the restatement, once: row -> (sent, words, msgs, status, info)."""
    out = {}
    for row in R.ROWS:
        sent, words = R.make_words(*row)
        out[row] = (sent, words) + R.decode(row[0], row[1], words)
    return out


def test_generator_and_dimensions(lib):
    for t, pb in [(1, 8), (2, 16), (3, 24), (8, 64), (16, 124), (31, 200)]:
        c = lib.Bch(t)
        assert (c.n, c.t, c.parity_bits, c.k) == (255, t, pb, 255 - pb) and R.dims(255, t) == (255 - pb, pb)
        g = c.generator()
        assert g.dtype == np.uint8 and np.array_equal(g, R.generator(t)) and g[0] == 1 and g[-1] == 1
    assert lib.Bch(1).generator().tolist() == [1, 0, 0, 0, 1, 1, 1, 0, 1]  # the field's polynomial 0x11D
    f = lib.Bch.for_info_bits(8)
    assert (f.n, f.k, f.t, f.parity_bits) == (184, 120, 8, 64) and lib.BCH_INFO_BITS == 120
    assert (lib.Bch.for_info_bits(1, 1).n, lib.Bch.for_info_bits(3, 100).n) == (9, 124)


@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: f"bch{r[0]}_t{r[1]}_e{r[2]}")
def test_encode_and_decode_equal_the_restatement(lib, decoded, row):
    n, t, _ = row
    sent, words, msgs, status, info = decoded[row]
    c = lib.Bch(t, n)
    assert np.array_equal(c.encode(sent), R.encode(n, t, sent)) and np.array_equal(c.encode(sent[0]), R.encode(n, t, sent[:1])[0])
    raw = words[:, :c.k]  # byte values other than 0 / 1: copied as they are, bit 0 in the parity
    assert np.array_equal(c.encode(raw), R.encode(n, t, raw))
    hm, hs, hl = c.decode_counted(words, locator_len=True)
    assert hs.dtype == np.int32 and np.array_equal(hs, status), np.flatnonzero(hs != status)[:8]
    assert np.array_equal(hm, msgs)
    assert hl.tolist() == [i["locator_len"] for i in info]
    # the locator vector never exceeds 2 t + 1 entries (what the kernel's one lane per entry needs)
    assert hl.max() <= 2 * t + 1
    one = c.decode_counted(words[3])
    assert np.array_equal(one[0], msgs[3]) and one[1] == status[3]
    for w in range(len(words)):
        if status[w] < 0:
            assert np.array_equal(hm[w], words[w, :c.k])  # a failed word hands back received[:k]
            with pytest.raises(lib.BchUncorrectable) as e:
                c.decode(words[w])
            assert np.array_equal(e.value.message, words[w, :c.k]) and e.value.errors == -status[w]
        else:
            assert np.array_equal(c.decode(words[w]), msgs[w])


def test_input_set_holds_every_path(decoded):
    """What binds: a clean word, a corrected word, a word rejected by the residual, a root below
    the shortening offset that is not applied, and a miscorrection with status >= 0; words hold
    byte values other than 0 and 1."""
    seen = set()
    for row, (sent, words, msgs, status, info) in decoded.items():
        n, t, errors = row
        assert (words > 1).any()
        for w, rec in enumerate(info):
            seen.add(rec["path"])
            if rec["outside"]:
                seen.add("outside")
                assert n < 255
            right = np.array_equal(msgs[w] != 0, sent[w] != 0)
            if rec["path"] == "fixed":
                assert 0 <= status[w] <= t
                seen.add("corrected" if right and status[w] > 0 else "miscorrected" if not right else "fixed0")
            elif rec["path"] == "clean":
                assert status[w] == 0 and right
            else:
                assert status[w] <= -1
        if errors <= t:  # 0 -> 1 and 1 -> 0 errors within t are corrected, unless the flipped element keeps other bits
            plain = [w for w in range(len(words)) if w % 5 != 4]
            assert all(status[w] == errors for w in plain)
            assert all(np.array_equal(msgs[w] != 0, sent[w] != 0) for w in plain)
    assert {"clean", "corrected", "resid", "outside", "miscorrected"} <= seen, seen
    # every (184, 8) word with an error that arrives as 2 is rejected by the residual: ^= 1 leaves it set
    _, words, _, status, _ = decoded[(184, 8, 4)]
    assert all(status[w] < 0 for w in range(len(words)) if (words[w] == 2).any() and w % 5 == 4)
    # a perfect code: every word of (255, 1) with two errors is miscorrected to a codeword one flip away
    assert (decoded[(255, 1, 2)][3] == 1).all()


# ---- the reference's own properties (tests/unit/fec.rs:428-520) -----------------------------
@pytest.mark.parametrize("t", [1, 2, 3, 8])
def test_corrects_up_to_t_errors_and_is_systematic(lib, t):
    c = lib.Bch(t)
    assert c.n == 255 and c.n - c.k == c.parity_bits and c.k < c.n
    rng = np.random.default_rng([42, t])
    msg = rng.integers(0, 2, c.k, dtype=np.uint8)
    cw = c.encode(msg)
    assert cw.shape == (255,) and np.array_equal(cw[:c.k], msg)
    assert np.array_equal(c.decode(cw), msg)  # zero errors round-trip
    rx = cw.copy()
    rx[rng.choice(255, t, replace=False)] ^= 1
    assert np.array_equal(c.decode(rx), msg)
    assert c.decode_counted(rx)[1] == t


def test_shortened_code_corrects_and_beyond_t_never_returns_the_message(lib):
    c = lib.Bch(3, 128)
    rng = np.random.default_rng(43)
    msg = rng.integers(0, 2, c.k, dtype=np.uint8)
    rx = c.encode(msg)
    rx[[2, 61, 120]] ^= 1
    assert c.n == 128 and np.array_equal(c.decode(rx), msg)
    c = lib.Bch(2)
    msg = rng.integers(0, 2, c.k, dtype=np.uint8)
    rx = c.encode(msg)
    rx[[1, 40, 80, 120, 160, 200]] ^= 1
    got, status = c.decode_counted(rx)
    assert status < 0 or not np.array_equal(got, msg)


# ---- argument errors ------------------------------------------------------------------------
def test_constructor_and_host_argument_errors(lib):
    for bad in ((0, 255), (1, 0), (1, 256), (1, 8), (8, 64), (128, 255), (10 ** 9, 255), (-1, 255)):
        with pytest.raises(ValueError):
            lib.Bch(*bad)
    for bad in ((8, 0), (8, 192), (0, 120)):
        with pytest.raises(ValueError):
            lib.Bch.for_info_bits(*bad)
    assert issubclass(lib.BchUncorrectable, ValueError)
    c = lib.Bch.for_info_bits(8)
    for bad in (lambda: c.encode(np.zeros(119, np.uint8)), lambda: c.encode(np.zeros(120, np.int16)),
                lambda: c.encode(np.zeros((1, 1, 120), np.uint8)), lambda: c.decode_counted(np.zeros(183, np.uint8)),
                lambda: c.decode(np.zeros((2, 184), np.uint8)), lambda: c.decode(list(range(184)))):
        with pytest.raises(ValueError):
            bad()


def test_device_entries_refuse_bad_arguments_before_any_launch(lib):
    """Every check runs before anything touches a device, so this passes without one. The
    device entries hold the locator with one lane per entry, so t stops at 31."""
    bits = np.zeros((2, 400), np.uint8)
    D, E = lib.bch_decode_batch, lib.bch_encode_batch
    for bad in (lambda: D(bits, 0), lambda: D(bits, 32), lambda: D(bits, 8, info_bits=0), lambda: D(bits, 8, info_bits=192),
                lambda: D(bits.astype(np.int8), 8), lambda: D(bits.reshape(2, 2, 200), 8), lambda: D(bits[:, :183], 8),
                lambda: D(bits.astype(np.float32), 8),
                lambda: E(bits, 0), lambda: E(bits, 32), lambda: E(bits, 8, info_bits=300), lambda: E(bits[:, :0], 8),
                lambda: E(bits.astype(np.int32), 8), lambda: E(bits.reshape(2, 2, 200), 8)):
        with pytest.raises(ValueError):
            bad()
    assert lib.Bch(64).t == 64  # the host has no such limit
