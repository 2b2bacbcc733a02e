"""GPU: the batched LDPC(174,91) + CRC-14 decode (csrc/k_ldpc.hip) and the ft8_decode /
ft4_decode pipeline against tests/np_ref_ldpc.py, everything exact.

The batch is np_ref_ldpc.batch (96 noisy words and the edge cases, decoded once per rule by
the restatement and shared). The smallest launch that can go wrong is one codeword; the
whole batch puts workgroups that exit at once next to neighbours that run all 20
iterations.

End to end: an encoded frame (payload bits from default_rng(7)) in the suite's search
buffer, 2 symbols late and 5 bins up, complex Gaussian noise from default_rng(11). The
noise powers were chosen on the CPU with the restatement's own sync:
  FT8  150: top candidate has 0 hard errors;  300: 4 hard errors, sum_product converges in 1 iteration
  FT4   40: 0 hard errors;                    100: 4 hard errors, sum_product converges in 2 iterations
(under the reference rule the high-power words end with 12 (FT8) and 6 (FT4) checks unsatisfied)."""
import functools

import numpy as np
import pytest

import np_ref_ldpc as R
import np_ref_sync as S

pytestmark = pytest.mark.gpu

PROTOCOLS = ("ft8", "ft4")
POWERS = {"ft8": (150.0, 300.0), "ft4": (40.0, 100.0)}
FIELDS = ("payload", "status", "iterations", "errors")


def _tuples(rec):
    rec = np.atleast_1d(rec)
    return [(r["payload"].tobytes(), int(r["status"]), int(r["iterations"]), int(r["errors"])) for r in rec.ravel()]


@functools.lru_cache(maxsize=None)
def _want(protocol, rule, max_iter=20):
    if max_iter == 20:
        plain, errors, iterations = R.batch_decoded(protocol, rule)
    else:
        plain, errors, iterations = R.decode_batch(R.batch(protocol)[0], max_iter, rule)
    return R.records(protocol, plain, errors, iterations), plain


# ---- 1. the batch and the edge cases, exact ------------------------------------------
@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_whole_batch_equals_the_restatement(gpu_lib, protocol, rule):
    import orion_sdr

    llr, names, _ = R.batch(protocol)
    want, want_plain = _want(protocol, rule)
    res, plain = orion_sdr.ldpc_decode_batch(np.array(llr), protocol, rule, 20, return_plain=True)
    assert res.dtype == orion_sdr.RESULT_DTYPE and res.shape == (len(names),) and plain.shape == (len(names), 174)
    got = _tuples(res)
    bad = [names[k] for k in range(len(names)) if got[k] != want[k] or not np.array_equal(plain[k], want_plain[k])]
    assert not bad, bad
    assert not res["pad"].any()


@pytest.mark.parametrize("rule", R.RULES)
def test_one_and_three_codewords(gpu_lib, rule):
    """Launches of 1 and 3 workgroups, over every word of the batch in turn for size 1 would
    be slow: the words chosen run 0, a few and all 20 iterations."""
    import orion_sdr

    llr, names, _ = R.batch("ft8")
    want, want_plain = _want("ft8", rule)
    _, _, iterations = R.batch_decoded("ft8", "sum_product")
    at_once = int(np.flatnonzero(iterations == 0)[0])
    some = int(np.flatnonzero((iterations >= 3) & (iterations < 20))[0])
    full = int(np.flatnonzero(iterations == 20)[0])
    for k in (at_once, some, full, names.index("zeros"), names.index("nan3"), names.index("flip1/1")):
        res, plain = orion_sdr.ldpc_decode_batch(np.array(llr[k:k + 1]), "ft8", rule, return_plain=True)
        assert _tuples(res) == [want[k]] and np.array_equal(plain[0], want_plain[k]), names[k]
        res = orion_sdr.ldpc_decode_batch(np.array(llr[k]), "ft8", rule)  # shape [174] -> a 0-d record array
        assert res.shape == () and _tuples(res) == [want[k]]
    idx = [full, at_once, some]
    res, plain = orion_sdr.ldpc_decode_batch(np.array(llr[idx]), "ft8", rule, return_plain=True)
    assert _tuples(res) == [want[k] for k in idx] and np.array_equal(plain, want_plain[idx])


@pytest.mark.parametrize("max_iter", [0, 1])
@pytest.mark.parametrize("rule", R.RULES)
def test_max_iter_0_and_1(gpu_lib, rule, max_iter):
    import orion_sdr

    llr, names, _ = R.batch("ft8")
    want, want_plain = _want("ft8", rule, max_iter)
    res, plain = orion_sdr.ldpc_decode_batch(np.array(llr), "ft8", rule, max_iter, return_plain=True)
    assert _tuples(res) == want and np.array_equal(plain, want_plain)


# ---- 2. the entry points agree ----------------------------------------------------------
def test_entry_points_agree(gpu_lib):
    import torch

    import orion_sdr

    llr, names, _ = R.batch("ft4")
    x = np.array(llr)
    for rule in R.RULES:
        host, host_plain = orion_sdr.ldpc_decode_batch(x, "ft4", rule, return_plain=True)
        dev, dev_plain = orion_sdr.ldpc_decode_batch(torch.from_numpy(x).cuda(), "ft4", rule, return_plain=True)
        assert host.tobytes() == dev.tobytes() and host_plain.tobytes() == dev_plain.tobytes()
        assert orion_sdr.ldpc_decode_batch(x, "ft4", rule).tobytes() == host.tobytes()
        assert orion_sdr.ldpc_decode_batch(torch.from_numpy(x).cuda(), "ft4", rule).tobytes() == host.tobytes()


def test_sync_layout_skips_unused_slots(gpu_lib):
    """[nch][max_cand][174] with count: the same records as the flat layout in the used
    slots; the unused ones all zero (status 0) and not decoded, although valid words sit
    in them."""
    import torch

    import orion_sdr

    llr, names, _ = R.batch("ft8")
    nch, mc = 3, 7
    x = np.array(llr[:nch * mc]).reshape(nch, mc, 174)
    x[1, 5] = llr[names.index("inf")]  # a valid word in a slot past the count
    count = np.array([mc, 4, 0], np.uint32)
    flat = orion_sdr.ldpc_decode_batch(x.reshape(-1, 174), "ft8", "sum_product").reshape(nch, mc)
    assert flat[1, 5]["status"] == 2
    for arr, cnt in ((x, count), (torch.from_numpy(x).cuda(), torch.from_numpy(count.view(np.int32)).cuda())):
        res, plain = orion_sdr.ldpc_decode_batch(arr, "ft8", "sum_product", count=cnt, return_plain=True)
        assert res.shape == (nch, mc)
        for ch in range(nch):
            k = int(count[ch])
            assert res[ch, :k].tobytes() == flat[ch, :k].tobytes()
            assert res[ch, k:].tobytes() == bytes(16 * (mc - k)) and not plain[ch, k:].any()


# ---- 3. reference versus sum_product ------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_one_wrong_bit_fails_under_reference_and_decodes_under_sum_product(gpu_lib, protocol):
    import orion_sdr

    llr, names, payloads = R.batch(protocol)
    idx = [k for k, n in enumerate(names) if n.startswith("flip1/")]
    assert len(idx) == 4
    x = np.array(llr[idx])
    assert (R.count_errors((x <= 0).astype(np.uint8)) > 0).all()
    ref = orion_sdr.ldpc_decode_batch(x, protocol, "reference")
    sp = orion_sdr.ldpc_decode_batch(x, protocol, "sum_product")
    assert (ref["status"] == 0).all() and (ref["iterations"] == 20).all() and (ref["errors"] > 0).all()
    assert (sp["status"] == 2).all() and [r["payload"].tobytes() for r in sp] == [payloads[k] for k in idx]


# ---- 4. end to end ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _buffer(protocol, power, late=S.LATE_SYMS):
    iq = R.search_buffer(protocol, R.frame_payload(7), power, late)
    iq.setflags(write=False)
    return iq


def _max_hz(protocol):
    mode = S.FT8 if protocol == "ft8" else S.FT4
    return float(np.float32(S.BASE_HZ) + np.float32(10.0) * mode["spacing"])


def _decode(protocol, iq, rule, batch=False):
    import orion_sdr

    fn = getattr(orion_sdr, f"{protocol}_decode" + ("_batch" if batch else ""))
    return fn(iq, S.FS, S.BASE_HZ, _max_hz(protocol), S.T_MIN, S.T_MAX, S.MAX_CAND, rule=rule)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_end_to_end(gpu_lib, protocol):
    import orion_sdr

    mode = S.FT8 if protocol == "ft8" else S.FT4
    payload = R.frame_payload(7)
    bits = R.codeword_bits(protocol, payload)
    low, high = POWERS[protocol]
    for power in (low, high):
        iq = np.array(_buffer(protocol, power))
        sync = getattr(orion_sdr, f"{protocol}_sync")(iq, S.FS, S.BASE_HZ, _max_hz(protocol), S.T_MIN, S.T_MAX, S.MAX_CAND)
        for rule in R.RULES:
            out = _decode(protocol, iq, rule)
            # the sync outputs are the sync call's own
            assert len(out["candidates"]) == len(sync) == S.MAX_CAND
            for c, s in zip(out["candidates"], sync):
                assert (c["time_sym"], c["freq_bin"], c["score"]) == (s["time_sym"], s["freq_bin"], s["score"])
            assert out["llr"].tobytes() == np.array([s["llr"] for s in sync]).tobytes()
            top = out["candidates"][0]
            assert (top["time_sym"], top["freq_bin"]) == (S.LATE_SYMS, S.UP_BINS)
            hard = int((((out["llr"][0] <= 0).astype(np.uint8)) != bits).sum())
            print(f"{protocol} power {power} {rule}: {hard} hard errors in the top candidate, "
                  f"record {_tuples(out['results'][0])[0][1:]}")
            # every record equals the restatement run on the device's own LLRs
            plain, errors, iterations = R.decode_batch(out["llr"], 20, rule)
            assert _tuples(out["results"]) == R.records(protocol, plain, errors, iterations)
            if power == low:
                assert hard == 0
                assert out["first_ok"] == 0 and out["payload"] == payload
            else:
                assert 1 <= hard <= 12
                if rule == "reference":
                    assert out["first_ok"] == -1 and out["payload"] is None and out["carrier_hz"] is None
                else:
                    assert out["first_ok"] == 0 and out["payload"] == payload
            if out["first_ok"] == 0:
                carrier = np.float32(S.BASE_HZ) + np.float32(top["freq_bin"]) * mode["spacing"]
                assert np.float32(out["carrier_hz"]) == carrier and out["snr_db"] == top["score"]


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_batched_pipeline_equals_per_channel_calls(gpu_lib, protocol):
    import torch

    high = POWERS[protocol][1]
    iq = np.stack([_buffer(protocol, high, late) for late in (0, 1, 2)])
    for arr in (iq, torch.from_numpy(iq).cuda()):
        outs = _decode(protocol, arr, "sum_product", batch=True)
        assert len(outs) == 3
        for ch, out in enumerate(outs):
            one = _decode(protocol, np.array(iq[ch]), "sum_product")
            assert out["candidates"] == one["candidates"] and out["llr"].tobytes() == one["llr"].tobytes()
            assert out["results"].tobytes() == one["results"].tobytes()
            assert (out["first_ok"], out["payload"], out["carrier_hz"], out["snr_db"]) == \
                (one["first_ok"], one["payload"], one["carrier_hz"], one["snr_db"])
            assert out["first_ok"] == 0 and out["payload"] == R.frame_payload(7)
            assert out["candidates"][0]["time_sym"] == ch


# ---- 5. bad arguments ------------------------------------------------------------------------
def test_bad_arguments(gpu_lib):
    import orion_sdr

    x = np.zeros((2, 174), np.float32)
    with pytest.raises(orion_sdr.OrionError, match="error -3"):
        orion_sdr.ldpc_decode_batch(x, "ft8", rule=2)
    with pytest.raises(orion_sdr.OrionError, match="error -3"):
        orion_sdr.ldpc_decode_batch(x, "ft8", max_iter=256)
    iq = np.zeros(4000, np.complex64)
    with pytest.raises(orion_sdr.OrionError, match="error -3"):
        orion_sdr.ft8_decode(iq, S.FS, S.BASE_HZ, _max_hz("ft8"), 0, 0, 2, rule=7)
    with pytest.raises(orion_sdr.OrionError, match="error -3"):
        orion_sdr.ft4_decode(iq, S.FS, S.BASE_HZ, _max_hz("ft4"), 0, 0, 2, max_iter=256)
    with pytest.raises(ValueError):
        orion_sdr.ldpc_decode_batch(np.zeros((2, 173), np.float32), "ft8")
