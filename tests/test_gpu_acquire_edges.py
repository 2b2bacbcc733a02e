"""GPU: the edges of the burst acquisition (k_acquire.hip under orion_sdr.ofdm_sync_batch and
OfdmBurstDemod.receive_frames) that noisy frames on the link 64 / 8 / 62 never reach.

Exact-arithmetic captures (tests/np_ref_acquire.py): Gaussian integers with parts in -9..9, so
that every product and partial sum of the Schmidl & Cox walk is an integer below 2^24 (asserted)
and p and r are exact in float32 in any summation order: the device and the host must both equal
an int64 reference. They bring what noise never does: all keys equal over 1, 4, 5, 6, 255, 256,
257 and 513 offsets; a tie between the winners and offsets in lower lanes of a later sweep; a
score that equals the threshold; an offset exactly one cluster length past the earliest; two kept
offsets; none. Each capture's edge is asserted on the restatement alone first, then everything the
device returns is held to the host through test_gpu_acquire.check_sync, and a capture run alone
must give the bytes of its row of the batch.

The metric's walk: repeat_len 1, and preambles that stage exactly 4096 samples (the last LDS
launch) and 4099 (the first global one, odd repeat_len), 301 offsets; the rows are of odd length,
8-byte aligned only, wherever num_repeats repeat_len is even.

The half-band tie of the integer search: a decisive frame times (-1)^n. The correlations at
-n_fft / 2 and +n_fft / 2 are the same sum, computed by two lanes (two waves at n_fft 64 and 128,
one lane's two trips at 256); the host's own values are asserted to tie bit for bit, and the
device must answer the lower shift and decode.

Two more link geometries, 128 / 9 with 66 data carriers (137 samples per symbol) and 256 / 16 with
200: receive_frames against receive by test_gpu_acquire.check_receive, from numpy and from a CUDA
tensor on a caller's stream, and ofdm_sync_batch by check_sync, whose decisiveness guard must leave
out no first-ranked candidate of a frame-bearing capture (outside the half-band test). No new
tolerance: equality where the host's bits are claimed, 7 ulp for cfo_hz, D + 1e-6 for the corrected
IQ, e_dev <= 4 e_host for the equalized symbols against the float64 restatement on the device's own
corrected rows.

Measured on an MI355X, equalized symbols, e_host / e_dev (the rule allows e_dev = 4 e_host):
  128 / 9, one batch:   MCS 0, 4 bytes 1.148e-7 / 1.185e-7; MCS 2, 40 bytes 1.214e-7 / 1.267e-7;
                        MCS 3, 300 bytes 1.238e-7 / 1.240e-7
  128 / 9, alone:       1.283e-7 / 1.283e-7; 1.314e-7 / 1.283e-7; 1.238e-7 / 1.240e-7
  256 / 16, one batch:  MCS 2, 40 bytes 1.457e-7 / 1.457e-7; MCS 3, 300 bytes 1.536e-7 / 1.532e-7
  256 / 16, alone:      1.400e-7 / 1.400e-7; 1.536e-7 / 1.532e-7
  half band (shifted, plain): 64 / 8 1.460e-7 / 1.458e-7, 1.343e-7 / 1.343e-7; 128 / 9 1.303e-7 / 1.284e-7,
                        1.314e-7 / 1.283e-7; 256 / 16 1.448e-7 / 1.448e-7, 1.400e-7 / 1.400e-7
The 66 and 200 carriers a wave now reduces leave e_dev within 5 % of e_host. Corrected IQ at most
2.41e-5 against a bound of 2.5e-5; cfo_hz at most 2 ulp from the host on the walk captures."""
import numpy as np
import pytest

import np_ref_acquire as A
from test_acquire_oracle import geometry_cases, half_band_case, half_band_facts, lib_pre
from test_gpu_acquire import FS, check_receive, check_sync, u32

pytestmark = pytest.mark.gpu
FILLER_SEED = 9


def assert_exact_sums(out, c, x, pre, start):
    """Row c of p and r equals the int64 reference, converted to float32."""
    nd = out["p"].shape[1]
    pr, pi, rr, bound = A.sc_sums_exact(x, pre, start, start + nd)
    assert bound < 2 ** 24  # the condition under which any order of summation is exact in f32
    assert np.array_equal(out["p"][c].real, pr.astype(np.float32)) and np.array_equal(out["p"][c].imag, pi.astype(np.float32))
    assert np.array_equal(out["r"][c], rr.astype(np.float32))


def assert_alone_equals_row(lib, x, pre, start, end, thr, out):
    """Every capture of the batch run alone: the same bytes as its row."""
    for c in range(len(x)):
        one = lib.ofdm_sync_batch(np.ascontiguousarray(x[c:c + 1]), FS, pre, start, end, thr)
        for k, v in out.items():
            assert one[k].dtype == v.dtype and one[k].tobytes() == v[c:c + 1].tobytes(), (c, k)


def assert_device_facts(out, c, facts, start=0):
    """Row c of the device's choices against the restatement's facts."""
    assert out["p"].shape[1] == facts["nd"] and int((out["score"][c] >= 0).sum()) == facts["kept"]
    assert float(out["r_peak"][c]) == facts["r_peak"] and out["top_start"][c].tolist() == facts["top"]
    if facts["accepted"] is None:
        assert (int(out["accepted_start"][c]), int(out["accepted_in_top"][c]), int(out["accepted_integer_cfo_bins"][c])) == (-1, -1, 0)
        assert float(out["accepted_score"][c]) == 0.0 and float(out["accepted_cfo_hz"][c]) == 0.0
        return
    assert int(out["accepted_start"][c]) == facts["accepted"] and float(out["accepted_score"][c]) == facts["accepted_score"]
    rank = facts["accepted_rank"]
    assert int(out["accepted_in_top"][c]) == (rank if rank < A.TOP_N else -1)
    if rank >= A.TOP_N:
        assert int(out["accepted_integer_cfo_bins"][c]) == 0
    for d, s in facts["score_at"].items():
        assert float(out["score"][c][d - start]) == s


# ---- A. exact-arithmetic captures ------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.crafted_cases()))
def test_crafted_capture(gpu_lib, name):
    lib = gpu_lib
    pre, cap, thr, want = A.crafted_cases()[name]
    facts = A.crafted_facts(cap, pre, thr)
    A.assert_facts(facts, want)  # the capture holds its edge on the restatement alone
    lp = lib_pre(lib, pre)
    x = np.stack([cap, A.int_noise(cap.size, FILLER_SEED)])  # a second row: the batch stride is live
    out = lib.ofdm_sync_batch(x, FS, lp, 0, cap.size, thr)
    for c in range(2):
        assert_exact_sums(out, c, x[c], pre, 0)
    check_sync(lib, lp, x, out, 0, cap.size, thr)
    assert_device_facts(out, 0, facts)
    assert_device_facts(out, 1, A.crafted_facts(x[1], pre, thr))
    assert_alone_equals_row(lib, x, lp, 0, cap.size, thr, out)


@pytest.mark.parametrize("start,end,nd", A.ONES_RANGES)
def test_all_ones_every_offset_ties(gpu_lib, start, end, nd):
    """score 1 and key 1 at every offset: the ranking is the offsets in order, whatever the lane,
    the wave or the sweep they fall in; nd on either side of five and of the 256 threads."""
    lib = gpu_lib
    pre, lp = (2, 32, None), lib.OfdmPreamble(2, 32)
    x = np.stack([np.ones(900, np.complex64), A.int_noise(900, FILLER_SEED)])
    facts = A.crafted_facts(x[0], pre, 0.5, start, end)
    A.assert_facts(facts, A.ones_facts(start, nd))
    out = lib.ofdm_sync_batch(x, FS, lp, start, end)
    assert out["p"].shape == (2, nd)
    assert (out["p"][0] == 32).all() and (out["r"][0] == 32).all() and (out["score"][0] == 1).all()
    assert not u32(out["cfo_hz"][0]).any()  # atan2(0, 32) / den: exactly +0
    assert out["top_start"][0].tolist() == list(range(start, start + min(nd, 5))) + [-1] * (5 - min(nd, 5))
    assert (int(out["accepted_start"][0]), int(out["accepted_in_top"][0])) == (start, 0)
    for c in range(2):
        assert_exact_sums(out, c, x[c], pre, start)
    check_sync(lib, lp, x, out, start, end)
    assert_device_facts(out, 0, facts, start)
    assert_alone_equals_row(lib, x, lp, start, end, 0.5, out)


# ---- B. the metric kernel's walk and staging limits ------------------------------------------
@pytest.mark.parametrize("num,rl", A.WALKS)
def test_walk_and_staging_limits(gpu_lib, num, rl):
    from conftest import report

    lib = gpu_lib
    pre, lp = (num, rl, None), lib.OfdmPreamble(num, rl)
    caps = A.walk_captures(num, rl)
    x = np.stack([caps["noise"], caps["integers"]])
    n = x.shape[1]
    assert n == num * rl + 301  # odd wherever num rl is even: there the second row is 8-byte aligned only
    out = lib.ofdm_sync_batch(x, FS, lp, 0, n)
    assert out["p"].shape == (2, 301)
    assert_exact_sums(out, 1, x[1], pre, 0)
    worst = check_sync(lib, lp, x, out, 0, n)  # p, r and score bit for bit against the host
    assert_alone_equals_row(lib, x, lp, 0, n, 0.5, out)
    report(f"ofdm_sync_batch cfo_hz vs host, preamble ({num}, {rl}) [ulp]", worst, 7.0)


# ---- C. the half-band tie of the integer search ----------------------------------------------
@pytest.mark.parametrize("geometry", ["64_8"] + list(A.GEOMETRIES))
def test_half_band_tie_takes_the_lower_shift(gpu_lib, geometry):
    lib = gpu_lib
    cfg, t, pre, link, plain, data, start = half_band_case(geometry)
    xh = half_band_facts(lib, cfg, pre, plain, start)  # the tie, on the host's own values
    half = cfg.n_fft // 2
    x = np.stack([xh, plain])
    left = []
    out = lib.ofdm_sync_batch(x, FS, pre, 0, x.shape[1])
    check_sync(lib, pre, x, out, 0, x.shape[1], left_out=left)
    ranked_first = [c for c, j in left if j == 0]
    assert ranked_first == [0]  # the guard leaves out the tie, as it must, and nothing else ranked first
    for k in ("p", "r", "score", "cfo_hz", "top_start"):  # an even repeat_len: the shift changes no sum
        assert out[k][0].tobytes() == out[k][1].tobytes(), k
    assert int(out["top_start"][0][0]) == int(out["accepted_start"][0]) == start and int(out["accepted_in_top"][0]) == 0
    assert int(out["top_bins"][0][0]) == int(out["accepted_integer_cfo_bins"][0]) == -half
    assert int(out["top_bins"][1][0]) == int(out["accepted_integer_cfo_bins"][1]) == 0
    bd = lib.OfdmBurstDemod(cfg, t, pre)
    got = bd.receive_frames(x, debug=True)
    figures = check_receive(lib, bd, link, ["half band", "plain"], x, got)
    assert len(figures) == 2 and got["status"].tolist() == [0, 0]
    assert all(np.array_equal(p, data) for p in got["payloads"])


# ---- D. two more link geometries -------------------------------------------------------------
def resident(lib, bd, x):
    """receive_frames from a CUDA tensor on a stream of the caller's."""
    import torch

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
    s.synchronize()
    got = bd.receive_frames(xt, stream=s.cuda_stream, debug=True)
    s.synchronize()
    assert got["corrected"].is_cuda and got["weights"].is_cuda
    return got


@pytest.mark.parametrize("geometry", list(A.GEOMETRIES))
def test_receive_frames_at_other_geometries(gpu_lib, geometry):
    lib = gpu_lib
    frames = A.GEOMETRIES[geometry][1]
    cfg, t, pre, link, caps = geometry_cases(geometry, True)  # every capture as long as the longest: one batch
    names = list(caps)
    for name in names:  # the restatement alone decodes each
        want = A.receive(link, caps[name][0])
        assert want["error"] == 0 and np.array_equal(want["payload"], caps[name][1][2]) and want["start_sample"] == 77
    x = np.stack([caps[k][0] for k in names])
    bd = lib.OfdmBurstDemod(cfg, t, pre)
    left = []
    sync = lib.ofdm_sync_batch(x, FS, pre, 0, x.shape[1])
    check_sync(lib, pre, x, sync, 0, x.shape[1], left_out=left)
    assert sync["accepted_start"].tolist() == [77] * len(names) and not sync["accepted_integer_cfo_bins"].any()
    out = bd.receive_frames(x, debug=True)
    figures = check_receive(lib, bd, link, names, x, out)
    assert len(figures) == len(names) and not out["status"].any()
    for k, (mi, nbytes, nsym) in enumerate(frames):
        assert out["symbols"][k].shape == (nsym, len(link.data)) and int(out["mcs_index"][k]) == mi
        assert np.array_equal(out["payloads"][k], caps[names[k]][1][2])
    got = resident(lib, bd, x)
    for k in out:
        if k in ("payloads", "symbols"):
            assert all(np.array_equal(a, b) for a, b in zip(out[k], got[k])), k
        elif k in ("corrected", "weights"):
            assert np.array_equal(u32(got[k].cpu().numpy()), u32(out[k])), k
        else:
            assert np.array_equal(out[k], got[k]), k
    # each capture at its own length, 300 samples past its frame, alone
    _, _, _, _, own = geometry_cases(geometry)
    for name in names:
        x1 = own[name][0][None, :].copy()
        s1 = lib.ofdm_sync_batch(x1, FS, pre, 0, x1.shape[1])
        check_sync(lib, pre, x1, s1, 0, x1.shape[1], left_out=left)
        o1 = bd.receive_frames(x1, debug=True)
        assert len(check_receive(lib, bd, link, [name], x1, o1)) == 1 and np.array_equal(o1["payloads"][0], own[name][1][2])
    assert not [c for c, j in left if j == 0]  # the guard left out no first-ranked candidate
