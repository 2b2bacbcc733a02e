"""GPU: the batched OFDM burst acquisition (orion_sdr.ofdm_sync_batch over k_acquire.hip) against
the library's host layer (ofdm_sync, ofdm_sc_metric, earliest_accepted, ofdm_integer_cfo,
themselves held to tests/np_ref_acquire.py by tests/test_acquire_oracle.py): p, r, score, the kept
mask, r_peak, the first five of the ranking in order, earliest_accepted's choice and its score for
equality (floats as uint32); cfo_hz within 7 ulp (6 for the OpenCL-profile atan2 bound the device
library follows, one for the division), in absolute terms near zero; the integer offsets where the
host's own runner-up correlation is at most a quarter of its best. Captures straddle more than
one 256-offset workgroup and its LDS halo; one preamble walks further than a wave is wide, one
takes the global-memory path.

And the batched burst receiver (OfdmBurstDemod.receive_frames) against receive per capture, on the
decisive and structural captures of tests/test_acquire_oracle.py in one batch, from numpy and from
a CUDA tensor on a caller's stream: status, start, consume_to, header fields, payload and flags for
equality; the corrected IQ against the host Rotator recurrence driven by the device's own total
offset, max |d| / |x| <= D + 1e-6 with D the recurrence's own distance from the f64 closed form of
the same f32 step (computed here), 1e-6 the project's closed-form tolerance; the equalized symbols
after the phase tracker by nrmse against the restatement in float64 fed the device's corrected
rows, e_dev <= 4 e_host (the wave reduction's order and the device's atan2 and sincos may each add
about one host-sized rounding error, one to spare). Measured on an MI355X: cfo_hz at most 4 ulp;
corrected IQ 2.85e-5 against 2.9e-5 (D = 2.8e-5); e_host / e_dev between 1.37e-7 and 1.81e-7, equal
to three digits. The two-frame capture keeps the reference's quirk; decode_frames is unchanged."""
import numpy as np
import pytest

import np_ref_acquire as A
import np_ref_frame as R
from test_frame_layer_oracle import Z32, ZC, links

pytestmark = pytest.mark.gpu
FS = 1e6
PREAMBLES = [((2, 32), True), ((3, 16), True), ((2, 32), False), ((3, 6), False)]


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def batch_of(lib, prm, training):
    """(preamble, captures (5, 300 + frame length)): three frames at different offsets, carrier
    offsets and phases, one capture of noise alone, one that starts with a stretch of zeros."""
    cfg, t, pre, _ = links(lib, preamble=prm, training=training)
    mod = lib.OfdmFrameMod(cfg, t, pre)
    f = mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(3, 1), R.payload(40, 1)))
    n = 300 + f.size
    rows = [A.impair(f, off, cfo, ph, A.SIGMA, 10 + k, total=n) for k, (off, cfo, ph) in enumerate(A.OFFSETS)]
    rows.append(A.impair(f[:0], 0, 0.0, 0.0, A.SIGMA, 20, total=n))
    z = A.impair(f, 250, 9000.0, 0.3, A.SIGMA, 21, total=n)
    z[:150] = 0
    rows.append(z)
    return pre, np.stack(rows)


def cfo_distance(got, want, fs, repeat_len):
    """|got - want| in ulps of want, of the threshold (fs / (2 repeat_len)) 2^-12 below it."""
    floor = np.float32(fs / (2 * repeat_len) * 2.0 ** -12)
    ulp = np.spacing(np.maximum(np.abs(want), floor).astype(np.float32))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp.astype(np.float64)


def check_sync(lib, pre, x, out, start, end, thr=0.5, left_out=None):
    """Every output of ofdm_sync_batch for captures x against the host; returns the largest
    cfo_hz distance in ulps. left_out (a list) collects (capture, rank) of every candidate whose
    integer offset the decisiveness guard did not compare."""
    worst = 0.0
    for c in range(len(x)):
        p, r = lib.ofdm_sc_metric(x[c], FS, pre, start, end)
        res = lib.ofdm_sync(x[c], FS, pre, start, end)
        assert out["p"].shape[1] == p.size
        assert np.array_equal(u32(out["p"][c]), u32(p)) and np.array_equal(u32(out["r"][c]), u32(r)), c
        score, cfo = np.full(p.size, -1.0, np.float32), np.zeros(p.size, np.float32)
        for q in res:
            score[q.start_sample - start], cfo[q.start_sample - start] = q.score, q.cfo_hz
        kept = r > 0
        assert len(res) == int(kept.sum()) and np.array_equal(out["score"][c] >= 0, kept), c
        assert np.array_equal(u32(out["score"][c]), u32(score)), c
        assert u32(out["r_peak"][c:c + 1])[0] == u32(np.array([r[kept].max() if kept.any() else 0], np.float32))[0], c
        if kept.any():
            worst = max(worst, float(cfo_distance(out["cfo_hz"][c][kept], cfo[kept], FS, pre.repeat_len).max()))
        top = [q.start_sample for q in res[:5]] + [-1] * (5 - min(5, len(res)))
        assert out["top_start"][c].tolist() == top, c
        for j, q in enumerate(res[:5]):
            if pre.training:
                bins, c2 = lib.ofdm_integer_cfo(x[c], FS, pre.training[0], pre.training[1],
                                                q.start_sample + pre.num_repeats * pre.repeat_len, q.cfo_hz, corr=True)
                assert bins == q.integer_cfo_bins
                c2 = np.sort(c2.astype(np.float64))
                if c2[-2] <= 0.25 * c2[-1]:  # decisive on the host's own values
                    assert int(out["top_bins"][c][j]) == bins, (c, j)
                elif left_out is not None:
                    left_out.append((c, j))
            else:
                assert int(out["top_bins"][c][j]) == 0
        best = lib.earliest_accepted(res, thr, pre.total_len)
        if best is None:
            assert int(out["accepted_start"][c]) == -1 and int(out["accepted_in_top"][c]) == -1, c
            assert int(out["accepted_integer_cfo_bins"][c]) == 0
            continue
        assert int(out["accepted_start"][c]) == best.start_sample, c
        assert u32(out["accepted_score"][c:c + 1])[0] == u32(np.array([best.score], np.float32))[0], c
        k = best.start_sample - start
        assert u32(out["accepted_cfo_hz"][c:c + 1])[0] == u32(out["cfo_hz"][c][k:k + 1])[0], c
        where = top.index(best.start_sample) if best.start_sample in top else -1
        assert int(out["accepted_in_top"][c]) == where, c
        want = int(out["top_bins"][c][where]) if where >= 0 else 0
        assert int(out["accepted_integer_cfo_bins"][c]) == want, c
    return worst


@pytest.mark.parametrize("prm,training", PREAMBLES, ids=str)
def test_sync_batch_equals_ofdm_sync(gpu_lib, prm, training):
    from conftest import report

    lib = gpu_lib
    pre, x = batch_of(lib, prm, training)
    worst = 0.0
    for start, end in ((0, x.shape[1]), (7, x.shape[1] + 99), (7, 600)):
        out = lib.ofdm_sync_batch(x, FS, pre, start, end)
        nd = min(end, x.shape[1] - pre.total_len) - start
        assert nd > 256 and out["p"].shape == (5, nd)  # more than one workgroup of offsets
        worst = max(worst, check_sync(lib, pre, x, out, start, end))
        if start == 0:
            for k, (off, _, _) in enumerate(A.OFFSETS):  # the frames are found at their exact starts
                assert int(out["accepted_start"][k]) == off == int(out["top_start"][k][0])
            if prm == (2, 32):
                assert int(out["accepted_start"][3]) == -1  # noise alone: nothing accepted
                if training:
                    assert out["accepted_integer_cfo_bins"][:3].tolist() == [-2, 0, 2]
            assert (out["score"][4] < 0).any() and int(out["accepted_start"][4]) == 250  # the zero stretch is skipped
    report(f"ofdm_sync_batch cfo_hz vs host, preamble {prm} [ulp]", worst, 7.0)


def test_sync_batch_long_walk_and_global_path(gpu_lib):
    """n_fft 256 with repeat_len 128: a lane walks 128 terms, more than a wave is wide, through
    LDS; then 32 repeats of 128, whose 256 + 4096 samples exceed the LDS budget (the global path)."""
    from conftest import report

    lib = gpu_lib
    data = np.array([i for i in range(-100, 101) if i != 0], np.int32)
    cfg = lib.OfdmConfig(256, 16, data, Z32, ZC, FS, 0.0, 1.0, "qpsk")
    rng = np.random.default_rng(5)
    for num, rl, training in ((2, 128, True), (32, 128, False)):
        pre = lib.OfdmPreamble(num, rl)
        if training:
            pre = pre.with_training_symbol(256, 16)
        lead = lib.generate_ofdm_preamble(cfg, num, rl, *(pre.training or (None, None)))
        body = ((rng.standard_normal(600) + 1j * rng.standard_normal(600)) * 0.04).astype(np.complex64)
        f = np.concatenate([lead, body])
        x = np.stack([A.impair(f, off, cfo, ph, A.SIGMA, 30 + k, total=f.size + 300)
                      for k, (off, cfo, ph) in enumerate(((3, 1500.0, 0.1), (270, -9000.0, 2.5)))])
        out = lib.ofdm_sync_batch(x, FS, pre, 0, x.shape[1])
        worst = check_sync(lib, pre, x, out, 0, x.shape[1])
        assert out["accepted_start"].tolist() == [3, 270]
        report(f"ofdm_sync_batch cfo_hz vs host, preamble ({num}, {rl}) [ulp]", worst, 7.0)


def test_sync_batch_resident_on_a_stream_and_empty_ranges(gpu_lib):
    import torch

    lib = gpu_lib
    pre, x = batch_of(lib, (2, 32), True)
    want = lib.ofdm_sync_batch(x, FS, pre, 0, x.shape[1])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
    s.synchronize()
    got = lib.ofdm_sync_batch(xt, FS, pre, 0, x.shape[1], stream=s.cuda_stream)
    s.synchronize()
    for k, v in want.items():
        assert got[k].is_cuda and np.array_equal(u32(got[k].cpu().numpy()), u32(v)), k
    for args in ((0, 100, lib.OfdmPreamble(1, 32)), (500, 400, pre), (x.shape[1], x.shape[1] + 5, pre)):
        out = lib.ofdm_sync_batch(x, FS, args[2], args[0], args[1])
        assert out["p"].shape == (5, 0) and (out["accepted_start"] == -1).all() and (out["top_start"] == -1).all()
    with pytest.raises(ValueError):
        lib.ofdm_sync_batch(x[0], FS, pre, 0, 10)


# ---- the burst receiver ----------------------------------------------------------------------
def test_two_frame_capture_keeps_the_reference_quirk(gpu_lib):
    """The earliest accepted start is not among the five searched candidates: bins 0, and the
    frame, two spacings off, fails its header."""
    from test_acquire_oracle import two_frames

    lib = gpu_lib
    cfg, t, pre, _ = links(lib)
    x = np.stack([two_frames()])
    out = lib.ofdm_sync_batch(x, FS, pre, 0, x.shape[1])
    check_sync(lib, pre, x, out, 0, x.shape[1])
    assert int(out["accepted_start"][0]) == 50 and int(out["accepted_in_top"][0]) == -1
    assert int(out["accepted_integer_cfo_bins"][0]) == 0
    got = lib.OfdmBurstDemod(cfg, t, pre).receive_frames(x)
    assert int(got["status"][0]) == lib.RX_ERRORS["header_crc_mismatch"] and int(got["consume_to"][0]) == 50 + pre.total_len


def closed_form_distance(lib, total_cfo, n):
    """The largest distance between the host Rotator recurrence and the f64 closed form of the
    same f32 step, over n outputs."""
    phi = np.float64(np.float32(np.float32(np.float32(2.0 * np.pi) * np.float32(-total_cfo)) / np.float32(FS)))
    rec = lib.ofdm_rotator(-float(total_cfo), FS, n).astype(np.complex128)
    return float(np.abs(rec - np.exp(1j * phi * np.arange(1, n + 1))).max())


def check_receive(lib, bd, link, names, x, out, symbols=True):
    from conftest import nrmse, report

    pre, pre_len, n = bd.preamble, bd.preamble.total_len, x.shape[1]
    worst_iq, bound_iq, figures = 0.0, 0.0, []
    for k, name in enumerate(names):
        step = bd.receive(np.ascontiguousarray(x[k]))
        if step is None:
            assert int(out["status"][k]) == -1 and int(out["consume_to"][k]) == 0 and out["payloads"][k].size == 0, name
            continue
        assert int(out["status"][k]) == (step.error.code if step.error else 0), name
        assert int(out["start_sample"][k]) == step.timing_offset_samples and int(out["consume_to"][k]) == step.consume_to, name
        assert u32(out["sync_score"][k:k + 1])[0] == u32(np.array([step.sync_score], np.float32))[0], name
        frac = lib.earliest_accepted(lib.ofdm_sync(np.ascontiguousarray(x[k]), FS, pre, 0, n), bd.score_threshold, pre_len).cfo_hz
        floor = np.float32(FS / (2 * pre.repeat_len) * 2.0 ** -12)
        tol = 7 * float(np.spacing(max(abs(np.float32(frac)), floor))) + float(np.spacing(np.abs(step.cfo_hz)))
        assert abs(float(out["cfo_hz"][k]) - float(step.cfo_hz)) <= tol, name
        if step.error is None:
            md = step.packet.metadata
            assert (int(out["mcs_index"][k]), int(out["sequence_num"][k]), int(out["flags"][k])) == \
                (md.mcs_index, md.sequence_num, md.flags), name
            assert int(out["payload_len"][k]) == step.packet.payload.size and np.array_equal(out["payloads"][k], step.packet.payload)
            assert (bool(out["inner_ok"][k]), bool(out["outer_ok"][k]), bool(out["crc_ok"][k])) == \
                (step.inner_ok, step.outer_ok, step.crc_ok), name
        else:
            assert out["payloads"][k].size == 0
        if "corrected" not in out:
            continue
        # the corrected rows against the host recurrence driven by the device's own total offset
        st, total = step.timing_offset_samples, out["cfo_hz"][k]
        src = np.ascontiguousarray(x[k][st:])
        want = lib.ofdm_rotate_block(src, -float(total), FS)
        got = out["corrected"][k]
        assert not got[src.size:].any(), name
        worst_iq = max(worst_iq, float((np.abs(got[:src.size].astype(np.complex128) - want) / np.abs(src)).max()))
        bound_iq = max(bound_iq, closed_form_distance(lib, total, src.size))
        if step.error is None and symbols:
            # the equalized symbols: the restatement in float64 fed the device's own corrected rows is
            # the yardstick; the float32 host path on the same rows sets the scale
            row = np.ascontiguousarray(got[:src.size])
            mcs = bd.mcs_table.get(md.mcs_index)
            nsym = bd.payload_symbols(mcs, lib.block_plan(step.packet.payload.size, bd.scheme(mcs)))
            body = row[pre_len + bd.header_symbols * bd.sps:]
            truth = A.soft_demap_eq(link, mcs.constellation, body, nsym,
                                    A.equalizer_weights(A.estimate_channel(link, row, A.D), A.D), A.D)[1]
            host = bd._demap_host(mcs.constellation, body, nsym, bd._channel_host(row))[1]
            figures.append((name, nrmse(host, truth), nrmse(out["symbols"][k], truth)))
    if "corrected" in out:
        report("receive_frames corrected IQ vs host Rotator, max |d| / |x|", worst_iq, bound_iq + 1e-6)
        for name, e_host, e_dev in figures:
            print(f"[parity] receive_frames {name}: e_host {e_host:.3e}")
            report(f"receive_frames {name}: equalized symbols, e_dev (tol 4 e_host)", e_dev, 4 * e_host)
    return figures


def test_receive_frames_equals_receive(gpu_lib):
    from test_acquire_oracle import cases

    lib = gpu_lib
    cfg, t, pre, link, c = cases()
    names = list(c)
    x = np.stack([c[k][0] for k in names])
    bd = lib.OfdmBurstDemod(cfg, t, pre)
    out = bd.receive_frames(x, debug=True)
    figures = check_receive(lib, bd, link, names, x, out)
    assert len(figures) == 6 and [int(s) for s in out["status"]] == [0] * 6 + [-1, -1, 3, 2]
    plain = bd.receive_frames(x)
    assert "corrected" not in plain and all(np.array_equal(plain[k], out[k]) for k in plain if k != "payloads")
    assert all(np.array_equal(a, b) for a, b in zip(plain["payloads"], out["payloads"]))
    # too short for a preamble and a symbol: need more everywhere; no training symbol: a host matter
    assert (bd.receive_frames(x[:, :pre.total_len + 71])["status"] == -1).all()
    cfg2, t2, pre2, _ = links(lib, training=False)
    with pytest.raises(ValueError):
        lib.OfdmBurstDemod(cfg2, t2, pre2).receive_frames(x)


def test_receive_frames_resident_on_a_stream(gpu_lib):
    import torch

    from test_acquire_oracle import cases

    lib = gpu_lib
    cfg, t, pre, link, c = cases()
    names = list(c)
    x = np.stack([c[k][0] for k in names])
    bd = lib.OfdmBurstDemod(cfg, t, pre)
    want = bd.receive_frames(x, debug=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
    s.synchronize()
    got = bd.receive_frames(xt, stream=s.cuda_stream, debug=True)
    s.synchronize()
    assert got["corrected"].is_cuda and got["weights"].is_cuda
    for k in want:
        if k in ("payloads", "symbols"):
            assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(want[k], got[k])), k
        elif k in ("corrected", "weights"):
            assert np.array_equal(u32(got[k].cpu().numpy()), u32(want[k])), k
        else:
            assert np.array_equal(want[k], got[k]), k


def test_decode_frames_is_unchanged(gpu_lib):
    """A sanity call after the shared part of decode_frames moved: the noisy known-start set and
    a row cut short, every field against the host decoder."""
    from test_gpu_frame_layer import check_frames

    lib = gpu_lib
    cfg, t, _, _ = links(lib)
    dem = lib.OfdmFrameDemod(cfg, t)
    _, rx = R.noisy_frame_set()
    rx = rx[:8].copy()
    check_frames(lib, dem, rx, dem.decode_frames(rx))
    cut = np.ascontiguousarray(rx[:, :-1])
    out = dem.decode_frames(cut)
    assert (out["error"] == lib.RX_ERRORS["malformed_header"]).all() and all(p.size == 0 for p in out["payloads"])
    check_frames(lib, dem, cut, out)
    assert (dem.decode_frames(rx[:, :100].copy())["error"] == lib.RX_ERRORS["malformed_header"]).all()
