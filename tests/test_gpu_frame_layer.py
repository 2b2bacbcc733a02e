"""GPU: the batched frame layer (OfdmFrameMod.modulate_frames, OfdmFrameDemod.decode_frames and
k_frame_assemble under them) against the library's host layer (modulate_frame / decode, themselves
held to tests/np_ref_frame.py by tests/test_frame_layer_oracle.py), for equality: IQ as uint32 for
both reference concatenations and the DVB-style one, with and without a window; every returned
field of decode_frames on the noisy set, a corrupted header symbol, a longer table at the
transmitter, a row cut short, and one batch mixing two MCS entries and two payload lengths; both
again at the geometries 128 / 9 / 66 carriers and 256 / 16 / 200; torch tensors in and out on a
stream of the caller's."""
import numpy as np
import pytest

import np_ref_frame as R
from test_frame_layer_oracle import links, same32, table

pytestmark = pytest.mark.gpu

LINKS = {
    "ldpc_bch": dict(),
    "conv_rs": dict(mcs=R.CONV_RS_TABLE),
    "dvb": dict(mcs=R.DVB_TABLE, **R.DVB_FRAME),
    "pn_after_per_frame": dict(scrambler=("additive", 0b1001, 7, "per_frame"), scrambler_pos="after_inner"),
}


def host_decode(lib, dem, row):
    """decode as decode_frames reports it: (error, mcs_index, sequence_num, flags, payload)."""
    try:
        p = dem.decode(np.ascontiguousarray(row))
        return 0, p.metadata.mcs_index, p.metadata.sequence_num, p.metadata.flags, p.payload
    except lib.RxError as e:
        return e.code, None, None, None, None


def check_frames(lib, dem, rx, out):
    E = lib.RX_ERRORS
    for k in range(len(rx)):
        err, mi, seq, flags, pay = host_decode(lib, dem, rx[k])
        assert int(out["error"][k]) == err, k
        if err == 0:
            assert (int(out["mcs_index"][k]), int(out["sequence_num"][k]), int(out["flags"][k])) == (mi, seq, flags), k
            assert int(out["payload_len"][k]) == pay.size and np.array_equal(out["payloads"][k], pay), k
            assert out["crc_ok"][k] or dem.f["payload_crc"] == "none"
        else:
            assert out["payloads"][k].size == 0
        if err in (0, E["crc_mismatch"]):  # the payload chain ran: its flags are the host chain's
            mcs = dem.mcs_table.get(int(out["mcs_index"][k]))
            sch = dem.scheme(mcs)
            n = int(out["payload_len"][k])
            nsym = dem.payload_symbols(mcs, lib.block_plan(n, sch))
            nh = dem.header_symbols
            seed = lib.unpack_header_fields(lib.decode_chain(dem._llrs_host("bpsk", rx[k], nh), 14, dem.header_scheme).bytes)[4]
            o = lib.decode_chain(dem._llrs_host(mcs.constellation, rx[k][nh * dem.sps:], nsym), n, sch, seed, dem.f["ldpc_decode_rule"])
            assert (bool(out["inner_ok"][k]), bool(out["outer_ok"][k]), bool(out["crc_ok"][k])) == (o.inner_ok, o.outer_ok, o.crc_ok), k


@pytest.mark.parametrize("roll_off", [0, 2])
@pytest.mark.parametrize("name", list(LINKS))
def test_modulate_frames_equals_modulate_frame(gpu_lib, name, roll_off):
    lib = gpu_lib
    cfg, t, pre, _ = links(lib, roll_off=roll_off, **LINKS[name])
    mod = lib.OfdmFrameMod(cfg, t, pre)
    for mi in range(len(t)):
        for n in (96, 37):
            pay = np.stack([R.payload(n, 10 * k + mi) for k in range(3)])
            seq = np.array([0, 7, 0xFFFFFFFF], np.int64)
            flags = np.array([0, 255, 3], np.int64)
            seeds = np.array([0, 0x12345678, 0xFFFFFFFF], np.int64)
            got = mod.modulate_frames(pay, mi, sequence_nums=seq, flags=flags, seeds=seeds)
            assert got.dtype == np.complex64 and got.shape == (3, mod.frame_len(mi, n))
            for k in range(3):
                f = lib.FramePacket(lib.FrameMetadata(int(seq[k]), mi, int(flags[k])), pay[k])
                assert same32(got[k], mod.modulate_frame(f, int(seeds[k]))), (mi, n, k)
    plain = mod.modulate_frames(pay, 0)  # the defaults: sequence number, flags and seed 0
    assert same32(plain[1], mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(0, 0), pay[1])))


def test_decode_frames_on_the_noisy_set(gpu_lib):
    lib = gpu_lib
    cfg, t, _, _ = links(lib)
    dem = lib.OfdmFrameDemod(cfg, t)
    sent, rx = R.noisy_frame_set()
    out = dem.decode_frames(rx.copy())
    check_frames(lib, dem, rx, out)
    ok = out["error"] == 0
    assert (~ok).any() and (ok & ~out["inner_ok"]).any() and (ok & out["inner_ok"] & out["outer_ok"]).any()
    for k in np.flatnonzero(ok):
        assert np.array_equal(out["payloads"][k], sent[k]) and out["sequence_num"][k] == k


@pytest.mark.parametrize("name", ["conv_rs", "dvb", "pn_after_per_frame"])
def test_decode_frames_other_links(gpu_lib, name):
    lib = gpu_lib
    cfg, t, pre, _ = links(lib, **LINKS[name])
    mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
    pay = np.stack([R.payload(96, k) for k in range(5)])
    iq = mod.modulate_frames(pay, 0, sequence_nums=np.arange(5), seeds=np.arange(5) * 0x01010101)[:, pre.total_len:]
    rx = np.stack([R.awgn(iq[k], (0.0, 0.05, 0.09, 0.12, 0.3)[k], k) for k in range(5)])
    out = dem.decode_frames(rx)
    check_frames(lib, dem, rx, out)
    assert out["error"][0] == 0 and np.array_equal(out["payloads"][0], pay[0])


def test_decode_frames_errors_and_grouping(gpu_lib):
    lib = gpu_lib
    cfg, t, pre, link = links(lib)
    mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
    E, lead = lib.RX_ERRORS, pre.total_len
    longer = table(lib, link.mcs + [("qpsk", ("ldpc", "n512r12"), None)])
    frames = [mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(k, mi, k), R.payload(n, k)), k)[lead:]
              for k, (mi, n) in enumerate([(1, 96), (2, 96), (1, 37), (2, 37), (1, 96), (2, 37), (1, 96), (1, 96)])]
    frames.append(lib.OfdmFrameMod(cfg, longer, pre).modulate_frame(lib.FramePacket(lib.FrameMetadata(8, 4), R.payload(96, 8)))[lead:])
    width = max(f.size for f in frames)
    rx = np.zeros((len(frames), width), np.complex64)
    for k, f in enumerate(frames):
        rx[k, :f.size] = f
    rx[4, 72:144] = -rx[4, 72:144]  # a header symbol turned over, the next erased
    rx[4, 144:216] = 0
    rx[6, 9 * 72 + 72:9 * 72 + 6 * 72] = 0  # payload symbols erased
    out = dem.decode_frames(rx)
    check_frames(lib, dem, rx, out)
    assert out["error"].tolist() == [0, 0, 0, 0, E["header_crc_mismatch"], 0, E["crc_mismatch"], 0, E["malformed_header"]]
    assert out["mcs_index"].tolist()[:4] == [1, 2, 1, 2] and out["payload_len"].tolist()[:4] == [96, 96, 37, 37]
    # rows cut short: the longest frames no longer fit, the shorter ones still decode
    cut = np.ascontiguousarray(rx[:, :frames[1].size + 5])
    out = dem.decode_frames(cut)
    check_frames(lib, dem, cut, out)
    assert out["error"][0] == E["malformed_header"] and out["error"][1] == 0 and out["error"][3] == 0
    out = dem.decode_frames(np.ascontiguousarray(rx[:, :9 * 72 - 1]))  # not even a header
    assert (out["error"] == E["malformed_header"]).all()


@pytest.mark.parametrize("geometry", ["128_9", "256_16"])
def test_other_geometries(gpu_lib, geometry):
    """128 / 9 with 66 data carriers (137 samples per symbol, 8 header symbols) and 256 / 16 with
    200 (3 header symbols): modulate_frames against modulate_frame with and without a window, and
    decode_frames on one batch mixing every frame of the geometry: clean, lightly noisy, noisy enough
    to fail the QAM payloads, and one row drowned."""
    import np_ref_acquire as A

    lib = gpu_lib
    geo, frames = A.GEOMETRIES[geometry]
    rows, sent = [], []
    for roll_off in (0, 2):
        cfg, t, pre, _ = links(lib, roll_off=roll_off, **geo)
        mod = lib.OfdmFrameMod(cfg, t, pre)
        assert mod.sps == geo["n_fft"] + geo["cp_len"] and mod.n_data == len(geo["data"])
        for mi, n, nsym in frames:
            pay = np.stack([R.payload(n, 10 * k + mi) for k in range(3)])
            seq, flags = np.array([0, 7, 0xFFFFFFFF], np.int64), np.array([0, 255, 3], np.int64)
            seeds = np.array([0, 0x12345678, 0xFFFFFFFF], np.int64)
            got = mod.modulate_frames(pay, mi, sequence_nums=seq, flags=flags, seeds=seeds)
            assert got.dtype == np.complex64 and got.shape == (3, pre.total_len + (mod.header_symbols + nsym) * mod.sps)
            for k in range(3):
                f = lib.FramePacket(lib.FrameMetadata(int(seq[k]), mi, int(flags[k])), pay[k])
                assert same32(got[k], mod.modulate_frame(f, int(seeds[k]))), (roll_off, mi, n, k)
            if roll_off == 0:
                rows += [R.awgn(got[k][pre.total_len:], (0.0, 0.004, 0.02)[k], 50 + k) for k in range(3)]
                sent += [(mi, pay[k]) for k in range(3)]
    rows.append(R.awgn(rows[0], 0.5, 60))  # drowned: no header
    cfg, t, pre, _ = links(lib, **geo)
    dem = lib.OfdmFrameDemod(cfg, t)
    rx = np.zeros((len(rows), max(r.size for r in rows)), np.complex64)
    for k, r in enumerate(rows):
        rx[k, :r.size] = r
    out = dem.decode_frames(rx)
    check_frames(lib, dem, rx, out)
    E = lib.RX_ERRORS
    for k, (mi, pay) in enumerate(sent):
        if k % 3 < 2:  # the clean and the lightly noisy rows decode; the third is the host's verdict, whichever
            assert out["error"][k] == 0 and out["mcs_index"][k] == mi and np.array_equal(out["payloads"][k], pay), k
    assert out["error"][-1] == E["header_crc_mismatch"] and (out["error"] == E["crc_mismatch"]).any()
    cut = np.ascontiguousarray(rx[:, :min(r.size for r in rows) + 5])  # the longer frames no longer fit
    check_frames(lib, dem, cut, dem.decode_frames(cut))


def test_torch_tensors_on_a_stream_of_the_callers(gpu_lib):
    import torch

    lib = gpu_lib
    cfg, t, pre, _ = links(lib, roll_off=2, **LINKS["pn_after_per_frame"])
    mod, dem = lib.OfdmFrameMod(cfg, t, pre), lib.OfdmFrameDemod(cfg, t)
    pay = np.stack([R.payload(96, k) for k in range(5)])
    seeds = np.arange(5, dtype=np.int64) * 977
    want = mod.modulate_frames(pay, 1, seeds=seeds)
    s = torch.cuda.Stream()
    tp, ts = torch.from_numpy(pay).cuda(), torch.from_numpy(seeds).cuda()
    torch.cuda.synchronize()
    got = mod.modulate_frames(tp, 1, seeds=ts, stream=s.cuda_stream)
    s.synchronize()
    assert got.is_cuda and got.dtype == torch.complex64 and same32(got.cpu().numpy(), want)
    body = got[:, pre.total_len:].contiguous()
    out = dem.decode_frames(body, stream=s.cuda_stream)
    ref = dem.decode_frames(want[:, pre.total_len:].copy())
    assert out["error"].tolist() == ref["error"].tolist() == [0] * 5
    assert all(np.array_equal(a, b) and np.array_equal(a, p) for a, b, p in zip(out["payloads"], ref["payloads"], pay))
    with pytest.raises(ValueError):
        mod.modulate_frames(tp[:, ::2], 1)
    with pytest.raises(ValueError):
        mod.modulate_frames(pay, 9)
    with pytest.raises(ValueError):
        dem.decode_frames(body.to(torch.complex128))
    lp = lib.OfdmFrameMod(cfg.with_tx_lowpass(lib.TxLowpass.for_null_band(64, 31, 31, 60.0)), t, pre)
    with pytest.raises(ValueError):  # the batched path takes no TX low-pass
        lp.modulate_frames(pay, 1)


def test_tx_lowpass_runs_last_over_the_whole_frame(gpu_lib):
    """The host path's spectral mask (TxLowpass.apply filters on the device): the S&C repeats
    included, after the window; off by default and then byte-identical."""
    lib = gpu_lib
    cfg, t, pre, _ = links(lib, roll_off=2)
    lp = lib.TxLowpass.for_null_band(64, 31, 31, 60.0)
    f = lib.FramePacket(lib.FrameMetadata(2, 1), R.payload(96, 2))
    plain = lib.OfdmFrameMod(cfg, t, pre).modulate_frame(f)
    masked = lib.OfdmFrameMod(cfg.with_tx_lowpass(lp), t, pre).modulate_frame(f)
    assert masked.shape == plain.shape and same32(masked, lp.apply(plain)) and not same32(masked, plain)
    assert same32(lib.OfdmFrameMod(cfg.with_tx_lowpass(None), t, pre).modulate_frame(f), plain)
