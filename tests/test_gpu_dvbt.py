"""GPU: the DVB-T kernels (k_dvbt_mod, k_gi_metric / k_gi_select, k_dvbt_demod, k_tps_decode) and the
batched frame classes on top of them against the library's host path, which tests/test_dvbt_oracle.py
holds to the numpy restatement. Everything is compared as uint32 but the acquisition's cfo_hz, which
differs through atan2f alone: its bound is CFO_ULP_BOUND below.

Shapes: 70 symbols cover both phase cycles and the TPS reset after symbol 67; three frames carry
different TPS words; one row of coded bits is shorter than the capacity; guards 1/32 and 1/4 are
the two ends of the prefix length (one and two 256-sample steps of k_gi_metric's tile loop)."""
import numpy as np
import pytest

import np_ref_dvbt as R

pytestmark = pytest.mark.gpu
F = np.float32

# cfo_hz = -atan2f(gamma.im, gamma.re) fs / (TAU n_fft): gamma carries the host's bits, so the device
# and the host differ by atan2f's last places only. Measured over every capture of this file's sync
# sets (32 searches) and end-to-end sets on an MI355X: 0 ulp in 28 searches, 1 ulp in three, 2 ulp
# in one (guard 1/4, max_symbols 1, the rotated capture); 1 ulp at most end to end. The bound is
# twice the largest, at least 2.
CFO_ULP_MEASURED = 2
CFO_ULP_BOUND = max(2 * CFO_ULP_MEASURED, 2)


def same32(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex64 if (a.dtype.kind == "c" or b.dtype.kind == "c") else np.float32
    a, b = np.atleast_1d(a.astype(dt)), np.atleast_1d(b.astype(dt))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ulp_distance(a, b):
    a, b = np.atleast_1d(np.asarray(a, F)), np.atleast_1d(np.asarray(b, F))

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int(np.max(np.abs(key(a) - key(b)))) if a.size else 0


@pytest.fixture(scope="module")
def link(gpu_lib):
    """The capstone frame and the noisy capture set, built once."""
    lib = gpu_lib
    p = lib.DvbTFrameParams(*R.CAPTURE_PARAMS)
    payload = R.sample_payload(R.CAPTURE_PAYLOAD_LEN)
    fr = lib.DvbTFrameMod(p).modulate(payload)
    rows, names, short = R.capture_set(fr.iq, fr.n_symbols, fr.samples_per_symbol)
    return dict(params=p, payload=payload, frame=fr, rows=rows, names=names, short=short)


# ---- k_dvbt_mod -----------------------------------------------------------------------------
@pytest.mark.parametrize("v", [2, 4, 6])
@pytest.mark.parametrize("roll", [0, 16])
@pytest.mark.parametrize("cp", [64, 512])
def test_symbols_level_modulator(gpu_lib, v, cp, roll):
    lib = gpu_lib
    rng = np.random.default_rng(100 + v + cp)
    n_symbols, frames = 70, 3
    row_bits = n_symbols * 1512 * v
    bits = rng.integers(0, 2, (frames, row_bits), dtype=np.uint8)
    nbits = np.array([row_bits, row_bits - 5 * 1512 * v - 3, row_bits])  # row 1 ends inside a carrier of symbol 64
    tps = np.stack([R.tps_pack(fn, con, "3/4", "1/8", cell) for fn, con, cell in ((0, "qpsk", 0), (3, "qam64", 0xFF), (1, "qam16", 0x5A))])
    got = lib.dvb_t_mod_symbols_batch(bits, v, cp, tps, n_symbols, roll, nbits=nbits)
    assert got.shape == (frames, n_symbols * (2048 + cp)) and got.dtype == np.complex64
    for k in range(frames):
        want = lib.dvb_t_mod_symbols(bits[k, :nbits[k]], v, cp, tps[k], n_symbols, roll)
        assert same32(got[k], want), k
    assert not same32(got[0, :68 * (2048 + cp)], got[2, :68 * (2048 + cp)])


# ---- k_gi_metric / k_gi_select --------------------------------------------------------------
def sync_sets(lib):
    """(cp, captures (ncap, n), fs): the oracle file's edge set plus a windowed and a multipath capture."""
    fs = R.fs_1mhz()
    out = []
    for guard, con, rate in (("1/32", "qpsk", "1/2"), ("1/4", "qam16", "3/4")):
        cp = R.GUARD_CP[guard]
        sps = 2048 + cp
        p = lib.DvbTFrameParams(guard, con, rate, 1, 0x33)
        six = lib.DvbTFrameMod(p).modulate(R.sample_payload(100)).iq[:6 * sps]
        win = lib.DvbTFrameMod(p).with_symbol_window(cp // 4).modulate(R.sample_payload(100)).iq[:6 * sps]
        n = 8 * sps
        caps = [R.place(six, lead, n - lead - len(six)) for lead in (0, 200, sps - 1, sps - 12)]
        caps.append(np.zeros(n, np.complex64))                                   # every metric ties
        caps.append(R.place(win, 0, n - len(win)))                                # windowed, no lead-in: the unwrap
        caps.append(R.awgn(R.place(R.two_tap(six), 300, n - 300 - len(six)), 0.3 * R.rms(six), 31))
        caps.append(R.rotate(R.awgn(R.place(six, 77, n - 77 - len(six)), 0.1 * R.rms(six), 32), float(fs) / 2048 * 0.3, fs))
        out.append((cp, np.stack(caps).astype(np.complex64), fs))
    return out


def host_sync(lib, row, cp, fs, search_len, cfg):
    return lib.dvb_t_gi_metric(np.ascontiguousarray(row), 2048, cp, float(fs), search_len, cfg)


def test_gi_sync_batch(gpu_lib):
    lib = gpu_lib
    worst = 0
    for cp, caps, fs in sync_sets(lib):
        sps = 2048 + cp
        for max_symbols in (1, 4):
            cfg = lib.GiSyncConfig(max_symbols=max_symbols)
            got = lib.dvb_t_gi_sync_batch(caps, 2048, cp, float(fs), sps, cfg)
            for c, row in enumerate(caps):
                want, metric = host_sync(lib, row, cp, fs, sps, cfg)
                assert got["found"][c] == 1 and got["start"][c] == want.start_sample, (cp, max_symbols, c)
                assert same32(got["metric"][c], metric), (cp, max_symbols, c)
                for k, w in (("gamma", want.gamma), ("phi", want.phi), ("score", want.score)):
                    assert same32(got[k][c], w), (k, cp, max_symbols, c)
                d = ulp_distance(got["cfo_hz"][c], want.cfo_hz)
                print(f"cfo_hz cp={cp} max_symbols={max_symbols} capture={c}: {d} ulp")
                worst = max(worst, d)
        # one sample too short: found = 0 for every capture, as the host's None
        short = np.ascontiguousarray(caps[:2, :2 * sps - 2])
        got = lib.dvb_t_gi_sync_batch(short, 2048, cp, float(fs), sps)
        assert not got["found"].any() and host_sync(lib, short[0], cp, fs, sps, None)[0] is None
        exact = np.ascontiguousarray(caps[:2, :2 * sps - 1])
        got = lib.dvb_t_gi_sync_batch(exact, 2048, cp, float(fs), sps)
        assert got["found"].all() and got["start"][1] == host_sync(lib, exact[1], cp, fs, sps, None)[0].start_sample
    print(f"cfo_hz: largest distance {worst} ulp")
    assert worst <= CFO_ULP_BOUND


# ---- k_dvbt_demod ---------------------------------------------------------------------------
@pytest.mark.parametrize("v,cp", [(2, 64), (4, 512), (6, 128)])
def test_symbols_level_demodulator(gpu_lib, v, cp):
    lib = gpu_lib
    rng = np.random.default_rng(200 + v)
    n_symbols, sps = 9, 2048 + cp
    bits = rng.integers(0, 2, n_symbols * 1512 * v, dtype=np.uint8)
    iq = lib.dvb_t_mod_symbols(bits, v, cp, R.tps_pack(2, "qam16", "2/3", "1/4", 9), n_symbols)
    starts = np.array([0, 13, 700, 1], np.int32)
    n = n_symbols * sps + 700
    caps = []
    for k, st in enumerate(starts):
        x = R.awgn(R.place(R.two_tap(iq), int(st), n - int(st) - len(iq)), 0.1 * R.rms(iq), 300 + k)
        x[int(st) + 3 * sps:int(st) + 4 * sps] = 0  # a silent symbol: every estimate under the floor, the erasure branch
        caps.append(x)
    caps = np.stack(caps).astype(np.complex64)
    found = np.array([1, 1, 1, 0], np.int32)
    for backoff in (0, cp // 2):
        got = lib.dvb_t_demod_symbols_batch(caps, starts, found, n_symbols, cp, backoff, v, syms=True)
        for c in range(3):
            llr, cells, syms = lib.dvb_t_demod_symbols(np.ascontiguousarray(caps[c, starts[c]:starts[c] + n_symbols * sps]),
                                                       n_symbols, cp, backoff, v, syms=True)
            assert same32(got["llr"][c], llr) and same32(got["cells"][c], cells) and same32(got["syms"][c], syms), (backoff, c)
        assert not got["llr"][3].any() and not got["cells"][3].any()  # not found: nothing written
        assert not got["syms"][1, 3].any() and got["syms"][1, 2].any()
    late = lib.dvb_t_demod_symbols_batch(caps, np.array([0, 0, 701, 0], np.int32), np.ones(4, np.int32), n_symbols, cp, 0, v)
    assert not late["llr"][2].any() and late["llr"][1].any()  # a frame that does not fit is skipped


# ---- k_tps_decode ---------------------------------------------------------------------------
def test_tps_decode(gpu_lib):
    lib = gpu_lib
    rng = np.random.default_rng(400)
    base = R.tps_pack(3, "qam64", "5/6", "1/16", 0xC3)

    def cells_of(bits, seed):
        c = R.tps_encode(bits, 70)[:70] * np.complex64(0.4 + 0.7j)
        r = np.random.default_rng(seed)
        return (c + (r.standard_normal(c.shape) + 1j * r.standard_normal(c.shape)) * 0.1).astype(np.complex64)

    def flipped(idx):
        b = base.copy()
        b[list(idx)] ^= 1
        return b

    words = [base, flipped([1]), flipped([67]), flipped([1, 67]), flipped([30, 31]), flipped([5, 40, 66]), flipped([2, 3, 4])]
    for field, value in (((24, 26), 0b11), ((29, 32), 0b110)):  # reserved codes in valid BCH words
        info = base[1:54].copy()
        a, b = field
        info[a:b] = [(value >> (b - a - 1 - j)) & 1 for j in range(b - a)]
        words.append(np.concatenate([[0], R.tps_bch_encode(info)]).astype(np.uint8))
    cells = [cells_of(w, 500 + k) for k, w in enumerate(words)]
    zero = R.tps_encode(base, 70).astype(np.complex64)
    zero[20] = 0  # the sums of symbols 20 and 21 are exactly 0: both bits 0, whatever was sent
    zero[40, :16], zero[40, 16] = np.array([1, -1] * 8), 0
    zero[41, :16], zero[41, 16] = 1, 0
    cells.append(zero)
    cells = np.stack(cells)
    got = lib.dvb_t_tps_decode_batch(cells)
    for k, c in enumerate(cells):
        dec = lib.TpsDecoder()
        for row in c[:68]:
            dec.feed_symbol(row)
        w = dec.word()
        assert (got["status"][k] == 0) == (w is not None), k
        if w is not None:
            f = got["fields"][k]
            assert (int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4])) == \
                (w.frame_number, {"qpsk": 1, "qam16": 2, "qam64": 3}[w.constellation], lib.FEC_RATES[w.code_rate_hp],
                 lib.DVB_T_GUARDS[w.guard], w.cell_id), k
        else:
            assert not got["fields"][k].any()
    assert list(got["status"][:5]) == [0] * 5 and list(got["status"][7:9]) == [1, 1]
    few = lib.dvb_t_tps_decode_batch(np.ascontiguousarray(cells[:2, :67]))
    assert list(few["status"]) == [1, 1]


# ---- end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("guard,con,rate,n", [("1/32", "qpsk", "1/2", 37), ("1/8", "qam16", "3/4", 400), ("1/4", "qam64", "7/8", 37)])
def test_modulate_frames_equals_modulate(gpu_lib, guard, con, rate, n):
    lib = gpu_lib
    p = lib.DvbTFrameParams(guard, con, rate, 0, 0)
    payloads = np.random.default_rng(600 + n).integers(0, 256, (3, n), dtype=np.uint8)
    fn, ci = [0, 3, 1], [0, 255, 0x5A]
    mod = lib.DvbTFrameMod(p).with_symbol_window(8)
    got = mod.modulate_frames(payloads, frame_numbers=fn, cell_ids=ci)
    for k in range(3):
        want = lib.DvbTFrameMod(p.with_frame(fn[k], ci[k])).with_symbol_window(8).modulate(payloads[k])
        assert got.shape[1] == want.iq.size and same32(got[k], want.iq), k


def check_decode_frames(lib, demod, rows, n_symbols, payload_len, res):
    worst = 0
    for c, row in enumerate(rows):
        try:
            want = demod.decode(np.ascontiguousarray(row), n_symbols, payload_len)
        except lib.DvbTRxError as e:
            assert res["error"][c] == e.code, (c, e.kind, res["error"][c])
            assert res["payloads"][c].size == 0
            if e.kind != "acquisition":
                assert res["timing_offset_samples"][c] == lib.dvb_t_gi_sync(np.ascontiguousarray(row), 2048, demod.params.cp_len, demod.params.fs, 2048 + demod.params.cp_len).start_sample
            continue
        d = want.diagnostics
        assert res["error"][c] == 0 and np.array_equal(res["payloads"][c], want.payload), c
        t = want.tps
        assert (res["frame_number"][c], res["constellation"][c], res["code_rate"][c], res["guard"][c], res["cell_id"][c]) == \
            (t.frame_number, {"qpsk": 1, "qam16": 2, "qam64": 3}[t.constellation], lib.FEC_RATES[t.code_rate_hp],
             lib.DVB_T_GUARDS[t.guard], t.cell_id), c
        assert res["timing_offset_samples"][c] == d["timing_offset_samples"] and same32(res["sync_score"][c], d["sync_score"])
        assert res["integer_cfo_bins"][c] == -1 and d["integer_cfo_bins"] is None
        assert bool(res["outer_fec_ok"][c]) == d["outer_fec_ok"] and res["rs_corrected_bytes"][c] == d["rs_corrected_bytes"]
        worst = max(worst, ulp_distance(res["cfo_hz"][c], d["cfo_hz"]))
    print(f"decode_frames cfo_hz: largest distance {worst} ulp")
    assert worst <= CFO_ULP_BOUND


def test_decode_frames_equals_decode(gpu_lib, link):
    lib = gpu_lib
    demod = lib.DvbTFrameDemod(link["params"])
    fr = link["frame"]
    res = lib.DvbTFrameDemod(link["params"]).decode_frames(link["rows"], fr.n_symbols, link["payload"].size)
    E = lib.DVB_T_RX_ERRORS
    assert list(res["error"]) == [0, 0, 0, E["payload_decode"], E["tps_decode"], E["incomplete"]]
    check_decode_frames(lib, demod, link["rows"], fr.n_symbols, link["payload"].size, res)
    short = np.stack([link["short"], link["short"]])
    res = demod.decode_frames(short, fr.n_symbols, link["payload"].size)
    assert list(res["error"]) == [E["acquisition"]] * 2
    check_decode_frames(lib, demod, short, fr.n_symbols, link["payload"].size, res)


def test_resident_tensors_on_a_stream(gpu_lib, link):
    import torch

    lib = gpu_lib
    p, fr = link["params"], link["frame"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rows = torch.from_numpy(link["rows"][:4]).cuda()
        payloads = torch.from_numpy(np.stack([link["payload"], link["payload"][::-1].copy()])).cuda()
    stream.synchronize()
    iq = lib.DvbTFrameMod(p).modulate_frames(payloads, stream=stream.cuda_stream)
    assert iq.is_cuda and iq.dtype == torch.complex64
    res = lib.DvbTFrameDemod(p).decode_frames(rows, fr.n_symbols, link["payload"].size, stream=stream.cuda_stream)
    stream.synchronize()
    assert same32(iq[0].cpu().numpy(), fr.iq)
    assert same32(iq[1].cpu().numpy(), lib.DvbTFrameMod(p).modulate(link["payload"][::-1].copy()).iq)
    check_decode_frames(lib, lib.DvbTFrameDemod(p), link["rows"][:4], fr.n_symbols, link["payload"].size, res)
    sync = lib.dvb_t_gi_sync_batch(rows, 2048, p.cp_len, p.fs, fr.samples_per_symbol, stream=stream.cuda_stream)
    stream.synchronize()
    want = [lib.dvb_t_gi_sync(np.ascontiguousarray(r), 2048, p.cp_len, p.fs, fr.samples_per_symbol).start_sample for r in link["rows"][:4]]
    assert sync["start"].is_cuda and list(sync["start"].cpu().numpy()) == want and want[0] == 200


def test_decode_frames_of_modulate_frames(gpu_lib):
    lib = gpu_lib
    p = lib.DvbTFrameParams("1/16", "qam16", "2/3", 0, 0)
    payloads = np.random.default_rng(700).integers(0, 256, (4, 300), dtype=np.uint8)
    fn, ci = [0, 1, 2, 3], [1, 2, 3, 250]
    mod = lib.DvbTFrameMod(p)
    n_symbols, _ = mod.plan(300)
    iq = mod.modulate_frames(payloads, frame_numbers=fn, cell_ids=ci)
    caps = np.stack([R.place(iq[k], 100 * k, 400 - 100 * k) for k in range(4)])
    res = lib.DvbTFrameDemod(p).decode_frames(caps, n_symbols, 300)
    assert not res["error"].any() and list(res["timing_offset_samples"]) == [0, 100, 200, 300]
    for k in range(4):
        assert np.array_equal(res["payloads"][k], payloads[k])
    assert list(res["frame_number"]) == fn and list(res["cell_id"]) == ci
    assert set(res["constellation"]) == {2} and set(res["code_rate"]) == {1} and set(res["guard"]) == {1}


def test_batched_path_refuses_host_only_options(gpu_lib, link):
    lib = gpu_lib
    p = link["params"]
    with pytest.raises(ValueError):
        lib.DvbTFrameMod(p).with_tx_lowpass(lib.DvbTFrameMod.tx_lowpass_for_2k(45, 60.0)).modulate_frames(np.zeros((1, 10), np.uint8))
    with pytest.raises(ValueError):
        lib.DvbTFrameDemod(p).with_integer_cfo_correction(True).decode_frames(link["rows"][:1], 68, 184)


def test_masked_frame_with_no_lead_in_acquires_at_zero(gpu_lib):
    """The mask rows of the reference's zero-lead-in test (the TX low-pass is a device filter)."""
    lib = gpu_lib
    p = lib.DvbTFrameParams("1/8", "qpsk", "1/2", 1, 0x33)
    payload = R.sample_payload(184)
    for roll in (0, 8):
        fr = lib.DvbTFrameMod(p).with_symbol_window(roll).with_tx_lowpass(lib.DvbTFrameMod.tx_lowpass_for_2k(45, 60.0)).modulate(payload)
        got = lib.DvbTFrameDemod(p).with_rx_window_backoff(32).decode(fr.iq, fr.n_symbols, 184)
        assert got.diagnostics["timing_offset_samples"] == 0 and np.array_equal(got.payload, payload)
