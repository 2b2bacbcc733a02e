"""CPU: OFDM burst acquisition and the burst receiver on the host (orion_sdr.ofdm_sync,
earliest_accepted, ofdm_integer_cfo, ofdm_rotate_block, ofdm_remove_common_phase_error,
OfdmBurstDemod.receive, OfdmFrameStreamDemod) against tests/np_ref_acquire.py at float32, every
field of every result bit for bit: four preambles (with and without a training symbol, one whose
repeat length is no multiple of four), the range rules, a clean frame, frames at three offsets
with carrier offsets of -2, 0 and 2 subcarrier spacings plus a fraction, the reference's
two-frames-in-one-capture behaviour, receive on decisive and structural captures, the stream
demodulator on three frames fed in chunks, and goldens. Crafted captures of Gaussian integers
(exact ties, a score on the threshold, an offset on the cluster's far edge, two kept offsets, none;
p and r also against an int64 reference), walks of one sample and around 4096 staged samples, the
half-band carrier offset whose two correlations tie exactly, and receive at two more geometries,
128 / 9 with 66 carriers and 256 / 16 with 200: the inputs of tests/test_gpu_acquire_edges.py."""
import functools
import os

import numpy as np
import pytest

import np_ref_acquire as A
import np_ref_frame as R
from test_frame_layer_oracle import links, same32, table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acquire_golden.npz")
FS = 1e6
PREAMBLES = [((2, 32), True), ((3, 16), True), ((2, 32), False), ((3, 6), False)]


@pytest.fixture(scope="module")
def lib():
    import orion_sdr

    return orion_sdr


def bits32(v):
    return np.array([v], np.float32).view(np.uint32)[0]


def same_results(got, want):
    """A list of OfdmSyncResult against the restatement's tuples, floats as uint32."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.start_sample, bits32(g.cfo_hz), g.integer_cfo_bins, bits32(g.score)) == \
            (w[0], bits32(w[1]), w[2], bits32(w[3])), (g, w)


def ref_pre(pre):
    return pre.num_repeats, pre.repeat_len, pre.training


def frame(lib, prm=(2, 32), training=True, mi=1, n=40, seq=3, seed=1):
    cfg, t, pre, link = links(lib, preamble=prm, training=training)
    f = lib.OfdmFrameMod(cfg, t, pre).modulate_frame(lib.FramePacket(lib.FrameMetadata(seq, mi), R.payload(n, seed)))
    return cfg, t, pre, link, f


# ---- ofdm_sync -----------------------------------------------------------------------------
@pytest.mark.parametrize("prm,training", PREAMBLES, ids=str)
def test_sync_against_the_restatement(lib, prm, training):
    _, _, pre, _, f = frame(lib, prm, training)
    for k, (off, cfo, ph) in enumerate(A.OFFSETS):
        x = A.impair(f, off, cfo, ph, A.SIGMA, 10 + k)
        got = lib.ofdm_sync(x, FS, pre, 0, x.size)
        same_results(got, A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size))
        assert got[0].start_sample == off and all(0.0 <= r.score <= 1.0 for r in got)
        p, r = lib.ofdm_sc_metric(x, FS, pre, 0, x.size)
        wp, wr = A.sc_sums(x, ref_pre(pre), 0, x.size - pre.total_len)
        assert same32(p, wp) and np.array_equal(r.view(np.uint32), wr.view(np.uint32))
        assert all(q.integer_cfo_bins == 0 for q in got[5:])  # the integer search visits five
    if training and prm == (2, 32):  # repeat_len = n_fft / 2: the fraction spans +-1 bin, the bins come out even
        bins = [lib.ofdm_sync(A.impair(f, off, cfo, ph, A.SIGMA, 10 + k), FS, pre, 0, 4000)[0].integer_cfo_bins
                for k, (off, cfo, ph) in enumerate(A.OFFSETS)]
        assert bins == [-2, 0, 2]


def test_sync_range_rules(lib):
    _, _, pre, _, f = frame(lib)
    x = A.impair(f, 101, 2300.0, 1.0, A.SIGMA, 3)
    rp = ref_pre(pre)
    for start, end in ((40, x.size), (0, x.size + 1000), (0, 150), (120, 10 ** 12)):
        got = lib.ofdm_sync(x, FS, pre, start, end)
        same_results(got, A.ofdm_sync(x, FS, rp, start, end))
        assert got and min(q.start_sample for q in got) >= start
        assert max(q.start_sample for q in got) < min(end, x.size - pre.total_len)
    # a range too short, an inverted one, a capture shorter than the preamble, and the guards
    for args in ((500, 500), (600, 500), (x.size - pre.total_len, x.size)):
        assert lib.ofdm_sync(x, FS, pre, *args) == [] == A.ofdm_sync(x, FS, rp, *args)
    assert lib.ofdm_sync(x[:pre.total_len], FS, pre, 0, 10 ** 6) == []
    assert lib.ofdm_sync(x, FS, lib.OfdmPreamble(1, 32), 0, x.size) == []
    assert lib.ofdm_sync(x, FS, lib.OfdmPreamble(2, 0), 0, x.size) == []
    assert lib.ofdm_sync(x, 0.0, pre, 0, x.size) == [] and lib.ofdm_sync(x, -1.0, pre, 0, x.size) == []
    # an all-zero stretch: offsets whose window holds no energy are skipped, the rest ranked as ever
    z = x.copy()
    z[:90] = 0
    got = lib.ofdm_sync(z, FS, pre, 0, z.size)
    same_results(got, A.ofdm_sync(z, FS, rp, 0, z.size))
    assert len(got) == z.size - pre.total_len - (90 - 64 + 1) and got[0].start_sample == 101
    assert min(q.start_sample for q in got) == 90 - 64 + 1
    assert lib.ofdm_sync(np.zeros(800, np.complex64), FS, pre, 0, 800) == []


def test_clean_frame_is_found_at_its_start(lib):
    _, _, pre, _, f = frame(lib)
    x = np.concatenate([np.zeros(37, np.complex64), f, np.zeros(50, np.complex64)])
    got = lib.ofdm_sync(x, FS, pre, 0, x.size)
    same_results(got, A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size))
    assert got[0].start_sample == 37 and abs(float(got[0].score) - 1.0) <= 4 * np.finfo(np.float32).eps
    assert got[0].integer_cfo_bins == 0 and abs(float(got[0].cfo_hz)) < 1.0
    best = lib.earliest_accepted(got, 0.5, pre.total_len)
    assert best.start_sample == 37 == A.earliest_accepted(A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size), 0.5, pre.total_len)[0]


def test_integer_cfo_and_earliest_accepted_against_the_restatement(lib):
    _, _, pre, _, f = frame(lib)
    x = A.impair(f, 200, 42875.0, 0.5, A.SIGMA, 12)
    for start, frac in ((200, 11599.2), (200, -4000.0), (197, 11599.2), (x.size - 100, 0.0)):
        bins, c2 = lib.ofdm_integer_cfo(x, FS, 64, 8, start + 64, frac, corr=True)
        wb, wc = A.integer_cfo_bins(x, FS, (64, 8), start + 64, frac, corr=True)
        assert bins == wb and (wc is None or np.array_equal(c2.view(np.uint32), wc.view(np.uint32)))
    assert lib.ofdm_integer_cfo(x, FS, 64, 8, x.size - 71, 0.0) == 0  # no room for the symbol
    res = lib.ofdm_sync(x, FS, pre, 0, x.size)
    ref = A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size)
    for thr, cl in ((0.5, pre.total_len), (0.9, 1), (0.5, 0), (0.999, 136), (1.5, 136)):
        g, w = lib.earliest_accepted(res, thr, cl), A.earliest_accepted(ref, thr, cl)
        assert (g is None) == (w is None) and (g is None or g.start_sample == w[0])
    assert lib.earliest_accepted([], 0.5, 10) is None
    # the lowest shift wins a tie: an all-zero symbol correlates to zero at every shift
    assert lib.ofdm_integer_cfo(np.zeros(200, np.complex64), FS, 64, 8, 0, 0.0) == -32 == \
        A.integer_cfo_bins(np.zeros(200, np.complex64), FS, (64, 8), 0, 0.0)


# ---- crafted captures: exact ties, the threshold and the cluster edge, few kept offsets --------
def lib_pre(lib, pre):
    p = lib.OfdmPreamble(pre[0], pre[1])
    return p.with_training_symbol(*pre[2]) if pre[2] else p


def same_sums_exact(p, r, x, pre, start, end):
    """p and r (float32) against the int64 reference, which must stay in f32's exact range."""
    pr, pi, rr, bound = A.sc_sums_exact(x, pre, start, end)
    assert bound < 2 ** 24
    assert np.array_equal(p.real, pr.astype(np.float32)) and np.array_equal(p.imag, pi.astype(np.float32))
    assert np.array_equal(r, rr.astype(np.float32))


@pytest.mark.parametrize("name", list(A.crafted_cases()))
def test_crafted_captures(lib, name):
    """The restatement holds each capture's edge; the host agrees with it result for result, and
    its sums are the integers they must be."""
    pre, x, thr, want = A.crafted_cases()[name]
    facts = A.crafted_facts(x, pre, thr)
    A.assert_facts(facts, want)
    lp = lib_pre(lib, pre)
    ref = A.ofdm_sync(x, FS, pre, 0, x.size)
    got = lib.ofdm_sync(x, FS, lp, 0, x.size)
    same_results(got, ref)
    p, r = lib.ofdm_sc_metric(x, FS, lp, 0, x.size)
    same_sums_exact(p, r, x, pre, 0, facts["nd"])
    best = lib.earliest_accepted(got, thr, lp.total_len)
    assert (None if best is None else best.start_sample) == facts["accepted"]


@pytest.mark.parametrize("start,end,nd", A.ONES_RANGES)
def test_all_ones_every_offset_ties(lib, start, end, nd):
    x, pre = np.ones(900, np.complex64), (2, 32, None)
    facts = A.crafted_facts(x, pre, 0.5, start, end)
    A.assert_facts(facts, A.ones_facts(start, nd))
    got = lib.ofdm_sync(x, FS, lib_pre(lib, pre), start, end)
    same_results(got, A.ofdm_sync(x, FS, pre, start, end))
    assert len(got) == nd and all(q.score == 1 and q.cfo_hz == 0 for q in got)
    assert [q.start_sample for q in got] == list(range(start, start + nd))  # a stable sort of equal keys
    assert lib.earliest_accepted(got, 0.5, 64).start_sample == start
    p, r = lib.ofdm_sc_metric(x, FS, lib_pre(lib, pre), start, end)
    same_sums_exact(p, r, x, pre, start, start + nd)
    assert (p == 32).all() and (r == 32).all()


@pytest.mark.parametrize("num,rl", A.WALKS)
def test_walk_lengths_against_the_restatement(lib, num, rl):
    """A walk of one sample, and the preambles on either side of the device's staging limit."""
    pre, lp = (num, rl, None), lib.OfdmPreamble(num, rl)
    for kind, x in A.walk_captures(num, rl).items():
        assert x.size == num * rl + 301
        same_results(lib.ofdm_sync(x, FS, lp, 0, x.size), A.ofdm_sync(x, FS, pre, 0, x.size))
        p, r = lib.ofdm_sc_metric(x, FS, lp, 0, x.size)
        assert p.size == 301
        if kind == "integers":
            same_sums_exact(p, r, x, pre, 0, 301)


def half_band_facts(lib, cfg, pre, x, start):
    """What makes the half-band capture a tie, on the host's own values: the S&C sums and the
    fraction are the unshifted capture's bit for bit, the two largest |corr|^2 are bit-equal at
    -/+ n_fft / 2 and the third is at most a quarter of them. Returns the shifted capture."""
    assert pre.repeat_len % 2 == 0
    xh = A.half_band(x)
    for a, b in zip(lib.ofdm_sc_metric(x, FS, pre, 0, x.size), lib.ofdm_sc_metric(xh, FS, pre, 0, x.size)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    res, plain = lib.ofdm_sync(xh, FS, pre, 0, x.size), lib.ofdm_sync(x, FS, pre, 0, x.size)
    assert all((a.start_sample, bits32(a.cfo_hz), bits32(a.score)) == (b.start_sample, bits32(b.cfo_hz), bits32(b.score))
               for a, b in zip(res, plain))
    half = cfg.n_fft // 2
    assert res[0].start_sample == start and res[0].integer_cfo_bins == -half
    _, c2 = lib.ofdm_integer_cfo(xh, FS, cfg.n_fft, cfg.cp_len, start + pre.num_repeats * pre.repeat_len, res[0].cfo_hz, corr=True)
    order = np.argsort(-c2.astype(np.float64), kind="stable")
    assert (order[:2] - half).tolist() == [-half, half] and bits32(c2[order[0]]) == bits32(c2[order[1]])
    assert c2[order[2]] <= 0.25 * c2[order[0]]
    return xh


@pytest.mark.parametrize("geometry", ["64_8"] + list(A.GEOMETRIES))
def test_half_band_offset_is_an_exact_tie_and_the_lower_shift_wins(lib, geometry):
    cfg, t, pre, link, x, data, start = half_band_case(geometry)
    xh = half_band_facts(lib, cfg, pre, x, start)
    want = A.receive(link, xh)
    assert want["error"] == 0 and np.array_equal(want["payload"], data) and want["start_sample"] == start
    check_step(lib, lib.OfdmBurstDemod(cfg, t, pre).receive(xh), want)
    wb, wc = A.integer_cfo_bins(xh, FS, (cfg.n_fft, cfg.cp_len), start + pre.num_repeats * pre.repeat_len,
                                A.ofdm_sync(xh, FS, ref_pre(pre), 0, xh.size)[0][1], corr=True)
    assert wb == -cfg.n_fft // 2 and bits32(wc[0]) == bits32(wc[-1]) == bits32(wc.max())


@functools.lru_cache(maxsize=None)
def half_band_case(geometry):
    """(cfg, table, preamble, link, the capture before the shift, payload, start): a decisive
    frame at the plan 64 / 8 or at one of the two further geometries."""
    import orion_sdr as lib

    if geometry == "64_8":
        cfg, t, pre, link, f = frame(lib)
        x, data, start = A.impair(f, 101, 2300.0, 1.0, A.SIGMA, 11), R.payload(40, 1), 101
    else:
        cfg, t, pre, link, caps = geometry_cases(geometry)
        x, (_, _, data) = caps["mcs2_40"]
        start = 77
    x.flags.writeable = False
    return cfg, t, pre, link, x, data, start


# ---- two more link geometries ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_cases(geometry, common_length=False):
    """(cfg, table, preamble, link, name -> (capture, (mcs_index, sequence_num, payload))) of
    A.GEOMETRIES, shared with the GPU tests; with common_length every capture is as long as the
    longest, so that they stack."""
    import orion_sdr as lib

    geo, frames = A.GEOMETRIES[geometry]
    cfg, t, pre, link = links(lib, **geo)
    mod = lib.OfdmFrameMod(cfg, t, pre)

    def frame_of(mi, seq, data):
        return mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(seq, mi, seq % 5), data), seq)

    total = 300 + max(mod.frame_len(mi, n) for mi, n, _ in frames) if common_length else None
    caps = A.geometry_captures(frame_of, frames, total)
    for v in caps.values():
        v[0].flags.writeable = False
    return cfg, t, pre, link, caps


@pytest.mark.parametrize("geometry,k", [(g, k) for g in A.GEOMETRIES for k in range(len(A.GEOMETRIES[g][1]))])
def test_receive_at_other_geometries(lib, geometry, k):
    cfg, t, pre, link, caps = geometry_cases(geometry)
    mi, nbytes, nsym = A.GEOMETRIES[geometry][1][k]
    x, (_, seq, data) = caps[f"mcs{mi}_{nbytes}"]
    assert x.size == lib.OfdmFrameMod(cfg, t, pre).frame_len(mi, nbytes) + 300 <= 4600
    want = A.receive(link, x)
    # the restatement alone decodes this capture
    assert want is not None and want["error"] == 0 and np.array_equal(want["payload"], data) and want["start_sample"] == 77
    assert want["symbols"].shape == (nsym, len(link.data))
    step = lib.OfdmBurstDemod(cfg, t, pre).receive(x)
    check_step(lib, step, want)
    assert step.packet == lib.FramePacket(lib.FrameMetadata(seq, mi, seq % 5), data)
    res = lib.ofdm_sync(x, FS, pre, 0, x.size)
    same_results(res, A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size))
    assert res[0].start_sample == 77 and res[0].integer_cfo_bins == 0


@functools.lru_cache(maxsize=None)
def two_frames():
    import orion_sdr as lib

    cfg, t, pre, link, a = frame(lib, mi=1, n=40, seq=0, seed=5)
    b = lib.OfdmFrameMod(cfg, t, pre).modulate_frame(lib.FramePacket(lib.FrameMetadata(1, 1), R.payload(40, 6)))
    x = A.two_frame_capture(a, b)
    x.flags.writeable = False
    return x


def test_two_frames_pin_the_reference_quirk(lib):
    """earliest_accepted picks the first frame's true start, which is not among the five
    candidates the integer search visited: its bins stay 0 although the offset is two spacings."""
    cfg, t, pre, link = links(lib)
    x = two_frames()
    res = lib.ofdm_sync(x, FS, pre, 0, x.size)
    same_results(res, A.ofdm_sync(x, FS, ref_pre(pre), 0, x.size))
    best = lib.earliest_accepted(res, 0.5, pre.total_len)
    assert best.start_sample == 50 and best.start_sample not in [q.start_sample for q in res[:5]]
    # 17000 Hz is the fraction found plus two spacings of 15625 Hz: a search at 50 would have said 2
    assert best.integer_cfo_bins == 0 and lib.ofdm_integer_cfo(x, FS, 64, 8, 50 + 64, best.cfo_hz) == 2
    step = lib.OfdmBurstDemod(cfg, t, pre).receive(x)
    want = A.receive(link, x)
    assert step.error == lib.RxError("header_crc_mismatch") and want["error"] == 3
    assert step.consume_to == 50 + pre.total_len == want["consume_to"] and step.packet is None


# ---- receive -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """(cfg, table, preamble, link, name -> (capture, what)), shared with the GPU tests."""
    import orion_sdr as lib

    cfg, t, pre, link = links(lib)
    longer = table(lib, link.mcs + [("qpsk", ("ldpc", "n512r12"), None)])
    mods = {False: lib.OfdmFrameMod(cfg, t, pre), True: lib.OfdmFrameMod(cfg, longer, pre)}

    def frame_of(mi, seq, data, longer_table=False):
        return mods[longer_table].modulate_frame(lib.FramePacket(lib.FrameMetadata(seq, mi, seq % 5), data), seq)

    total = 300 + mods[False].frame_len(0, 40)
    c = A.receive_cases(frame_of, total, pre.total_len, 72)
    for v in c.values():
        v[0].flags.writeable = False
    return cfg, t, pre, link, c


def check_step(lib, step, want):
    """A BurstStep (or None) against the restatement's step (or None), every field."""
    assert (step is None) == (want is None)
    if step is None:
        return
    assert step.consume_to == want["consume_to"] and step.timing_offset_samples == want["start_sample"]
    assert bits32(step.cfo_hz) == bits32(want["cfo_hz"]) and bits32(step.sync_score) == bits32(want["sync_score"])
    if want["error"]:
        assert step.packet is None and step.error.code == want["error"]
        return
    md = step.packet.metadata
    assert step.error is None and (md.mcs_index, md.sequence_num, md.flags) == (want["mcs_index"], want["sequence_num"], want["flags"])
    assert np.array_equal(step.packet.payload, want["payload"])
    assert (step.inner_ok, step.outer_ok, step.crc_ok) == (want["inner_ok"], want["outer_ok"], want["crc_ok"])
    assert (step.symbols is None) == (want["symbols"] is None)
    assert step.symbols is None or same32(step.symbols, np.ascontiguousarray(want["symbols"], np.complex64))


@pytest.mark.parametrize("name", ["mcs0_4", "mcs0_40", "mcs1_4", "mcs1_40", "mcs2_4", "mcs2_40"])
def test_receive_decisive_cases(lib, name):
    cfg, t, pre, link, c = cases()
    x, (mi, seq, data, off) = c[name]
    want = A.receive(link, x)
    # the condition that keeps the test honest: the restatement alone decodes this capture
    assert want is not None and want["error"] == 0 and np.array_equal(want["payload"], data) and want["start_sample"] == off
    step = lib.OfdmBurstDemod(cfg, t, pre).receive(x)
    check_step(lib, step, want)
    assert step.packet == lib.FramePacket(lib.FrameMetadata(seq, mi, seq % 5), data) and step.inner_ok and step.outer_ok
    nsym = step.symbols.shape[0]
    assert (nsym >= 4) == (name != "mcs2_4")  # the phase tracker runs on all but the 3-symbol QAM-16 payload
    assert step.consume_to == off + lib.OfdmFrameMod(cfg, t, pre).frame_len(mi, data.size)


def test_receive_structural_cases(lib):
    cfg, t, pre, link, c = cases()
    bd = lib.OfdmBurstDemod(cfg, t, pre)
    E = lib.RX_ERRORS
    assert bd.receive(c["noise"][0]) is None and A.receive(link, c["noise"][0]) is None
    assert bd.receive(c["cut"][0]) is None and A.receive(link, c["cut"][0]) is None  # need more, nothing consumed
    assert bd.receive(c["noise"][0][:pre.total_len + 71]) is None  # shorter than a preamble and one symbol
    step, want = bd.receive(c["header"][0]), A.receive(link, c["header"][0])
    check_step(lib, step, want)
    assert step.error.code == E["header_crc_mismatch"] and step.consume_to == 33 + pre.total_len
    step, want = bd.receive(c["longer"][0]), A.receive(link, c["longer"][0])
    check_step(lib, step, want)
    assert step.error.code == E["malformed_header"] and step.consume_to == 60 + pre.total_len
    # a cut inside the header is incomplete as well, where the known-start decode reports malformed_header
    x = c["mcs1_40"][0]
    assert bd.receive(x[:101 + pre.total_len + 5 * 72]) is None and A.receive(link, x[:101 + pre.total_len + 5 * 72]) is None
    # without a training symbol the body takes the known-start path (no carrier offset to survive)
    cfg2, t2, pre2, link2 = links(lib, training=False)
    f = lib.OfdmFrameMod(cfg2, t2, pre2).modulate_frame(lib.FramePacket(lib.FrameMetadata(2, 1), R.payload(40, 3)))
    x = A.impair(f, 64, 0.0, 0.0, 0.001, 9)
    check_step(lib, lib.OfdmBurstDemod(cfg2, t2, pre2).receive(x), A.receive(link2, x))


def test_phase_tracker_against_the_restatement(lib):
    rng = np.random.default_rng(8)
    for order, nsym in (("bpsk", 9), ("qpsk", 4), ("qam16", 7), ("qam64", 5), ("qpsk", 3)):
        bits = rng.integers(0, 2, nsym * 62 * R.RO.BITS[order], dtype=np.uint8)
        s = R.RO.map_bits(order, bits).reshape(nsym, 62).astype(np.complex128)
        ramp = np.exp(1j * (0.05 + 0.02 * np.arange(nsym)))[:, None]
        s = (s * ramp + (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape)) * 0.02).astype(np.complex64)
        got = lib.ofdm_remove_common_phase_error(order, s)
        assert same32(got, A.remove_common_phase_error(order, s))
        if nsym < 4:
            assert same32(got, s)
        else:  # the ramp is gone: what is left sits on the constellation again
            ideal = R.RO.map_bits(order, bits).reshape(nsym, 62)
            assert np.abs(got - ideal).max() < 0.12 < np.abs(s - ideal).max() + 0.1
    x = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64)
    assert same32(lib.ofdm_rotate_block(x, -4321.5, FS), A.rotate_block(x, -4321.5, FS))


# ---- the stream demodulator ----------------------------------------------------------------
def test_stream_demod_three_frames_in_chunks(lib):
    cfg, t, pre, link = links(lib)
    mod = lib.OfdmFrameMod(cfg, t, pre)
    sent = [R.payload(24, 70 + k) for k in range(3)]
    frames = [mod.modulate_frame(lib.FramePacket(lib.FrameMetadata(k, 1), sent[k])) for k in range(3)]
    burst = np.concatenate(frames + [np.zeros(400, np.complex64)])
    x = A.impair(burst, 20, 3100.0, 0.4, A.SIGMA, 44, total=20 + burst.size)
    sd, ref = lib.OfdmFrameStreamDemod(cfg, t, pre).with_score_threshold(0.5), A.StreamDemod(link)
    got, fed = [], 0
    for a in range(0, x.size, 500):
        chunk = np.ascontiguousarray(x[a:a + 500])
        before = sd.len() + chunk.size
        steps, want = sd.feed(chunk), ref.feed(chunk)
        assert len(steps) == len(want)
        for s, w in zip(steps, want):
            check_step(lib, s, w)
        assert sd.len() == before - sum(s.consume_to for s in steps) == len(ref.buf)  # the buffer shrinks by each consume_to
        got += steps
    got += sd.flush()
    assert [s.packet.metadata.sequence_num for s in got] == [0, 1, 2]
    assert all(np.array_equal(s.packet.payload, sent[k]) for k, s in enumerate(got))
    sd.clear()
    assert sd.len() == 0 and sd.is_empty() and sd.flush() == []


def test_goldens(lib):
    g = np.load(GOLDEN)
    cfg, t, pre, link, c = cases()
    x = c["mcs1_40"][0]
    assert same32(x, g["capture"])
    res = lib.ofdm_sync(x, FS, pre, 0, x.size)
    assert [q.start_sample for q in res[:16]] == g["starts"].tolist()
    assert np.array_equal(np.array([q.cfo_hz for q in res[:16]], np.float32).view(np.uint32), g["cfo_hz"].view(np.uint32))
    assert np.array_equal(np.array([q.score for q in res[:16]], np.float32).view(np.uint32), g["score"].view(np.uint32))
    assert [q.integer_cfo_bins for q in res[:16]] == g["bins"].tolist()
    step = lib.OfdmBurstDemod(cfg, t, pre).receive(x)
    assert same32(step.symbols, g["symbols"]) and np.array_equal(step.packet.payload, g["payload"])
    assert (step.consume_to, step.timing_offset_samples) == tuple(g["step"].tolist()) and bits32(step.cfo_hz) == g["cfo_total"].view(np.uint32)[0]
