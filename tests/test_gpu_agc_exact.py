"""Exact tests of the envelope engine (csrc/k_agc.hip: AgcRms, AgcRmsIq, CwKeyedMod), every
path and both fixers. Every comparison is bitwise against oracle.agc / oracle.cw_mod: the
tolerance is zero.

Which kernel a call reaches is EnvelopeRunner's choice restated in tests/agc_ref.py
(path_of: 'seq' k_agc_seq, one chunk; 'wave' k_agc_wave, 2..4096 chunks; 'lane' k_agc, more
than 4096 chunks, i.e. at least 4096 * 256 + 1 samples in one device call), on the warm-up
length the block reports. Which fixer a case needs comes from agc_ref.predict, from the
reference alone: chunks pass 2 flags are re-walked by k_agc_fix_runs, wrong chunks it does
not flag only by the one-wave k_agc_fix. tests/test_agc_ref.py asserts both for the whole
case table without a GPU; each case asserts them again before it runs. Every call goes
through process_device on torch tensors, so the call size is the test's own (process() cuts
host arrays of 2^21 samples or more into device calls that never reach the lane path:
test_host_cut_is_wave_path).

NaN inputs. The reference is well defined: f32::max returns the other operand (the seed
max(d0, 1e-12) and the rms floor max(sqrt(env), 1e-6)), `d > env` is false for NaN, so one
NaN sample makes the envelope NaN for the rest of the stream and every later gain
clamp(target / 1e-6) = max_gain; the oracle's o_maxf and the device's fmaxf agree with it.
CW: f32::clamp(NaN) is NaN, the envelope and every later output are NaN. Asserted:
NaN positions equal and all other bits equal; NaN payloads are not compared.
"""
import numpy as np
import pytest

import agc_ref as A

pytestmark = pytest.mark.gpu

f32 = np.float32
CASE = {c.name: c for c in A.CASES}


# ---- helpers ------------------------------------------------------------------------------
NCO_TABLE = 1 << 22  # outputs of the tone oscillator that are the reference recurrence's own (default 2^20)


def make(lib, kind, cfg):
    """A fresh block. CwKeyedMod's tone Nco is the reference's, bit for bit, for the outputs
    its table holds (osc.hpp: 2^20 by default, the fitted drift model after that); the
    streams here run to 2.2 M samples, so the table is sized to hold them all and every
    output bit is the envelope engine's to get right."""
    blk = {"agc": lib.AgcRms, "agc_iq": lib.AgcRmsIq, "cw": lib.CwKeyedMod}[kind](*cfg)
    if kind == "cw":
        blk.configure_option("nco_table", NCO_TABLE)
    return blk


def warm(blk, kind, cfg):
    """The warm-up length the block runs with: AGC reports it (taps()[3]); CW's follows from
    the coefficients it reports. Both asserted against agc_ref's restatement."""
    t = blk.taps()
    co = np.asarray(A.coefs(kind, cfg), f32)
    assert np.array_equal(np.asarray(t[:2], f32).view(np.uint32), co.view(np.uint32)), (t[:2], co)
    W = A.warmup_len(max(f32(t[0]), f32(t[1])))
    if kind != "cw":
        assert int(t[3]) == W, (t, W)
    assert W == A.warm_of(kind, cfg)
    return W


def reference(oracle, x, kind, cfg, calls=None):
    if kind == "cw":
        return oracle.cw_mod(x, *cfg)  # no per-call rule: the cut cannot matter
    return oracle.agc(x, *cfg, calls=calls)[0]


def run_dev(blk, x, calls=None):
    """x through process_device in calls of the given lengths (one call by default)."""
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs, at = [], 0
    for c in calls or [len(x)]:
        outs.append(blk.process_device(xd[at:at + c]))
        at += c
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy()


def u32(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32)


def assert_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    g, r = u32(got), u32(ref)
    diff = np.flatnonzero(g != r)
    per = 2 if np.iscomplexobj(ref) else 1
    assert len(diff) == 0, (f"{what}: {len(diff)} of {len(g)} words differ, first at sample {diff[0] // per} "
                            f"(got {got[diff[0] // per]!r}, reference {ref[diff[0] // per]!r})")
    print(f"[parity] {what}: {len(ref)} samples bit-exact")


# ---- one call, every path -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASE))
def test_one_call(gpu_lib, oracle, name):
    """One process_device call per case of agc_ref.CASES: the lane path at 4097 chunks (ragged
    last chunk), 4098 chunks and at the AGC bench's own (48e3, 0.2, 5.0) with L = 311; the
    wave path at 2 chunks, 4096 chunks and a last chunk of one sample; the sequential path at
    n in {1, 63, 64, 65, 257}. Inputs: noise with level steps (no re-run: 0 wrong chunks),
    DC / tone plateaus (the fixed-point band: the run fixer, then pass 3 along the plateau),
    one inf at sample 3L + 7 (the envelope never forgets: everything after is re-walked) or
    placed so that the last chunk alone is wrong (its warm-up is the only one that misses it);
    CW ragged keying, key-ups longer than W + L (undetermined chunks: k_agc_fix_runs), equal
    rise and fall (the one-coefficient walks) and a 0.1 ms fall onto the subnormal plateau."""
    c = CASE[name]
    blk = make(gpu_lib, c.kind, c.cfg)
    W = warm(blk, c.kind, c.cfg)
    assert A.path_of(c.n, W) == c.path
    x = c.make()
    p = A.predict(x, c.cfg, c.kind, oracle)
    assert p.path == c.path and p.W == W
    if c.fix == "none":
        assert A.predict_bad(x, c.cfg, c.kind, oracle) == []
    else:
        assert p.flagged and (p.late or c.fix == "runs")
    ref = reference(oracle, x, c.kind, c.cfg)
    if "subnormal" in name:
        assert A.subnormal_run(ref) >= A.SUB_ZEROS
    got = run_dev(blk, x)
    assert_bits(got, ref, f"{name} [{c.path}; {p.chunks} chunks, {len(p.flagged)} flagged, "
                          f"{len(p.undetermined)} undetermined, {len(p.late)} for pass 3]")
    # what pass 2 flagged on the device is what the reference alone predicts: the warm-ups
    # are the specified ones (start, length, seed), not merely repaired afterwards
    assert [int(v) for v in blk.taps(2)] == [p.chunks, len(p.flagged)]


# ---- streaming: the carried envelope and oscillator count across paths ----------------------
STREAM_CALLS = [A.N_LANE_RAGGED, A.N_WAVE, 3001, 1, A.N_WAVE, 700]
STREAM_PATHS = ["lane", "wave", "seq", "seq", "wave", "seq"]
STREAMS = {
    "agc-re-plateaus": ("agc", A.AGC, lambda n: A.plateaus(n, False, 48e3, 31, 40_000)),
    "agc-iq-plateaus": ("agc_iq", A.AGC, lambda n: A.plateaus(n, True, 48e3, 32, 40_000)),
    "agc-re-noise": ("agc", A.AGC, lambda n: A.noise_steps(n, False, 33)),
    "agc-iq-noise": ("agc_iq", A.AGC, lambda n: A.noise_steps(n, True, 34)),
    "cw-keyups": ("cw", A.CW, lambda n: A.cw_long_keyups(n, 35, 6000, 30_000)),
    "cw-same-ragged": ("cw", A.CW_SAME, lambda n: A.cw_ragged(n, 36)),
    "cw-subnormal": ("cw", A.CW_SUB, lambda n: A.cw_long_keyups(n, 37, 3000, 2 * A.SUB_ZEROS + 2000)),
}


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_changes_path(gpu_lib, oracle, name):
    """One stream in calls that go lane, wave, seq, a 1-sample call, wave again, seq: the
    carried envelope (and CwKeyedMod's oscillator count) crosses every boundary. The AGC
    oracle is cut identically (the reference applies its seed rule per call)."""
    kind, cfg, mk = STREAMS[name]
    blk = make(gpu_lib, kind, cfg)
    W = warm(blk, kind, cfg)
    assert [A.path_of(c, W) for c in STREAM_CALLS] == STREAM_PATHS
    x = mk(sum(STREAM_CALLS))
    got = run_dev(blk, x, STREAM_CALLS)
    assert_bits(got, reference(oracle, x, kind, cfg, STREAM_CALLS), f"stream {name} {STREAM_PATHS}")


@pytest.mark.parametrize("iq", [False, True])
@pytest.mark.parametrize("cfg", [A.AGC, A.AGC_SHORT], ids=["stalls", "reseeds"])
def test_stream_silence_then_signal(gpu_lib, oracle, iq, cfg):
    """A first call of zeros, then signal, then zeros, then signal. AGC: the
    envelope stalls on a subnormal and is carried. AGC_SHORT: it decays to exactly 0, so the
    second and fourth call reseed from their first sample (agc.rs:57-60), as the oracle does
    when cut identically."""
    kind = A.kind_of(iq)
    blk = make(gpu_lib, kind, cfg)
    W = warm(blk, kind, cfg)
    calls = [A.N_WAVE, A.N_WAVE, A.N_WAVE, 1025]
    assert [A.path_of(c, W) for c in calls] == ["wave"] * 3 + ["wave" if cfg is A.AGC_SHORT else "seq"]
    x = A.noise_steps(sum(calls), iq, 41, seg=1000)
    x[:A.N_WAVE] = 0
    x[2 * A.N_WAVE:3 * A.N_WAVE] = 0
    end_first = oracle.agc(x[:calls[0]], *cfg)[1]
    assert (end_first == 0.0) == (cfg is A.AGC_SHORT)
    got = run_dev(blk, x, calls)
    assert_bits(got, reference(oracle, x, kind, cfg, calls), f"silence then signal {kind} {cfg}")
    if cfg is A.AGC_SHORT:  # the cut is visible: an uncut reference differs
        assert not np.array_equal(u32(got), u32(reference(oracle, x, kind, cfg)))


def test_stream_cw_silence_then_keying(gpu_lib, oracle):
    """CwKeyedMod: a first call of zeros (lane path), then keying (wave path)."""
    blk = make(gpu_lib, "cw", A.CW)
    x = np.concatenate([np.zeros(A.N_LANE_RAGGED, f32), A.cw_ragged(A.N_WAVE, 42)])
    got = run_dev(blk, x, [A.N_LANE_RAGGED, A.N_WAVE])
    assert_bits(got, oracle.cw_mod(x, *A.CW), "cw silence then keying")


# ---- reset, run to run ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["agc-re-lane-plateaus", "agc-iq-lane-inf", "cw-lane-keyups", "cw-wave-same-keyups-last1",
                                  "agc-iq-wave-plateaus-last1"])
def test_reset_and_run_to_run(gpu_lib, oracle, name):
    """reset(), then the same bits again; a second handle gives the same bits; and without
    reset the call continues the stream (the reference over x twice)."""
    c = CASE[name]
    x = c.make()
    ref = reference(oracle, x, c.kind, c.cfg)
    blk = make(gpu_lib, c.kind, c.cfg)
    first = run_dev(blk, x)
    blk.reset()
    again = run_dev(blk, x)
    other = run_dev(make(gpu_lib, c.kind, c.cfg), x)
    assert_bits(first, ref, f"{name} first")
    assert_bits(again, ref, f"{name} after reset")
    assert_bits(other, ref, f"{name} second handle")
    cont = run_dev(blk, x)
    both = reference(oracle, np.concatenate([x, x]), c.kind, c.cfg, [len(x), len(x)])
    assert_bits(cont, both[len(x):], f"{name} continued without reset")


# ---- in place on the lane path --------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True])
@pytest.mark.parametrize("k", [0, 1, 1000, -1, -1000])
def test_lane_in_place(gpu_lib, oracle, iq, k):
    """AgcRms / AgcRmsIq with overlapping device ranges on the lane path (the plateaus case:
    both fixers read the input after outputs were written): k = 0 `out is x`; k > 0
    out = buf[k:], x = buf[:-k]; k < 0 x = buf[|k|:], out = buf[:-|k|]. Each equals the
    non-aliased result (the oracle's) bitwise."""
    import torch

    c = CASE[f"agc-{'iq' if iq else 're'}-lane-plateaus"]
    x = c.make()
    ref = reference(oracle, x, c.kind, c.cfg)
    n, s = len(x), abs(k)
    buf = torch.zeros(n + s, dtype=torch.complex64 if iq else torch.float32, device="cuda")
    src, dst = (buf[:n], buf[s:]) if k >= 0 else (buf[s:], buf[:n])
    src.copy_(torch.from_numpy(x))
    blk = make(gpu_lib, c.kind, c.cfg)
    assert A.path_of(n, warm(blk, c.kind, c.cfg)) == "lane"
    out = blk.process_device(src, dst)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    assert_bits(out.cpu().numpy(), ref, f"lane in place iq={iq} k={k}")


# ---- the host cut ---------------------------------------------------------------------------
def test_host_cut_is_wave_path(gpu_lib, oracle):
    """AgcRmsIq.process on 2^21 + 5 host samples: Block::host_chunked cuts it into device
    calls of 2^20, 2^20 and 5 samples, which are 4096 chunks each at most: the device calls
    process() makes are wave-path (and one sequential), never lane-path. Bit-exact with
    the oracle cut the same way."""
    n = (1 << 21) + 5
    calls = A.host_cut(n, 8)
    blk = make(gpu_lib, "agc_iq", A.AGC)
    W = warm(blk, "agc_iq", A.AGC)
    assert calls == [1 << 20, 1 << 20, 5]
    assert [A.path_of(c, W) for c in calls] == ["wave", "wave", "seq"] and A.n_chunks(1 << 20, W) == 4096
    x = A.plateaus(n, True, 48e3, 51, 40_000)
    got = blk.process(x)
    assert_bits(got, reference(oracle, x, "agc_iq", A.AGC, calls), "AgcRmsIq.process host cut")


# ---- NaN ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,path", [("agc", "lane"), ("agc_iq", "lane"), ("agc", "wave"), ("agc_iq", "wave"),
                                       ("cw", "lane"), ("cw", "wave")])
def test_nan_sample(gpu_lib, oracle, kind, path):
    """One NaN at sample 3L + 7 (module docstring): NaN positions equal, all other bits equal."""
    n = A.N_LANE_RAGGED if path == "lane" else A.N_WAVE
    if kind == "cw":
        cfg, x = A.CW, A.cw_ragged(n, 61)
        x[3 * 256 + 7] = np.nan
    else:
        cfg, x = A.AGC, A.noise_steps(n, kind == "agc_iq", 62)
        x[3 * 256 + 7] = np.nan  # the real part
    blk = make(gpu_lib, kind, cfg)
    assert A.path_of(n, warm(blk, kind, cfg)) == path
    ref = reference(oracle, x, kind, cfg).view(f32)
    got = run_dev(blk, x).view(f32)
    nan = np.isnan(ref)
    assert nan.any() and not nan.all()
    if kind != "cw":  # after the NaN sample: max_gain * x, finite
        assert np.count_nonzero(nan) == 1 and np.array_equal(ref[-8:], (f32(20.0) * x.view(f32)[-8:]).astype(f32))
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))
    print(f"[parity] nan {kind} {path}: {np.count_nonzero(nan)} NaN words in place, {np.count_nonzero(~nan)} words bit-exact")
