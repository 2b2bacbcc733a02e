"""tests/agc_ref.py against the C oracle, and the case table of tests/test_gpu_agc_exact.py
against agc_ref: the conditions that keep the GPU cases honest (each reaches the kernel it
names, and each fixer case really has chunks only that fixer can repair). No GPU needed."""
import numpy as np
import pytest

import agc_ref as A

f32 = np.float32


def _beq(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---- the step and the coefficients ----------------------------------------------------
@pytest.mark.parametrize("cfg", [A.CW, A.CW_FAST, A.CW_SAME, A.CW_SUB, A.CW_SHORT])
def test_cw_step_is_the_oracles(oracle, cfg):
    """At tone 0 the Nco is (1, 0) and y.real = env * 1: the numpy step, its coefficients and
    its clamp are the oracle's, bit for bit, through rises, falls, values outside [0, 1]
    and the subnormal plateau after a 0.1 ms fall."""
    x = np.concatenate([A.cw_ragged(6000, 1, dot=300), np.zeros(3000, f32), np.ones(2500, f32), np.zeros(1500, f32)])
    ref = oracle.cw_mod(x, cfg[0], 0.0, cfg[2], cfg[3])
    env = A.cw_env(x, cfg)
    assert _beq(env, ref.real)
    assert not np.any(ref.imag)
    if cfg is A.CW_SUB:
        t = env[-500:]
        assert np.all(t != 0) and np.all(np.abs(t) < 2.0 ** -126), "the 0.1 ms fall did not stall on a subnormal"


@pytest.mark.parametrize("iq", [False, True])
@pytest.mark.parametrize("cfg", [A.AGC, A.AGC_BENCH, A.AGC_SHORT])
def test_agc_true_envelopes_are_the_oracles_on_prefixes(oracle, iq, cfg):
    """The predictor's truth: env_seq's envelope after k samples is oracle.agc's end
    envelope over x[:k], for noise, plateaus and a stream with one inf."""
    n = 5000
    for x in (A.noise_steps(n, iq, 2, seg=700), A.plateaus(n, iq, 48e3, 3, 900),
              A.with_inf(A.noise_steps(n, iq, 4, seg=700), 777)):
        E = A.agc_env(x, cfg, iq)
        for k in (1, 2, 255, 256, 257, 776, 777, 778, 779, 1024, 3979, 4999, 5000):
            assert _beq(E[k - 1], f32(oracle.agc(x[:k], *cfg)[1])), (cfg, iq, k)


@pytest.mark.parametrize("iq", [False, True])
def test_lanes_walk_is_a_fresh_oracle_run(oracle, iq):
    """lanes_walk (the CW predictor's side-by-side warm-ups) against fresh oracle.agc runs."""
    x = A.noise_steps(6000, iq, 5, seg=500)
    kind = A.kind_of(iq)
    d = A.drive(kind, x)
    att, rel = A.agc_coefs(*A.AGC[:3])
    s = np.array([0, 17, 300, 2048, 5000])
    e = np.array([3979, 1000, 301, 6000, 5255])
    got = A.lanes_walk(d, s, e, np.maximum(d[s], f32(1e-12)), att, rel, False, 3979)
    ref = [oracle.agc(x[a:b], *A.AGC)[1] for a, b in zip(s, e)]
    assert _beq(got, ref)


def test_dispatch_mirror():
    """warmup_len / chunk_len / path_of at known sizes: 48 kHz with a 5 ms release has
    W = 4974, L = 311 (tools/agc_bench.py prints both); a lane-per-chunk call needs more than
    4096 chunks; W >= n / 4 is one sequential wave."""
    att, rel = A.agc_coefs(48e3, 0.2, 5.0)
    W = A.warmup_len(max(att, rel))
    assert (W, A.chunk_len(1 << 20, W), A.n_chunks(1 << 20, W)) == (4974, 311, 3372)
    assert A.path_of(4096 * 311, W) == "wave" and A.path_of(4096 * 311 + 1, W) == "lane"
    assert A.path_of(4 * W + 3, W) == "seq" and A.path_of(4 * W + 4, W) == "wave"
    assert A.warmup_len(1.0) == -1 and A.path_of(1 << 24, -1) == "seq"
    assert A.warmup_len(0.0) == 0
    W4 = A.warm_of("agc", A.AGC)
    assert W4 == 3979 and A.chunk_len(A.N_LANE, W4) == 256
    assert [A.path_of(n, W4) for n in (4096 * 256, 4096 * 256 + 1)] == ["wave", "lane"]
    # the host cut: device calls of 2^20 cf32 samples are 4096 chunks at most, never the lane path
    assert A.host_cut((1 << 21) + 5, 8) == [1 << 20, 1 << 20, 5]
    assert A.host_cut((1 << 21) - 1, 8) == [(1 << 21) - 1]
    assert all(A.path_of(c, W4) != "lane" for c in A.host_cut((1 << 21) + 5, 8))


# ---- the GPU file's case table ---------------------------------------------------------
@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_case_reaches_its_path_and_fixers(oracle, case):
    """Every single-call GPU case: the path it names, and from the predictor: 'none' cases
    have 0 chunks with a wrong entry (the count is exact: no re-run at all); 'runs' cases
    have chunks pass 2 flags (k_agc_fix_runs); 'both' cases also have wrong chunks pass 2
    does not flag (k_agc_fix)."""
    x = case.make()
    assert len(x) == case.n
    p = A.predict(x, case.cfg, case.kind, oracle)
    print(f"[agc_ref] {case.name}: n {case.n} W {p.W} L {p.L} chunks {p.chunks} path {p.path}; "
          f"bad {len(p.bad)} undetermined {len(p.undetermined)} flagged {len(p.flagged)} late {len(p.late)}")
    assert p.path == case.path
    if case.fix == "none":
        assert p.bad == [] and p.flagged == []
    else:
        assert len(p.flagged) >= 1 and len(p.bad) >= 1
        assert all(c * p.L > p.W for c in p.bad), "a chunk that starts from the carried state cannot be wrong"
        if case.fix == "both":
            assert len(p.late) >= 1
    if case.name.endswith("inf-last"):
        assert p.bad == p.flagged == [p.chunks - 1], "the last chunk alone must be wrong, and flagged"
    if case.kind == "cw":
        assert p.late == [], "a determined CW chunk is exact (the bracket is monotone)"


def test_table_covers_every_path_policy_and_fixer():
    """seq, wave and lane by each of the three policies; each fixer needed on the wave path
    and on the lane path."""
    have = {(c.kind, c.path) for c in A.CASES}
    assert have == {(k, p) for k in ("agc", "agc_iq", "cw") for p in ("seq", "wave", "lane")}
    for path in ("wave", "lane"):
        assert any(c.path == path and c.fix == "both" for c in A.CASES)
        assert any(c.path == path and c.fix == "runs" and c.kind == "cw" for c in A.CASES)
    sizes = {(c.path, c.n) for c in A.CASES}
    assert {("lane", A.N_LANE_RAGGED), ("lane", A.N_LANE), ("lane", A.N_LANE_BENCH), ("wave", A.N_WAVE_MAX),
            ("wave", A.N_WAVE), ("wave", 257)} <= sizes
    assert {n for p, n in sizes if p == "seq"} == set(A.N_SEQ)


def test_subnormal_cases_are_not_vacuous(oracle):
    """The CW_SUB cases: after each key-up the reference's own output is nonzero and
    subnormal for at least 2^14 samples (a device that flushed denormals would differ)."""
    for name in ("cw-lane-subnormal", "cw-wave-subnormal"):
        case = next(c for c in A.CASES if c.name == name)
        x = case.make()
        run = A.subnormal_run(oracle.cw_mod(x, *case.cfg))
        print(f"[agc_ref] {name}: longest nonzero subnormal stretch of |y| {run} samples")
        assert run >= A.SUB_ZEROS


def test_silence_reseeds_only_the_short_agc(oracle):
    """The streaming cases' first call of zeros: AGC_SHORT's envelope decays to exactly 0, so
    the reference reseeds on the next call (agc.rs:57-60); AGC's stalls on a subnormal."""
    for iq in (False, True):
        z = np.zeros(A.N_WAVE, np.complex64 if iq else f32)
        assert oracle.agc(z, *A.AGC_SHORT)[1] == 0.0
        e = oracle.agc(z, *A.AGC)[1]
        assert 0.0 < e < 2.0 ** -126
